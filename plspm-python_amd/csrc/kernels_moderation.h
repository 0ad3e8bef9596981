// kernels_moderation.h -- moderation analysis of every bootstrap replicate by the two-stage approach (the definitions: moderation_core.h): the
// replicate's stage-1 scores are formed from its own record weights, row by row, their products are summed with the row multiplicities, and the second stage is
// regressed on the extended correlation matrix.  Four kernels on the handle's stream behind the metric solver of a pass, fp64 throughout, no floating-point
// atomics, every sum in one fixed order -- a record depends on the replicate's draws and its bootstrap record, not on B, the pass or the sub-batch.
//   moderation_counts_kernel    one workgroup per replicate: the LDS histogram of its N draws (the Philox draws of replicate rep0 + b, or explicit index rows; the
//                               precedent: kernels_resample.h) -> the dense uint16 multiplicities, transposed [lane group][row][64] so that the lanes of the row
//                               pass read one row's counts as one 128-byte run
//   moderation_prepare_kernel   one wave per replicate, opening like assess_kernel (kernels_moments.h, both moment layouts): mu, s, v normalised per block, the sign
//                               -> the score map of the needed LVs as coefficients of the resident mean-shifted columns and one offset per LV, transposed
//                               [lane group][coefficient][64] (the coef_table_kernel layout), and the needed LVs' correlations rc
//   moderation_rows_kernel      the row pass.  Lane = replicate, 64 per group; the group's table in LDS (TABLE_LDS) or, where table and values do not fit
//                               together, read from memory as 512-byte runs; a wave takes one row block; the row of Xa is wave-uniform and comes through the scalar
//                               cache; a lane keeps its sums in registers, count x value x value; partial sums per (row block, sum, replicate) leave as plain
//                               vector stores.  Only the columns of the needed LVs are read.
//   moderation_finish_kernel    one wave per replicate: the partials added in row-block order, then moderation_core.h moderation_record on a wave executor
#pragma once
#include "kernels_moments.h"
#include "moderation_core.h"

struct ModCountsArgs {
    int N; long nb;
    const int* idx;                                // explicit rows [nb][N] of the pass, or null: Philox draws
    uint64_t seed; int64_t rep0;                   // replicate id of the pass's first problem
    int ones;                                      // every multiplicity 1 (the full sample)
    unsigned short* cnt;                           // [groups][N][64]
};

__global__ void __launch_bounds__(256) moderation_counts_kernel(const ModCountsArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mod_counts_lds[];
    unsigned* hist = reinterpret_cast<unsigned*>(mod_counts_lds);      // 16-bit counters, two per word (a count never exceeds N <= 65535)
    const int tid = threadIdx.x, N = a.N;
    const long b = blockIdx.x;
    unsigned short* __restrict__ out = a.cnt + ((b >> 6) * (long)N) * 64 + (b & 63);
    if (a.ones) {
        for (int i = tid; i < N; i += 256) out[(long)i * 64] = 1;
        return;
    }
    const int nwords = (N + 1) >> 1;
    for (int i = tid; i < nwords; i += 256) hist[i] = 0u;
    __syncthreads();
    if (a.idx) {
        const int* __restrict__ my = a.idx + b * (long)N;
        for (int i = tid; i < N; i += 256) {
            const int r = my[i];
            if ((unsigned)r < (unsigned)N) atomicAdd(&hist[r >> 1], (r & 1) ? 0x10000u : 1u);      // (a row outside [0, N) raises the batch's own error word)
        }
    } else {
        const uint64_t rep = (uint64_t)(a.rep0 + b);
        const int nq = (N + 3) >> 2;
        for (int q = tid; q < nq; q += 256) {
            const u32x4 u = resample_quad(a.seed, rep, (uint32_t)q);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < N) { const unsigned r = to_index(u.v[j], (uint32_t)N); atomicAdd(&hist[r >> 1], (r & 1u) ? 0x10000u : 1u); }
        }
    }
    __syncthreads();
    for (int i = tid; i < N; i += 256) out[(long)i * 64] = (unsigned short)((hist[i >> 1] >> ((i & 1) << 4)) & 0xffffu);
}

struct ModPrepareArgs {
    MomentLayout mom;
    plspm::ModDesc d;
    int R;                                         // bootstrap record width (weights at 0, loadings at R - P, status at R)
    const int* boff;
    const double* rows; long row_stride;
    double* table;                                 // [groups][ncoef + nl][64]
    double* rcn;                                   // [nb][nl x nl]
    long nb;
};

template <bool DENSE>
__global__ void __launch_bounds__(64 * plspm::kModPrepareWaves) moderation_prepare_kernel(const ModPrepareArgs a) {
    extern __shared__ double mod_prepare_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * plspm::kModPrepareWaves + wave;
    if (b >= a.nb) return;
    const double* __restrict__ rec = a.rows + b * a.row_stride;
    if (!(rec[a.R] == 0.0)) return;                // (a failed replicate: the finish kernel writes its record)
    const plspm::ModLayout& y = a.d.lay;
    const int P = a.mom.P, ld = a.mom.ld, nl = y.nl, ncoef = y.ncoef;
    double* isd = mod_prepare_lds + (long)wave * plspm::moderation_prepare_doubles(y);
    double *mu = isd + P, *v = mu + P, *nrm = v + P, *sg = nrm + nl;
    const int *need = a.d.list(plspm::MO_NEED), *ccol = a.d.list(plspm::MO_COEF_COL), *clv = a.d.list(plspm::MO_COEF_LV), *coff = a.d.list(plspm::MO_COEF_OFF);
    const double* __restrict__ M = a.mom.gram + b * a.mom.gstride;
    const double inv_n = 1.0 / assess_moment<DENSE>(M, ld, P, P);
    for (int c = lane; c < ncoef; c += 64) {
        const int p = ccol[c];
        const MvStats mv = mv_stats<DENSE>(M, ld, p, P, inv_n);
        isd[p] = mv.varies ? 1.0 / mv.sd : 0.0; mu[p] = mv.mean; v[p] = mv.varies ? rec[p] * mv.sd : 0.0;
    }
    wave_sync();
    auto cor = [&](int p, int q) -> double { return (p == q) ? 1.0 : fma(-mu[p], mu[q], assess_moment<DENSE>(M, ld, p, q) * inv_n) * (isd[p] * isd[q]); };
    // the diagonal blocks: v'Rv and the sign of the needed LVs
    for (int li = 0; li < nl; ++li) {
        const int b0 = a.boff[need[li]], b1 = a.boff[need[li] + 1];
        double sT = 0.0, sU = 0.0;
        for (int c0 = b0; c0 < b1; c0 += 64) {
            const bool on = c0 + lane < b1;
            const int q = on ? c0 + lane : b1 - 1;
            double tq = 0.0;
            for (int p = b0; p < b1; ++p) tq = fma(v[p], cor(p, q), tq);
            sT += wv::allsum(on ? v[q] * tq : 0.0);
            sU += wv::allsum(on ? tq * rec[a.R - P + q] : 0.0);
        }
        if (lane == 0) { nrm[li] = 1.0 / sqrt(sT); sg[li] = (sU < 0.0) ? -1.0 : 1.0; }
    }
    wave_sync();
    // the score map: y_l = sum_p coef_p xa_p + off_l, xa the resident mean-shifted columns (mu is their mean)
    const long g = b >> 6, r = b & 63, ntab = ncoef + nl;
    double* __restrict__ tab = a.table + g * ntab * 64 + r;
    for (int li = 0; li < nl; ++li) {
        double off = 0.0;
        for (int c0 = coff[li]; c0 < coff[li + 1]; c0 += 64) {
            const int c = c0 + lane;
            double mine = 0.0;
            if (c < coff[li + 1]) {
                const int p = ccol[c];
                const double coef = sg[li] * v[p] * nrm[li] * isd[p];
                tab[(long)c * 64] = coef;
                mine = coef * mu[p];
            }
            off += wv::allsum(mine);
        }
        if (lane == 0) tab[(long)(ncoef + li) * 64] = -off;
    }
    // the needed LVs' correlations
    double* __restrict__ rc = a.rcn + b * (long)nl * nl;
    for (int li = 0; li < nl; ++li) {
        const int p0 = a.boff[need[li]], p1 = a.boff[need[li] + 1];
        if (lane == 0) rc[li * nl + li] = 1.0;
        for (int mi = li + 1; mi < nl; ++mi) {
            const int b0 = a.boff[need[mi]], b1 = a.boff[need[mi] + 1];
            double pt = 0.0;
            for (int c0 = b0; c0 < b1; c0 += 64) {
                const bool on = c0 + lane < b1;
                const int q = on ? c0 + lane : b1 - 1;
                double tq = 0.0;
                for (int p = p0; p < p1; ++p) tq = fma(v[p], cor(p, q), tq);
                pt += wv::allsum(on ? v[q] * tq : 0.0);
            }
            if (lane == 0) { const double x = sg[li] * sg[mi] * pt * (nrm[li] * nrm[mi]); rc[li * nl + mi] = x; rc[mi * nl + li] = x; }
        }
    }
    (void)clv;
}

struct ModRowsArgs {
    const double* Xa; int N, PA;
    plspm::ModDesc d;
    const int* boff;
    const unsigned short* cnt;                     // [groups][N][64]
    const double* table;                           // [groups][ncoef + nl][64]
    double* partial;                               // [row_blocks][nsums][nbpad]
    long nbpad;                                    // 64 x groups
    int row_block, row_blocks;
};

template <int NACC, bool TABLE_LDS>
__global__ void __launch_bounds__(64 * plspm::kModRowsWaves) moderation_rows_kernel(const ModRowsArgs a) {
    extern __shared__ double mod_rows_lds[];
    const plspm::ModLayout& y = a.d.lay;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nl = y.nl, T = y.T, ncoef = y.ncoef, nsums = y.nsums, ntab = ncoef + nl;
    const long g = blockIdx.y;
    const double* __restrict__ tg = a.table + g * (long)ntab * 64;
    if (TABLE_LDS) {
        for (int e = threadIdx.x; e < ntab * 64; e += 64 * plspm::kModRowsWaves) mod_rows_lds[e] = tg[e];
        __syncthreads();
    }
    const int rb = (int)blockIdx.x * plspm::kModRowsWaves + wave;      // wave-uniform: rows [rb row_block, (rb + 1) row_block)
    if (rb >= a.row_blocks) return;                                     // (behind the one barrier)
    const double* tab = (TABLE_LDS ? mod_rows_lds : tg) + lane;
    double* val = mod_rows_lds + (TABLE_LDS ? (long)ntab * 64 : 0) + (long)wave * plspm::moderation_values_doubles(y) + lane;      // [1 + nl + T][64]: a lane reads what it wrote
    const int *need = a.d.list(plspm::MO_NEED), *coff = a.d.list(plspm::MO_COEF_OFF), *tsa = a.d.list(plspm::MO_TERM_SA), *tsb = a.d.list(plspm::MO_TERM_SB),
              *sab = a.d.list(plspm::MO_SUM_AB);
    val[0] = 1.0;
    double acc[NACC];
#pragma unroll
    for (int s = 0; s < NACC; ++s) acc[s] = 0.0;
    const int i0 = rb * a.row_block, i1 = min(a.N, i0 + a.row_block);
    const unsigned short* __restrict__ cnt = a.cnt + (g * (long)a.N) * 64 + lane;
    for (int i = i0; i < i1; ++i) {
        const double c = (double)cnt[(long)i * 64];
        const double* __restrict__ x = a.Xa + (long)i * a.PA;           // wave-uniform: scalar loads
        for (int li = 0; li < nl; ++li) {
            const double* __restrict__ xb = x + a.boff[need[li]];
            const int c0 = coff[li], k = coff[li + 1] - c0;
            const double* tb = tab + (long)c0 * 64;
            double s0 = tab[(long)(ncoef + li) * 64], s1 = 0.0;
            int q = 0;
            for (; q + 1 < k; q += 2) { s0 = fma(xb[q], tb[(long)q * 64], s0); s1 = fma(xb[q + 1], tb[(long)(q + 1) * 64], s1); }
            if (q < k) s0 = fma(xb[q], tb[(long)q * 64], s0);
            val[(1 + li) * 64] = s0 + s1;
        }
        for (int t = 0; t < T; ++t) val[(1 + nl + t) * 64] = val[(1 + tsa[t]) * 64] * val[(1 + tsb[t]) * 64];
#pragma unroll
        for (int s = 0; s < NACC; ++s)
            if (s < nsums) { const int ab = sab[s]; acc[s] = fma(c * val[ab & 0xffff], val[ab >> 16], acc[s]); }
    }
    double* __restrict__ out = a.partial + ((long)rb * nsums) * a.nbpad + g * 64 + lane;
#pragma unroll
    for (int s = 0; s < NACC; ++s)
        if (s < nsums) out[(long)s * a.nbpad] = acc[s];
}

struct ModFinishArgs {
    plspm::ModDesc d;
    int R, e_total, row_blocks;
    long nbpad;
    double n;                                      // rows of a data set: the multiplicities of a replicate add up to N
    const double* partial; const double* rcn;
    const double* rows; long row_stride;
    double* out; long nb;                          // record b at out + b * (W + 2)
};

// the wave executor: lanes stride over the indices; the hand-over between lanes is the wave's own LDS order
struct ModWaveExec {
    static constexpr int kcap = 8;                 // regressions on at most 8 regressors in registers (solver_core.h spd_solve)
    int lane;
    template <class F> __device__ __forceinline__ void par(int n, F f) { for (int i = lane; i < n; i += 64) f(i); wave_sync(); }
    template <class F> __device__ __forceinline__ void one(F f) { if (lane == 0) f(); wave_sync(); }
};

__global__ void __launch_bounds__(64) moderation_finish_kernel(const ModFinishArgs a) {
    extern __shared__ double mod_finish_lds[];
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    const plspm::ModLayout& y = a.d.lay;
    const int W = plspm::moderation_width(y), nsums = y.nsums, nl = y.nl;
    const double* __restrict__ rec = a.rows + b * a.row_stride;
    double* __restrict__ out = a.out + b * (long)(W + 2);
    const double st = rec[a.R];
    if (!(st == 0.0)) { wave_void_record(out, W, st, rec[a.R + 1], lane); return; }
    plspm::ModWs w;
    plspm::moderation_carve(w, mod_finish_lds, y, a.e_total);
    for (int s = lane; s < nsums; s += 64) {
        const double* __restrict__ p = a.partial + (long)s * a.nbpad + b;
        double t = 0.0;
        for (int rb = 0; rb < a.row_blocks; ++rb) t += p[((long)rb * nsums) * a.nbpad];      // row-block order
        w.tot[s] = t;
    }
    for (int e = lane; e < nl * nl; e += 64) w.rcn[e] = a.rcn[b * (long)nl * nl + e];
    wave_sync();
    ModWaveExec ex{lane};
    plspm::moderation_record(ex, a.d, w, a.n, rec, a.R, out);
}
