// kernels_assess.h -- measurement-model assessment of every bootstrap replicate: Cronbach's alpha, rho_A, rho_C and AVE per latent variable,
// HTMT, HTMT2 and the construct correlation per pair of latent variables, from the replicate's moment matrix -- which only exists between the Gram and the
// next pass -- and the weights and loadings of its record.  One wave per replicate, four waves per workgroup; the waves share nothing and meet at no workgroup
// barrier (a wave without a replicate, or with a failed one, leaves at once).  fp64 throughout; no atomics; every sum in one fixed order.
//
// With n, the column sums and the cross products M of the mean-shifted columns:  mu_p = M_p1 / n,  c_pq = M_pq / n - mu_p mu_q,  s_p = sqrt(c_pp),
// r_pq = c_pq / (s_p s_q) (r_pp = 1),  v_p = w_p s_p.  Lane q serves MV q of a window of 64 columns; the per-MV values 1 / s, mu and v live in the wave's LDS slice.
//   pass 1, per block l:  rows p of the block x the block's own columns -> sum_{p<q} |r|, log |r|, r;  t_q = sum_p v_p r_pq;  v'Rv, v'v, sum v^4, sum t_q lambda_q
//                         (the sign of the fit: t is the loading before the sign rule, lambda the one behind it), sum lambda, sum lambda^2 -- butterfly sums
//   pass 2, per block i:  rows p of block i x every column behind the block -> per column sum_p |r|, sum_p log |r|, v_q sum_p v_p r_pq, reduced by the block
//                         of q: one lane per block adds its segment of the window in ascending order
// The loads of sixteen rows are issued together (the kernel is a chain of memory round trips, not of arithmetic: one trip per row made it 0.15 ms on the
// headline's 5,000 replicates, a third of the step).  Row p is read along the lanes: in the dense layout (upper triangle, entry (r, c >= r) at r * ld + c) contiguously wherever q >= p, which is all of pass 2;
// the entries of a diagonal block below its diagonal (pass 1, q < p) are read down their column.  The tile-packed layout is read through packed_index.
#pragma once
#include "kernels_moments.h"

constexpr int ASSESS_WAVES = 4;

struct AssessArgs {
    MomentLayout mom;
    int L, R;                                      // LVs, record width (weights at 0, loadings at R - P, status at R, iterations at R + 1)
    const int* boff; const int* lvof; const int* mode;
    const double* rows; long row_stride;
    double* out; long nb;                          // record b at out + b * (A + 2), A = 4 L + 3 L (L - 1) / 2
    double* side;                                  // optional [nb x 3 L]: per LV the fit's sign | v'Rv | v'v as pass 1 ends with them (kernels_plsc.h reads them); null: no store
    long long* marks;                              // phase clocks of problem 0 (`make marks`; null in the release library)
};
#ifdef PLSPM_DEBUG_MARKS
#define ASSESS_MARK(k) do { if (a.marks && b == 0 && lane == 0) a.marks[k] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define ASSESS_MARK(k) do { } while (0)
#endif

constexpr int ASSESS_ROWS = 16;                    // rows of a block whose loads are in flight together (one memory round trip per batch, not per row)

// (doubles of one wave's LDS slice: solver_core.h assess_wave_doubles, where the launch plan sees it too)

// sum of log |r| over a column as ONE logarithm: the factors are multiplied up, and after every fourth the product's exponent moves into an integer (|r| <= 1
// up to rounding and >= 1e-19 or so unless it is exactly 0, so four factors neither overflow nor underflow; a zero stays a zero: log 0 = -inf, exp(-inf) = 0)
__device__ __forceinline__ double assess_log_of(double prod, int ex) {
    int e;
    prod = frexp(prod, &e);
    return fma((double)(ex + e), 0.693147180559945309417, log(prod));
}

template <bool DENSE>
__global__ void __launch_bounds__(64 * ASSESS_WAVES) assess_kernel(const AssessArgs a) {
    extern __shared__ double assess_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * ASSESS_WAVES + wave;
    if (b >= a.nb) return;
    const int P = a.mom.P, L = a.L, ld = a.mom.ld;
    const int npairs = L * (L - 1) / 2, A = 4 * L + 3 * npairs;
    const double* __restrict__ rec = a.rows + b * a.row_stride;
    double* __restrict__ out = a.out + b * (long)(A + 2);
    const double st = rec[a.R];
    if (!(st == 0.0)) { wave_void_record(out, A, st, rec[a.R + 1], lane); return; }
    if (lane == 0) { out[A] = st; out[A + 1] = rec[a.R + 1]; }
    double* isd = assess_lds + (long)wave * plspm::assess_wave_doubles(P, L);
    double *mu = isd + P, *v = mu + P, *lam = v + P, *bm = lam + P, *bg = bm + L, *bt = bg + L, *bs = bt + L, *pa = bs + L, *pg = pa + L, *pt = pg + L, *win = pt + L;
    const double* __restrict__ M = a.mom.gram + b * a.mom.gstride;
    ASSESS_MARK(0);
    const double inv_n = 1.0 / assess_moment<DENSE>(M, ld, P, P);
    for (int p = lane; p < P; p += 64) {
        const MvStats mv = mv_stats<DENSE>(M, ld, p, P, inv_n);
        isd[p] = 1.0 / mv.sd; mu[p] = mv.mean; v[p] = rec[p] * mv.sd; lam[p] = rec[a.R - P + p];
    }
    wave_sync();
    ASSESS_MARK(1);

    // ---- pass 1: the diagonal blocks
    for (int l = 0; l < L; ++l) {
        const int b0 = a.boff[l], b1 = a.boff[l + 1], k = b1 - b0;
        double sA = 0.0, sG = 0.0, sR = 0.0, sT = 0.0, s2 = 0.0, s4 = 0.0, sU = 0.0, sL = 0.0, sL2 = 0.0;
        for (int c0 = b0; c0 < b1; c0 += 64) {
            const bool on = c0 + lane < b1;
            const int q = on ? c0 + lane : b1 - 1;
            const double muq = mu[q], isq = isd[q];
            double aq = 0.0, rq = 0.0, tq = 0.0, prod = 1.0;
            int ex = 0;
            for (int p0 = b0; p0 < b1; p0 += ASSESS_ROWS) {
                double mm[ASSESS_ROWS];
#pragma unroll
                for (int u = 0; u < ASSESS_ROWS; ++u) mm[u] = assess_moment<DENSE>(M, ld, min(p0 + u, b1 - 1), q);
#pragma unroll
                for (int u = 0; u < ASSESS_ROWS; ++u) {
                    const int p = p0 + u;
                    if (p < b1) {                                              // (uniform)
                        const double r = (p == q) ? 1.0 : fma(-mu[p], muq, mm[u] * inv_n) * (isd[p] * isq);
                        tq = fma(v[p], r, tq);
                        if (p < q) { const double ar = fabs(r); aq += ar; rq += r; prod *= ar; }
                        if ((u & 3) == 3) { int e; prod = frexp(prod, &e); ex += e; }      // (see assess_log_of)
                    }
                }
            }
            const double gq = assess_log_of(prod, ex);
            const double vq = v[q], lq = lam[q];
            sA += wv::allsum(on ? aq : 0.0); sG += wv::allsum(on ? gq : 0.0); sR += wv::allsum(on ? rq : 0.0);
            sT += wv::allsum(on ? vq * tq : 0.0); s2 += wv::allsum(on ? vq * vq : 0.0); s4 += wv::allsum(on ? (vq * vq) * (vq * vq) : 0.0);
            sU += wv::allsum(on ? tq * lq : 0.0); sL += wv::allsum(on ? lq : 0.0); sL2 += wv::allsum(on ? lq * lq : 0.0);
        }
        if (lane == 0) {
            double alpha = 1.0, rho_a = 1.0, rho_c = 1.0, ave = 1.0, m = 1.0, g = 1.0;
            if (k > 1) {
                const double np2 = 0.5 * k * (k - 1);
                alpha = fmax(0.0, (double)k / (k - 1) * (2.0 * sR) / (k + 2.0 * sR));
                if (a.mode[l] != plspm::MODE_B) {
                    const double f = 1.0 / sT, vv = s2 * f, v4 = s4 * f * f;      // v normalised so that v'Rv = 1
                    rho_a = vv * vv * ((sT - s2) * f) / (vv * vv - v4);
                }
                rho_c = sL * sL / (sL * sL + (k - sL2));
                ave = sL2 / k;
                m = sA / np2; g = exp(sG / np2);
            }
            out[l] = alpha; out[L + l] = rho_a; out[2 * L + l] = rho_c; out[3 * L + l] = ave;
            bm[l] = m; bg[l] = g; bt[l] = sT; bs[l] = (sU < 0.0) ? -1.0 : 1.0;
            if (a.side) { double* sd = a.side + b * 3L * L; sd[l] = (sU < 0.0) ? -1.0 : 1.0; sd[L + l] = sT; sd[2 * L + l] = s2; }
        }
    }
    wave_sync();
    ASSESS_MARK(2);

    // ---- pass 2: block i against every block behind it
    long pbase = 0;
    for (int i = 0; i + 1 < L; ++i) {
        const int b0 = a.boff[i], b1 = a.boff[i + 1];
        for (int j = i + 1 + lane; j < L; j += 64) { pa[j] = 0.0; pg[j] = 0.0; pt[j] = 0.0; }
        wave_sync();
        for (int c0 = b1; c0 < P; c0 += 64) {
            const bool on = c0 + lane < P;
            const int q = on ? c0 + lane : P - 1;
            const double muq = mu[q], isq = isd[q];
            double aq = 0.0, tq = 0.0, prod = 1.0;
            int ex = 0;
            for (int p0 = b0; p0 < b1; p0 += ASSESS_ROWS) {
                double mm[ASSESS_ROWS];
#pragma unroll
                for (int u = 0; u < ASSESS_ROWS; ++u) mm[u] = assess_moment<DENSE>(M, ld, min(p0 + u, b1 - 1), q);
#pragma unroll
                for (int u = 0; u < ASSESS_ROWS; ++u) {
                    const int p = p0 + u;
                    if (p < b1) {                                              // (uniform)
                        const double r = fma(-mu[p], muq, mm[u] * inv_n) * (isd[p] * isq);
                        const double ar = fabs(r);
                        tq = fma(v[p], r, tq); aq += ar; prod *= ar;
                        if ((u & 3) == 3) { int e; prod = frexp(prod, &e); ex += e; }
                    }
                }
            }
            const double gq = assess_log_of(prod, ex);
            win[lane] = on ? aq : 0.0; win[64 + lane] = on ? gq : 0.0; win[128 + lane] = on ? tq * v[q] : 0.0;
            wave_sync();
            const int cl = min(c0 + 63, P - 1), jf = a.lvof[c0], jl = a.lvof[cl];      // the blocks this window touches: at most 64
            const int j = jf + lane;
            if (j <= jl) {
                const int s0 = max(a.boff[j], c0) - c0, s1 = min(a.boff[j + 1], cl + 1) - c0;
                double xa = 0.0, xg = 0.0, xt = 0.0;
                for (int s = s0; s < s1; ++s) { xa += win[s]; xg += win[64 + s]; xt += win[128 + s]; }
                pa[j] += xa; pg[j] += xg; pt[j] += xt;
            }
            wave_sync();
        }
        const double ki = b1 - b0, mi = bm[i], gi = bg[i], ti = bt[i], si = bs[i];
        for (int j = i + 1 + lane; j < L; j += 64) {
            const double cnt = ki * (a.boff[j + 1] - a.boff[j]);
            const long e = 4L * L + pbase + (j - i - 1);
            out[e] = (pa[j] / cnt) / sqrt(mi * bm[j]);
            out[e + npairs] = exp(pg[j] / cnt) / sqrt(gi * bg[j]);
            out[e + 2L * npairs] = si * bs[j] * pt[j] / sqrt(ti * bt[j]);
        }
        wave_sync();
        pbase += L - 1 - i;
    }
    ASSESS_MARK(3);
}
