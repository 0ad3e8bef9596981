// kernels_micom.h -- MICOM, the measurement invariance of composite models (Henseler, Ringle and Sarstedt 2016), for every permutation of a two-group
// permutation call: compositional invariance (step 2) and the equality of the pooled composite's means and variances (step 3) per latent variable, from BOTH
// halves' moment matrices -- which only exist between the Gram and the next pass --, the weights of their two records and the pooled inputs of the call.
// One wave per permutation, four waves per workgroup; the waves share nothing and meet at no workgroup barrier (a wave without a permutation, or with a failed
// one, leaves at once).  fp64 throughout; no atomics; every sum in one fixed order.
//
// Per group g (problem 2r: a, 2r + 1: b), with n_g, the column sums and the cross products M_g of the mean-shifted columns:  mu_p = M_p1 / n,
// c_pq = M_pq / n - mu_p mu_q,  s_p = sqrt(c_pp) (zero below treated_sd's threshold, as assess_kernel),  v_p = w_p s_p.  Pooled, fixed for the call: u [P] and
// the diagonal blocks of R_0 (micom_pooled_kernel).  Per block l:
//     c = v_a' R_0 v_b / sqrt((v_a' R_0 v_a)(v_b' R_0 v_b)),   dmean = sum u_p (mu_a,p - mu_b,p),   dlogvar = log(n_a / (n_a - 1) u' C_a u) - log(n_b / (n_b - 1) u' C_b u)
// Lane q serves column q of a window of 64 columns of the block: each of the five quadratic forms is a column product per lane (rows p of the block, the row's
// factor broadcast out of LDS) followed by a butterfly sum.  The per-MV values v_a, v_b, mu_a, mu_b are staged PER BLOCK in the wave's LDS slice, so the slice
// depends on the largest block and not on P: 4 k_max doubles.  The loads of eight rows -- three matrices each -- are issued together (one memory round trip per
// batch of rows, not per row: kernels_assess.h).  Only the diagonal blocks of the three matrices are read.
#pragma once
#include "kernels_moments.h"

constexpr int MICOM_WAVES = 4;
constexpr int MICOM_ROWS = 8;                      // rows of a block whose loads (M_a, M_b, R_0) are in flight together
constexpr int MICOM_COUNT_NT = 256;

struct MicomArgs {
    MomentLayout mom;
    int L, R, kb;                                  // LVs, record width (weights at 0, status at R, iterations at R + 1), largest block
    const int* boff;
    const double* rows; long row_stride;           // record of problem j at rows + j * row_stride
    const double* u; const double* r0;             // pooled: u [P]; R_0's diagonal blocks, block l row-major [k_l x k_l] behind those before it
    double* out; long np;                          // record r at out + r * (3 L + 2)
};

// doubles of one wave's LDS slice: v_a, v_b, mu_a, mu_b of the current block
__host__ __device__ inline long micom_wave_doubles(int kb) { return 4L * kb; }

template <bool DENSE>
__global__ void __launch_bounds__(64 * MICOM_WAVES) micom_kernel(const MicomArgs a) {
    extern __shared__ double micom_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long r = (long)blockIdx.x * MICOM_WAVES + wave;
    if (r >= a.np) return;
    const int P = a.mom.P, L = a.L, ld = a.mom.ld, W = 3 * L;
    const double* __restrict__ recA = a.rows + 2 * r * a.row_stride;
    const double* __restrict__ recB = recA + a.row_stride;
    double* __restrict__ out = a.out + r * (long)(W + 2);
    const double sa = recA[a.R], sb = recB[a.R];
    const double st = (sa == 0.0) ? sb : sa;       // 0 iff both are PLSPM_OK, else the first problem's status, or else the second's
    if (!(st == 0.0)) { wave_void_record(out, W, st, fmax(recA[a.R + 1], recB[a.R + 1]), lane); return; }      // a failed half
    if (lane == 0) { out[W] = st; out[W + 1] = fmax(recA[a.R + 1], recB[a.R + 1]); }
    double* va = micom_lds + (long)wave * micom_wave_doubles(a.kb);
    double *vb = va + a.kb, *mua = vb + a.kb, *mub = mua + a.kb;
    const double* __restrict__ Ma = a.mom.gram + 2 * r * a.mom.gstride;
    const double* __restrict__ Mb = Ma + a.mom.gstride;
    const double na = assess_moment<DENSE>(Ma, ld, P, P), nb = assess_moment<DENSE>(Mb, ld, P, P);
    const double inv_na = 1.0 / na, inv_nb = 1.0 / nb;
    long roff = 0;
    for (int l = 0; l < L; ++l) {
        const int b0 = a.boff[l], b1 = a.boff[l + 1], k = b1 - b0;
        for (int p = b0 + lane; p < b1; p += 64) {
            const MvStats sa_p = mv_stats<DENSE>(Ma, ld, p, P, inv_na), sb_p = mv_stats<DENSE>(Mb, ld, p, P, inv_nb);      // (a column that is constant in its group: sd 0)
            va[p - b0] = recA[p] * sa_p.sd; vb[p - b0] = recB[p] * sb_p.sd; mua[p - b0] = sa_p.mean; mub[p - b0] = sb_p.mean;
        }
        wave_sync();
        const double* __restrict__ R0 = a.r0 + roff;
        double qaa = 0.0, qbb = 0.0, qab = 0.0, qba = 0.0, qua = 0.0, qub = 0.0, dm = 0.0;
        for (int c0 = b0; c0 < b1; c0 += 64) {
            const bool on = c0 + lane < b1;
            const int q = on ? c0 + lane : b1 - 1, j = q - b0;
            const double muaq = mua[j], mubq = mub[j], vaq = va[j], vbq = vb[j], uq = a.u[q];
            double taa = 0.0, tbb = 0.0, tua = 0.0, tub = 0.0;
            for (int p0 = b0; p0 < b1; p0 += MICOM_ROWS) {
                double xa[MICOM_ROWS], xb[MICOM_ROWS], xr[MICOM_ROWS];
#pragma unroll
                for (int t = 0; t < MICOM_ROWS; ++t) {
                    const int p = min(p0 + t, b1 - 1);
                    xa[t] = assess_moment<DENSE>(Ma, ld, p, q); xb[t] = assess_moment<DENSE>(Mb, ld, p, q); xr[t] = R0[(long)(p - b0) * k + j];
                }
#pragma unroll
                for (int t = 0; t < MICOM_ROWS; ++t) {
                    const int p = p0 + t;
                    if (p < b1) {                                              // (uniform)
                        const int i = p - b0;
                        const double up = a.u[p];
                        taa = fma(va[i], xr[t], taa); tbb = fma(vb[i], xr[t], tbb);
                        tua = fma(up, fma(-mua[i], muaq, xa[t] * inv_na), tua);
                        tub = fma(up, fma(-mub[i], mubq, xb[t] * inv_nb), tub);
                    }
                }
            }
            qaa += wv::allsum(on ? vaq * taa : 0.0); qbb += wv::allsum(on ? vbq * tbb : 0.0); qab += wv::allsum(on ? vbq * taa : 0.0); qba += wv::allsum(on ? vaq * tbb : 0.0);
            qua += wv::allsum(on ? uq * tua : 0.0); qub += wv::allsum(on ? uq * tub : 0.0); dm += wv::allsum(on ? uq * (muaq - mubq) : 0.0);
        }
        if (lane == 0) {
            // (v_a' R_0 v_b as the mean of its two orders of summation: exchanging the groups exchanges the two sums, and c is the same bit for bit)
            out[l] = 0.5 * (qab + qba) / sqrt(qaa * qbb);
            out[L + l] = dm;
            out[2 * L + l] = log(na / (na - 1.0) * qua) - log(nb / (nb - 1.0) * qub);
        }
        wave_sync();                        // (the next block's staging overwrites the slice)
        roff += (long)k * k;
    }
}

// The pooled inputs, once per upload: from the tile-packed moments M of ALL resident rows and the full-sample solver problem's record (weights at 0, status at R):
// s_0 [P];  the diagonal blocks of R_0 (r_pp = 1; both triangles from one expression, so the blocks are exactly symmetric);  v_0,p = w_0,p s_0,p normalised per block
// so that v_0' R_0,ll v_0 = 1;  u_p = v_0,p / s_0,p (NaN everywhere when that problem's status is not PLSPM_OK).  One wave.
__global__ void __launch_bounds__(64) micom_pooled_kernel(const double* __restrict__ M, int T, int P, int L, const int* __restrict__ boff, const double* __restrict__ rec, int R,
                                                          double* __restrict__ u, double* __restrict__ s0, double* __restrict__ r0) {
    const int lane = threadIdx.x;
    const double inv_n = 1.0 / M[packed_index(T, P, P)];
    const bool ok = rec[R] == 0.0;
    for (int p = lane; p < P; p += 64) s0[p] = mv_stats<false>(M, T, p, P, inv_n).sd;
    __syncthreads();
    long roff = 0;
    for (int l = 0; l < L; ++l) {
        const int b0 = boff[l], b1 = boff[l + 1], k = b1 - b0;
        double* R0 = r0 + roff;
        for (int e = lane; e < k * k; e += 64) {
            const int i = e / k, j = e - i * k, p = b0 + i, q = b0 + j;
            const double mp = M[packed_index(T, p, P)] * inv_n, mq = M[packed_index(T, q, P)] * inv_n;
            R0[e] = (p == q) ? 1.0 : fma(-mp, mq, M[packed_index(T, p, q)] * inv_n) * ((1.0 / s0[p]) * (1.0 / s0[q]));
        }
        __syncthreads();
        double vrv = 0.0;
        for (int c0 = b0; c0 < b1; c0 += 64) {
            const bool on = c0 + lane < b1;
            const int q = on ? c0 + lane : b1 - 1, j = q - b0;
            double t = 0.0;
            for (int i = 0; i < k; ++i) t = fma(rec[b0 + i] * s0[b0 + i], R0[(long)i * k + j], t);
            vrv += wv::allsum(on ? (rec[q] * s0[q]) * t : 0.0);
        }
        const double f = 1.0 / sqrt(vrv);
        for (int p = b0 + lane; p < b1; p += 64) u[p] = ok ? ((rec[p] * s0[p]) * f) / s0[p] : __builtin_nan("");
        roff += (long)k * k;
    }
}

// Counts on the B MICOM records in HBM (pitch W + 2, status in column W): per column j (one workgroup each), over the valid records (status 0),
// below_j = #{r : x_rj <= obs_j} and exceed_j = #{r : |x_rj| >= |obs_j|}; a NaN on either side is neither.  Column 0's workgroup also writes the number of valid records.
__global__ void __launch_bounds__(MICOM_COUNT_NT) micom_count_kernel(const double* __restrict__ rec, long B, int W, const double* __restrict__ obs, unsigned long long* __restrict__ below,
                                                                     unsigned long long* __restrict__ exceed, unsigned long long* __restrict__ used) {
    __shared__ unsigned part[3][MICOM_COUNT_NT / 64];
    const int j = blockIdx.x, tid = threadIdx.x;
    const double o = obs[j], lim = fabs(o);
    unsigned nb = 0u, ne = 0u, nu = 0u;
    for (long r = tid; r < B; r += MICOM_COUNT_NT) {
        const double* x = rec + r * (long)(W + 2);
        if (x[W] == 0.0) {
            ++nu;
            if (x[j] <= o) ++nb;
            if (fabs(x[j]) >= lim) ++ne;
        }
    }
    nb = wv::allsum(nb); ne = wv::allsum(ne); nu = wv::allsum(nu);
    if ((tid & 63) == 0) { part[0][tid >> 6] = nb; part[1][tid >> 6] = ne; part[2][tid >> 6] = nu; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long sb = 0ull, se = 0ull, su = 0ull;
        for (int w = 0; w < MICOM_COUNT_NT / 64; ++w) { sb += part[0][w]; se += part[1][w]; su += part[2][w]; }
        below[j] = sb; exceed[j] = se;
        if (j == 0) *used = su;
    }
}
