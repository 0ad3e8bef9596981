// kernels_cv.h -- Device kernels of the k-fold cross-validation (plspm_cv.hip): the folds of every repetition, the training sets as 0/1 count
// rows in the int8 Gram's fragment layout, the training moments of every problem, and the out-of-sample prediction errors.
// Device code of ONE translation unit (plspm_cv.hip); not a stand-alone header.
//
// Folds of repetition r (include/plspm_hip.h plspm_cv_device): row i carries the key cv_quad(seed, r, i >> 2).v[i & 3] (philox.h); the rows
// ordered by (key, row), the one at position j belongs to fold (j * k) / N.  Folds 0 .. f - 1 together hold the c_f = ceil(f N / k) smallest
// pairs, so k - 1 nested thresholds over the one key stream say it all:
//   cv_threshold_kernel    one workgroup per (repetition, f = 1 .. k - 1): radix select (11 + 11 + 10 bits) of the c_f-th smallest key and the row cut among
//                          its ties -- perm_threshold_kernel's select (kernels_permute.h) on this stream, kept in step with it; constants and scan: rank_select.h;
//   cv_assign_kernel       fold(i) = #{f : (key_i, i) is not among the c_f smallest} -- a binary search over the nested thresholds;
//   cv_order_kernel        per (repetition, fold): its rows in ascending order into the repetition's index, and the fold's offset;
//   cv_counts_kernel       problem q = r k + f: count 1 on the rows with fold != f, as 0/1 count rows (count_rows.h).
// Behind the solver:
//   cv_fold_moments_kernel     per problem the cross-products [x', 1][x', 1]' over its HELD-OUT rows (x' = the resident mean-shifted row);
//   cv_train_moments_kernel    training = (sum of the repetition's folds) - fold, in place;
//   cv_compose_kernel          the affine map of a problem's fit: x_hat = C [1; x_raw] for the target indicators;
//   cv_apply_kernel            e = x - C [1; x] on the held-out rows and its sums per (problem, target).
#pragma once
#include "rank_select.h"
#include "count_rows.h"

#define CV_NT 256                 // threads per workgroup of the kernels here that are not rank_select.h's or count_rows.h's (cv_compose_kernel: one wave)
// (cv_threshold_kernel and cv_order_kernel call rank_select.h's block_scan, which is written for RANK_NT threads: they take RANK_NT, whatever CV_NT becomes)

// rows of folds 0 .. f - 1 of a repetition of N rows in k folds
__host__ __device__ __forceinline__ int cv_fold_start(int f, int N, int k) { return (int)(((long long)f * N + k - 1) / k); }

// thr[r * (k - 1) + f - 1] = (thr_key, row_cut) of boundary f = blockIdx.y + 1 of repetition rep0 + r (r = blockIdx.x): row i is in a fold below f iff
// key < thr_key || (key == thr_key && i < row_cut).  Dynamic LDS: N keys when `cache` (N <= RANK_CACHE_ROWS), else none.
__global__ void __launch_bounds__(RANK_NT) cv_threshold_kernel(int N, int k, uint64_t seed, int64_t rep0, int cache, uint2* __restrict__ thr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned* keys = reinterpret_cast<unsigned*>(smem_raw);
    __shared__ unsigned hist[RANK_BINS];
    __shared__ unsigned scan4[RANK_NT / 64];
    __shared__ unsigned sh_bin, sh_k, sh_cut;
    const int tid = threadIdx.x;
    const uint64_t r = (uint64_t)(rep0 + (int64_t)blockIdx.x);
    const int f = (int)blockIdx.y + 1;
    const int nq = (N + 3) >> 2;
    unsigned prefix = 0u, mask = 0u, kk = (unsigned)cv_fold_start(f, N, k);      // kk: rank (from 1) of the threshold among the keys that match `prefix` on `mask`
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
        const unsigned dmask = pass == 2 ? 0x3ffu : 0x7ffu;
        for (int i = tid; i < RANK_BINS; i += RANK_NT) hist[i] = 0u;
        __syncthreads();
        if (pass == 0 || !cache) {
            for (int q = tid; q < nq; q += RANK_NT) {
                const u32x4 u = cv_quad(seed, r, (uint32_t)q);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = 4 * q + j;
                    if (i < N) {
                        const unsigned key = u.v[j];
                        if (cache) keys[i] = key;
                        if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & dmask], 1u);
                    }
                }
            }
        } else {
            for (int i = tid; i < N; i += RANK_NT) {
                const unsigned key = keys[i];
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & dmask], 1u);
            }
        }
        __syncthreads();
        // the digit that holds rank kk: thread t owns the bins 8t .. 8t + 7
        unsigned own = 0u;
#pragma unroll
        for (int b = 0; b < 8; ++b) own += hist[8 * tid + b];
        unsigned tot;
        const unsigned before = block_scan(own, scan4, &tot);
        if (before < kk && kk <= before + own) {
            unsigned c = before;
            int b = 0;
            for (; b < 7; ++b) { const unsigned h = hist[8 * tid + b]; if (kk <= c + h) break; c += h; }
            sh_bin = (unsigned)(8 * tid + b); sh_k = kk - c;
        }
        __syncthreads();
        prefix |= sh_bin << shift; mask |= dmask << shift; kk = sh_k;
    }
    const unsigned eq = hist[prefix & 0x3ffu];              // rows whose key equals the threshold (last pass: every key matched the other 22 bits)
    unsigned cut = (unsigned)N;                               // kk == eq: all of them are below the boundary
    if (kk < eq) {
        // ties straddle the boundary (uniform over the workgroup): the kk-th row of key == thr_key in row order is the last one below it
        unsigned need = kk;
        for (int q0 = 0; q0 < nq; q0 += RANK_NT) {
            const int q = q0 + tid;
            unsigned hit = 0u, c = 0u;                       // hit: bit j = row 4q + j has the threshold key
            if (q < nq) {
                u32x4 u;
                if (cache) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) u.v[j] = (4 * q + j < N) ? keys[4 * q + j] : 0u;
                } else u = cv_quad(seed, r, (uint32_t)q);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4 * q + j < N && u.v[j] == prefix) { hit |= 1u << j; ++c; }
            }
            unsigned tot;
            const unsigned before = block_scan(c, scan4, &tot);
            if (before < need && need <= before + c) {
                unsigned seen = before;
                for (int j = 0; j < 4; ++j)
                    if ((hit >> j) & 1u) { if (++seen == need) { sh_cut = (unsigned)(4 * q + j + 1); break; } }
            }
            if (tot >= need) break;                          // (tot: the same on every thread)
            need -= tot;
        }
        __syncthreads();
        cut = sh_cut;
    }
    if (tid == 0) thr[(long)blockIdx.x * (k - 1) + (f - 1)] = make_uint2(prefix, cut);
}

// fold[r][i] of repetition rep0 + r, r = blockIdx.x: the first boundary the row is below (k - 1: none).  One thread per four rows, blockIdx.y the chunk of
// 1024 rows (the repetitions go in grid.x, which has no 65,535 limit).
__global__ void __launch_bounds__(CV_NT) cv_assign_kernel(int N, int k, uint64_t seed, int64_t rep0, const uint2* __restrict__ thr, uint8_t* __restrict__ fold) {
    __shared__ uint2 sthr[255];
    const int r = blockIdx.x;
    for (int t = threadIdx.x; t < k - 1; t += CV_NT) sthr[t] = thr[(long)r * (k - 1) + t];
    __syncthreads();
    const int q = (int)blockIdx.y * CV_NT + threadIdx.x;
    if (4 * q >= N) return;
    const u32x4 u = cv_quad(seed, (uint64_t)(rep0 + r), (uint32_t)q);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned i = (unsigned)(4 * q + j);
        if ((int)i >= N) break;
        const unsigned key = u.v[j];
        int lo = 0, hi = k - 1;                               // the memberships are nested: below boundary t => below boundary t + 1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (below(sthr[mid], key, i)) hi = mid; else lo = mid + 1;
        }
        fold[(long)r * N + i] = (uint8_t)lo;
    }
}

// Workgroup (r = blockIdx.x, f = blockIdx.y): off[r][f] = #{i : fold < f} (and off[r][k] = N), idx[r][off ..] = the rows of fold f, ascending.
__global__ void __launch_bounds__(RANK_NT) cv_order_kernel(int N, int k, const uint8_t* __restrict__ fold, int* __restrict__ idx, int* __restrict__ off) {
    __shared__ unsigned scan4[RANK_NT / 64];
    const int r = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const uint8_t* fr = fold + (long)r * N;
    unsigned lower = 0u;
    for (int i = tid; i < N; i += RANK_NT) lower += fr[i] < f ? 1u : 0u;
    unsigned base;
    (void)block_scan(lower, scan4, &base);
    if (tid == 0) { off[(long)r * (k + 1) + f] = (int)base; if (f == k - 1) off[(long)r * (k + 1) + k] = N; }
    int* out = idx + (long)r * N;
    for (int i0 = 0; i0 < N; i0 += RANK_NT) {
        const int i = i0 + tid;
        const unsigned mine = (i < N && fr[i] == f) ? 1u : 0u;
        unsigned tot;
        const unsigned before = block_scan(mine, scan4, &tot);
        if (mine) out[base + before] = i;
        base += tot;
    }
}

// Counts of the chunk's problems prob0 + p, p < nprob: 1 on the rows outside the problem's fold.
__global__ void __launch_bounds__(COUNT_NT) cv_counts_kernel(int N, int KB, int MT, int k, int64_t prob0, int nprob, const uint8_t* __restrict__ fold, uint4* __restrict__ Cd) {
    int p, c;
    if (!count_row_thread(nprob, KB, p, c)) return;
    const int64_t q = prob0 + p;
    const int64_t r = q / k;
    const unsigned f = (unsigned)(q - r * k);
    const int nv = count_row_rows(N, c);
    unsigned bits = 0u;                                       // bit t: row 16c + t is a training row
    if (nv) {
        const uint8_t* fp = fold + r * (int64_t)N + 16 * c;
        for (int t = 0; t < nv; ++t)
            if (fp[t] != f) bits |= 1u << t;
    }
    count_row_store(Cd, MT, c, p, bits);
}

// packed upper triangle of a symmetric C1 x C1 matrix, row-major: (p, q), p <= q
__host__ __device__ __forceinline__ long cv_tri(int C1, int p, int q) { return (long)p * C1 - (long)p * (p - 1) / 2 + (q - p); }

// mom[q][cv_tri(p, p')] = sum over the held-out rows of problem q = blockIdx.x of x'_p x'_p', over the C1 = P + 1 columns of the resident matrix (column P: ones --
// the column sums and the row count).  Lane = a 4 x 4 tile of the triangle (64 per sweep), wave w = the rows w, w + 4, ... of the slice; the four waves' partial sums
// meet in LDS in a fixed order.  Xa: [N][PA], PA >= C1 a multiple of 16 (whole 16-column tiles) with zeros
// beyond column P, so the 4-wide loads of the last tile stay inside the row and aligned.
__global__ void __launch_bounds__(CV_NT) cv_fold_moments_kernel(const double* __restrict__ Xa, int PA, int C1, int N, int k, const int* __restrict__ idx, const int* __restrict__ off,
                                                                double* __restrict__ mom, long MS) {
    __shared__ double red[3][16][64];
    const int q = blockIdx.x, r = q / k, f = q - r * k;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int* rows = idx + (long)r * N;
    const int j0 = off[(long)r * (k + 1) + f], j1 = off[(long)r * (k + 1) + f + 1];
    const int TP = (C1 + 3) >> 2, ntile = TP * (TP + 1) / 2;
    double* out = mom + (long)q * MS;
    for (int t0 = 0; t0 < ntile; t0 += 64) {
        const int t = t0 + lane;
        int bi = 0, bj = 0;
        if (t < ntile) { int rem = t; while (rem >= TP - bi) { rem -= TP - bi; ++bi; } bj = bi + rem; }
        double acc[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0;
        if (t < ntile) {
            for (int j = j0 + w; j < j1; j += 4) {
                const double* x = Xa + (long)rows[j] * PA;
                const d4 a = *reinterpret_cast<const d4*>(x + 4 * bi);
                const d4 b = *reinterpret_cast<const d4*>(x + 4 * bj);
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) acc[4 * ii + jj] = fma(a[ii], b[jj], acc[4 * ii + jj]);
            }
        }
        if (w > 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) red[w - 1][e][lane] = acc[e];
        }
        __syncthreads();
        if (w == 0 && t < ntile) {
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int e = 4 * ii + jj, p = 4 * bi + ii, pp = 4 * bj + jj;
                    if (p <= pp && pp < C1) out[cv_tri(C1, p, pp)] = ((acc[e] + red[0][e][lane]) + red[1][e][lane]) + red[2][e][lane];
                }
        }
        __syncthreads();
    }
}

// mom[r k + f] <- (sum over f' of mom[r k + f']) - mom[r k + f]: the training moments of every problem of repetition r = blockIdx.x
__global__ void __launch_bounds__(CV_NT) cv_train_moments_kernel(int k, double* __restrict__ mom, long MS) {
    double* base = mom + (long)blockIdx.x * k * MS;
    for (long e = threadIdx.x; e < MS; e += CV_NT) {
        double tot = 0.0;
        for (int f = 0; f < k; ++f) tot += base[f * MS + e];
        for (int f = 0; f < k; ++f) base[f * MS + e] = tot - base[f * MS + e];
    }
}

struct CvModel {
    int P, L, T, n_eff, scaled, technique;      // technique 0: direct antecedents, 1: earliest antecedents
    const int* lvof;         // [P] LV of every device column
    const int* boff;         // [L + 1]
    const int* pred_off;     // [L + 1] CSR of the predecessors
    const int* pred_idx;     // [n_edges]
    const int* edge_eff;     // [n_edges] the effect pair (record section `direct`) of every edge
    const int* tcol;         // [T] device column of every target
    const double* shift;     // [P]
};

// coef[q] = C_q [T][P + 1] with x_hat_t = C[t][0] + sum_p C[t][1 + p] x_raw,p of problem q = blockIdx.x (one wave), from its record [weights | r2 | total | direct |
// loadings] and its training moments; NaN when its status is not OK.  Dynamic LDS: (3 P + L + L L) doubles.
//   score of LV l for a row x:  y_l = s_l cs sum_{p in l} w_p (x_p - mean_p)      (cs = 1 / g of the training rows when `scaled`; s_l = the sign the fit gave the scores:
//                               sum_p w_p loading_p sd_p = s_l var(y_l) -- the record's weights are not sign-corrected, its loadings and paths are)
//   predicted score of LV j:    sum_i beta_ji y_i over j's predecessors (technique 1: the predicted score of a predecessor that has predecessors itself)
//   indicator p of LV j:        mean_p + loading_p sd0_p * predicted score       (sd0: population sd of the training rows; the scores' is 1)
__global__ void __launch_bounds__(64) cv_compose_kernel(CvModel md, const double* __restrict__ rec, int RS, const int* __restrict__ status, const double* __restrict__ mom, long MS,
                                                        double* __restrict__ coef) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int P = md.P, L = md.L, T = md.T, C1 = P + 1, lane = threadIdx.x;
    double* mean = reinterpret_cast<double*>(smem_raw);      // of the shifted column
    double* sd0 = mean + P;
    double* g = sd0 + P;
    double* sgn = g + P;
    double* A = sgn + L;
    const long q = blockIdx.x;
    double* out = coef + q * (long)T * C1;
    if (status[q] != 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int e = lane; e < T * C1; e += 64) out[e] = nan;
        return;
    }
    const double* M = mom + q * MS;
    const double* row = rec + q * (long)RS;
    const double* wgt = row;
    const double* direct = row + P + L + md.n_eff;
    const double* load = direct + md.n_eff;
    const double n = M[cv_tri(C1, P, P)], inv_n = 1.0 / n;
    double tot = 0.0;
    for (int p = lane; p < P; p += 64) {
        const double mu = M[cv_tri(C1, p, P)], d = M[cv_tri(C1, p, p)];
        const double var = d - (mu * mu) * inv_n;
        mean[p] = mu * inv_n;
        sd0[p] = sqrt((var > 0.0 ? var : 0.0) * inv_n);
        tot += mu + n * md.shift[p];
    }
    double cs = 1.0;
    if (md.scaled) {
        // g = std1(all n P raw training values) * sqrt((n - 1) / n), around the grand mean (solver_core.h moments_to_cov)
        tot = wv::allsum(tot);
        const double np_ = n * (double)P, grand = tot / np_;
        double ss = 0.0;
        for (int p = lane; p < P; p += 64) {
            const double d = md.shift[p] - grand;
            ss += M[cv_tri(C1, p, p)] + 2.0 * d * M[cv_tri(C1, p, P)] + n * d * d;
        }
        ss = wv::allsum(ss);
        cs = 1.0 / sqrt(ss / (np_ - 1.0) * ((n - 1.0) / n));
    }
    __syncthreads();
    for (int l = lane; l < L; l += 64) {
        double s = 0.0;
        for (int p = md.boff[l]; p < md.boff[l + 1]; ++p) s += wgt[p] * load[p] * sd0[p];
        sgn[l] = s < 0.0 ? -1.0 : 1.0;
    }
    for (int e = lane; e < L * L; e += 64) A[e] = 0.0;
    __syncthreads();
    for (int p = lane; p < P; p += 64) g[p] = sgn[md.lvof[p]] * cs * wgt[p];
    // A[j][l]: the predicted score of LV j as a combination of the rows' own scores (LVs in path order: predecessors come first)
    for (int j = 0; j < L; ++j) {
        for (int e = md.pred_off[j]; e < md.pred_off[j + 1]; ++e) {
            const int i = md.pred_idx[e];
            const double beta = direct[md.edge_eff[e]];
            const bool chain = md.technique == 1 && md.pred_off[i + 1] > md.pred_off[i];
            for (int l = lane; l < L; l += 64) A[j * L + l] += beta * (chain ? A[i * L + l] : (l == i ? 1.0 : 0.0));
        }
        __syncthreads();
    }
    for (int t = 0; t < T; ++t) {
        const int p = md.tcol[t], j = md.lvof[p];
        const double slope = load[p] * sd0[p];
        double part = 0.0;
        for (int pp = lane; pp < P; pp += 64) {
            const double c = slope * A[j * L + md.lvof[pp]] * g[pp];
            out[t * C1 + 1 + pp] = c;
            part += c * (mean[pp] + md.shift[pp]);
        }
        part = wv::allsum(part);
        if (lane == 0) out[t * C1] = (mean[p] + md.shift[p]) - part;
    }
}

// sum over the groups of `nrg` consecutive lanes (4, 8 or 16): the first steps of wv::allreduce's butterfly
__device__ __forceinline__ double cv_group_sum(double v, int nrg) {
    v += wv::dpp<wv::QP_XOR1>(v);
    v += wv::dpp<wv::QP_XOR2>(v);
    if (nrg >= 8) v += wv::dpp<wv::ROW_HALF_MIRROR>(v);
    if (nrg >= 16) v += wv::dpp<wv::ROW_MIRROR>(v);
    return v;
}

// LDS of cv_apply_kernel for T targets of P columns with row groups of nrg x 4 rows: the transposed matrix [P + 1][TS], the row tile [P][4 nrg + 2],
// the targets' training means [T] (doubles), their columns [T] and the tile's rows [4 nrg] (ints)
__host__ __device__ __forceinline__ size_t cv_apply_lds(int P, int T, int nrg) {
    const int TS = (T + 3) & ~3, XS = 4 * nrg + 2;
    return ((size_t)(P + 1) * TS + (size_t)P * XS + (size_t)TS) * sizeof(double) + ((size_t)TS + 4 * nrg) * sizeof(int);
}

// Errors of problem q = blockIdx.x on its held-out rows: e = x_t - C_q[t] . [1; x_raw] in fp64 and, per target t, sse = sum e^2, sae = sum |e|,
// sst = sum (x_t - training mean_t)^2 -- one plain store each -- and rows[q] = the rows it covered.  A matrix with a NaN covers nothing (all sums and rows[q] zero).
// Thread (row group rg = tid % nrg: four rows of the tile, target group tid / nrg: four targets) keeps a 4 x 4 block of C x in registers; the matrix is staged
// once per problem (transposed, the upload's shift folded into its intercepts), the rows tile by tile through the fold-order index.
// pred_sum [N][T] / pred_cnt [N] (may be null): the predictions of every covered row are added up, the rows counted -- atomics, since the problems
// of different repetitions cover the same rows side by side.
__global__ void __launch_bounds__(CV_NT) cv_apply_kernel(const double* __restrict__ Xa, int PA, int P, int T, int N, int k, int nrg, const int* __restrict__ idx, const int* __restrict__ off,
                                                         const int* __restrict__ tcol, const double* __restrict__ shift, const double* __restrict__ coef, const double* __restrict__ mom, long MS,
                                                         double* __restrict__ sse, double* __restrict__ sae, double* __restrict__ sst, long long* __restrict__ nrows,
                                                         double* __restrict__ pred_sum, int* __restrict__ pred_cnt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int C1 = P + 1, TS = (T + 3) & ~3, RB = 4 * nrg, XS = RB + 2, tid = threadIdx.x;
    double* Ct = reinterpret_cast<double*>(smem_raw);         // [C1][TS]: row 0 the intercepts, row 1 + p the coefficients of column p
    double* Xs = Ct + (long)C1 * TS;                          // [P][XS]
    double* tmean = Xs + (long)P * XS;                        // [TS] training mean of the (shifted) target column
    int* stcol = reinterpret_cast<int*>(tmean + TS);          // [TS]
    int* srow = stcol + TS;                                   // [RB]
    const long q = blockIdx.x;
    const int r = (int)(q / k), f = (int)(q - (long)r * k);
    const double* Cq = coef + q * (long)T * C1;
    const double* M = mom + q * MS;
    for (int e = tid; e < C1 * TS; e += CV_NT) Ct[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < T * C1; e += CV_NT) { const int t = e / C1, c = e - t * C1; Ct[c * TS + t] = Cq[e]; }
    const double inv_n = 1.0 / M[cv_tri(C1, P, P)];
    for (int t = tid; t < TS; t += CV_NT) {
        const int col = t < T ? tcol[t] : 0;
        stcol[t] = col;
        tmean[t] = M[cv_tri(C1, col, P)] * inv_n;
    }
    __syncthreads();
    // x_raw = x' + shift: intercept' = C[t][0] + sum_p C[t][1 + p] shift_p - shift_t, so that e = x'_t - intercept' - sum_p C[t][1 + p] x'_p
    int bad = 0;
    for (int t = tid; t < T; t += CV_NT) {
        double c0 = Ct[t];
        for (int p = 0; p < P; ++p) c0 = fma(Ct[(1 + p) * TS + t], shift[p], c0);
        c0 -= shift[stcol[t]];
        bad |= (c0 != c0) ? 1 : 0;
        Ct[t] = c0;
    }
    bad = __syncthreads_or(bad);
    const int rg = tid % nrg, tg = tid / nrg;
    const bool active = 4 * tg < T;
    const int j0 = off[(long)r * (k + 1) + f], j1 = off[(long)r * (k + 1) + f + 1];
    const int* rows = idx + (long)r * N;
    double s2[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0}, st[4] = {0.0, 0.0, 0.0, 0.0};
    if (!bad) {
        for (int jb = j0; jb < j1; jb += RB) {
            for (int rr = tid; rr < RB; rr += CV_NT) {
                const int row = jb + rr < j1 ? rows[jb + rr] : -1;
                srow[rr] = row;
                if (pred_cnt && row >= 0) atomicAdd(&pred_cnt[row], 1);
            }
            __syncthreads();
            for (int e = tid; e < RB * P; e += CV_NT) {
                const int rr = e / P, p = e - rr * P;
                const int row = srow[rr];
                Xs[p * XS + rr] = row >= 0 ? Xa[(long)row * PA + p] : 0.0;
            }
            __syncthreads();
            if (active) {
                double acc[4][4];
#pragma unroll
                for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) acc[ii][jj] = 0.0;
                const double* xp = Xs + 4 * rg;
                const double* cp = Ct + TS + 4 * tg;
                for (int p = 0; p < P; ++p) {
                    const double2 x01 = *reinterpret_cast<const double2*>(xp + p * XS), x23 = *reinterpret_cast<const double2*>(xp + p * XS + 2);
                    const double2 c01 = *reinterpret_cast<const double2*>(cp + p * TS), c23 = *reinterpret_cast<const double2*>(cp + p * TS + 2);
                    const double xv[4] = {x01.x, x01.y, x23.x, x23.y}, cv[4] = {c01.x, c01.y, c23.x, c23.y};
#pragma unroll
                    for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) acc[ii][jj] = fma(xv[ii], cv[jj], acc[ii][jj]);
                }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int t = 4 * tg + jj;
                    if (t < T) {
                        const int col = stcol[t];
                        const double c0 = Ct[t], tm = tmean[t];
#pragma unroll
                        for (int ii = 0; ii < 4; ++ii) {
                            const int row = srow[4 * rg + ii];
                            if (row >= 0) {
                                const double x = Xs[col * XS + 4 * rg + ii];
                                const double pred = c0 + acc[ii][jj];
                                const double e = x - pred, d = x - tm;
                                s2[jj] = fma(e, e, s2[jj]); s1[jj] += fabs(e); st[jj] = fma(d, d, st[jj]);
                                if (pred_sum) atomicAdd(&pred_sum[(long)row * T + t], pred + shift[col]);
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const double a = cv_group_sum(s2[jj], nrg), b = cv_group_sum(s1[jj], nrg), c = cv_group_sum(st[jj], nrg);
        const int t = 4 * tg + jj;
        if (rg == 0 && t < T) { sse[q * T + t] = a; sae[q * T + t] = b; sst[q * T + t] = c; }
    }
    if (tid == 0) nrows[q] = bad ? 0 : (long long)(j1 - j0);
}
