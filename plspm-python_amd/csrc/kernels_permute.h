// kernels_permute.h -- Device kernels of the two-group permutation test (plspm_permute.hip): random splits of an exact size as 0/1 count rows
// in the int8 Gram's fragment layout, and the exceedance counts of the permutation statistic on the records left in HBM.
// Device code of ONE translation unit (plspm_permute.hip); not a stand-alone header.
//
// Split of permutation r (include/plspm_hip.h plspm_permutation_device): row i carries the key permute_quad(seed, r, i >> 2).v[i & 3]
// (philox.h); group a = the n1 rows with the smallest (key, row) pairs.  Two passes:
//   perm_threshold_kernel  one workgroup per permutation: radix select (11 + 11 + 10 bits) of the n1-th smallest key -> thr_key, and the row cut among
//                          the rows whose key equals it (a scan in row order, only when such ties straddle the cut); constants and scan: rank_select.h;
//   perm_counts_kernel     member(i) = below((thr_key, row_cut), key_i, i), local to every 16-row piece: problem 2p gets the members, problem
//                          2p + 1 the complement, as 0/1 count rows (count_rows.h).
#pragma once
#include "rank_select.h"
#include "count_rows.h"

#define PERM_NT 256                 // threads per workgroup of perm_exceed_kernel

// thr[p] = (thr_key, row_cut) of permutation perm0 + p.  1 <= n1 <= N.  Dynamic LDS: N keys when `cache` (N <= RANK_CACHE_ROWS), else none.
__global__ void __launch_bounds__(RANK_NT) perm_threshold_kernel(int N, int n1, uint64_t seed, int64_t perm0, int cache, uint2* __restrict__ thr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned* keys = reinterpret_cast<unsigned*>(smem_raw);
    __shared__ unsigned hist[RANK_BINS];
    __shared__ unsigned scan4[RANK_NT / 64];
    __shared__ unsigned sh_bin, sh_k, sh_cut;
    const int tid = threadIdx.x;
    const uint64_t r = (uint64_t)(perm0 + (int64_t)blockIdx.x);
    const int nq = (N + 3) >> 2;
    unsigned prefix = 0u, mask = 0u, k = (unsigned)n1;      // k: rank (from 1) of the threshold among the keys that match `prefix` on `mask`
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
        const unsigned dmask = pass == 2 ? 0x3ffu : 0x7ffu;
        for (int i = tid; i < RANK_BINS; i += RANK_NT) hist[i] = 0u;
        __syncthreads();
        if (pass == 0 || !cache) {
            for (int q = tid; q < nq; q += RANK_NT) {
                const u32x4 u = permute_quad(seed, r, (uint32_t)q);
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
        // the digit that holds rank k: thread t owns the bins 8t .. 8t + 7
        unsigned own = 0u;
#pragma unroll
        for (int b = 0; b < 8; ++b) own += hist[8 * tid + b];
        unsigned tot;
        const unsigned before = block_scan(own, scan4, &tot);
        if (before < k && k <= before + own) {
            unsigned c = before;
            int b = 0;
            for (; b < 7; ++b) { const unsigned h = hist[8 * tid + b]; if (k <= c + h) break; c += h; }
            sh_bin = (unsigned)(8 * tid + b); sh_k = k - c;
        }
        __syncthreads();
        prefix |= sh_bin << shift; mask |= dmask << shift; k = sh_k;
    }
    const unsigned eq = hist[prefix & 0x3ffu];              // rows whose key equals the threshold (last pass: every key matched the other 22 bits)
    unsigned cut = (unsigned)N;                               // k == eq: all of them are members
    if (k < eq) {
        // ties straddle the cut (uniform over the workgroup): the k-th row of key == thr_key in row order is the last member
        unsigned need = k;
        for (int q0 = 0; q0 < nq; q0 += RANK_NT) {
            const int q = q0 + tid;
            unsigned hit = 0u, c = 0u;                       // hit: bit j = row 4q + j has the threshold key
            if (q < nq) {
                u32x4 u;
                if (cache) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) u.v[j] = (4 * q + j < N) ? keys[4 * q + j] : 0u;
                } else u = permute_quad(seed, r, (uint32_t)q);
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
    if (tid == 0) thr[blockIdx.x] = make_uint2(prefix, cut);
}

// Counts of the chunk's problems 2p (group a) and 2p + 1 (group b) for its permutations p < nperm (ids perm0 + p); `member` (explicit
// memberships, [nperm][N] bytes 0/1) replaces the thresholds when not null.  (2p even: both problems in the same count tile, two adjacent pieces.)
__global__ void __launch_bounds__(COUNT_NT) perm_counts_kernel(int N, int KB, int MT, uint64_t seed, int64_t perm0, int nperm, const uint2* __restrict__ thr,
                                                               const uint8_t* __restrict__ member, uint4* __restrict__ Cd) {
    int p, c;
    if (!count_row_thread(nperm, KB, p, c)) return;
    const int i0 = 16 * c;
    const unsigned valid = count_row_valid(N, c);
    unsigned bits = 0u;                                       // bit t: row i0 + t is in group a
    if (valid) {
        if (member) {
            const uint8_t* mp = member + (long)p * N + i0;
            for (int t = 0; t < 16; ++t)
                if (((valid >> t) & 1u) && mp[t]) bits |= 1u << t;
        } else {
            const uint2 th = thr[p];
            const uint64_t r = (uint64_t)(perm0 + p);
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const u32x4 u = permute_quad(seed, r, (uint32_t)(4 * c + qq));
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (below(th, u.v[j], (unsigned)(i0 + 4 * qq + j))) bits |= 1u << (4 * qq + j);
            }
            bits &= valid;
        }
    }
    count_row_store(Cd, MT, c, 2 * p, bits);
    count_row_store(Cd, MT, c, 2 * p + 1, ~bits & valid);
}

// Exceedance counts of B permutations whose records (pitch RS, status in column R) sit in pairs (2p: group a, 2p + 1: group b): per column j
// (one workgroup each) #{p : both OK, |d_pj| >= |d_obs,j|} with d_pj = rec[2p][j] - rec[2p + 1][j]; a NaN on either side is "not >=".  Column 0's
// workgroup also writes the number of valid permutations.
__global__ void __launch_bounds__(PERM_NT) perm_exceed_kernel(const double* __restrict__ rec, long B, int RS, int R, const double* __restrict__ dobs,
                                                              unsigned long long* __restrict__ exceed, unsigned long long* __restrict__ used) {
    __shared__ unsigned part[2][PERM_NT / 64];
    const int j = blockIdx.x, tid = threadIdx.x;
    const double lim = fabs(dobs[j]);
    unsigned cnt = 0u, nu = 0u;
    for (long p = tid; p < B; p += PERM_NT) {
        const double* a = rec + 2 * p * (long)RS;
        const double* b = a + RS;
        if (a[R] == 0.0 && b[R] == 0.0) {
            ++nu;
            if (fabs(a[j] - b[j]) >= lim) ++cnt;
        }
    }
    cnt = wv::allsum(cnt); nu = wv::allsum(nu);
    if ((tid & 63) == 0) { part[0][tid >> 6] = cnt; part[1][tid >> 6] = nu; }
    __syncthreads();
    if (tid == 0) {
        unsigned long long sc = 0ull, su = 0ull;
        for (int w = 0; w < PERM_NT / 64; ++w) { sc += part[0][w]; su += part[1][w]; }
        exceed[j] = sc;
        if (j == 0) *used = su;
    }
}
