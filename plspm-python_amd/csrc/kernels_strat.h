// kernels_strat.h -- Device kernels of the stratified (within-group) bootstrap of the two-group test (plspm_permute.hip): resamples drawn
// inside each group as int8 counts in the int8 Gram's fragment layout, and the all-pairs counts of Henseler's PLS-MGA test on the records in HBM.
// Device code of ONE translation unit (plspm_permute.hip); not a stand-alone header.
//
// Draws of problem s (include/plspm_hip.h plspm_stratified_bootstrap_device): draw j of group g takes rows_g[to_index(strat_quad(seed, s,
// j >> 2).v[j & 3], n_g)] (philox.h); resample r is problem 2r (group a) and 2r + 1 (group b).
//   strat_counts_kernel  one workgroup per (problem, window of 65,536 rows), a 16-bit LDS histogram like resample_i8_kernel<false>
//                        (kernels_gram_i8.h): every window walks all n_g draws of its problem and counts the rows that fall into it; the
//                        group's row list is read straight from global memory (L2; measured faster) or from LDS (ROWS_LDS, copied in
//                        once per workgroup; option "strat_rows" 2)
//   strat_u_kernel       the records' u = 2 centre_g - x (NaN where the record failed) as column-major rows per group: tiles of 64 records
//                        x 32 columns through LDS, so that the pair kernel reads its column contiguously
//   strat_pair_kernel    per column j: #{(i, k) : u_a,i > u_b,k}; a workgroup holds 2,048 group-a values in registers (8 per thread) and
//                        streams all group-b values through LDS -- a NaN on either side compares false, so failed records count nothing
#pragma once
#include "philox.h"
#include "wave_ops.h"

#define STRAT_HIST_KB 1024          // k-blocks (65,536 rows) per window: 16-bit counters, 128 KB of LDS at most
#define STRAT_U_NT 256              // threads of strat_u_kernel (tiles of 64 records x 32 columns)
#define STRAT_PAIR_NT 256           // threads of strat_pair_kernel
#define STRAT_PAIR_PER 8            // group-a values per thread
#define STRAT_PAIR_TILE 2048        // group-b values per LDS tile (16 KB)

// Counts of the chunk's problems [prob0, prob0 + gridDim.x) (problem index inside the call: resample p = prob / 2, group g = prob % 2).
// rows_ab: [n_a rows of group a | n_b rows of group b], ascending.  draws: explicit [B][N] rows (entries [0, n_a) group a's, [n_a, N) group
// b's) or null.  err bit 0: a drawn row outside [0, N), bit 1: a multiplicity above 127.  Dynamic LDS: the histogram (KBw * 32 words), then
// (ROWS_LDS) max(n_a, n_b) row indices.
template <bool ROWS_LDS>
__global__ void __launch_bounds__(1024) strat_counts_kernel(int N, int KB, int MT, int n_a, uint64_t seed, int64_t rep0, int64_t prob0, const int* __restrict__ rows_ab,
                                                           const int* __restrict__ draws, uint4* __restrict__ Cd, int* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    unsigned* hist = reinterpret_cast<unsigned*>(smem_raw);          // rows 2w, 2w + 1 of the window in the halves of word w
    const int tid = threadIdx.x, nthr = blockDim.x;
    const long b = blockIdx.x;
    const int64_t prob = prob0 + b;
    const int g = (int)(prob & 1);
    const int64_t p = prob >> 1;
    const int ng = g ? N - n_a : n_a;
    const int* rows = rows_ab + (g ? n_a : 0);
    const int kb0 = (int)blockIdx.y * STRAT_HIST_KB, KBw = min(STRAT_HIST_KB, KB - kb0);
    const unsigned r0 = (unsigned)kb0 * 64u, rspan = (unsigned)KBw * 64u;
    const int nwords = KBw * 32;
    int* lrows = reinterpret_cast<int*>(hist + nwords);
    for (int i = tid; i < nwords; i += nthr) hist[i] = 0u;
    if (ROWS_LDS && !draws)
        for (int i = tid; i < ng; i += nthr) lrows[i] = rows[i];
    __syncthreads();
    auto count = [&](unsigned w) { atomicAdd(&hist[w >> 1], (w & 1u) ? 0x10000u : 1u); };
    if (draws) {
        const int* my = draws + p * (int64_t)N + (g ? n_a : 0);
        for (int i = tid; i < ng; i += nthr) {
            const int r = my[i];
            if ((unsigned)r < (unsigned)N) { const unsigned w = (unsigned)r - r0; if (w < rspan) count(w); }
            else if (blockIdx.y == 0) atomicOr(err, 1);
        }
    } else {
        const uint64_t s = 2u * (uint64_t)(rep0 + p) + (uint64_t)g;
        const int nq = (ng + 3) >> 2;
        for (int q = tid; q < nq; q += nthr) {
            const u32x4 u = strat_quad(seed, s, (uint32_t)q);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < ng) {
                    const int k = to_index(u.v[j], (uint32_t)ng);
                    const unsigned w = (unsigned)(ROWS_LDS ? lrows[k] : rows[k]) - r0;
                    if (w < rspan) count(w);
                }
        }
    }
    __syncthreads();
    // read-out: resample_i8_kernel<false>'s, layout shape 16 (block (k-block, count tile) of 1 KB, piece c % 4 * 16 + problem % 16)
    const int mt = (int)(b >> 4), rr = (int)(b & 15);
    const uint4* h4 = reinterpret_cast<const uint4*>(hist);
    bool over = false;
    for (int c = tid; c < KBw * 4; c += nthr) {
        const uint4 lo = h4[2 * c], hi = h4[2 * c + 1];
        const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        unsigned o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned a = w[2 * k], bb = w[2 * k + 1];
            over |= ((a | bb) & 0xff80ff80u) != 0u;
            o[k] = (a & 0xffu) | ((a >> 8) & 0xff00u) | ((bb & 0xffu) << 16) | ((bb << 8) & 0xff000000u);
        }
        Cd[((long)(kb0 + (c >> 2)) * MT + mt) * 64 + (c & 3) * 16 + rr] = make_uint4(o[0], o[1], o[2], o[3]);
    }
    if (over) atomicOr(err, 2);
}

// U[g][j][p] = 2 centre_g[j] - rec[2p + g][j] for records of status OK, NaN otherwise (pitch Bp per column).  Workgroup (column tile x, record
// tile y): records 64y .. 64y + 63 (32 resamples), columns 32x .. 32x + 31.  The workgroups of column tile 0 also count the OK records of each
// group into used[0] / used[1].
__global__ void __launch_bounds__(STRAT_U_NT) strat_u_kernel(const double* __restrict__ rec, long B, int RS, int R, const double* __restrict__ ctr,
                                                             double* __restrict__ U, long Bp, unsigned long long* __restrict__ used) {
    __shared__ double tile[32][65];
    __shared__ unsigned ok[64];
    const int tid = threadIdx.x;
    const int j0 = (int)blockIdx.x * 32;
    const long e0 = (long)blockIdx.y * 64;
    if (tid < 64) {
        const long e = e0 + tid;
        ok[tid] = (e < 2 * B && rec[e * RS + R] == 0.0) ? 1u : 0u;
    }
    __syncthreads();
    const int cl = tid & 31;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int el = (tid >> 5) + 8 * k;
        const long e = e0 + el;
        const int j = j0 + cl;
        double v = __builtin_nan("");
        if (e < 2 * B && j < R && ok[el]) v = 2.0 * ctr[(el & 1) * R + j] - rec[e * RS + j];
        tile[cl][el] = v;
    }
    __syncthreads();
    const int el = tid & 63;
    const long pidx = (e0 + el) >> 1;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = (tid >> 6) + 4 * k, j = j0 + c;
        if (j < R && pidx < B) U[((long)(el & 1) * R + j) * Bp + pidx] = tile[c][el];
    }
    if (blockIdx.x == 0 && tid < 64) {
        const unsigned na = wv::allsum((tid & 1) ? 0u : ok[tid]), nb = wv::allsum((tid & 1) ? ok[tid] : 0u);
        if (tid == 0) {
            if (na) atomicAdd(&used[0], (unsigned long long)na);
            if (nb) atomicAdd(&used[1], (unsigned long long)nb);
        }
    }
}

// above[j] += #{(i, k) : U[0][j][i] > U[1][j][k]} over the group-a values i of this workgroup (blockIdx.y: 2,048 of them) and all B group-b
// values.  `above` is zeroed by the caller.  Per-thread counts stay below 2^32 (B <= 2^29 comparisons per value); the sum is 64-bit.
__global__ void __launch_bounds__(STRAT_PAIR_NT) strat_pair_kernel(const double* __restrict__ U, long B, long Bp, int R, unsigned long long* __restrict__ above) {
    __shared__ __attribute__((aligned(16))) double ub[STRAT_PAIR_TILE];
    __shared__ unsigned long long part[STRAT_PAIR_NT / 64];
    const int j = blockIdx.x, tid = threadIdx.x;
    const double* Ua = U + (long)j * Bp;
    const double* Ub = U + ((long)R + j) * Bp;
    const long a0 = (long)blockIdx.y * (STRAT_PAIR_NT * STRAT_PAIR_PER);
    double ua[STRAT_PAIR_PER];
    unsigned cnt[STRAT_PAIR_PER];
#pragma unroll
    for (int k = 0; k < STRAT_PAIR_PER; ++k) {
        const long i = a0 + (long)k * STRAT_PAIR_NT + tid;
        ua[k] = i < B ? Ua[i] : __builtin_nan("");
        cnt[k] = 0u;
    }
    for (long t0 = 0; t0 < B; t0 += STRAT_PAIR_TILE) {
        const int nt = (int)min((long)STRAT_PAIR_TILE, B - t0);
        __syncthreads();
        for (int k = tid; k < STRAT_PAIR_TILE; k += STRAT_PAIR_NT) ub[k] = k < nt ? Ub[t0 + k] : __builtin_nan("");
        __syncthreads();
        const double2* u2 = reinterpret_cast<const double2*>(ub);
        for (int k = 0; k < (nt + 1) / 2; ++k) {
            const double2 v = u2[k];                                // (the same address on every lane: one broadcast read)
#pragma unroll
            for (int e = 0; e < STRAT_PAIR_PER; ++e) cnt[e] += (unsigned)(ua[e] > v.x) + (unsigned)(ua[e] > v.y);
        }
    }
    unsigned long long s = 0ull;
#pragma unroll
    for (int e = 0; e < STRAT_PAIR_PER; ++e) s += cnt[e];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0ull;
        for (int w = 0; w < STRAT_PAIR_NT / 64; ++w) t += part[w];
        if (t) atomicAdd(&above[j], t);
    }
}
