// rank_select.h -- What the two radix selects over a Philox key stream (philox.h) share: perm_threshold_kernel (kernels_permute.h: the n1-th smallest key of a
// permutation) and cv_threshold_kernel (kernels_cv.h: the fold boundaries of a repetition).  Device code; included by plspm_permute.hip and plspm_cv.hip.
//
// Row i carries the key <stream>_quad(seed, rep, i >> 2).v[i & 3]; the rows are ordered by (key, row).  The `rank` smallest pairs are the rows with
// below(th, key, i) for th = (thr_key, row_cut): thr_key the rank-th smallest key, row_cut the row cut among the rows whose key equals it.  Here: the constants,
// that predicate and the block scan.  The select itself (three radix passes, the key cache, the tie scan) stays written out in each of the two kernels: moved
// into a __device__ function -- inlined by force or not, templated or not -- the same text compiles to other code (the block scans lose a term, the short loops
// behind them move against the 64-byte instruction lines) and perm_threshold_kernel ran 8 % slower.  A fix to one body goes into the other.
#pragma once
#include "philox.h"
#include "wave_ops.h"

#define RANK_NT 256                 // threads per workgroup of the selection, of the block scan and of the kernels that call them
#define RANK_BINS 2048              // radix digits of 11 bits
#define RANK_CACHE_ROWS 12288       // up to this many rows the keys stay in LDS (48 KB) after the first radix pass instead of being drawn again

// row i with key `key` is among the smallest pairs that th = (thr_key, row_cut) cuts off
__device__ __forceinline__ bool below(uint2 th, unsigned key, unsigned i) { return key < th.x || (key == th.x && i < th.y); }

// exclusive prefix sum over the 256 threads of a workgroup; *total = the sum of all.  Ends behind a barrier (lds4 is free again).
__device__ __forceinline__ unsigned block_scan(unsigned v, unsigned* lds4, unsigned* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned inc = wv::inclusive_scan(v);
    if (lane == 63) lds4[w] = inc;
    __syncthreads();
    unsigned base = 0u, tot = 0u;
#pragma unroll
    for (int k = 0; k < RANK_NT / 64; ++k) { const unsigned t = lds4[k]; base += (k < w) ? t : 0u; tot += t; }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}
