// count_rows.h -- 0/1 count rows for the int8 Gram: what the kernels share that write a problem's rows as counts 0 / 1 instead of resample counts -- the
// two-group permutation test (kernels_permute.h), the k-fold cross-validation (kernels_cv.h) and the jackknife (kernels_jack.h).  Device code and the host's
// grid; included by plspm_permute.hip, plspm_cv.hip and plspm_jackknife.hip.
//
// Layout: exactly resample_i8_kernel's at shape 16 (kernels_gram_i8.h "fragment-major", the contract with run_gram_i8): 1 KB blocks [k-block of 64 rows][count
// tile of 16 problems][g 0..3][problem % 16][16 B], block index kb * MT + mt.  Piece c of a problem = its rows 16c .. 16c + 15, one byte each, at k-block c / 4,
// g = c % 4 -- every 65,536-row window alike.  Pieces of rows >= N are zero, as the resample kernels leave them.
// Thread (p = 8 x + tid % 8, piece c = 32 y + tid / 8) of workgroup (x, y): the eight problems of a thread group fill consecutive pieces of one fragment row.
#pragma once

#define COUNT_NT 256                // threads per workgroup of the count-row kernels

// four 0/1 bits -> four bytes
__device__ __forceinline__ unsigned spread4(unsigned n) { return (n & 1u) | ((n & 2u) << 7) | ((n & 4u) << 14) | ((n & 8u) << 21); }

// this thread's (p, c) among the chunk's `np` problems (or pairs of them) and KB k-blocks; false: it has none
__device__ __forceinline__ bool count_row_thread(int np, int KB, int& p, int& c) {
    const int tid = threadIdx.x;
    p = (int)blockIdx.x * 8 + (tid & 7);
    c = (int)blockIdx.y * (COUNT_NT / 8) + (tid >> 3);
    return p < np && c < KB * 4;
}
// the rows of piece c that exist: 16, fewer in the tail piece at N, none beyond; and their mask (bit t: row 16c + t exists)
__device__ __forceinline__ int count_row_rows(int N, int c) {
    const int left = N - 16 * c;
    return left >= 16 ? 16 : (left > 0 ? left : 0);
}
__device__ __forceinline__ unsigned count_row_valid(int N, int c) { return (1u << count_row_rows(N, c)) - 1u; }
// piece c of problem `prob` of the chunk (MT count tiles): bit t of `bits` = the count of row 16c + t
__device__ __forceinline__ void count_row_store(uint4* __restrict__ Cd, int MT, int c, int prob, unsigned bits) {
    uint4 a;
    a.x = spread4(bits & 15u); a.y = spread4((bits >> 4) & 15u); a.z = spread4((bits >> 8) & 15u); a.w = spread4(bits >> 12);
    Cd[((long)(c >> 2) * MT + (prob >> 4)) * 64 + (c & 3) * 16 + (prob & 15)] = a;
}

// the grid that gives every (p < np, piece of KB k-blocks) its thread
inline dim3 count_rows_grid(int64_t np, int KB) { return dim3((unsigned)((np + 7) / 8), (unsigned)((KB * 4 + COUNT_NT / 8 - 1) / (COUNT_NT / 8))); }
