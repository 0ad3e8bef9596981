// kernels_fimix.h -- FIMIX-PLS on the device (plspm_fimix.hip).
//   fimix_em_kernel          one workgroup per problem, persistent through its whole EM loop: fimix_core.h fimix_problem on the workgroup's executor.  The
//                            parameters, the segments' moments and the regression slots live in LDS; Y streams from L2 / HBM once per sweep; workgroups never
//                            talk to each other.  fp64 throughout.
//   fimix_posterior_kernel   a grid over the rows for one stored problem: its parameters from the record into LDS, fimix_core.h fimix_row per row, P [N x K]
//                            written through an LDS tile so that a workgroup's rows leave as one contiguous block.
#pragma once
#include "fimix_route.h"
#include "wave_ops.h"

namespace plspm {

// The workgroup as fimix_core.h's executor.  A sum: wv::allsum inside a wave (one fixed tree), lane 0's value to red[q][wave], the waves added in ascending order.
struct FimixGroupExec {
    int waves;
    __device__ __forceinline__ int tid() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int nthreads() const { return (int)blockDim.x; }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ void put(double* red, int q, double v) {
        v = wv::allsum(v);
        if ((threadIdx.x & 63) == 0) red[q * waves + (int)(threadIdx.x >> 6)] = v;
    }
    __device__ __forceinline__ double get(const double* red, int q) const {
        double s = red[q * waves];
        for (int wi = 1; wi < waves; ++wi) s += red[q * waves + wi];
        return s;
    }
};

__global__ __launch_bounds__(kFimixThreads) void fimix_em_kernel(FimixDesc d, const double* __restrict__ Y, long N, const int* __restrict__ k_of, int Kmax, const unsigned char* __restrict__ init,
                                                      uint64_t seed, int64_t start_offset, int max_iter, double tol, int nslots, double* __restrict__ rows, int* __restrict__ status,
                                                      int* __restrict__ iters) {
    extern __shared__ double fimix_lds[];
    const long p = blockIdx.x;
    FimixWs w;
    fimix_carve(w, fimix_lds, d.L, d.n_dir, d.n_endo, Kmax, kFimixThreads / 64, kFimixAcc, nslots);
    FimixGroupExec ex{kFimixThreads / 64};
    const int W = fimix_record_width(Kmax, d.n_dir, d.n_endo);
    fimix_problem<kFimixAcc>(ex, d, w, Y, N, k_of[p], Kmax, init ? init + p * N : nullptr, seed, (uint64_t)(start_offset + p), max_iter, tol, rows + p * (W + 2), status + p, iters + p);
}

constexpr int FIMIX_POST_NT = 256;
template <int KP>
__device__ __forceinline__ void fimix_posterior_rows(const FimixDesc& d, const FimixWs& w, const double* Y, long N, int K, double* tile) {
    const long i = (long)blockIdx.x * FIMIX_POST_NT + threadIdx.x;
    if (i >= N) return;
    double p[KP], lse;
    fimix_row<KP>(d, w, K, Y + i * d.L, p, lse);
#pragma unroll
    for (int k = 0; k < KP; ++k) if (k < K) tile[threadIdx.x * K + k] = p[k];
}
// rec: the problem's record (pitch 2 + Kmax (1 + n_dir + n_endo) + 2); LDS: fimix_param_doubles(L, n_dir, n_endo, 0) + 256 K doubles
__global__ __launch_bounds__(FIMIX_POST_NT) void fimix_posterior_kernel(FimixDesc d, const double* __restrict__ Y, long N, int K, int Kmax, const double* __restrict__ rec,
                                                                        double* __restrict__ out) {
    extern __shared__ double fimix_lds[];
    FimixWs w;
    fimix_carve(w, fimix_lds, d.L, d.n_dir, d.n_endo, 0, 0, 0, 0);
    double* tile = w.red;
    const int tid = (int)threadIdx.x;
    const double* beta = rec + 2 + Kmax;
    const double* psi = beta + Kmax * d.n_dir;
    for (int c = tid; c < K * d.n_dir; c += FIMIX_POST_NT) { const int k = c / d.n_dir, e = c - k * d.n_dir; w.beta[e * kFimixMaxK + k] = beta[k * d.n_dir + d.dir_of[e]]; }
    for (int c = tid; c < K * d.n_endo; c += FIMIX_POST_NT) {
        const int k = c / d.n_endo, je = c - k * d.n_endo;
        const double v = psi[k * d.n_endo + je];
        w.psi[je * kFimixMaxK + k] = v; w.ipsi[je * kFimixMaxK + k] = 1.0 / (2.0 * v);
    }
    if (tid < K) w.nk[tid] = rec[2 + tid] * (double)N;
    __syncthreads();
    if (tid < K) {          // c_k as fimix_core.h fimix_const forms it, from the record's rho itself
        double s = 0.0;
        for (int je = 0; je < d.n_endo; ++je) s += log(6.283185307179586476925286766559 * w.psi[je * kFimixMaxK + tid]);
        w.cst[tid] = log(rec[2 + tid]) - 0.5 * s;
    }
    __syncthreads();
    switch (fimix_kpad(K)) {
        case 1: fimix_posterior_rows<1>(d, w, Y, N, K, tile); break;
        case 2: fimix_posterior_rows<2>(d, w, Y, N, K, tile); break;
        case 4: fimix_posterior_rows<4>(d, w, Y, N, K, tile); break;
        case 8: fimix_posterior_rows<8>(d, w, Y, N, K, tile); break;
        default: fimix_posterior_rows<16>(d, w, Y, N, K, tile); break;
    }
    __syncthreads();
    const long r0 = (long)blockIdx.x * FIMIX_POST_NT;
    const long nr = N - r0 < FIMIX_POST_NT ? N - r0 : FIMIX_POST_NT;
    for (long c = tid; c < nr * K; c += FIMIX_POST_NT) out[r0 * K + c] = tile[c];
}

}  // namespace plspm
