// philox.h -- Philox4x32-10 resampling streams (host + device inline functions; every translation unit may include it).
#pragma once
#include <cstdint>

// ------------------------------------------------------------------------------------------------ Philox4x32-10
struct u32x4 { uint32_t v[4]; };
__host__ __device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }
// (device, round 5: both halves of a product from ONE v_mad_u64_u32 -- hipcc emits v_mul_hi_u32 + v_mul_lo_u32 for the two expressions below, 38 multiplies
//  per four draws where 19 do; same bits.  tools/ubench/resample_rng.hip: resample kernel 52.1 -> 46.7 us at 10,000 rows, 706 -> 625 us at 100,000)
__host__ __device__ __forceinline__ void mul_hilo32(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long p;
    asm("v_mad_u64_u32 %0, vcc, %1, %2, 0" : "=v"(p) : "v"(a), "v"(b) : "vcc");
    hi = (uint32_t)(p >> 32); lo = (uint32_t)p;
#else
    const uint64_t p = (uint64_t)a * (uint64_t)b;
    hi = (uint32_t)(p >> 32); lo = (uint32_t)p;
#endif
}
__host__ __device__ __forceinline__ u32x4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0, lo0, hi1, lo1;
        mul_hilo32(0xD2511F53u, c0, hi0, lo0);
        mul_hilo32(0xCD9E8D57u, c2, hi1, lo1);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    u32x4 o; o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}
// The streams: word (i & 3) of Philox(counter = (i >> 2, STREAM, lo32(rep), hi32(rep)), key = seed) belongs to element i of repetition `rep`.  Counter word 1
// names the stream, so no two of them ever share a block:
//   0  resample_quad  bootstrap: resample index i (0 <= i < N) of replicate `rep`, mapped to [0, N) by the 32x32 -> high-word multiply (bias <= N / 2^32)
//   1  permute_quad   two-group permutation test: sort key of row i in permutation `rep`; group a = the n1 rows with the smallest (key, row) pairs
//                     (rank_select.h, kernels_permute.h, plspm_permutation_members)
//   2  strat_quad     stratified (within-group) bootstrap of the two-group test: draw j of problem `rep`; resample r makes problem 2r (group a, n_a draws from
//                     its rows) and 2r + 1 (group b) -- kernels_strat.h, plspm_stratified_draws
//   3  cv_quad        k-fold cross-validation: sort key of row i in repetition `rep`; the rows ordered by (key, row), the one at position j belongs to fold
//                     (j * k) / N -- rank_select.h, kernels_cv.h, plspm_cv_folds
//   4  fimix_quad     FIMIX-PLS: initial segment of row i in start `rep`, mapped to [0, K) by the high-word multiply, floor(u K) for u = word / 2^32 --
//                     kernels_fimix.h, plspm_fimix_starts
template <uint32_t STREAM>
__host__ __device__ __forceinline__ u32x4 stream_quad(uint64_t seed, uint64_t rep, uint32_t q) {
    return philox4x32_10(q, STREAM, (uint32_t)rep, (uint32_t)(rep >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}
constexpr uint32_t STREAM_RESAMPLE = 0u, STREAM_PERMUTE = 1u, STREAM_STRAT = 2u, STREAM_CV = 3u, STREAM_FIMIX = 4u;
__host__ __device__ __forceinline__ u32x4 resample_quad(uint64_t seed, uint64_t rep, uint32_t q) { return stream_quad<STREAM_RESAMPLE>(seed, rep, q); }
__host__ __device__ __forceinline__ u32x4 permute_quad(uint64_t seed, uint64_t perm, uint32_t q) { return stream_quad<STREAM_PERMUTE>(seed, perm, q); }
__host__ __device__ __forceinline__ u32x4 strat_quad(uint64_t seed, uint64_t s, uint32_t q) { return stream_quad<STREAM_STRAT>(seed, s, q); }
__host__ __device__ __forceinline__ u32x4 cv_quad(uint64_t seed, uint64_t rep, uint32_t q) { return stream_quad<STREAM_CV>(seed, rep, q); }
__host__ __device__ __forceinline__ u32x4 fimix_quad(uint64_t seed, uint64_t start, uint32_t q) { return stream_quad<STREAM_FIMIX>(seed, start, q); }
__host__ __device__ __forceinline__ int32_t to_index(uint32_t u, uint32_t n) { return (int32_t)mulhi32(u, n); }
__host__ __device__ __forceinline__ int fimix_start_segment(uint64_t seed, uint64_t start, uint32_t i, uint32_t K) {
    const u32x4 u = fimix_quad(seed, start, i >> 2);
    const uint32_t j = i & 3u, word = j == 0 ? u.v[0] : j == 1 ? u.v[1] : j == 2 ? u.v[2] : u.v[3];      // (no indexed register array on the device)
    return (int)mulhi32(word, K);
}
