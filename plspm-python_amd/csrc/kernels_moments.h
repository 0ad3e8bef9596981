// kernels_moments.h -- what the one-wave-per-problem kernels behind the solver open with (kernels_assess.h, kernels_plsc.h, kernels_modelfit.h, kernels_geodesic.h, kernels_micom.h):
// where a problem's moment matrix lies, the per-MV statistics out of it, the record of a failed problem and the wave's LDS hand-over.
#pragma once

// The moment matrices (of P MVs) of a launch's problems: problem j at gram + j * gstride.  DENSE: [(P+1) x ld] upper triangles, ld = cov_ld(P), entry (r, c >= r) at
// r * ld + c; else the tile-packed layout, ld = its tile count T (packed_index).  Row / column P holds the column sums, the entry (P, P) the row count n.
struct MomentLayout { const double* gram; long gstride; int ld, P; };

template <bool DENSE> __device__ __forceinline__ double assess_moment(const double* __restrict__ M, int ld, int p, int q) {
    if (DENSE) { const int r = min(p, q), c = max(p, q); return M[(long)r * ld + c]; }
    return M[packed_index(ld, p, q)];
}

// Mean and standard deviation of MV p out of the moment matrix M (inv_n = 1 / M_PP):  mu = M_pP / n,  s = sqrt(M_pp / n - mu^2).
// A column that is constant in this problem: its variance is rounding residue of either sign -- zero by solver_core.h treated_sd's threshold, so that what
// divides by it is inf or NaN by IEEE's rules and not a number made of noise; the solver gives such an item weight and loading 0 and status OK.
struct MvStats { double mean, sd; bool varies; };
template <bool DENSE> __device__ __forceinline__ MvStats mv_stats(const double* __restrict__ M, int ld, int p, int P, double inv_n) {
    const double m = assess_moment<DENSE>(M, ld, p, P) * inv_n, m2 = assess_moment<DENSE>(M, ld, p, p) * inv_n, var = fma(-m, m, m2);
    const bool varies = var > 1e-9 * m2;
    return {m, varies ? sqrt(var) : ((var == var) ? 0.0 : var), varies};
}

// the record [width | status | iterations] of a problem that failed: status and iterations through, NaN everywhere
__device__ __forceinline__ void wave_void_record(double* __restrict__ out, int width, double status, double iterations, int lane) {
    if (lane == 0) { out[width] = status; out[width + 1] = iterations; }
    for (int c = lane; c < width; c += 64) out[c] = __builtin_nan("");
}

// the lanes of a wave hand values to each other through its LDS slice: the wave's own LDS order, no workgroup barrier
__device__ __forceinline__ void wave_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
