// kernels_geodesic.h -- the geodesic discrepancy of every bootstrap replicate (the definitions and every step: geodesic_core.h): the replicate's
// moment matrix, which only exists between the Gram and the next pass, the PLSc record kernels_plsc.h wrote for it (loadings, construct correlations, direct
// effects) and the status of its model-fit record -> the geodesic record
//     d_g_sat | d_g_est | status | iterations.
// One wave per replicate; the waves of a workgroup -- as many as its LDS holds, four at most, read from blockDim -- share nothing and meet at no workgroup
// barrier (a wave without a replicate, or with a failed or inadmissible one, leaves at once).  fp64 throughout; no atomics; every sum in one fixed order.
//   per-MV step:  kernels_modelfit.h's -- mu_p, 1 / s_p and lambda*_p into the LDS slice -- and modelfit_core.h modelfit_phi for rc and Phi^
//   the rest is geodesic_core.h geodesic_record on a wave executor; r_pq comes out of the Gram wherever a triangle is filled, the lanes along a row of its
//   upper triangle (contiguous in the dense layout)
#pragma once
#include "kernels_moments.h"
#include "kernels_plsc.h"
#include "geodesic_core.h"

constexpr int GEODESIC_WAVES = 4;                  // at most; the launcher takes fewer where the LDS slices are large (plspm_derived.hip launch_geodesic)

struct GeodesicArgs {
    MomentLayout mom;
    int R;                                         // bootstrap record width (status at R)
    plspm::ModelDesc md;
    const unsigned char* factor;                   // [L]
    const double* rows; long row_stride;
    const double* plsc;                            // [nb x (R + npairs + 2)]
    const double* modelfit;                        // [nb x 6]
    double* out; long nb;                          // record b at out + b * 4
    long long* marks;                              // phase clocks of problem 0 (`make marks`; null in the release library)
};

// the wave executor with a sum: every lane adds its own indices in ascending order, then one butterfly over the lanes
struct GeodesicWaveExec : PlscWaveExec {
    template <class F> __device__ __forceinline__ double sum(int n, F f) {
        double s = 0.0;
        for (int i = lane; i < n; i += 64) s += f(i);
        s = wv::allsum(s);
        sync();
        return s;
    }
};

template <bool DENSE>
__global__ void __launch_bounds__(64 * GEODESIC_WAVES) geodesic_kernel(const GeodesicArgs a) {
    extern __shared__ double geodesic_lds[];
    constexpr int F = plspm::GEODESIC_WIDTH, MF = plspm::MODELFIT_WIDTH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * (blockDim.x >> 6) + wave;
    if (b >= a.nb) return;
    const int P = a.md.P, L = a.md.L, R = a.R, ld = a.mom.ld;
    const int W = R + L * (L - 1) / 2;
    const double* __restrict__ rec = a.rows + b * a.row_stride;
    const double* __restrict__ pc = a.plsc + b * (long)(W + 2);
    double* __restrict__ out = a.out + b * (long)(F + 2);
    const double st = rec[R], mst = a.modelfit[b * (long)(MF + 2) + MF];
    if (!(st == 0.0) || mst == (double)plspm::ST_INADMISSIBLE) {      // a failed replicate keeps its status, an inadmissible one the model-fit record's: NaN in both
        wave_void_record(out, F, (st == 0.0) ? mst : st, rec[R + 1], lane);
        return;
    }
    plspm::GeodesicWs w;
    plspm::geodesic_carve(w, geodesic_lds + (long)wave * plspm::geodesic_ws_doubles(P, L), P, L);
    GeodesicWaveExec ex{{lane, (b == 0) ? a.marks : nullptr}};
    const double* __restrict__ M = a.mom.gram + b * a.mom.gstride;
    ex.mark(0);
    const double inv_n = 1.0 / assess_moment<DENSE>(M, ld, P, P);
    for (int p = lane; p < P; p += 64) {
        const MvStats mv = mv_stats<DENSE>(M, ld, p, P, inv_n);
        w.mf.isd[p] = 1.0 / mv.sd; w.mf.mu[p] = mv.mean; w.mf.lam[p] = pc[R - P + p];
    }
    ex.sync();
    plspm::modelfit_phi(ex, a.md, w.mf, pc + R, pc + P + L + a.md.n_eff);
    ex.mark(1);
    const auto corr = [&](int p, int q) { return fma(-w.mf.mu[p], w.mf.mu[q], assess_moment<DENSE>(M, ld, p, q) * inv_n) * (w.mf.isd[p] * w.mf.isd[q]); };
    plspm::geodesic_record(ex, a.md, w, a.factor, corr, mst, rec[R + 1], out, (double*)nullptr);
}
