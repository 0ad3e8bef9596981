// kernels_modelfit.h -- model fit of every bootstrap replicate (the definitions: modelfit_core.h): the replicate's moment matrix, which only
// exists between the Gram and the next pass, and the PLSc record kernels_plsc.h just wrote for it (loadings, construct correlations, direct effects) -> the
// model-fit record
//     srmr_sat | d_uls_sat | srmr_est | d_uls_est | status | iterations.
// One wave per replicate, four waves per workgroup; the waves share nothing and meet at no workgroup barrier (a wave without a replicate, or with a failed
// one, leaves at once).  fp64 throughout; no atomics; every sum in one fixed order.
//   per-MV step:    lane p serves MV p of a window of 64 -- mu_p and 1 / s_p from the Gram's diagonal, row P (column sums) and the entry (P, P) = n, with
//                   assess_kernel's rule for a column that is constant in the resample (a ballot finds one); lambda*_p from the PLSc record; into the LDS slice
//   per-LV-pair:    modelfit_core.h modelfit_phi on the wave executor: rc unpacked, Phi^ by the recursion, one row of an endogenous LV across the lanes
//   residual sweep: rows p ascending, sixteen rows' loads in flight together; lane q serves column q of a window of 64 behind the rows (dense layout: row p is
//                   contiguous along the lanes); every lane keeps the two running sums over all its entries, one butterfly sum of each at the end
#pragma once
#include "kernels_moments.h"
#include "modelfit_core.h"

constexpr int MODELFIT_WAVES = 4;
constexpr int MODELFIT_ROWS = 16;                  // rows whose loads are in flight together (kernels_assess.h ASSESS_ROWS)

struct ModelfitArgs {
    MomentLayout mom;
    int R;                                         // bootstrap record width (status at R)
    plspm::ModelDesc md;
    const unsigned char* factor;                   // [L]
    const double* rows; long row_stride;
    const double* plsc;                            // [nb x (R + npairs + 2)]
    double* out; long nb;                          // record b at out + b * 6
    long long* marks;                              // phase clocks of problem 0 (`make marks`; null in the release library)
};

template <bool DENSE>
__global__ void __launch_bounds__(64 * MODELFIT_WAVES) modelfit_kernel(const ModelfitArgs a) {
    extern __shared__ double modelfit_lds[];
    constexpr int F = plspm::MODELFIT_WIDTH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * MODELFIT_WAVES + wave;
    if (b >= a.nb) return;
    const int P = a.md.P, L = a.md.L, R = a.R, ld = a.mom.ld;
    const int W = R + L * (L - 1) / 2;
    const double* __restrict__ rec = a.rows + b * a.row_stride;
    const double* __restrict__ pc = a.plsc + b * (long)(W + 2);
    double* __restrict__ out = a.out + b * (long)(F + 2);
    const double st = rec[R], pst = pc[W];
    if (!(st == 0.0) || pst == (double)plspm::ST_INADMISSIBLE) {      // a failed replicate keeps its status, an inadmissible one the PLSc record's: NaN everywhere
        wave_void_record(out, F, (st == 0.0) ? pst : st, rec[R + 1], lane);
        return;
    }
    plspm::ModelfitWs w;
    plspm::modelfit_carve(w, modelfit_lds + (long)wave * plspm::modelfit_ws_doubles(P, L), P, L);
    PlscWaveExec ex{lane, (b == 0) ? a.marks : nullptr};
    const double* __restrict__ M = a.mom.gram + b * a.mom.gstride;
    ex.mark(0);
    const double inv_n = 1.0 / assess_moment<DENSE>(M, ld, P, P);
    bool constant = false;
    for (int p = lane; p < P; p += 64) {
        const MvStats mv = mv_stats<DENSE>(M, ld, p, P, inv_n);
        constant = constant || !mv.varies;
        w.isd[p] = 1.0 / mv.sd; w.mu[p] = mv.mean; w.lam[p] = pc[R - P + p];
    }
    constant = __ballot(constant) != 0ull;
    ex.sync();
    ex.mark(1);
    plspm::modelfit_phi(ex, a.md, w, pc + R, pc + P + L + a.md.n_eff);
    ex.mark(2);

    double sat = 0.0, est = 0.0;
    for (int p0 = 0; p0 + 1 < P; p0 += MODELFIT_ROWS) {
        for (int c0 = (p0 + 1) & ~63; c0 < P; c0 += 64) {
            const bool on = c0 + lane < P;
            const int q = on ? c0 + lane : P - 1;
            const int lq = a.md.lvof[q];
            const double muq = w.mu[q], isq = w.isd[q], lamq = w.lam[q];
            double mm[MODELFIT_ROWS];
#pragma unroll
            for (int u = 0; u < MODELFIT_ROWS; ++u) mm[u] = assess_moment<DENSE>(M, ld, min(p0 + u, P - 1), q);
#pragma unroll
            for (int u = 0; u < MODELFIT_ROWS; ++u) {
                const int p = p0 + u;
                if (p < P && on && p < q) {
                    const double r = fma(-w.mu[p], muq, mm[u] * inv_n) * (w.isd[p] * isq);
                    plspm::modelfit_residual(w, a.factor, L, a.md.lvof[p], lq, w.lam[p], lamq, r, sat, est);
                }
            }
        }
    }
    sat = wv::allsum(sat); est = wv::allsum(est);
    ex.mark(3);
    if (lane == 0) plspm::modelfit_store(P, sat, est, constant, pst, rec[R + 1], out);
    ex.mark(4);
}
