// kernels_plsc.h -- consistent PLS of every bootstrap replicate (the definitions: plsc_core.h): the replicate's bootstrap record, the assessment
// record kernels_assess.h just wrote for it (rho_a, lv_cor) and that kernel's side output (per LV the fit's sign, v'Rv and v'v) -> the PLSc record
//     weights[P] | r2[L] | total[n_eff] | direct[n_eff] | loadings[P] | lv_cor_c[npairs] | status | iterations.
// One wave per replicate, four waves per workgroup; the waves share nothing and meet at no workgroup barrier (a wave without a replicate, or with a failed
// one, leaves at once).  fp64 throughout; no atomics; every sum in one fixed order.
//   per-MV step: lane p serves MV p of a window of 64 -- s_p = sqrt(c_pp) from the Gram's diagonal, row P (column sums) and the entry (P, P) = n, with
//                assess_kernel's rule for a column that is constant in the resample; v_p = w_p s_p into the wave's LDS slice
//   the rest is plsc_core.h plsc_record on a wave executor: lanes over LVs (Q, the loading factors), over the L x L entries of rc, one lane per endogenous LV
//                for its regression (<= 8 predecessors in registers, more through the LDS scratch), one lane per column for the effects, lanes over the stores
// Nothing of pass 1 of the assessment is computed again: the block sums arrive through AssessArgs::side.
#pragma once
#include "kernels_moments.h"
#include "plsc_core.h"

constexpr int PLSC_WAVES = 4;

struct PlscArgs {
    MomentLayout mom;
    int R, A;                                      // bootstrap record width (status at R), assessment record width (rho_a at L, lv_cor at 4 L + 2 npairs)
    plspm::ModelDesc md;
    const unsigned char* factor;                   // [L]
    const double* rows; long row_stride;
    const double* assess;                          // [nb x (A + 2)]
    const double* side;                            // [nb x 3 L]
    double* out; long nb;                          // record b at out + b * (R + npairs + 2)
    long long* marks;                              // phase clocks of problem 0 (`make marks`; null in the release library)
};

// the wave executor: lanes stride over the indices; the hand-over between lanes is the wave's own LDS order
struct PlscWaveExec {
    static constexpr int kcap = 8;                 // regressions on at most 8 predecessors in registers (solver_core.h spd_solve)
    int lane;
    long long* marks;
#ifdef PLSPM_DEBUG_MARKS
    __device__ __forceinline__ void mark(int id) { if (marks && lane == 0) marks[id] = (long long)__builtin_readcyclecounter(); }
#else
    __device__ __forceinline__ void mark(int) {}
#endif
    __device__ __forceinline__ void sync() { wave_sync(); }
    template <class F> __device__ __forceinline__ void par(int n, F f) { for (int i = lane; i < n; i += 64) f(i); sync(); }
    template <class F> __device__ __forceinline__ void one(F f) { if (lane == 0) f(); sync(); }
    template <class F> __device__ __forceinline__ bool any(int n, F f) {
        bool hit = false;
        for (int i = lane; i < n; i += 64) hit = f(i) || hit;
        return __ballot(hit) != 0ull;
    }
};

template <bool DENSE>
__global__ void __launch_bounds__(64 * PLSC_WAVES) plsc_kernel(const PlscArgs a) {
    extern __shared__ double plsc_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * PLSC_WAVES + wave;
    if (b >= a.nb) return;
    const int P = a.md.P, L = a.md.L, R = a.R, ld = a.mom.ld;
    const int npairs = L * (L - 1) / 2, W = R + npairs;
    const double* __restrict__ rec = a.rows + b * a.row_stride;
    double* __restrict__ out = a.out + b * (long)(W + 2);
    const double st = rec[R];
    if (!(st == 0.0)) { wave_void_record(out, W, st, rec[R + 1], lane); return; }
    plspm::PlscWs w;
    plspm::plsc_carve(w, plsc_lds + (long)wave * plspm::plsc_ws_doubles(P, L, a.md.kmax), P, L, a.md.kmax);
    PlscWaveExec ex{lane, (b == 0) ? a.marks : nullptr};
    const double* __restrict__ M = a.mom.gram + b * a.mom.gstride;
    ex.mark(8);
    const double inv_n = 1.0 / assess_moment<DENSE>(M, ld, P, P);
    for (int p = lane; p < P; p += 64) w.v[p] = rec[p] * mv_stats<DENSE>(M, ld, p, P, inv_n).sd;
    ex.sync();
    ex.mark(9);
    const double* __restrict__ as = a.assess + b * (long)(a.A + 2);
    plspm::plsc_record(ex, a.md, w, a.factor, as + L, as + 4 * L + 2 * npairs, a.side + b * 3L * L, rec, R, out);
}
