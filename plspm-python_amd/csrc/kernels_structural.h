// kernels_structural.h -- structural-model assessment of every bootstrap replicate (the definitions: structural_core.h): the replicate's bootstrap
// record (its direct effects) and the assessment record kernels_assess.h just wrote for it (lv_cor) -> the structural record
//     f2[n_dir] | vif[n_dir] | specific[n_spec] | status | iterations.
// One wave per replicate, up to four waves per workgroup; the waves share nothing and meet at no workgroup barrier (a wave without a replicate, or with a failed
// one, leaves at once).  fp64 throughout; no atomics; every sum in one fixed order.  The kernel reads no moment matrix.
//   the whole record is structural_core.h structural_record on a wave executor: lanes over the L x L entries of rc and over the chains in one sweep (the loads of
//   lv_cor and of the chains' direct entries are issued together), one lane per LV for R2(j | pred(j)), one lane per direct path for its two drop-one solves
//   (<= 8 regressors in registers, more through the lane's slot of LDS scratch).  A wave's LDS slice holds rc, the R2 values and `nslots` slots: 64 where they
//   fit, fewer beyond that -- the lanes past nslots then sit out and the indices go round more often (launch_structural decides).
#pragma once
#include "kernels_moments.h"
#include "structural_core.h"

constexpr int STRUCTURAL_WAVES = 4;

struct StructuralArgs {
    int R, A;                                      // bootstrap record width (status at R), assessment record width (lv_cor at 4 L + 2 npairs)
    plspm::ModelDesc md;
    plspm::StructDesc sd;
    int waves, nslots;                             // waves per workgroup, regression slots per wave
    const double* rows; long row_stride;
    const double* assess;                          // [nb x (A + 2)]
    double* out; long nb;                          // record b at out + b * (2 n_dir + n_spec + 2)
    long long* marks;                              // phase clocks of problem 0 (`make marks`; null in the release library)
};

// the wave executor: lanes stride over the indices; the hand-over between lanes is the wave's own LDS order
struct StructuralWaveExec {
    static constexpr int kcap = 8;                 // regressions on at most 8 regressors in registers (solver_core.h spd_solve)
    int lane;
    long long* marks;
#ifdef PLSPM_DEBUG_MARKS
    __device__ __forceinline__ void mark(int id) { if (marks && lane == 0) marks[id] = (long long)__builtin_readcyclecounter(); }
#else
    __device__ __forceinline__ void mark(int) {}
#endif
    __device__ __forceinline__ void sync() { wave_sync(); }
    template <class F> __device__ __forceinline__ void par(int n, F f) { for (int i = lane; i < n; i += 64) f(i); sync(); }
    template <class F> __device__ __forceinline__ void slots(int n, int nslots, F f) {
        if (lane < nslots) for (int i = lane; i < n; i += nslots) f(i, lane);
        sync();
    }
    template <class F> __device__ __forceinline__ void one(F f) { if (lane == 0) f(); sync(); }
};

__global__ void __launch_bounds__(64 * STRUCTURAL_WAVES) structural_kernel(const StructuralArgs a) {
    extern __shared__ double structural_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * a.waves + wave;
    if (b >= a.nb) return;
    const int L = a.md.L, R = a.R, S = 2 * a.sd.n_dir + a.sd.n_spec;
    const double* __restrict__ rec = a.rows + b * a.row_stride;
    double* __restrict__ out = a.out + b * (long)(S + 2);
    const double st = rec[R];
    if (!(st == 0.0)) { wave_void_record(out, S, st, rec[R + 1], lane); return; }
    plspm::StructWs w;
    plspm::structural_carve(w, structural_lds + (long)wave * plspm::structural_ws_doubles(L, a.md.kmax, a.nslots), L);
    StructuralWaveExec ex{lane, (b == 0) ? a.marks : nullptr};
    ex.mark(0);
    const double* __restrict__ as = a.assess + b * (long)(a.A + 2);
    plspm::structural_record(ex, a.md, a.sd, w, a.nslots, as + 4 * L + L * (L - 1), rec, R, out);
}
