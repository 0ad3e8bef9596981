// kernels_tetrad.h -- confirmatory tetrad analysis of every bootstrap replicate (the definitions, the lists and the plan: tetrad_core.h): the
// replicate's moment matrix -- which only exists between the Gram and the next pass -- -> the tetrad record
//     tetrads[n_tet] | status | iterations.
// One wave per replicate, 4, 2 or 1 waves per workgroup as tetrad_plan sizes the slices; the waves share nothing and meet at no workgroup barrier (a wave without a
// replicate, or with a failed one, leaves at once).  fp64 throughout; no atomics; the hand-over between lanes is wave_sync() alone.  Of the bootstrap record the
// kernel reads the status and the iteration count only.
//   The whole record is tetrad_core.h tetrad_record on a wave executor:
//   1  per-MV statistics 1/s and mu into the slice, lanes over the MVs, as assess_kernel opens
//   2  the strict upper triangles of the tested blocks into the slice as x_pq: lane q serves a column of a window of 64, rows are read along the lanes (contiguous
//      in the dense layout, through packed_index in the tile-packed one), the loads of kTetradRows rows issued together: one memory round trip per batch of rows
//   3  lane t takes tetrads t, t + 64, ...: the 8-byte descriptors of kTetradBatch tetrads in flight together, then four LDS reads, two products, one
//      subtraction and one coalesced store each
#pragma once
#include "kernels_moments.h"
#include "tetrad_core.h"

constexpr int TETRAD_WAVES = 4;

struct TetradArgs {
    MomentLayout mom;
    plspm::TetradDescs td;
    int R, waves;                                  // bootstrap record width (status at R, iterations at R + 1); waves per workgroup
    long wave_doubles;
    const double* rows; long row_stride;
    double* out; long nb;                          // record b at out + b * (n_tet + 2)
};

template <bool DENSE> struct TetradMoments {
    const double* __restrict__ M; int ld;
    __device__ __forceinline__ double operator()(int p, int q) const { return assess_moment<DENSE>(M, ld, p, q); }
};

struct TetradWaveExec {
    int lane;
    __device__ __forceinline__ void mark(int) {}
    template <class F> __device__ __forceinline__ void lanes(F f) { f(lane); wave_sync(); }
};

template <bool DENSE>
__global__ void __launch_bounds__(64 * TETRAD_WAVES) tetrad_kernel(const TetradArgs a) {
    extern __shared__ double tetrad_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * a.waves + wave;
    if (b >= a.nb) return;
    const int W = a.td.n_tet;
    const double* __restrict__ rec = a.rows + b * a.row_stride;
    double* __restrict__ out = a.out + b * (long)(W + 2);
    const double st = rec[a.R];
    if (!(st == 0.0)) { wave_void_record(out, W, st, rec[a.R + 1], lane); return; }
    TetradWaveExec ex{lane};
    const TetradMoments<DENSE> mom{a.mom.gram + b * a.mom.gstride, a.mom.ld};
    plspm::tetrad_record(ex, a.td, mom, a.mom.P, tetrad_lds + (long)wave * a.wave_doubles, rec[a.R + 1], out);
}
