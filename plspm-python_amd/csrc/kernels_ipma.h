// kernels_ipma.h -- importance-performance map analysis of every bootstrap replicate (the definitions, the lists and the plan: ipma_core.h): the
// replicate's moment matrix -- which only exists between the Gram and the next pass --, the handle's shifts and the replicate's bootstrap record -> the record
//     perf [L] | sd [L] | total_u [n_eff] | direct_u [n_eff] | weight_r [P] | mvperf [P] | mvimp [n_t x P] | status | iterations.
// One wave per replicate, 4, 2 or 1 waves per workgroup as ipma_plan sizes the slices; the waves share nothing and meet at no workgroup barrier (a wave without a
// replicate, or with a failed one, leaves at once).  fp64 throughout; no atomics; the hand-over between lanes is wave_sync() alone.
//   The whole record is ipma_core.h ipma_record on a wave executor:
//   1  lanes over the MVs: 1/s, mu, v = w s, range / s and the indicator's performance into the slice, the performance to the record
//   2  lane p forms t_p = sum_q r_pq v_q over its own block: column p of the diagonal block (contiguous along the lanes in the dense layout wherever p >= q, down the
//      column below the diagonal; through packed_index in the tile-packed one), the loads of kIpmaRows rows issued together: one memory round trip per batch of rows
//   3  lanes over the LVs, a lane owns its block: the norm v'Rv, the sign, a_p and A_l, the rescaled weights, the performance and the sd -- LDS reads only
//   4  lanes over the effect pairs: total_u and direct_u; lanes over the MVs: the rescaled weights to the record, the flags
//   5  lanes over the MVs, target by target: the indicator importances; every store of 4 and 5 is coalesced
#pragma once
#include "kernels_moments.h"
#include "ipma_core.h"

constexpr int IPMA_WAVES = 4;

struct IpmaArgs {
    MomentLayout mom;
    plspm::IpmaDescs d;
    int R, waves;                                  // bootstrap record width (status at R, iterations at R + 1); waves per workgroup
    long wave_doubles, stride;                     // doubles of a wave's slice; the record pitch W + 2
    const double* rows; long row_stride;
    double* out; long nb;                          // record b at out + b * stride
};

template <bool DENSE> struct IpmaMoments {
    const double* __restrict__ M; int ld;
    __device__ __forceinline__ double operator()(int p, int q) const { return assess_moment<DENSE>(M, ld, p, q); }
};

struct IpmaWaveExec {
    int lane;
    template <class F> __device__ __forceinline__ void lanes(F f) { f(lane); wave_sync(); }
};

template <bool DENSE>
__global__ void __launch_bounds__(64 * IPMA_WAVES) ipma_kernel(const IpmaArgs a) {
    extern __shared__ double ipma_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long b = (long)blockIdx.x * a.waves + wave;
    if (b >= a.nb) return;
    const int W = (int)(a.stride - 2);
    const double* __restrict__ rec = a.rows + b * a.row_stride;
    double* __restrict__ out = a.out + b * a.stride;
    const double st = rec[a.R];
    if (!(st == 0.0)) { wave_void_record(out, W, st, rec[a.R + 1], lane); return; }
    IpmaWaveExec ex{lane};
    const IpmaMoments<DENSE> mom{a.mom.gram + b * a.mom.gstride, a.mom.ld};
    plspm::ipma_record(ex, a.d, mom, rec, ipma_lds + (long)wave * a.wave_doubles, rec[a.R + 1], out);
}
