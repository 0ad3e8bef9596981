// kernels_jack.h -- Device kernels, part 8: the jackknife (delete-one / delete-a-group).  Included by plspm_jackknife.hip only (wave_ops.h in front).
//   jack_counts_kernel   problem g: count 1 on the rows i with i % G != g, as 0/1 count rows (count_rows.h).
//   jack_stats_kernel    per record column: mean, d_g = mean - theta_(g), se and acceleration over the OK problems, every sum in one fixed order.
#pragma once
#include "count_rows.h"

constexpr int JACK_NT = 256;       // threads of a jack_stats_kernel workgroup

// Counts of the chunk's problems prob0 + p, p < nprob: 1 on the rows the problem keeps.
__global__ void __launch_bounds__(COUNT_NT) jack_counts_kernel(int N, int KB, int MT, int G, int64_t prob0, int nprob, uint4* __restrict__ Cd) {
    int p, c;
    if (!count_row_thread(nprob, KB, p, c)) return;
    const int g = (int)(prob0 + p);
    const int nv = count_row_rows(N, c);
    unsigned bits = 0u;                                       // bit t: row 16c + t stays in
    if (nv) {
        int r = (16 * c) % G;                                 // (16c + t) % G, stepped
        for (int t = 0; t < nv; ++t) {
            if (r != g) bits |= 1u << t;
            if (++r == G) r = 0;
        }
    }
    count_row_store(Cd, MT, c, p, bits);
}

// block-wide sum in one fixed order: 64-lane butterfly (wave_ops.h), then the four wave results in wave order
__device__ __forceinline__ double jack_sum_block(double v, double* redw, int lane, int wave) {
    v = wv::allsum(v);
    if (lane == 0) redw[wave] = v;
    __syncthreads();
    const double t = (redw[0] + redw[1]) + (redw[2] + redw[3]);
    __syncthreads();
    return t;
}

// Workgroup c = one record column.  records [G x stride] (row | status | iterations); the OK problems (status column exactly 0) in problem order:
// thread t takes problems t, t + 256, ...  out: mean [R] | std_error [R] | accel [R], then the number of OK problems (an int behind the 3R doubles).
//   mean = sum theta_(g) / n,  d_g = mean - theta_(g),  std_error = sqrt((n - 1) / n sum d^2),  accel = sum d^3 / (6 (sum d^2)^1.5) -- NaN where sum d^2 = 0
__global__ void __launch_bounds__(JACK_NT) jack_stats_kernel(const double* __restrict__ records, long G, int stride, int R, double* __restrict__ out, int* __restrict__ n_used) {
    static_assert(JACK_NT == 256, "jack_sum_block adds four wave results");
    __shared__ double redw[JACK_NT / 64];
    __shared__ unsigned cntw[JACK_NT / 64];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned cnt = 0u;
    double s = 0.0;
    for (long g = tid; g < G; g += JACK_NT)
        if (records[g * stride + R] == 0.0) { ++cnt; s += records[g * stride + c]; }
    cnt = wv::allsum(cnt);
    if (lane == 0) cntw[wave] = cnt;
    const double tot = jack_sum_block(s, redw, lane, wave);       // (its barriers publish cntw as well)
    const unsigned n = cntw[0] + cntw[1] + cntw[2] + cntw[3];
    const double mean = tot / (double)n;
    double s2 = 0.0, s3 = 0.0;
    for (long g = tid; g < G; g += JACK_NT)
        if (records[g * stride + R] == 0.0) { const double d = mean - records[g * stride + c]; s2 += d * d; s3 += d * d * d; }
    const double ss2 = jack_sum_block(s2, redw, lane, wave);
    const double ss3 = jack_sum_block(s3, redw, lane, wave);
    if (tid == 0) {
        const double nan = __builtin_nan("");
        out[c] = n ? mean : nan;
        out[R + c] = n ? sqrt((double)(n - 1u) / (double)n * ss2) : nan;
        out[2 * R + c] = (n && ss2 > 0.0) ? ss3 / (6.0 * (ss2 * sqrt(ss2))) : nan;
        if (c == 0) *n_used = (int)n;
    }
}
