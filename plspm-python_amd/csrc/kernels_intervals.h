// kernels_intervals.h -- Device kernels, part 5c: bootstrap confidence intervals (percentile, basic, BC, BCa) per record column.
// Included by plspm_bootstrap.hip only, behind kernels_summary.h, whose small pieces it shares (order_key, key_value, lerp_numpy, the SUM_* geometry,
// records_transpose_kernel in front of it); summary_kernel itself is left as it is -- its compaction and its radix select are restated here with
// per-column ranks, so that the summary's code, registers and time do not move.
#pragma once

constexpr int CI_PERCENTILE = 0, CI_BASIC = 1, CI_BC = 2, CI_BCA = 3;
constexpr int CI_LDS_VALUES = 16384;      // values of a column the LDS buffer holds (128 KiB); longer columns take the global scratch slice

// One workgroup of 1,024 threads per column c, over the m replicates whose status is OK; with alpha_lo / alpha_hi the two nominal levels:
//   1. compaction in replicate order (summary_kernel's: up to 8,192 values then live in registers);
//   2. one counting pass: below = #{theta* < original}, z0 = normcdfinv(below / m);
//   3. the two levels p_0 <= p_1 of the method -- percentile, basic: alpha_lo, alpha_hi;  BC (a = 0), BCa (a = accel[c]):
//      normcdf(z0 + (z0 + z) / (1 - a (z0 + z))) for z = normcdfinv(alpha_lo), normcdfinv(alpha_hi);
//   4. the order statistics floor(p_j (m - 1)) and their successors by radix select (summary_kernel's, two per-column ranks), numpy's linear interpolation.
// out[c*6 + {0..5}] = lower, upper, z0, accel, level.lower, level.upper.  NaN rules: everything where m = 0 or original is NaN; lower / upper / levels of BC and
// BCa where below is 0 or m; lower / upper / accel / levels of BCa where accel is NaN.  accel: NaN for percentile and basic, 0 for BC.
// `original`, `accel` and `out` may live in pinned host memory (the handle's staging area).
template <bool IN_LDS>
__global__ void __launch_bounds__(SUM_NT) intervals_kernel(const double* __restrict__ cols, long cols_ld, long B, int R, const double* __restrict__ original,
                                                            const double* __restrict__ accel, int method, double alpha_lo, double alpha_hi,
                                                            double* __restrict__ gbuf, int npad, double* __restrict__ out, int* __restrict__ n_used) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ unsigned hist[2][256];
    __shared__ int wcount[SUM_NB * SUM_NW];
    __shared__ int wtot[2];
    __shared__ unsigned wscan[2][4];
    __shared__ unsigned long long sel_prefix[2];
    __shared__ unsigned sel_rank[2], sel_cnt[2];
    __shared__ unsigned long long red_key[2][SUM_NW];
    __shared__ unsigned red_cnt[2][SUM_NW];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double orig = original[c];
    const double acc_in = (method == CI_BCA) ? accel[c] : 0.0;
    double* buf = IN_LDS ? reinterpret_cast<double*>(smem_raw) : gbuf + (long)c * npad;
    // 1. compaction in replicate order
    int m = 0;
    for (long s0 = 0; s0 < B; s0 += (long)SUM_NT * SUM_NB) {
        double val[SUM_NB], st[SUM_NB];
#pragma unroll
        for (int k = 0; k < SUM_NB; ++k) {
            st[k] = 1.0; val[k] = 0.0;
            if (s0 + (long)SUM_NT * k < B) {                        // (uniform: chunks beyond the last replicate load nothing)
                const long b = s0 + (long)SUM_NT * k + tid;
                const long bc = (b < B) ? b : B - 1;
                st[k] = cols[(long)R * cols_ld + bc];
                val[k] = cols[(long)c * cols_ld + bc];
            }
        }
        unsigned long long bal[SUM_NB];
#pragma unroll
        for (int k = 0; k < SUM_NB; ++k) {
            const bool ok = (s0 + (long)SUM_NT * k + tid < B) && st[k] == 0.0;
            bal[k] = __ballot(ok);
            if (lane == 0) wcount[k * SUM_NW + wave] = __popcll(bal[k]);
        }
        __syncthreads();
        int excl = 0;
        if (tid < SUM_NB * SUM_NW) {                                // waves 0 and 1: exclusive scan of the 128 counts in (chunk, wave) order
            const int v = wcount[tid];
            const int incl = wv::inclusive_scan(v);
            excl = incl - v;
            if (lane == 63) wtot[wave] = incl;
        }
        __syncthreads();
        if (tid < SUM_NB * SUM_NW) wcount[tid] = m + excl + (wave == 1 ? wtot[0] : 0);
        const int total = wtot[0] + wtot[1];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SUM_NB; ++k) {
            const bool ok = (s0 + (long)SUM_NT * k + tid < B) && st[k] == 0.0;
            if (ok) buf[wcount[k * SUM_NW + wave] + __popcll(bal[k] & ((1ull << lane) - 1ull))] = val[k];
        }
        m += total;
        __syncthreads();
    }
    if (tid == 0 && c == 0) *n_used = m;
    const bool cached = m <= SUM_NT * SUM_RI;
    double item[SUM_RI];
#pragma unroll
    for (int j = 0; j < SUM_RI; ++j) item[j] = (cached && tid + SUM_NT * j < m) ? buf[tid + SUM_NT * j] : 0.0;
    auto each = [&](auto f) {
        if (cached) {
#pragma unroll
            for (int j = 0; j < SUM_RI; ++j) if (tid + SUM_NT * j < m) f(item[j]);
        } else {
            for (int i = tid; i < m; i += SUM_NT) f(buf[i]);
        }
    };
    // 2. the replicates strictly below the original (Efron's rule), and the smallest and largest key on the way
    unsigned below = 0u;
    unsigned long long kmin = ~0ull, kmax = 0ull;
    each([&](double x) {
        below += (x < orig) ? 1u : 0u;
        const unsigned long long k = order_key(x); kmin = (k < kmin) ? k : kmin; kmax = (k > kmax) ? k : kmax;
    });
    below = wv::allsum(below); kmin = wv::allmin(kmin); kmax = wv::allmax(kmax);
    if (lane == 0) { red_cnt[0][wave] = below; red_key[0][wave] = kmin; red_key[1][wave] = kmax; }
    __syncthreads();
    below = 0u; kmin = red_key[0][0]; kmax = red_key[1][0];
#pragma unroll
    for (int w = 0; w < SUM_NW; ++w) {
        below += red_cnt[0][w];
        const unsigned long long a = red_key[0][w], b = red_key[1][w]; kmin = (a < kmin) ? a : kmin; kmax = (b > kmax) ? b : kmax;
    }
    // 3. the two levels (every thread computes the same numbers)
    const double nan = __builtin_nan("");
    const bool any = m > 0 && orig == orig;
    const double z0 = any ? normcdfinv((double)below / (double)m) : nan;
    double p[2] = {alpha_lo, alpha_hi}, acc_out = nan;
    if (method == CI_BC || method == CI_BCA) {
        acc_out = acc_in;
        const double zz[2] = {normcdfinv(alpha_lo), normcdfinv(alpha_hi)};
#pragma unroll
        for (int j = 0; j < 2; ++j) p[j] = (below == 0u || below == (unsigned)m) ? nan : normcdf(z0 + (z0 + zz[j]) / (1.0 - acc_in * (z0 + zz[j])));
        if (acc_in != acc_in) p[0] = p[1] = nan;
    }
    if (!any) { p[0] = p[1] = nan; acc_out = nan; }
    const bool valid = p[0] == p[0] && p[1] == p[1];
    // 4. order statistics lo_j = floor(p_j (m-1)) (and their successors) by radix select
    double q_out[2] = {nan, nan};
    if (valid) {                                                   // (uniform; m > 0)
        const double pos[2] = {p[0] * (double)(m - 1), p[1] * (double)(m - 1)};
        const int lo[2] = {(int)floor(pos[0]), (int)floor(pos[1])};
        const unsigned long long diff = kmin ^ kmax;
        const int shared_bytes = diff ? (__clzll((long long)diff) >> 3) : 8;
        unsigned long long mask = shared_bytes ? (shared_bytes == 8 ? ~0ull : ~0ull << (64 - 8 * shared_bytes)) : 0ull;
        __syncthreads();                                           // (red_key is written again below)
        if (tid < 2) { sel_prefix[tid] = kmin & mask; sel_rank[tid] = (unsigned)lo[tid]; sel_cnt[tid] = (unsigned)m; }
        for (int shift = 56 - 8 * shared_bytes; shift >= 0; shift -= 8) {
            if (tid < 512) (&hist[0][0])[tid] = 0u;
            __syncthreads();
            if (sel_cnt[0] <= 1u && sel_cnt[1] <= 1u) break;       // (uniform: read behind the barrier)
            const unsigned long long p0 = sel_prefix[0], p1 = sel_prefix[1];
            // run-length aggregation per thread and per wave (summary_kernel: heavy ties would be 64-way same-address LDS atomics)
            unsigned run_d[2] = {0u, 0u}, run_n[2] = {0u, 0u};
            each([&](double x) {
                const unsigned long long k = order_key(x);
                const unsigned d = (unsigned)(k >> shift) & 255u;
                const bool hit[2] = {(k & mask) == p0, (k & mask) == p1};
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (hit[j]) {
                        if (run_n[j] && run_d[j] != d) { atomicAdd(&hist[j][run_d[j]], run_n[j]); run_n[j] = 0u; }
                        run_d[j] = d; ++run_n[j];
                    }
                }
            });
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const unsigned long long have = __ballot(run_n[j] != 0u);
                if (have) {                                        // (uniform)
                    const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)run_d[j], __ffsll((long long)have) - 1);
                    if (__all(run_n[j] == 0u || run_d[j] == d0)) {
                        const unsigned n = wv::allsum(run_n[j]);
                        if (lane == 0) atomicAdd(&hist[j][d0], n);
                    } else if (run_n[j]) atomicAdd(&hist[j][run_d[j]], run_n[j]);
                }
            }
            __syncthreads();
            // inclusive scan of the 256 bins of both histograms: bin t is owned by thread t (waves 0 .. 3)
            unsigned mine[2] = {0u, 0u}, incl[2] = {0u, 0u}, rank[2] = {0u, 0u};
            if (tid < 256) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    mine[j] = hist[j][tid];
                    incl[j] = wv::inclusive_scan(mine[j]);
                    if (lane == 63) wscan[j][wave] = incl[j];
                }
            }
            __syncthreads();
            if (tid < 256) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    for (int w = 0; w < wave; ++w) incl[j] += wscan[j][w];
                    rank[j] = sel_rank[j];
                }
            }
            __syncthreads();                                       // everyone has read wscan / sel_rank
            if (tid < 256) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const unsigned excl = incl[j] - mine[j];
                    if (rank[j] >= excl && rank[j] < incl[j]) { sel_prefix[j] |= (unsigned long long)tid << shift; sel_rank[j] = rank[j] - excl; sel_cnt[j] = mine[j]; }
                }
            }
            mask |= 0xffull << shift;
            __syncthreads();
        }
        // a bin with a single value: the remaining digits are that value's; then the successor of each selected value
        __syncthreads();
        if (mask != ~0ull) {
            const unsigned long long pj[2] = {sel_prefix[0], sel_prefix[1]};
            each([&](double x) {
                const unsigned long long k = order_key(x);
                if ((k & mask) == pj[0]) red_key[0][0] = k;        // (one writer, or equal values)
                if ((k & mask) == pj[1]) red_key[1][0] = k;
            });
            __syncthreads();
            if (tid < 2) sel_prefix[tid] = red_key[tid][0];
            __syncthreads();
        }
        unsigned cnt[2] = {0u, 0u};
        unsigned long long nxt[2] = {~0ull, ~0ull};
        const unsigned long long vk[2] = {sel_prefix[0], sel_prefix[1]};
        each([&](double x) {
            const unsigned long long k = order_key(x);
#pragma unroll
            for (int j = 0; j < 2; ++j) { if (k <= vk[j]) ++cnt[j]; else nxt[j] = (k < nxt[j]) ? k : nxt[j]; }
        });
        __syncthreads();                                           // (red_key was read above)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            cnt[j] = wv::allsum(cnt[j]);
            nxt[j] = wv::allmin(nxt[j]);
            if (lane == 0) { red_cnt[j][wave] = cnt[j]; red_key[j][wave] = nxt[j]; }
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                unsigned total = 0u;
                unsigned long long nk = ~0ull;
                for (int w = 0; w < SUM_NW; ++w) { total += red_cnt[j][w]; nk = (red_key[j][w] < nk) ? red_key[j][w] : nk; }
                const double a = key_value(vk[j]);
                const bool has_next = lo[j] + 1 < m;
                const double b2 = !has_next ? a : (((int)total >= lo[j] + 2) ? a : key_value(nk));
                q_out[j] = lerp_numpy(a, b2, pos[j] - (double)lo[j]);
            }
        }
    }
    if (tid == 0) {
        double* o = out + (long)c * 6;
        o[0] = (method == CI_BASIC) ? 2.0 * orig - q_out[1] : q_out[0];
        o[1] = (method == CI_BASIC) ? 2.0 * orig - q_out[0] : q_out[1];
        o[2] = z0;
        o[3] = acc_out;
        o[4] = p[0];
        o[5] = p[1];
    }
}
