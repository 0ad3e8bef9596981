// kernels_rebus.h -- Device kernels, part 15: REBUS-PLS.  Included by plspm_rebus.hip only (wave_ops.h in front).
//   rebus_counts_kernel    problem k: count 1 on the rows whose label is k, as 0/1 count rows (count_rows.h).
//   rebus_moments_kernel   per (class, row slice): n, sum x', sum x'^2 of the class's rows in the slice, in one fixed order.
//   rebus_compose_kernel   one wave per class: the slices' sums in slice order, then rebus_core.h rebus_compose -> the class's parameters and validity flag.
//   rebus_residual_kernel  a tile of 64 rows per workgroup, staged once; lane = row, wave = class: A_ik, B_ik and the tile's partial sums at fixed slots;
//                          FINAL adds the members-only sums of every squared residual, STORE writes every residual (K = 1).
//   rebus_within_kernel    the tiles' members-only sums in tile order.
//   rebus_assign_kernel    the totals in a fixed order, CM, the argmin; writes label and CM, counts `changed` and the class sizes (integer atomics).
// No floating-point atomics anywhere: every sum has one order, so a repeated call gives the same bits.
#pragma once
#include "count_rows.h"
#include "rebus_route.h"

// Counts of the chunk's problems prob0 + p, p < nprob: 1 on the rows of class prob0 + p.
__global__ void __launch_bounds__(COUNT_NT) rebus_counts_kernel(int N, int KB, int MT, int64_t prob0, int nprob, const int* __restrict__ label, uint4* __restrict__ Cd) {
    int p, c;
    if (!count_row_thread(nprob, KB, p, c)) return;
    const int k = (int)(prob0 + p);
    const int nv = count_row_rows(N, c);
    unsigned bits = 0u;                                       // bit t: row 16c + t belongs to class k
    const int* lp = label + 16 * c;
    for (int t = 0; t < nv; ++t)
        if (lp[t] == k) bits |= 1u << t;
    count_row_store(Cd, MT, c, p, bits);
}

// Workgroup (k, s): the rows [s slice_rows, (s + 1) slice_rows) of class k.  Wave w takes the slice's rows w, w + 4, ... (the label is uniform in a wave), lane =
// column within a chunk of 64; the four waves' sums meet in LDS in wave order.  out [(k slices + s)][2 P + 1]: S1 [P] | S2 [P] | n.
__global__ void __launch_bounds__(256) rebus_moments_kernel(const double* __restrict__ Xa, int PA, int P, int N, long slice_rows, const int* __restrict__ label, double* __restrict__ out) {
    __shared__ double red[2][3][64];
    __shared__ int cnt[4];
    const int k = blockIdx.x, s = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long r0 = (long)s * slice_rows, r1 = lmin(N, r0 + slice_rows);
    double* o = out + ((long)k * gridDim.y + s) * (2 * P + 1);
    for (int p0 = 0; p0 < P; p0 += 64) {
        const int p = p0 + lane;
        double s1 = 0.0, s2 = 0.0;
        int n = 0;
        for (long i = r0 + w; i < r1; i += 4) {
            if (label[i] != k) continue;
            ++n;
            if (p < P) { const double x = Xa[i * PA + p]; s1 += x; s2 = fma(x, x, s2); }
        }
        if (w > 0) { red[0][w - 1][lane] = s1; red[1][w - 1][lane] = s2; }
        if (p0 == 0 && lane == 0) cnt[w] = n;
        __syncthreads();
        if (w == 0 && p < P) {
            o[p] = ((s1 + red[0][0][lane]) + red[0][1][lane]) + red[0][2][lane];
            o[P + p] = ((s2 + red[1][0][lane]) + red[1][1][lane]) + red[1][2][lane];
        }
        if (p0 == 0 && threadIdx.x == 0) o[2 * P] = (double)(cnt[0] + cnt[1] + cnt[2] + cnt[3]);
        __syncthreads();
    }
}

struct RebusWaveExec {
    __device__ int lane() const { return threadIdx.x; }
    __device__ int lanes() const { return 64; }
    __device__ double sum(double v) const { return wv::allsum(v); }
    __device__ int any(int v) const { return __syncthreads_or(v); }
    __device__ void sync() const { __syncthreads(); }
};

// Class k = blockIdx.x, one wave.  Dynamic LDS: (4 P + L) doubles (S1 | S2 | rebus_compose's scratch).
__global__ void __launch_bounds__(64) rebus_compose_kernel(plspm::RebusModel md, const double* __restrict__ rec, int RS, const int* __restrict__ status, const double* __restrict__ mom,
                                                           int slices, double* __restrict__ par, int* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int P = md.P, lane = threadIdx.x, k = blockIdx.x, MW = 2 * P + 1;
    double* S1 = reinterpret_cast<double*>(smem_raw);
    double* S2 = S1 + P;
    double* work = S2 + P;
    const double* mk = mom + (long)k * slices * MW;
    for (int e = lane; e < 2 * P; e += 64) {
        double s = 0.0;
        for (int sl = 0; sl < slices; ++sl) s += mk[(long)sl * MW + e];
        S1[e] = s;
    }
    double n = 0.0;
    for (int sl = 0; sl < slices; ++sl) n += mk[(long)sl * MW + 2 * P];
    __syncthreads();
    RebusWaveExec ex;
    const int ok = plspm::rebus_compose(ex, md, rec + (long)k * RS, status[k], n, S1, S2, par + (long)k * plspm::rebus_param_doubles(P, md.L, md.n_endo), work);
    if (lane == 0) flags[k] = ok;
}

// Tile t = blockIdx.x: rows [64 t, 64 t + 64) of Xa [N][PA] -- one contiguous block, loaded coalesced -- into LDS [64][xs]; then per LDS load of `cpl` classes'
// parameters, wave w takes the classes w, w + 4, ... of the load and lane = row.  Dynamic LDS: cpl PD | 64 xs | L x 256 doubles.
//   Aout, Bout [K][N]; partA, partB [K][tiles]: the tile's sums over its rows (butterfly order), plain stores at fixed slots.
//   FINAL: within [tiles][K][P + n_endo] = the sums of e^2 / f^2 over the tile's rows whose label is the class.   STORE: resid [N][P + n_endo] (class 0).
template <bool FINAL, bool STORE>
__global__ void __launch_bounds__(256) rebus_residual_kernel(const double* __restrict__ Xa, int PA, int P, int L, int n_endo, int N, int K, int cpl, int xs, const int* __restrict__ boff,
                                                             const int* __restrict__ endo, const double* __restrict__ par, const int* __restrict__ label, double* __restrict__ Aout,
                                                             double* __restrict__ Bout, double* __restrict__ partA, double* __restrict__ partB, double* __restrict__ within,
                                                             double* __restrict__ resid) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int PD = plspm::rebus_param_doubles(P, L, n_endo), tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double* pars = reinterpret_cast<double*>(smem_raw);
    double* Xs = pars + (long)cpl * PD;
    double* ys = Xs + 64 * xs;
    const long tile = blockIdx.x, tiles = gridDim.x, i0 = tile * 64;
    const int nrows = (int)lmin(64, N - i0);
    const double* src = Xa + i0 * PA;
    for (int r = w; r < 64; r += 4)
        for (int p = lane; p < P; p += 64) Xs[r * xs + p] = r < nrows ? src[(long)r * PA + p] : 0.0;
    const long row = i0 + lane;
    const bool live = lane < nrows;
    const int mine = (FINAL && live) ? label[row] : -1;
    const int W = P + n_endo;
    const double* xr = Xs + lane * xs;
    double* yr = ys + tid;
    for (int c0 = 0; c0 < K; c0 += cpl) {
        const int kc = K - c0 < cpl ? K - c0 : cpl;
        __syncthreads();                                      // the tile is staged; the previous load's readers are done
        for (int e = tid; e < kc * PD; e += 256) pars[e] = par[(long)c0 * PD + e];
        __syncthreads();
        for (int kk = w; kk < kc; kk += 4) {
            const int k = c0 + kk;
            const plspm::RebusParamsT<const double> pr = plspm::rebus_params<const double>(pars + (long)kk * PD, P, L, n_endo);
            double* wk = FINAL ? within + (tile * K + k) * W : nullptr;
            const bool member = mine == k;
            double A, B;
            plspm::rebus_row(P, L, n_endo, boff, endo, pr, [&](int p) { return xr[p]; }, [&](int l) -> double& { return yr[l * 256]; },
                             [&](int idx, double v) {
                                 if (STORE) { if (live) resid[row * W + idx] = v; }
                                 if (FINAL) {
                                     const double s = wv::allsum(member ? v * v : 0.0);
                                     if (lane == 0) wk[idx] = s;
                                 }
                             },
                             A, B);
            if (live) { Aout[(long)k * N + row] = A; Bout[(long)k * N + row] = B; }
            const double sa = wv::allsum(live ? A : 0.0), sb = wv::allsum(live ? B : 0.0);
            if (lane == 0) { partA[k * tiles + tile] = sa; partB[k * tiles + tile] = sb; }
        }
    }
}

// within_out [K][P + n_endo] = the tiles' sums in tile order.  Workgroup k; a thread per value.
__global__ void __launch_bounds__(256) rebus_within_kernel(const double* __restrict__ within, long tiles, int K, int W, double* __restrict__ out) {
    const int k = blockIdx.x;
    for (int e = threadIdx.x; e < W; e += 256) {
        double s = 0.0;
        for (long t = 0; t < tiles; ++t) s += within[(t * K + k) * W + e];
        out[k * W + e] = s;
    }
}

// A thread per row.  The totals of every class first (thread t adds the tiles t, t + 256, ... in order, then a fixed tree over the 256 threads; every workgroup
// computes the same bits), then CM_ik and the argmin.  Nothing is written while a class is invalid (flags): labels and counters stay.
//   cm (may be null) [N][K];  assign != 0: label[i] <- argmin, ctr[0] += #changed, ctr[1 + k] += the new size of class k (one integer atomic per workgroup and slot).
__global__ void __launch_bounds__(256) rebus_assign_kernel(int N, int K, long tiles, const double* __restrict__ Aall, const double* __restrict__ Ball, const double* __restrict__ partA,
                                                           const double* __restrict__ partB, const int* __restrict__ flags, int assign, int* __restrict__ label, double* __restrict__ cm,
                                                           int* __restrict__ ctr) {
    __shared__ double red[256];
    __shared__ double tot[2 * plspm::kRebusMaxClasses];
    __shared__ int cnt[1 + plspm::kRebusMaxClasses];
    const int tid = threadIdx.x;
    int valid = 1;
    for (int k = 0; k < K; ++k) valid &= flags[k] != 0;
    if (!valid) return;
    if (tid <= K) cnt[tid] = 0;
    for (int s = 0; s < 2 * K; ++s) {
        const double* part = (s < K ? partA + (long)s * tiles : partB + (long)(s - K) * tiles);
        double v = 0.0;
        for (long t = tid; t < tiles; t += 256) v += part[t];
        red[tid] = v;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (tid < h) red[tid] += red[tid + h];
            __syncthreads();
        }
        if (tid == 0) tot[s] = red[0];
        __syncthreads();
    }
    const long i = (long)blockIdx.x * 256 + tid;
    if (i < N) {
        int best = -1;
        double bv = 0.0;
        for (int k = 0; k < K; ++k) {
            const double v = plspm::rebus_cm(Aall[(long)k * N + i], Ball[(long)k * N + i], tot[k], tot[K + k], (double)N);
            if (cm) cm[i * K + k] = v;
            if (v == v && (best < 0 || v < bv)) { best = k; bv = v; }
        }
        if (assign) {
            const int old = label[i];
            if (best < 0) best = old;
            if (best != old) { label[i] = best; atomicAdd(&cnt[0], 1); }
            atomicAdd(&cnt[1 + best], 1);
        }
    }
    if (assign) {
        __syncthreads();
        if (tid <= K && cnt[tid]) atomicAdd(&ctr[tid], cnt[tid]);
    }
}
