// fimix_core.h -- FIMIX-PLS: a finite mixture of inner-model regressions on the latent variable scores, one whole EM problem as ONE portable
// function the device kernel (kernels_fimix.h, one workgroup per problem) and a stand-alone host program (tests/fimix_host) both run.
//
// Inputs of one problem: the scores Y [N x L] (row-major), K segments, an initial hard assignment of the rows (init [N] bytes below K, or the Philox draw of
// philox.h fimix_start_segment).  With E the LVs that have predecessors (LV order), pred(j) the predecessors of j, segment k models every j in E as
//     y_ij = sum_{p in pred(j)} beta_kjp y_ip + e,  e ~ N(0, psi_kj)
// Iteration t = 1, 2, ...   (P^0: one-hot of the assignment)
//     M-step on P^(t-1)   n_k = sum_i P_ik, rho_k = n_k / N, m_k[a,b] = sum_i P_ik y_ia y_ib for the entries (a, b) some regression reads (fimix_entries);
//                         beta_kj: m_k[pred,pred] beta = m_k[pred,j] by solver_core.h spd_solve; psi_kj = (m_k[j,j] - beta_kj . m_k[pred,j]) / n_k
//     collapse            ST_SINGULAR at that t when an n_k < 1, a psi_kj <= 1e-10 m_k[j,j] / n_k, or a regression without an answer: NaN record
//     E-step              a_ik = c_k - sum_j r_ikj^2 / (2 psi_kj), c_k = ln rho_k - 1/2 sum_j ln(2 pi psi_kj); lse_i = max + ln sum exp(a - max);
//                         lnL = sum_i lse_i; P_ik = exp(a_ik - lse_i); H = -sum_ik P_ik (a_ik - lse_i), a zero P_ik adding nothing.  ST_NONFINITE: lnL not finite
//     stop                ST_OK when t >= 2 and |lnL^t - lnL^(t-1)| <= tol; ST_NOT_CONVERGED at t = max_iter with the complete record of that t
// One sweep over Y per iteration does the E-step with theta^t and accumulates the moments for theta^(t+1) from the posteriors it has just computed: no [N x K]
// posteriors are stored.  A thread keeps ACC accumulators: KP segments (K padded to a power of two) x ACC / KP entries; a model with more entries sweeps once per
// chunk of entries, the posteriors recomputed.  Chunk 0 carries lnL, H and n_k, and the stop rule is decided behind it.
// Record, width 2 + Kmax (1 + n_dir + n_endo):  lnL | H | rho[Kmax] | beta[Kmax][n_dir] | psi[Kmax][n_endo], beta in from-major direct-path order, psi in LV order,
// NaN in the slots k >= K; status and iterations behind it as doubles.
//
// Execution model: every thread of the group runs fimix_problem().  ex.tid() / ex.nthreads(): rows tid, tid + T, ... are a thread's; ex.sync(): the group's
// barrier; ex.put(red, q, v) hands in a thread's share of sum q, and behind a barrier ex.get(red, q) is the group's sum in ONE fixed order (thread-strided
// partials, a fixed tree inside a wave, the waves in ascending order).  Every value that crosses threads lives in the workspace.
#pragma once
#include "solver_core.h"
#if !defined(__HIPCC__) && !defined(__host__)      // (a host compiler without the HIP headers: philox.h's functions are plain inline functions there)
#define __host__
#define __device__
#define __forceinline__ inline
#endif
#include "philox.h"

namespace plspm {

constexpr int kFimixMaxK = 16;       // segments of one problem at most
constexpr int kFimixKcap = 4;        // largest regression solved in registers (solver_core.h spd_solve): the kernel's threads carry ACC accumulators beside it

PLSPM_HD int fimix_kpad(int K) { return K <= 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16; }
PLSPM_HD int fimix_record_width(int kmax, int n_dir, int n_endo) { return 2 + kmax * (1 + n_dir + n_endo); }

// The moment entries (a <= b) some regression reads: a, b in pred(j) + {j} for an endogenous j; by a, then b.  ent (may be null): a | b << 16.  Returns their number.
inline int fimix_entries(int L, const int* pred_off, const int* pred_idx, int* ent) {
    int n = 0;
    for (int a = 0; a < L; ++a)
        for (int b = a; b < L; ++b) {
            bool need = false;
            for (int j = 0; j < L && !need; ++j) {
                if (pred_off[j + 1] == pred_off[j]) continue;
                bool ha = a == j, hb = b == j;
                for (int e = pred_off[j]; e < pred_off[j + 1]; ++e) { ha = ha || pred_idx[e] == a; hb = hb || pred_idx[e] == b; }
                need = ha && hb;
            }
            if (need) { if (ent) ent[n] = a | (b << 16); ++n; }
        }
    return n;
}

// What the path matrix fixes.  Edge e of the predecessor lists (pred_off [L + 1] / pred_idx: to-major) is direct path dir_of[e] of the record (from-major).
struct FimixDesc {
    int L, n_endo, n_dir, kmax, E;      // kmax: the most predecessors of one LV
    const int* pred_off;                // [L + 1]
    const int* pred_idx;                // [n_dir]
    const int* endo;                    // [n_endo] the LVs with predecessors, ascending
    const int* dir_of;                  // [n_dir]
    const int* ent;                     // [E] a | b << 16
};

// One problem's workspace.  Parameter tables have the segment as their fast index, pitch kFimixMaxK.
//   mom [K][L x L] | beta [n_dir][16] | ipsi, psi [n_endo][16] | cst, nk, rho [16] | scal [8]: 0 lnL, 1 H, 2 lnL of the iteration before, 3 collapse flag |
//   red [waves][ACC + 18] | slot [nslots][regression_scratch_doubles(kmax)]
struct FimixWs { double *mom, *beta, *ipsi, *psi, *cst, *nk, *rho, *scal, *red, *slot; int nslots; };
PLSPM_HD long fimix_param_doubles(int L, int n_dir, int n_endo, int K) { return (long)K * L * L + (long)kFimixMaxK * (n_dir + 2 * n_endo + 3) + 8; }
PLSPM_HD long fimix_ws_doubles(int L, int n_dir, int n_endo, int kmax, int K, int waves, int acc, int nslots) {
    return fimix_param_doubles(L, n_dir, n_endo, K) + (long)waves * (acc + kFimixMaxK + 2) + (long)nslots * regression_scratch_doubles(kmax);
}
PLSPM_HD void fimix_carve(FimixWs& w, double* base, int L, int n_dir, int n_endo, int K, int waves, int acc, int nslots) {
    double* p = base;
    w.mom = p; p += (long)K * L * L;
    w.beta = p; p += kFimixMaxK * n_dir; w.ipsi = p; p += kFimixMaxK * n_endo; w.psi = p; p += kFimixMaxK * n_endo;
    w.cst = p; p += kFimixMaxK; w.nk = p; p += kFimixMaxK; w.rho = p; p += kFimixMaxK; w.scal = p; p += 8;
    w.red = p; p += (long)waves * (acc + kFimixMaxK + 2);
    w.slot = p; w.nslots = nslots;
}

// One row's E-step: a_k (k < K; minus infinity behind), the log-sum-exp, P_k in place of a_k; returns sum_k P_k ln P_k.
template <int KP>
PLSPM_HD double fimix_row(const FimixDesc& d, const FimixWs& w, int K, const double* y, double (&p)[KP], double& lse) {
    double a[KP], r[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) a[k] = w.cst[k];
    for (int je = 0; je < d.n_endo; ++je) {
        const int j = d.endo[je];
        const double yj = y[j];
#pragma unroll
        for (int k = 0; k < KP; ++k) r[k] = yj;
        for (int e = d.pred_off[j]; e < d.pred_off[j + 1]; ++e) {
            const double yp = y[d.pred_idx[e]];
            const double* b = w.beta + e * kFimixMaxK;
#pragma unroll
            for (int k = 0; k < KP; ++k) r[k] -= b[k] * yp;
        }
        const double* ip = w.ipsi + je * kFimixMaxK;
#pragma unroll
        for (int k = 0; k < KP; ++k) a[k] -= r[k] * r[k] * ip[k];
    }
    double mx = a[0];
#pragma unroll
    for (int k = 1; k < KP; ++k) if (k < K) mx = a[k] > mx ? a[k] : mx;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) { r[k] = k < K ? exp(a[k] - mx) : 0.0; s += r[k]; }
    lse = mx + log(s);
    double h = 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        const double lp = a[k] - lse;
        p[k] = k < K ? exp(lp) : 0.0;
        if (k < K && p[k] > 0.0) h += p[k] * lp;
    }
    return h;
}

// The M-step finish of regression (k, je) on segment k's moments: beta, psi, 1 / (2 psi); false when the segment collapses on it.
PLSPM_HD bool fimix_regress(const FimixDesc& d, const FimixWs& w, int k, int je, double* scratch) {
    const int L = d.L, j = d.endo[je], e0 = d.pred_off[j], kk = d.pred_off[j + 1] - e0;
    const double* M = w.mom + (long)k * L * L;
    double* x = scratch + 2 * d.kmax * d.kmax;
    const bool ok = spd_solve<kFimixKcap>(M, L, d.pred_idx + e0, kk, j, x, scratch);
    double s = 0.0;
    for (int r = 0; r < kk; ++r) { s += x[r] * M[d.pred_idx[e0 + r] * L + j]; w.beta[(e0 + r) * kFimixMaxK + k] = x[r]; }
    const double mjj = M[j * L + j], nk = w.nk[k], psi = (mjj - s) / nk;
    w.psi[je * kFimixMaxK + k] = psi;
    w.ipsi[je * kFimixMaxK + k] = 1.0 / (2.0 * psi);
    return ok && psi > 1e-10 * mjj / nk;      // (a NaN fails it)
}
// rho_k and c_k of segment k, behind its regressions (the sweep that follows writes the next n_k)
PLSPM_HD double fimix_const(const FimixDesc& d, const FimixWs& w, int k, long N) {
    double s = 0.0;
    for (int je = 0; je < d.n_endo; ++je) s += log(6.283185307179586476925286766559 * w.psi[je * kFimixMaxK + k]);
    w.rho[k] = w.nk[k] / (double)N;
    return log(w.rho[k]) - 0.5 * s;
}
// The stop rule behind the E-step of iteration t: -1 to go on, else the status the problem ends with.
PLSPM_HD int fimix_stop(int t, double lnl, double before, double tol, int max_iter) {
    if (!isfinite(lnl)) return ST_NONFINITE;
    if (t >= 2 && fabs(lnl - before) <= tol) return ST_OK;
    return t >= max_iter ? ST_NOT_CONVERGED : -1;
}

// One sweep over the rows for the entries [e0, e0 + ACC / KP): the posteriors (`first`: the initial assignment), chunk 0's lnL, H and n_k, the chunk's moments into w.mom.
template <int KP, int ACC, class Ex>
PLSPM_HD void fimix_sweep(Ex& ex, const FimixDesc& d, FimixWs& w, const double* Y, long N, int K, bool first, const unsigned char* init, uint64_t seed, uint64_t start, int e0) {
    constexpr int CE = ACC / KP;
    const int L = d.L, T = ex.nthreads();
    double acc[KP][CE], nk[KP], lnl = 0.0, hs = 0.0;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        nk[k] = 0.0;
#pragma unroll
        for (int c = 0; c < CE; ++c) acc[k][c] = 0.0;
    }
    for (long i = ex.tid(); i < N; i += T) {
        const double* y = Y + i * L;
        double p[KP];
        if (first) {
            const int s = init ? (int)init[i] : fimix_start_segment(seed, start, (uint32_t)i, (uint32_t)K);
#pragma unroll
            for (int k = 0; k < KP; ++k) p[k] = k == s ? 1.0 : 0.0;
        } else {
            double lse;
            const double h = fimix_row<KP>(d, w, K, y, p, lse);
            lnl += lse; hs += h;
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) nk[k] += p[k];
#pragma unroll
        for (int c = 0; c < CE; ++c) {
            if (e0 + c < d.E) {         // (the same for every thread: the entry's two columns come from a scalar load)
                const int ent = d.ent[e0 + c];
                const double pr = y[ent & 0xffff] * y[ent >> 16];
#pragma unroll
                for (int k = 0; k < KP; ++k) acc[k][c] += p[k] * pr;
            }
        }
    }
    // the group's sums in the executor's fixed order: value q = entry c, segment k at c * KP + k; behind them n_k, lnL, sum P ln P
    int q = 0;
#pragma unroll
    for (int c = 0; c < CE; ++c) {
#pragma unroll
        for (int k = 0; k < KP; ++k) ex.put(w.red, q++, acc[k][c]);
    }
    if (e0 == 0) {
#pragma unroll
        for (int k = 0; k < KP; ++k) ex.put(w.red, q++, nk[k]);
        ex.put(w.red, q++, lnl);
        ex.put(w.red, q++, hs);
    }
    ex.sync();
    for (int v = ex.tid(); v < q; v += T) {
        const double sum = ex.get(w.red, v);
        if (v < ACC) {
            const int c = v / KP, k = v - c * KP;
            if (e0 + c < d.E && k < K) {
                const int ent = d.ent[e0 + c], a = ent & 0xffff, b = ent >> 16;
                double* M = w.mom + (long)k * L * L;
                M[a * L + b] = sum; M[b * L + a] = sum;
            }
        } else if (v < ACC + KP) { if (v - ACC < K) w.nk[v - ACC] = sum; }
        else if (v == ACC + KP) w.scal[0] = sum;
        else w.scal[1] = -sum;
    }
    ex.sync();
}

template <int KP, int ACC, class Ex>
PLSPM_HD void fimix_run(Ex& ex, const FimixDesc& d, FimixWs& w, const double* Y, long N, int K, int Kmax, const unsigned char* init, uint64_t seed, uint64_t start, int max_iter,
                        double tol, double* rec, int* status, int* iters) {
    constexpr int CE = ACC / KP;
    const int tid = ex.tid(), T = ex.nthreads(), W = fimix_record_width(Kmax, d.n_dir, d.n_endo), ntask = K * d.n_endo;
    // (the slots k >= K of the parameter tables are read, and masked, by the padded segments of the E-step: zero, not what the block held before)
    for (int c = tid; c < kFimixMaxK * (d.n_dir + 2 * d.n_endo + 3); c += T) w.beta[c] = 0.0;
    ex.sync();
    for (int e0 = 0; e0 < d.E; e0 += CE) fimix_sweep<KP, ACC>(ex, d, w, Y, N, K, true, init, seed, start, e0);
    int t = 1, st;
    for (;; ++t) {
        // M-step finish on the moments of the sweep before: the regressions across the threads, at most nslots at a time
        if (tid == 0) { bool empty = false; for (int k = 0; k < K; ++k) empty = empty || !(w.nk[k] >= 1.0); w.scal[3] = empty ? 1.0 : 0.0; }
        ex.sync();
        for (int base = 0; base < ntask; base += w.nslots) {
            const int task = base + tid;
            if (tid < w.nslots && task < ntask)
                if (!fimix_regress(d, w, task / d.n_endo, task % d.n_endo, w.slot + (long)tid * regression_scratch_doubles(d.kmax))) w.scal[3] = 1.0;
            ex.sync();
        }
        if (w.scal[3] != 0.0) { st = ST_SINGULAR; break; }
        for (int k = tid; k < K; k += T) w.cst[k] = fimix_const(d, w, k, N);
        if (tid == 0) w.scal[2] = w.scal[0];
        ex.sync();
        // E-step with theta^t and the moments for theta^(t+1): chunk 0 decides, the other chunks run only when the problem goes on
        fimix_sweep<KP, ACC>(ex, d, w, Y, N, K, false, init, seed, start, 0);
        st = fimix_stop(t, w.scal[0], w.scal[2], tol, max_iter);
        if (st >= 0) break;
        for (int e0 = CE; e0 < d.E; e0 += CE) fimix_sweep<KP, ACC>(ex, d, w, Y, N, K, false, init, seed, start, e0);
    }
    const bool values = st == ST_OK || st == ST_NOT_CONVERGED;
    const double nan = NAN;
    for (int c = tid; c < W; c += T) {
        double v = nan;
        if (values) {
            if (c < 2) v = w.scal[c];
            else if (c < 2 + Kmax) { const int k = c - 2; if (k < K) v = w.rho[k]; }
            else if (c < 2 + Kmax * (1 + d.n_dir)) {
                const int q = c - 2 - Kmax, k = q / d.n_dir, dp = q - k * d.n_dir;
                if (k < K) for (int e = 0; e < d.n_dir; ++e) if (d.dir_of[e] == dp) v = w.beta[e * kFimixMaxK + k];
            } else { const int q = c - 2 - Kmax * (1 + d.n_dir), k = q / d.n_endo; if (k < K) v = w.psi[(q - k * d.n_endo) * kFimixMaxK + k]; }
        }
        rec[c] = v;
    }
    if (tid == 0) { rec[W] = (double)st; rec[W + 1] = (double)t; if (status) *status = st; if (iters) *iters = t; }
}

// One whole problem.  ACC: a thread's accumulators (a multiple of 16; fimix_route.h kFimixAcc).
template <int ACC, class Ex>
PLSPM_HD void fimix_problem(Ex& ex, const FimixDesc& d, FimixWs& w, const double* Y, long N, int K, int Kmax, const unsigned char* init, uint64_t seed, uint64_t start, int max_iter,
                            double tol, double* rec, int* status, int* iters) {
    switch (fimix_kpad(K)) {
        case 1: fimix_run<1, ACC>(ex, d, w, Y, N, K, Kmax, init, seed, start, max_iter, tol, rec, status, iters); break;
        case 2: fimix_run<2, ACC>(ex, d, w, Y, N, K, Kmax, init, seed, start, max_iter, tol, rec, status, iters); break;
        case 4: fimix_run<4, ACC>(ex, d, w, Y, N, K, Kmax, init, seed, start, max_iter, tol, rec, status, iters); break;
        case 8: fimix_run<8, ACC>(ex, d, w, Y, N, K, Kmax, init, seed, start, max_iter, tol, rec, status, iters); break;
        default: fimix_run<16, ACC>(ex, d, w, Y, N, K, Kmax, init, seed, start, max_iter, tol, rec, status, iters); break;
    }
}

// the executor of one host thread (tests/fimix_host): every row in ascending order
struct FimixSerialExec {
    int tid() const { return 0; }
    int nthreads() const { return 1; }
    void sync() {}
    void put(double* red, int q, double v) { red[q] = v; }
    double get(const double* red, int q) const { return red[q]; }
};

}  // namespace plspm
