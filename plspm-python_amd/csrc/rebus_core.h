// rebus_core.h -- the arithmetic of REBUS-PLS that the device kernels (kernels_rebus.h) and the host program of the tests (tests/rebus_host) share:
// the layout of one class's parameters, rebus_compose (a class's record and moments -> the affine maps of the row pass and its validity), rebus_row (one row under
// one class: A, B and every residual), the closeness measure and the assignment rule.  Portable C++: no HIP runtime; the executor says how the lanes of a wave share
// the loops (device: 64 lanes, butterfly sums; host: one lane).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define RB_HD __host__ __device__ __forceinline__
#else
#define RB_HD inline
#endif

namespace plspm {

constexpr double kRebusCollapse = 1e-10;       // a squared loading or an R^2 must lie above it (plspm.fimix.COLLAPSE_RTOL on quantities in [0, 1])

// What the compose step reads of the model.  Record: weights [P] | r2 [L] | total [n_eff] | direct [n_eff] | loadings [P] (device column order).
struct RebusModel {
    int P, L, n_endo, n_eff, scaled;
    const int* boff;          // [L + 1]
    const int* lvof;          // [P]
    const int* endo;          // [n_endo] the LVs that have predecessors, ascending
    const int* eff_of;        // [n_endo x L] the effect pair (record section `direct`) of path q -> endo[jj], -1 where the model has none
    const double* shift;      // [P] the upload's column shift: the resident value is x - shift
};

// One class's parameters, param_doubles = 5 P + L + n_endo (L + 1):
//   g [P]      y_l = c_l + sum_{p in l} g_p x'_p      (x' the resident value; g_p = s_l cs w_p, c_l = -sum g_p mean'_p)
//   a, b [P]   z_p = a_p x'_p + b_p                   (a = 1 / sd, b = -mean' / sd)
//   lam [P]    e_p = z_p - lam_p y_lv(p)
//   il2 [P]    1 / lam_p^2
//   c [L]
//   Bm [n_endo x L]  f_jj = y_endo[jj] - sum_q Bm[jj][q] y_q   (zero where the model has no path)
//   ir2 [n_endo]     1 / R^2
RB_HD int rebus_param_doubles(int P, int L, int n_endo) { return 5 * P + L + n_endo * (L + 1); }
template <class T> struct RebusParamsT { T *g, *a, *b, *lam, *il2, *c, *Bm, *ir2; };
template <class T> RB_HD RebusParamsT<T> rebus_params(T* base, int P, int L, int n_endo) {
    RebusParamsT<T> r;
    r.g = base; r.a = r.g + P; r.b = r.a + P; r.lam = r.b + P; r.il2 = r.lam + P; r.c = r.il2 + P; r.Bm = r.c + L; r.ir2 = r.Bm + n_endo * L;
    return r;
}

// the host's executor: one lane
struct RebusSerialExec {
    int lane() const { return 0; }
    int lanes() const { return 1; }
    double sum(double v) const { return v; }
    int any(int v) const { return v; }
    void sync() const {}
};

// One class: record `rec`, solver status, its rows' count n and the sums S1 [P] = sum x', S2 [P] = sum x'^2 of the resident columns -> params; work [2 P + L] is
// scratch all lanes see (mean' | sd | sign).  Returns 1 when the class is valid: status OK, every sd > 0, every squared loading and every R^2 of an LV with
// predecessors above kRebusCollapse; else 0 with NaN parameters.  The score rule is plspm_cv_predict's: class means, the class's `scaled` scalar, the record's
// weights and the sign s_l of sum_p w_p loading_p sd_p.
template <class Ex> RB_HD int rebus_compose(Ex& ex, const RebusModel& md, const double* rec, int status, double n, const double* S1, const double* S2, double* params, double* work) {
    const int P = md.P, L = md.L, ne = md.n_endo, lane = ex.lane(), nl = ex.lanes();
    const double* wgt = rec;
    const double* r2 = rec + P;
    const double* direct = rec + P + L + md.n_eff;
    const double* load = direct + md.n_eff;
    double* mean = work;
    double* sd = work + P;
    double* sgn = work + 2 * P;
    RebusParamsT<double> pr = rebus_params(params, P, L, ne);
    const double inv_n = 1.0 / n;
    int bad = (status != 0 || !(n >= 1.0)) ? 1 : 0;
    double tot = 0.0;
    for (int p = lane; p < P; p += nl) {
        const double mu = S1[p], var = S2[p] - (mu * mu) * inv_n;
        mean[p] = mu * inv_n;
        sd[p] = sqrt((var > 0.0 ? var : 0.0) * inv_n);
        if (!(sd[p] > 0.0)) bad = 1;
        tot += mu + n * md.shift[p];
    }
    double cs = 1.0;
    if (md.scaled) {
        // g = std1(all n P raw values of the class) * sqrt((n - 1) / n), around the grand mean (solver_core.h moments_to_cov)
        tot = ex.sum(tot);
        const double np_ = n * (double)P, grand = tot / np_;
        double ss = 0.0;
        for (int p = lane; p < P; p += nl) {
            const double d = md.shift[p] - grand;
            ss += S2[p] + 2.0 * d * S1[p] + n * d * d;
        }
        ss = ex.sum(ss);
        cs = 1.0 / sqrt(ss / (np_ - 1.0) * ((n - 1.0) / n));
    }
    ex.sync();
    for (int l = lane; l < L; l += nl) {
        double s = 0.0, cm = 0.0;
        for (int p = md.boff[l]; p < md.boff[l + 1]; ++p) { s += wgt[p] * load[p] * sd[p]; cm += wgt[p] * mean[p]; }
        sgn[l] = s < 0.0 ? -1.0 : 1.0;
        pr.c[l] = -(sgn[l] * cs) * cm;
    }
    ex.sync();
    for (int p = lane; p < P; p += nl) {
        const double l2 = load[p] * load[p];
        if (!(l2 > kRebusCollapse)) bad = 1;
        pr.g[p] = (sgn[md.lvof[p]] * cs) * wgt[p];
        pr.a[p] = 1.0 / sd[p];
        pr.b[p] = -mean[p] / sd[p];
        pr.lam[p] = load[p];
        pr.il2[p] = 1.0 / l2;
    }
    for (int e = lane; e < ne * L; e += nl) pr.Bm[e] = md.eff_of[e] >= 0 ? direct[md.eff_of[e]] : 0.0;
    for (int jj = lane; jj < ne; jj += nl) {
        const double r = r2[md.endo[jj]];
        if (!(r > kRebusCollapse)) bad = 1;
        pr.ir2[jj] = 1.0 / r;
    }
    bad = ex.any(bad);
    ex.sync();
    if (bad) {
        const double nan = NAN;
        const int PD = rebus_param_doubles(P, L, ne);
        for (int e = lane; e < PD; e += nl) params[e] = nan;
    }
    return bad ? 0 : 1;
}

// One row under one class.  x(p): the row's resident value of column p; y(l): a slot of the caller's for the score of LV l (read back after it is written);
// emit(idx, v): every residual as it is formed -- idx p < P: e_p, idx P + jj: f_jj.  A = sum_p e_p^2 / lam_p^2, B = sum_jj f_jj^2 / R^2_jj, each in index order.
template <class XF, class YF, class EF>
RB_HD void rebus_row(int P, int L, int n_endo, const int* boff, const int* endo, const RebusParamsT<const double>& pr, XF x, YF y, EF emit, double& A, double& B) {
    double a_sum = 0.0;
    for (int l = 0; l < L; ++l) {
        const int p0 = boff[l], p1 = boff[l + 1];
        double s = pr.c[l];
        for (int p = p0; p < p1; ++p) s = fma(pr.g[p], x(p), s);
        y(l) = s;
        for (int p = p0; p < p1; ++p) {
            const double e = fma(pr.a[p], x(p), pr.b[p]) - pr.lam[p] * s;
            emit(p, e);
            a_sum = fma(e * e, pr.il2[p], a_sum);
        }
    }
    double b_sum = 0.0;
    for (int jj = 0; jj < n_endo; ++jj) {
        const double* bm = pr.Bm + jj * L;
        double hat = 0.0;
        for (int q = 0; q < L; ++q) hat = fma(bm[q], y(q), hat);
        const double f = y(endo[jj]) - hat;
        emit(P + jj, f);
        b_sum = fma(f * f, pr.ir2[jj], b_sum);
    }
    A = a_sum; B = b_sum;
}

// CM_ik from the row's A, B and the class's totals over all N rows
RB_HD double rebus_cm(double A, double B, double SA, double SB, double N) {
    const double d = N - 2.0;
    return sqrt((A / (SA / d)) * (B / (SB / d)));
}
// argmin over k of cm[k * stride]: ties to the lowest k, a NaN never wins; a row whose every CM is NaN keeps `old`
RB_HD int rebus_argmin(const double* cm, long stride, int K, int old) {
    int best = -1;
    double bv = 0.0;
    for (int k = 0; k < K; ++k) {
        const double v = cm[k * stride];
        if (v == v && (best < 0 || v < bv)) { best = k; bv = v; }
    }
    return best < 0 ? old : best;
}

}  // namespace plspm
