// geodesic_core.h -- the geodesic discrepancy d_G of the saturated and of the estimated model: the portable part of a geodesic record, which the
// device kernel (kernels_geodesic.h, one wave per problem) and a stand-alone host program (tests/geodesic_host) both run.
//
// Inputs of one problem: modelfit_core.h's (lambda*, rc, Phi^ with beta, the factor mask) and the indicator correlations r_pq of its data set.
//     Sigma^(Phi)   modelfit_core.h's implied matrix, entry by entry (geodesic_implied below)
//     d_G(Sigma^) = 1/2 sum_k (ln phi_k)^2,  phi_k the eigenvalues of R^-1 Sigma^ = those of the symmetric C = G^-1 Sigma^ G^-T,  R = G G' (Cholesky)
// Geodesic record, width 2:  d_g_sat | d_g_est, then status and iterations as doubles.  Status: the model-fit record's; ST_INADMISSIBLE (NaN in both) where a
// Cholesky pivot of R is not above GEODESIC_PIVOT_MIN, where an eigenvalue of either model is not positive, and where a value is not finite.
//
// Steps, on two packed lower triangles (entry (i, j <= i) at i (i + 1) / 2 + j) of the problem's workspace:
//     factor      R into triangle A, its Cholesky factor in place, column by column: one member per row of the column
//     reduce      Sigma^ into triangle B;  row i below the diagonal <- t_i = G11^-1 s_i on the leading i x i block (one member per row, nothing shared);  then
//                 the rows in ascending order:  c_i = (t_i - C11 g_i) / g_ii,  c_ii = (s_ii - g_i' (2 t_i - C11 g_i)) / g_ii^2  (C11: the rows before it)
//     tridiagonal Householder reflections, in place; a column whose entries below the subdiagonal are all zero needs none (C = I: every column)
//     eigenvalues bisection on Sturm counts with a pivot floor between Gershgorin bounds, one member per eigenvalue index: halved until the interval is two
//                 adjacent doubles (GEODESIC_HALVINGS at most), which depends on the matrix alone
//     sum         1/2 sum ln^2 in the executor's one order
//
// Execution model: plsc_core.h's, and `ex.sum(n, f)`: the sum of f(i) over the indices, in one fixed order of the executor's, which every member receives.
#pragma once
#include "modelfit_core.h"

namespace plspm {

constexpr int GEODESIC_WIDTH = 2;
constexpr double GEODESIC_PIVOT_MIN = 1e-12;       // R has a unit diagonal: a pivot is the share of an indicator's variance that the indicators before it leave
constexpr int GEODESIC_HALVINGS = 128;

// one problem's workspace: modelfit_core.h's | triangles A, B [P (P + 1) / 2 each] | d, e, v, w [P each]
struct GeodesicWs { ModelfitWs mf; double *A, *B, *d, *e, *v, *w; };
PLSPM_HD long geodesic_ws_doubles(int P, int L) { return modelfit_ws_doubles(P, L) + (long)P * (P + 1) + 4L * P; }
PLSPM_HD void geodesic_carve(GeodesicWs& w, double* base, int P, int L) {
    modelfit_carve(w.mf, base, P, L);
    const long n2 = (long)P * (P + 1) / 2;
    w.A = base + modelfit_ws_doubles(P, L); w.B = w.A + n2; w.d = w.B + n2; w.e = w.d + P; w.v = w.e + P; w.w = w.v + P;
}

PLSPM_HD int geodesic_tri(int i, int j) { return i * (i + 1) / 2 + j; }                                         // j <= i (a triangle fits a workgroup's LDS: P < 200)
// sum_{k = 0 .. n-1} T(r0 + t, r0 + k) x[k] of the symmetric T, k ascending: along row r0 + t up to its diagonal, down column r0 + t behind it -- one loop
// of n steps whatever t is, so that the members of a group walk it together
PLSPM_HD double geodesic_symdot(const double* __restrict__ T, int r0, int t, int n, const double* __restrict__ x) {
    int at = geodesic_tri(r0 + t, r0);
    double s = 0.0;
#pragma unroll 4
    for (int k = 0; k < n; ++k) {
        s = fma(T[at], x[k], s);
        at += k < t ? 1 : r0 + k + 1;                         // (row r of the triangle has r + 1 entries)
    }
    return s;
}

// sigma^_pq of the model whose construct correlations are the square `phi` (w.rc, or w.ph below its diagonal); corr(p, q): r_pq, asked for composites only
template <class Corr>
PLSPM_HD double geodesic_implied(const double* phi, const unsigned char* factor, int L, int p, int q, int lp, int lq, double lam_p, double lam_q, Corr corr) {
    if (p == q) return 1.0;
    if (lp == lq) return factor[lp] ? lam_p * lam_q : corr(p, q);
    return (lam_p * lam_q) * phi[(lp > lq ? lp : lq) * L + (lp > lq ? lq : lp)];
}

// T (p, q <= p) <- f(p, q): column by column, the members along a column (a row of the Gram's upper triangle)
template <class Ex, class F>
PLSPM_HD void geodesic_fill(Ex& ex, double* T, int P, F f) {
    for (int q = 0; q < P; ++q) ex.par(P - q, [&](int t) { T[geodesic_tri(q + t, q)] = f(q + t, q); });
}

// A <- its Cholesky factor; false (every member) at the first pivot that is not above GEODESIC_PIVOT_MIN
template <class Ex>
PLSPM_HD bool geodesic_cholesky(Ex& ex, double* A, int P) {
    for (int j = 0; j < P; ++j) {
        const double* gj = A + geodesic_tri(j, 0);
        ex.par(P - j, [&](int t) {
            double* gi = A + geodesic_tri(j + t, 0);
            double s = gi[j];
#pragma unroll 4
            for (int k = 0; k < j; ++k) s = fma(-gi[k], gj[k], s);
            gi[j] = s;
        });
        const double pivot = gj[j];                           // (every member reads the same word behind the hand-over)
        if (!(pivot > GEODESIC_PIVOT_MIN)) return false;
        const double g = sqrt(pivot);
        ex.par(P - j, [&](int t) { double* x = A + geodesic_tri(j + t, j); *x = t ? *x / g : g; });
    }
    return true;
}

// B <- G^-1 B G^-T
template <class Ex>
PLSPM_HD void geodesic_reduce(Ex& ex, const double* G, double* B, int P) {
    ex.par(P, [&](int i) {
        double* row = B + geodesic_tri(i, 0);
        for (int k = 0; k < i; ++k) {
            const double* gk = G + geodesic_tri(k, 0);
            double s = row[k];
#pragma unroll 4
            for (int j = 0; j < k; ++j) s = fma(-gk[j], row[j], s);
            row[k] = s / gk[k];
        }
    });
    for (int i = 0; i < P; ++i) {
        const double* g = G + geodesic_tri(i, 0);
        double* row = B + geodesic_tri(i, 0);
        const double gam = g[i];
        const double s = ex.sum(i, [&](int j) {
            const double u = geodesic_symdot(B, 0, j, i, g);
            const double t = row[j];
            row[j] = (t - u) / gam;
            return g[j] * (2.0 * t - u);
        });
        ex.one([&]() { row[i] = (row[i] - s) / (gam * gam); });
    }
}

// B -> the diagonal d [P] and the subdiagonal e [P] (e_k couples k and k + 1; e_{P-1} = 0) of a tridiagonal matrix with B's eigenvalues; v, w [P]: scratch
template <class Ex>
PLSPM_HD void geodesic_tridiagonal(Ex& ex, double* B, int P, double* d, double* e, double* v, double* w) {
    for (int k = 0; k + 2 < P; ++k) {
        const int m = P - k - 1, r0 = k + 1;                  // x = B[r0 .. P-1][k]; the trailing block starts at (r0, r0)
        const double x0 = B[geodesic_tri(r0, k)];
        const double tail = ex.sum(m - 1, [&](int t) { const double x = B[geodesic_tri(r0 + 1 + t, k)]; return x * x; });
        if (tail == 0.0) {                                    // nothing below the subdiagonal: no reflection (and no 0 / 0 for a column of zeros)
            ex.one([&]() { e[k] = x0; });
            continue;
        }
        // No rescaling of the column (LAPACK dlarfg rescales): the entries of C are those of a correlation matrix reduced by a factor whose pivots are above
        // 1e-12, so a column that is not zero has squares between about 1e-34 (rounding residue of C = I) and 1e24 -- far from the 1e-308 at which sigma would
        // be a denormal and tau overflow.  A column out of that range would give NaN, and with it an inadmissible record, not a wrong value.
        const double sigma = fma(x0, x0, tail), nrm = sqrt(sigma), alpha = x0 > 0.0 ? -nrm : nrm;
        const double tau = 1.0 / (sigma - alpha * x0);        // 2 / v'v with v = x - alpha e_1: sigma + |x0| nrm > 0
        ex.par(m, [&](int t) { v[t] = B[geodesic_tri(r0 + t, k)] - (t ? 0.0 : alpha); });
        ex.par(m, [&](int t) { w[t] = tau * geodesic_symdot(B, r0, t, m, v); });
        const double half = 0.5 * tau * ex.sum(m, [&](int t) { return w[t] * v[t]; });
        ex.par(m, [&](int t) { w[t] = fma(-half, v[t], w[t]); });
        ex.par(m, [&](int t) {                                // the trailing block <- itself - v w' - w v': one member per row
            double* __restrict__ row = B + geodesic_tri(r0 + t, r0);
            const double* __restrict__ vv = v;
            const double* __restrict__ ww = w;
            const double vt = vv[t], wt = ww[t];
            int u = 0;
            for (; u + 4 <= t + 1; u += 4) {                  // (four entries' loads before the first store: a store keeps later loads behind it)
                const double w0 = ww[u], w1 = ww[u + 1], w2 = ww[u + 2], w3 = ww[u + 3], v0 = vv[u], v1 = vv[u + 1], v2 = vv[u + 2], v3 = vv[u + 3];
                const double a0 = row[u], a1 = row[u + 1], a2 = row[u + 2], a3 = row[u + 3];
                row[u] = fma(-vt, w0, fma(-wt, v0, a0)); row[u + 1] = fma(-vt, w1, fma(-wt, v1, a1));
                row[u + 2] = fma(-vt, w2, fma(-wt, v2, a2)); row[u + 3] = fma(-vt, w3, fma(-wt, v3, a3));
            }
            for (; u <= t; ++u) row[u] = fma(-vt, ww[u], fma(-wt, vv[u], row[u]));
        });
        ex.one([&]() { e[k] = alpha; });
    }
    ex.par(P, [&](int i) { d[i] = B[geodesic_tri(i, i)]; });
    ex.one([&]() {
        if (P >= 2) e[P - 2] = B[geodesic_tri(P - 1, P - 2)];
        e[P - 1] = 0.0;
    });
}

// the number of eigenvalues below x of the tridiagonal matrix (d, e2 the squared subdiagonal)
PLSPM_HD int geodesic_count(int P, const double* __restrict__ d, const double* __restrict__ e2, double x, double pivmin) {
    double q = d[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    int count = q < 0.0 ? 1 : 0;
#pragma unroll 4
    for (int i = 1; i < P; ++i) {
        q = d[i] - x - e2[i - 1] / q;
        if (fabs(q) < pivmin) q = -pivmin;
        count += q < 0.0 ? 1 : 0;
    }
    return count;
}

// (d, e) -> its eigenvalues in ascending order, lam [P]; e2 [P] takes the squares; scal [3]: the bounds and the pivot floor
template <class Ex>
PLSPM_HD void geodesic_eigenvalues(Ex& ex, int P, const double* d, const double* e, double* e2, double* lam, double* scal) {
    ex.one([&]() {
        double lo = d[0], hi = d[0], emax = 0.0;
        for (int i = 0; i < P; ++i) {
            const double r = (i ? fabs(e[i - 1]) : 0.0) + (i + 1 < P ? fabs(e[i]) : 0.0);
            lo = fmin(lo, d[i] - r); hi = fmax(hi, d[i] + r);
            emax = fmax(emax, e[i] * e[i]);
        }
        const double pivmin = 2.2250738585072014e-308 * fmax(1.0, emax);
        const double slack = 2.1 * 2.220446049250313e-16 * P * fmax(fabs(lo), fabs(hi)) + 4.2 * pivmin;
        scal[0] = lo - slack; scal[1] = hi + slack; scal[2] = pivmin;
    });
    ex.par(P, [&](int i) { e2[i] = e[i] * e[i]; });
    const double pivmin = scal[2];
    ex.par(P, [&](int k) {
        double lo = scal[0], hi = scal[1];
        for (int h = 0; h < GEODESIC_HALVINGS; ++h) {
            const double mid = lo + 0.5 * (hi - lo);
            // two adjacent doubles (or a bound that is not a number).  The members of a group leave at different counts; an eigenvalue smaller than about 2^-76 of the
            // interval's width stops at the cap instead, with an absolute error of 2^-128 of that width
            if (!(mid > lo && mid < hi)) break;
            if (geodesic_count(P, d, e2, mid, pivmin) <= k) lo = mid; else hi = mid;
        }
        lam[k] = lo + 0.5 * (hi - lo);
    });
}

// The record.  corr(p, q): r_pq of the data set (p != q); status, iterations: the model-fit record's; eig: null, or [2 P] for the eigenvalues of both models.
template <class Ex, class Corr>
PLSPM_HD void geodesic_record(Ex& ex, const ModelDesc& md, GeodesicWs& w, const unsigned char* factor, Corr corr, double status, double iterations, double* out, double* eig) {
    const int P = md.P, L = md.L;
    const double nan = sqrt(-1.0);
    geodesic_fill(ex, w.A, P, [&](int p, int q) { return p == q ? 1.0 : corr(p, q); });
    const bool definite = geodesic_cholesky(ex, w.A, P);
    ex.mark(2);
    double sat = nan, est = nan;
    bool bad = !definite;
    for (int model = 0; model < GEODESIC_WIDTH && definite; ++model) {
        const double* phi = model ? w.mf.ph : w.mf.rc;
        geodesic_fill(ex, w.B, P, [&](int p, int q) { return geodesic_implied(phi, factor, L, p, q, md.lvof[p], md.lvof[q], w.mf.lam[p], w.mf.lam[q], corr); });
        geodesic_reduce(ex, w.A, w.B, P);
        ex.mark(3 + 3 * model);
        geodesic_tridiagonal(ex, w.B, P, w.d, w.e, w.v, w.w);
        ex.mark(4 + 3 * model);
        geodesic_eigenvalues(ex, P, w.d, w.e, w.w, w.v, w.mf.scal);
        if (eig) ex.par(P, [&](int k) { eig[model * P + k] = w.v[k]; });
        bad = ex.any(P, [&](int k) { return !(w.v[k] > 0.0 && isfinite(w.v[k])); }) || bad;
        const double value = 0.5 * ex.sum(P, [&](int k) { const double l = log(w.v[k]); return l * l; });
        if (model) est = value; else sat = value;
        ex.mark(5 + 3 * model);
    }
    bad = bad || !(isfinite(sat) && isfinite(est));
    ex.one([&]() {
        out[0] = bad ? nan : sat; out[1] = bad ? nan : est;
        out[GEODESIC_WIDTH] = bad ? (double)ST_INADMISSIBLE : status; out[GEODESIC_WIDTH + 1] = iterations;
    });
    ex.mark(9);
}

// the executor of one host thread (tests/geodesic_host): every index, and every sum, in ascending order
struct GeodesicSerialExec : PlscSerialExec {
    template <class F> double sum(int n, F f) { double s = 0.0; for (int i = 0; i < n; ++i) s += f(i); return s; }
};

}  // namespace plspm
