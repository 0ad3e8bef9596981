// plsc_core.h -- consistent PLS (PLSc; Dijkstra & Henseler 2015): everything of a PLSc record behind the per-MV step, as ONE portable
// function the device kernel (kernels_plsc.h, one wave per problem) and a stand-alone host program (tests/plsc_host) both run.
//
// Inputs of one problem, all from the assessment of its data set (kernels_assess.h): the standardised weights v_p = w_p s_p as the record has them (not yet
// normalised), per LV the sign sigma_l of the fit, t_l = v_l' R_ll v_l and g_l = v_l' v_l, the record's rho_a [L] and signed construct correlations lv_cor
// [npairs] (i < j, i-major), and the factor mask.
//     Q_l      rho_a[l] for a factor, 1 otherwise
//     rc_ij    lv_cor_ij / sqrt(Q_i Q_j)  (i != j),  rc_ii = 1
//     inner model: solver_core.h inner_model_effects on rc in place of the score covariance -- per endogenous LV the normal equations on its predecessors
//              (pivot rule PLSPM_PIVOT_RTOL, fallback jacobi_pinv), R2_j = beta' rc_pj, indirect effects by forward substitution, total = direct + indirect
//     loadings of a factor l:  sigma_l (v_p / sqrt(t_l)) sqrt(Q_l) / (g_l / t_l) = sigma_l v_p sqrt(Q_l t_l) / g_l  (Dijkstra-Henseler's c w on the normalised v);
//              of any other LV: the record's.  Weights: the record's.
// PLSc record, width W = R + npairs:  weights[P] | r2[L] | total[n_eff] | direct[n_eff] | loadings[P] | lv_cor_c[npairs], then status and iterations as doubles.
// Status: ST_INADMISSIBLE (NaN in all W values) when a factor's rho_a is not finite or <= 0, or some |rc_ij| is not below 1 (a NaN included);
// ST_SINGULAR when a regression fails in the shared routine, ST_NONFINITE when an R2 is not finite -- the values stand, as in the solver.
//
// Execution model: solver_core.h's -- `ex.par(n, f)` spreads indices over the group and ends with the group's hand-over, `ex.one(f)` runs f once,
// `ex.any(n, f)` is a group-wide OR every member receives.  Whatever crosses members lives in the workspace.
#pragma once
#include "solver_core.h"

namespace plspm {

enum { ST_INADMISSIBLE = 4 };

// one problem's workspace: v [P] | rc, B, (I - B)^-1, indirect [L x L each] | r2, Q, loading factor [L each] | scal [8] | regression scratch
struct PlscWs {
    double* v;
    Workspace ws;          // Cs, Bm, Pw, Ind, r2, scal, scr: what inner_model_effects touches (everything else stays null)
    double *q, *cl;
};
PLSPM_HD long plsc_ws_doubles(int P, int L, int kmax) { return (long)P + 4L * L * L + 3L * L + 8 + (long)L * regression_scratch_doubles(kmax); }
PLSPM_HD void plsc_carve(PlscWs& w, double* base, int P, int L, int kmax) {
    double* p = base;
    w.ws = Workspace{};
    w.v = p; p += P;
    w.ws.Cs = p; p += L * L; w.ws.Bm = p; p += L * L; w.ws.Pw = p; p += L * L; w.ws.Ind = p; p += L * L;
    w.ws.r2 = p; p += L; w.q = p; p += L; w.cl = p; p += L;
    w.ws.scal = p; p += 8;
    w.ws.scr = p;
}

// side [3 L]: sigma | v'Rv | v'v per LV (kernels_assess.h AssessArgs::side);  rec: the bootstrap record (pitch R + 2);  out: the PLSc record (pitch R + npairs + 2)
template <class Ex>
PLSPM_HD void plsc_record(Ex& ex, const ModelDesc& md, PlscWs& w, const unsigned char* factor, const double* rho_a, const double* lv_cor, const double* side,
                          const double* rec, int R, double* out) {
    const int P = md.P, L = md.L, npairs = L * (L - 1) / 2, W = R + npairs;
    Workspace& ws = w.ws;
    ex.one([&]() { ws.scal[3] = (double)ST_OK; ws.scal[4] = 0.0; });
    ex.par(L, [&](int l) {
        const bool fac = factor[l] != 0;
        const double Q = fac ? rho_a[l] : 1.0;
        if (!(Q > 0.0 && isfinite(Q))) ws.scal[4] = 1.0;
        w.q[l] = Q;
        w.cl[l] = side[l] * sqrt(Q * side[L + l]) / side[2 * L + l];
    });
    ex.par(L * L, [&](int e) {
        const int i = e / L, j = e - i * L;
        double rc = 1.0;
        if (i != j) {
            const int a = i < j ? i : j, b = i < j ? j : i;
            rc = lv_cor[(long)a * L - (long)a * (a + 1) / 2 + (b - a - 1)] / sqrt(w.q[a] * w.q[b]);
            if (!(fabs(rc) < 1.0)) ws.scal[4] = 1.0;
        }
        ws.Cs[e] = rc;
    });
    ex.mark(10);
    if (ws.scal[4] != 0.0) {                                   // (every member reads the same word behind the hand-over)
        ex.par(W, [&](int c) { out[c] = sqrt(-1.0); });
        ex.one([&]() { out[W] = (double)ST_INADMISSIBLE; out[W + 1] = rec[R + 1]; });
        return;
    }
    inner_model_effects(ex, md, ws);
    ex.mark(11);
    ex.par(P, [&](int p) {
        const int l = md.lvof[p];
        out[p] = rec[p];
        out[R - P + p] = factor[l] ? w.cl[l] * w.v[p] : rec[R - P + p];
    });
    ex.par(L, [&](int l) { out[P + l] = ws.r2[l]; });
    ex.par(md.n_eff, [&](int e) {
        const int idx = md.eff_to[e] * L + md.eff_from[e];
        out[P + L + e] = ws.Bm[idx] + ws.Ind[idx]; out[P + L + md.n_eff + e] = ws.Bm[idx];
    });
    ex.par(L * L, [&](int e) {
        const int i = e / L, j = e - i * L;
        if (i < j) out[R + (long)i * L - (long)i * (i + 1) / 2 + (j - i - 1)] = ws.Cs[e];
    });
    const bool bad = ex.any(L, [&](int l) { return !isfinite(ws.r2[l]); });
    ex.one([&]() {
        int st = (int)ws.scal[3];
        if (st == ST_OK && bad) st = ST_NONFINITE;
        out[W] = (double)st; out[W + 1] = rec[R + 1];
    });
    ex.mark(12);
}

// the executor of one host thread (tests/plsc_host): every index in ascending order
struct PlscSerialExec {
    static constexpr int kcap = 8;
    void mark(int) {}
    template <class F> void par(int n, F f) { for (int i = 0; i < n; ++i) f(i); }
    template <class F> void one(F f) { f(); }
    template <class F> bool any(int n, F f) { bool hit = false; for (int i = 0; i < n; ++i) hit = f(i) || hit; return hit; }
};

}  // namespace plspm
