// modelfit_core.h -- model fit (SRMR, d_ULS of the saturated and of the estimated model): the portable part of a model-fit record -- the
// model-implied construct correlations and the residual of one indicator pair -- that the device kernel (kernels_modelfit.h, one wave per problem) and a
// stand-alone host program (tests/modelfit_host) both run.
//
// Inputs of one problem, all from its PLSc record (plsc_core.h): the loadings lambda*_p (a factor's corrected, any other LV's the fit's), the construct
// correlations rc_ij and the direct effects beta_jm on the effect pairs; beside them the indicator correlations r_pq of its data set and the factor mask.
//     Phi^ (estimated model), LVs in path order (every predecessor of j lies before j):
//              Phi^_jj = 1
//              j, k without predecessors:                 Phi^_jk = rc_jk
//              j with predecessors, every k < j:          Phi^_jk = sum_{m in pred(j)} beta_jm Phi^_mk, in ascending j: the structural residual of j is
//                                                         uncorrelated with everything before it
//              j without, an earlier k with predecessors: Phi^_jk = sum_{m in pred(k)} beta_km Phi^_jm, in ascending k: the residual of k is uncorrelated
//                                                         with an exogenous LV behind it as well
//     Phi  (saturated model) = rc
//     sigma^_pq(Phi), p != q:  blocks i != j: lambda*_p Phi_ij lambda*_q;  one block, a factor: lambda*_p lambda*_q;  one block, a composite: r_pq itself
//     d_uls = sum_{p<q} (r_pq - sigma^_pq)^2,  srmr = sqrt(2 d_uls / (P (P + 1)))
// Model-fit record, width 4:  srmr_sat | d_uls_sat | srmr_est | d_uls_est, then status and iterations as doubles.  Status: the PLSc record's; ST_INADMISSIBLE
// (NaN in all four) where that record is, where a column is constant in the data set, and where a value is not finite.
//
// Execution model: plsc_core.h's.  Phi^ shares one L x L square with beta: Phi^_jk (j > k) below the diagonal, beta_jm (m < j) at [m][j] above it.
#pragma once
#include "plsc_core.h"

namespace plspm {

constexpr int MODELFIT_WIDTH = 4;

// one problem's workspace: 1 / s, mu, lambda* [P each] | rc, Phi^ with beta [L x L each] | scal [8]
struct ModelfitWs { double *isd, *mu, *lam, *rc, *ph, *scal; };
PLSPM_HD long modelfit_ws_doubles(int P, int L) { return 3L * P + 2L * L * L + 8; }
PLSPM_HD void modelfit_carve(ModelfitWs& w, double* base, int P, int L) {
    w.isd = base; w.mu = w.isd + P; w.lam = w.mu + P; w.rc = w.lam + P; w.ph = w.rc + (long)L * L; w.scal = w.ph + (long)L * L;
}

PLSPM_HD double modelfit_phi_at(const double* ph, int L, int a, int b) { return a == b ? 1.0 : ph[(a > b ? a : b) * L + (a > b ? b : a)]; }

// lv_cor_c [npairs] (i < j, i-major) and direct [n_eff] of the PLSc record -> w.rc (full, symmetric) and w.ph (see above)
template <class Ex>
PLSPM_HD void modelfit_phi(Ex& ex, const ModelDesc& md, ModelfitWs& w, const double* lv_cor_c, const double* direct) {
    const int L = md.L;
    ex.par(L * L, [&](int e) {
        const int i = e / L, j = e - i * L;
        double rc = 1.0, ph = 1.0;
        if (i != j) {
            const int a = i < j ? i : j, b = i < j ? j : i;
            rc = lv_cor_c[(long)a * L - (long)a * (a + 1) / 2 + (b - a - 1)];
            ph = (i > j && md.pred_off[i + 1] == md.pred_off[i] && md.pred_off[j + 1] == md.pred_off[j]) ? rc : 0.0;
        }
        w.rc[e] = rc; w.ph[e] = ph;
    });
    ex.par(md.n_eff, [&](int e) { if (md.eff_from[e] < md.eff_to[e]) w.ph[md.eff_from[e] * L + md.eff_to[e]] = direct[e]; });
    bool endogenous_before = false;
    for (int j = 0; j < L; ++j) {
        const int o = md.pred_off[j], nk = md.pred_off[j + 1] - o;
        if (nk > 0) {
            ex.par(j, [&](int k) {
                double s = 0.0;
                for (int r = 0; r < nk; ++r) { const int m = md.pred_idx[o + r]; s = fma(w.ph[m * L + j], modelfit_phi_at(w.ph, L, m, k), s); }
                w.ph[j * L + k] = s;
            });
            endogenous_before = true;
        } else if (endogenous_before) {                      // an exogenous LV behind an endogenous one: its row needs its own earlier entries
            ex.one([&]() {
                for (int k = 0; k < j; ++k) {
                    const int ok = md.pred_off[k], nkk = md.pred_off[k + 1] - ok;
                    if (!nkk) continue;
                    double s = 0.0;
                    for (int r = 0; r < nkk; ++r) { const int m = md.pred_idx[ok + r]; s = fma(w.ph[m * L + k], w.ph[j * L + m], s); }
                    w.ph[j * L + k] = s;
                }
            });
        }
    }
}

// the squared residuals of the pair p < q (LVs lp <= lq, loadings lam_p, lam_q, correlation r) onto the two running sums
PLSPM_HD void modelfit_residual(const ModelfitWs& w, const unsigned char* factor, int L, int lp, int lq, double lam_p, double lam_q, double r, double& sat, double& est) {
    const double ll = lam_p * lam_q;
    if (lp == lq) {
        if (!factor[lp]) return;                             // a composite reproduces its own block
        const double d = r - ll;
        sat = fma(d, d, sat); est = fma(d, d, est);
        return;
    }
    const int e = lq * L + lp;
    const double ds = fma(-ll, w.rc[e], r), de = fma(-ll, w.ph[e], r);
    sat = fma(ds, ds, sat); est = fma(de, de, est);
}

// the record from the two sums; `constant`: a column of the data set is constant; plsc_status, iterations: the PLSc record's
PLSPM_HD void modelfit_store(int P, double sat, double est, bool constant, double plsc_status, double iterations, double* out) {
    const double f = 2.0 / ((double)P * (P + 1));
    double v[MODELFIT_WIDTH] = {sqrt(f * sat), sat, sqrt(f * est), est};
    double st = plsc_status;
    if (constant || !(isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]))) {
        st = (double)ST_INADMISSIBLE;
        for (int c = 0; c < MODELFIT_WIDTH; ++c) v[c] = sqrt(-1.0);
    }
    for (int c = 0; c < MODELFIT_WIDTH; ++c) out[c] = v[c];
    out[MODELFIT_WIDTH] = st; out[MODELFIT_WIDTH + 1] = iterations;
}

}  // namespace plspm
