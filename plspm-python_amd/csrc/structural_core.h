// structural_core.h -- structural-model assessment: the f2 effect size and the inner VIF of every direct path and every specific indirect
// effect of one data set, as ONE portable function the device kernel (kernels_structural.h, one wave per problem) and a stand-alone host program
// (tests/structural_host) both run.
//
// Inputs of one problem: the signed construct correlations lv_cor [npairs] (i < j, i-major) of its assessment record (kernels_assess.h) and its bootstrap
// record, of which the `direct` entries and the status are read.
//     rc          the L x L construct correlation matrix: lv_cor mirrored, rc_ii = 1
//     R2(j | S)   the R squared of regressing LV j on the LVs of the list S, on rc: solver_core.h spd_solve (pivot rule PLSPM_PIVOT_RTOL, fallback
//                 jacobi_pinv), R2 = beta' rc_Sj; exactly 0 for an empty S
//     per direct path i -> j, with S = pred(j) without i:
//       f2        (R2(j | pred(j)) - R2(j | S)) / (1 - R2(j | pred(j)))
//       vif       1 / (1 - R2(i | S))                                        (exactly 1 for an empty S)
//     per specific indirect effect, a chain i -> m_1 -> ... -> j with at least one mediator: the product of the record's `direct` entries along the chain,
//                 multiplied left to right
// Record, width S = 2 n_dir + n_spec:  f2[n_dir] | vif[n_dir] | specific[n_spec], then status and iterations as doubles.  Direct paths in the order of the
// effect pairs, chains by effect pair and then lexicographically by node sequence (the host enumerates them: StructDesc).
// Status: ST_SINGULAR when a regression fails in the shared routine, ST_NONFINITE when an f2 or vif is not finite (an R2 of 1) -- the values stand.
//
// Execution model: plsc_core.h's (`par` / `one`; no `any`: a lane that sees a non-finite value says so in the workspace), and `ex.slots(n, nslots, f)`: f(index, slot) over n indices of which at most nslots are in
// flight, each with a slot of regression scratch of its own; ends with the group's hand-over like par.
#pragma once
#include "solver_core.h"

namespace plspm {

// the direct paths and the chains of a model, built once on the host (plspm_structural_enable; tests/structural_host)
struct StructDesc {
    int n_dir, n_spec;
    const int* dir_from;        // [n_dir]
    const int* dir_to;          // [n_dir]
    const int* chain_off;       // [n_spec + 1] offsets into chain_eff / the node list
    const int* chain_eff;       // [chain_off[n_spec]] entry r of a chain (r < its nodes - 1): the effect pair of node r -> node r + 1; its last entry is unused
};

// per slot: the regression scratch and behind it the index list of a drop-one solve (at most kmax - 1 ints)
PLSPM_HD long structural_slot_doubles(int kmax) { return regression_scratch_doubles(kmax) + (kmax + 1) / 2; }
// one problem's workspace: rc [L x L] | r2 [L] | scal [8] | nslots slots
PLSPM_HD long structural_ws_doubles(int L, int kmax, int nslots) { return (long)L * L + L + 8 + (long)nslots * structural_slot_doubles(kmax); }

struct StructWs { double *rc, *r2, *scal, *slot; };
PLSPM_HD void structural_carve(StructWs& w, double* base, int L) {
    w.rc = base; w.r2 = base + (long)L * L; w.scal = w.r2 + L; w.slot = w.scal + 8;
}

// R2 of LV `col` on the k LVs of idx; x: k doubles, scratch: solver_core.h spd_solve's
template <int KCAP>
PLSPM_HD double structural_r2(const double* rc, int L, const int* idx, int k, int col, double* x, double* scratch, bool& ok) {
    if (k == 0) return 0.0;
    if (!spd_solve<KCAP>(rc, L, idx, k, col, x, scratch)) ok = false;
    double s = 0.0;
    for (int r = 0; r < k; ++r) s += x[r] * rc[idx[r] * L + col];
    return s;
}

// lv_cor: the assessment record's [npairs];  rec: the bootstrap record (pitch R + 2, direct at P + L + n_eff);  out: the structural record (pitch S + 2)
template <class Ex>
PLSPM_HD void structural_record(Ex& ex, const ModelDesc& md, const StructDesc& sd, StructWs& w, int nslots, const double* lv_cor, const double* rec, int R,
                                double* out) {
    const int L = md.L, km = md.kmax, n_dir = sd.n_dir, S = 2 * n_dir + sd.n_spec;
    const long slot_doubles = structural_slot_doubles(km);
    const double* direct = rec + md.P + L + md.n_eff;
    ex.one([&]() { w.scal[3] = (double)ST_OK; w.scal[4] = 0.0; });
    // one sweep builds rc and multiplies the chains: an index's load of lv_cor and its chain's loads (descriptor, then the record's direct entries) are
    // independent and in flight together
    ex.par(L * L > sd.n_spec ? L * L : sd.n_spec, [&](int e) {
        double v = 1.0;
        if (e < L * L) {
            const int i = e / L, j = e - i * L;
            if (i != j) {
                const int a = i < j ? i : j, b = i < j ? j : i;
                v = lv_cor[(long)a * L - (long)a * (a + 1) / 2 + (b - a - 1)];
            }
        }
        if (e < sd.n_spec) {
            const int e0 = sd.chain_off[e], e1 = sd.chain_off[e + 1] - 1;
            double prod = direct[sd.chain_eff[e0]];
            for (int r = e0 + 1; r < e1; ++r) prod *= direct[sd.chain_eff[r]];
            out[2 * n_dir + e] = prod;
        }
        if (e < L * L) w.rc[e] = v;
    });
    ex.mark(1);
    ex.slots(L, nslots, [&](int j, int slot) {
        double* scratch = w.slot + slot * slot_doubles;
        const int k = md.pred_off[j + 1] - md.pred_off[j];
        bool ok = true;
        w.r2[j] = structural_r2<Ex::kcap>(w.rc, L, md.pred_idx + md.pred_off[j], k, j, scratch + 2 * km * km, scratch, ok);
        if (!ok) w.scal[3] = (double)ST_SINGULAR;
    });
    ex.mark(2);
    ex.slots(n_dir, nslots, [&](int d, int slot) {
        double* scratch = w.slot + slot * slot_doubles;
        double* x = scratch + 2 * km * km;
        int* idx = (int*)(scratch + regression_scratch_doubles(km));
        const int i = sd.dir_from[d], j = sd.dir_to[d];
        int k = 0;
        for (int r = md.pred_off[j]; r < md.pred_off[j + 1]; ++r) if (md.pred_idx[r] != i) idx[k++] = md.pred_idx[r];
        bool ok = true;
        const double r2_j = structural_r2<Ex::kcap>(w.rc, L, idx, k, j, x, scratch, ok);
        const double r2_i = structural_r2<Ex::kcap>(w.rc, L, idx, k, i, x, scratch, ok);
        if (!ok) w.scal[3] = (double)ST_SINGULAR;
        const double full = w.r2[j];
        const double f2 = (full - r2_j) / (1.0 - full), vif = 1.0 / (1.0 - r2_i);
        if (!(isfinite(f2) && isfinite(vif))) w.scal[4] = 1.0;
        out[d] = f2;
        out[n_dir + d] = vif;
    });
    ex.mark(3);
    ex.one([&]() {
        int st = (int)w.scal[3];
        if (st == ST_OK && w.scal[4] != 0.0) st = ST_NONFINITE;
        out[S] = (double)st; out[S + 1] = rec[R + 1];
    });
    ex.mark(4);
}

// the executor of one host thread (tests/structural_host): every index in ascending order, one slot
struct StructSerialExec {
    static constexpr int kcap = 8;
    void mark(int) {}
    template <class F> void par(int n, F f) { for (int i = 0; i < n; ++i) f(i); }
    template <class F> void slots(int n, int, F f) { for (int i = 0; i < n; ++i) f(i, 0); }
    template <class F> void one(F f) { f(); }
};

}  // namespace plspm
