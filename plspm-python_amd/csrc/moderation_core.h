// moderation_core.h -- moderation analysis by the two-stage approach: the interaction terms of a model, the weighted row sums a term needs, the
// plan of a call, and the second stage of ONE data set -- the extended correlation matrix of the stage-1 scores and their products, the regressions and the
// record -- as one portable function the device kernel (kernels_moderation.h moderation_finish_kernel, one wave per replicate) and a stand-alone host program
// (tests/moderation_host) both run.  Free of the HIP runtime.
//
// A term t is (a, b, j): predictor LV a, moderator LV b, target LV j; a -> j and b -> j are paths of the model.  With the stage-1 scores y_l of a data set
// (mean 0, variance 1: plspm.quality's v, normalised per block, and its sign rule) and the product z_t = y_a y_b, not centred and not rescaled:
//     needed LVs   the union over the terms of pred(j) and j, ascending: the scores the row pass forms
//     sums of t    sum c z_t | sum c z_t^2 | sum c z_t y_l for l in pred(j) in LV order | sum c z_t y_j, c the row's multiplicity; behind the sums of every term:
//                  sum c z_t z_u for the terms t < u of one target, by (t, u)
//     m_t, s_t     mean sum c z_t / n and standard deviation sqrt(sum c z_t^2 / n - m_t^2) of the product -- zero unless the variance exceeds 1e-9 of the
//                  second moment (the rule of solver_core.h treated_sd), so that a constant product divides by zero and is reported, not a number made of noise
//     correlations LV x LV from the moments (rc, the assessment's lv_cor, as the prepare kernel forms it); cor(z_t, y_l) = (sum c z_t y_l / n) / s_t;
//                  cor(z_t, z_u) = (sum c z_t z_u / n - m_t m_u) / (s_t s_u)
//     per target j that has terms: j on pred(j) in LV order, then on its terms in term order, on that matrix by solver_core.h spd_solve; R2 = beta' r;
//                  f2_t = (R2 - R2 without term t) / (1 - R2)
// Record, width W = n_dir + 4 T + L:  direct2[n_dir] | interaction[T] | f2[T] | slope_low[T] | slope_high[T] | r2[L], then status and iterations as doubles.
// direct2 in the order of plspm_structural_paths; a target without terms keeps the bootstrap record's direct and r2 entries, bit for bit.
// Status: ST_SINGULAR when a regression fails in the shared routine, ST_NONFINITE when a value is not finite -- the values stand.
#pragma once
#include <algorithm>
#include <string>
#include <vector>
#include "solver_core.h"
#include "solver_route.h"         // kMaxLds

namespace plspm {

constexpr int kModMaxTerms = 8;
constexpr int kModMaxSums = 128;           // accumulators a lane of the row pass keeps in registers
constexpr long kModMaxRows = 65535;        // rows of one LDS histogram of 16-bit counters (batch_route.h kLdsHistRows)
constexpr int kModRowsWaves = 4;           // waves of a workgroup of the row pass: one row block each
constexpr int kModPrepareWaves = 4;

// the integer lists of a model's terms, one blob (host: moderation_build; device: the same ints)
enum ModList {
    MO_TERM_A, MO_TERM_B, MO_TERM_J,       // [T] LVs of a term
    MO_TERM_SA, MO_TERM_SB,                // [T] the needed-LV slots of a and b
    MO_TERM_DIR,                           // [T] the direct path a -> j
    MO_NEED,                               // [nl] the needed LVs, ascending
    MO_SLOT,                               // [L] needed-LV slot of an LV, -1: not needed
    MO_COEF_OFF,                           // [nl + 1] first coefficient of a needed LV
    MO_COEF_COL,                           // [ncoef] device column of a coefficient
    MO_COEF_LV,                            // [ncoef] its needed-LV slot
    MO_SUM_A, MO_SUM_B,                    // [nsums] the two values a sum multiplies: 0 the constant one, 1 + slot a score, 1 + nl + t a product
    MO_SUM_AB,                             // [nsums] the same as one word for the row pass: 64 a | 64 b << 16 (the values' places in a wave's LDS rows)
    MO_SUM_BASE,                           // [T] first sum of a term
    MO_CROSS,                              // [T x T] the sum z_t z_u (t < u, one target), -1: none
    MO_TGT,                                // [ntgt] the targets that have terms, ascending
    MO_TGT_OFF,                            // [ntgt + 1] into MO_TGT_TERMS
    MO_TGT_TERMS,                          // [T] the terms by target, in term order
    MO_TGT_JOB,                            // [ntgt] the target's first job: its full regression; job + 1 + q drops its q-th term
    MO_TGT_E,                              // [ntgt + 1] offset of the target's correlation matrix in the workspace
    MO_JOB_TGT, MO_JOB_DROP,               // [njobs]
    MO_DIR_FROM, MO_DIR_TO, MO_DIR_EFF,    // [n_dir] the direct paths and their effect pairs
    MO_PRED_OFF, MO_PRED_IDX,              // [L + 1], [n_edges]
    MO_LISTS
};
struct ModLayout {
    int T, nl, ncoef, nsums, ntgt, njobs, KM, n_dir, L, P, n_eff;      // KM: the most regressors of a target (predecessors + terms)
    int o[MO_LISTS];
    int ints;
};
struct ModDesc {
    ModLayout lay;
    const int* base;
    PLSPM_HD const int* list(int which) const { return base + lay.o[which]; }
};

PLSPM_HD int moderation_width(const ModLayout& y) { return y.n_dir + 4 * y.T + y.L; }

// ---- the plan: pure functions of the layout and the row count
PLSPM_HD int moderation_row_block(long N) { const long q = (N + 4095) / 4096; return 64 * (int)(q > 4 ? q : 4); }      // rows of a row block: at most 64 blocks
PLSPM_HD long moderation_table_doubles(const ModLayout& y) { return (long)(y.ncoef + y.nl) * 64; }                      // one lane group's table
PLSPM_HD long moderation_values_doubles(const ModLayout& y) { return (long)(1 + y.nl + y.T) * 64; }                     // one wave's values of a row
PLSPM_HD long moderation_job_doubles(int KM) { return regression_scratch_doubles(KM) + KM + (KM + 2) / 2; }             // scratch | x [KM] | the index list
PLSPM_HD long moderation_finish_doubles(const ModLayout& y, int e_total) {
    return (long)y.nsums + (long)y.nl * y.nl + 2L * y.T + e_total + y.njobs + (long)y.ntgt * y.KM + 4 + (long)y.njobs * moderation_job_doubles(y.KM);
}
PLSPM_HD long moderation_prepare_doubles(const ModLayout& y) { return 3L * y.P + 2L * y.nl; }

enum { MOD_OK = 0, MOD_REFUSE_ROWS, MOD_REFUSE_SUMS, MOD_REFUSE_VALUES, MOD_REFUSE_FINISH, MOD_REFUSE_PREPARE };
struct ModPlan {
    int width, nsums, nacc;                // nacc: the accumulators the row pass is compiled for (16, 32, 64 or 128)
    int row_block, row_blocks;
    bool table_in_lds;                     // the lane group's table is staged in LDS; else the lanes read it from memory
    size_t counts_lds, prepare_lds, rows_lds, finish_lds;
    int refused;
};
inline const char* moderation_refusal(int why) {
    switch (why) {
        case MOD_REFUSE_ROWS: return "moderation needs the row multiplicities as one LDS histogram of 16-bit counters: at most 65535 rows";
        case MOD_REFUSE_SUMS: return "the terms need more than 128 row sums per replicate, more than a lane of the row pass accumulates";
        case MOD_REFUSE_VALUES: return "the scores and products of one row of four waves need more than 160 KiB of LDS";
        case MOD_REFUSE_FINISH: return "the correlation matrices and regression slots of one replicate need more than 160 KiB of LDS";
        case MOD_REFUSE_PREPARE: return "the per-MV values of four replicates need more than 160 KiB of LDS";
        default: return "";
    }
}
inline ModPlan moderation_plan(const ModLayout& y, int e_total, long N) {
    ModPlan p{};
    p.width = moderation_width(y); p.nsums = y.nsums;
    p.nacc = y.nsums <= 16 ? 16 : y.nsums <= 32 ? 32 : y.nsums <= 64 ? 64 : 128;
    p.row_block = moderation_row_block(N);
    p.row_blocks = (int)((N + p.row_block - 1) / p.row_block);
    const size_t values = (size_t)kModRowsWaves * moderation_values_doubles(y) * sizeof(double), table = (size_t)moderation_table_doubles(y) * sizeof(double);
    p.table_in_lds = values + table <= kMaxLds;
    p.rows_lds = values + (p.table_in_lds ? table : 0);
    p.counts_lds = (size_t)((N + 1) / 2) * sizeof(unsigned);
    p.prepare_lds = (size_t)kModPrepareWaves * moderation_prepare_doubles(y) * sizeof(double);
    p.finish_lds = (size_t)moderation_finish_doubles(y, e_total) * sizeof(double);
    p.refused = N > kModMaxRows ? MOD_REFUSE_ROWS : y.nsums > kModMaxSums ? MOD_REFUSE_SUMS : (values > kMaxLds || 1 + y.nl + y.T > 511) ? MOD_REFUSE_VALUES
              : p.finish_lds > kMaxLds ? MOD_REFUSE_FINISH : p.prepare_lds > kMaxLds ? MOD_REFUSE_PREPARE : MOD_OK;
    return p;
}

// ---- the lists of a model's terms (host).  C[i * L + j] = 1 iff LV j -> LV i; boff [L + 1] the blocks' first device columns; the effect pairs as the library
// lists them.  Returns 0, or 1 with `why` set: a term the definitions do not cover.
struct ModBuild { ModLayout lay; std::vector<int> blob; int e_total; };
inline int moderation_build(int L, int P, const int* boff, const unsigned char* C, const int* pred_off, const int* pred_idx, int n_eff, const int* eff_from, const int* eff_to,
                            int T, const int* ta, const int* tb, const int* tj, ModBuild& out, std::string& why) {
    if (T < 1 || T > kModMaxTerms) { why = "between 1 and " + std::to_string(kModMaxTerms) + " interaction terms"; return 1; }
    for (int t = 0; t < T; ++t) {
        const int a = ta[t], b = tb[t], j = tj[t];
        const std::string name = "term " + std::to_string(t);
        if (a < 0 || a >= L || b < 0 || b >= L || j < 0 || j >= L) { why = name + ": latent variable out of range"; return 1; }
        if (a == b || a == j || b == j) { why = name + ": predictor, moderator and target must be three different latent variables"; return 1; }
        if (!C[j * L + a] || !C[j * L + b]) { why = name + ": both the predictor and the moderator need a path to the target (add the path)"; return 1; }
        for (int u = 0; u < t; ++u)
            if (tj[u] == j && ((ta[u] == a && tb[u] == b) || (ta[u] == b && tb[u] == a))) { why = name + ": the same pair and target as term " + std::to_string(u); return 1; }
    }
    std::vector<int> v[MO_LISTS];
    std::vector<int> slot((size_t)L, -1), need;
    for (int t = 0; t < T; ++t) {
        slot[tj[t]] = 0;
        for (int r = pred_off[tj[t]]; r < pred_off[tj[t] + 1]; ++r) slot[pred_idx[r]] = 0;
    }
    for (int l = 0; l < L; ++l) if (slot[l] == 0) { slot[l] = (int)need.size(); need.push_back(l); }
    const int nl = (int)need.size();
    v[MO_TERM_A].assign(ta, ta + T); v[MO_TERM_B].assign(tb, tb + T); v[MO_TERM_J].assign(tj, tj + T);
    v[MO_NEED] = need; v[MO_SLOT] = slot;
    for (int li = 0; li < nl; ++li) {
        v[MO_COEF_OFF].push_back((int)v[MO_COEF_COL].size());
        for (int p = boff[need[li]]; p < boff[need[li] + 1]; ++p) { v[MO_COEF_COL].push_back(p); v[MO_COEF_LV].push_back(li); }
    }
    v[MO_COEF_OFF].push_back((int)v[MO_COEF_COL].size());
    for (int e = 0; e < n_eff; ++e)
        if (C[eff_to[e] * L + eff_from[e]]) { v[MO_DIR_FROM].push_back(eff_from[e]); v[MO_DIR_TO].push_back(eff_to[e]); v[MO_DIR_EFF].push_back(e); }
    const int n_dir = (int)v[MO_DIR_FROM].size();
    for (int t = 0; t < T; ++t) {
        v[MO_TERM_SA].push_back(slot[ta[t]]); v[MO_TERM_SB].push_back(slot[tb[t]]);
        int d = 0;
        while (d < n_dir && !(v[MO_DIR_FROM][d] == ta[t] && v[MO_DIR_TO][d] == tj[t])) ++d;
        v[MO_TERM_DIR].push_back(d);
        v[MO_SUM_BASE].push_back((int)v[MO_SUM_A].size());
        const int z = 1 + nl + t;
        v[MO_SUM_A].push_back(z); v[MO_SUM_B].push_back(0);
        v[MO_SUM_A].push_back(z); v[MO_SUM_B].push_back(z);
        for (int r = pred_off[tj[t]]; r < pred_off[tj[t] + 1]; ++r) { v[MO_SUM_A].push_back(z); v[MO_SUM_B].push_back(1 + slot[pred_idx[r]]); }
        v[MO_SUM_A].push_back(z); v[MO_SUM_B].push_back(1 + slot[tj[t]]);
    }
    v[MO_CROSS].assign((size_t)T * T, -1);
    for (int t = 0; t < T; ++t)
        for (int u = t + 1; u < T; ++u)
            if (tj[t] == tj[u]) { v[MO_CROSS][t * T + u] = (int)v[MO_SUM_A].size(); v[MO_SUM_A].push_back(1 + nl + t); v[MO_SUM_B].push_back(1 + nl + u); }
    for (size_t q = 0; q < v[MO_SUM_A].size(); ++q) v[MO_SUM_AB].push_back(64 * v[MO_SUM_A][q] | (64 * v[MO_SUM_B][q]) << 16);
    int KM = 0, e_total = 0;
    for (int j = 0; j < L; ++j) {
        std::vector<int> mine;
        for (int t = 0; t < T; ++t) if (tj[t] == j) mine.push_back(t);
        if (mine.empty()) continue;
        const int k = pred_off[j + 1] - pred_off[j], m = (int)mine.size();
        v[MO_TGT].push_back(j);
        v[MO_TGT_OFF].push_back((int)v[MO_TGT_TERMS].size());
        v[MO_TGT_JOB].push_back((int)v[MO_JOB_TGT].size());
        v[MO_TGT_E].push_back(e_total);
        for (int q = -1; q < m; ++q) { v[MO_JOB_TGT].push_back((int)v[MO_TGT].size() - 1); v[MO_JOB_DROP].push_back(q); }
        v[MO_TGT_TERMS].insert(v[MO_TGT_TERMS].end(), mine.begin(), mine.end());
        KM = std::max(KM, k + m);
        e_total += (k + m + 1) * (k + m + 1);
    }
    v[MO_TGT_OFF].push_back((int)v[MO_TGT_TERMS].size());
    v[MO_TGT_E].push_back(e_total);
    v[MO_PRED_OFF].assign(pred_off, pred_off + L + 1);
    v[MO_PRED_IDX].assign(pred_idx, pred_idx + pred_off[L]);
    ModLayout& y = out.lay;
    y = ModLayout{};
    y.T = T; y.nl = nl; y.ncoef = (int)v[MO_COEF_COL].size(); y.nsums = (int)v[MO_SUM_A].size(); y.ntgt = (int)v[MO_TGT].size(); y.njobs = (int)v[MO_JOB_TGT].size();
    y.KM = KM; y.n_dir = n_dir; y.L = L; y.P = P; y.n_eff = n_eff;
    out.blob.clear();
    for (int k = 0; k < MO_LISTS; ++k) { y.o[k] = (int)out.blob.size(); out.blob.insert(out.blob.end(), v[k].begin(), v[k].end()); }
    out.blob.push_back(0);                 // (never empty)
    y.ints = (int)out.blob.size();
    out.e_total = e_total;
    return 0;
}

// ---- the second stage of one data set
// one problem's workspace: tot [nsums] | rcn [nl x nl] | zm, zs [T] | E [e_total] | r2 [njobs] | beta [ntgt x KM] | flag [4] | njobs slots
struct ModWs { double *tot, *rcn, *zm, *zs, *E, *r2, *beta, *flag, *slot; };
PLSPM_HD void moderation_carve(ModWs& w, double* base, const ModLayout& y, int e_total) {
    w.tot = base; w.rcn = w.tot + y.nsums; w.zm = w.rcn + (long)y.nl * y.nl; w.zs = w.zm + y.T; w.E = w.zs + y.T; w.r2 = w.E + e_total; w.beta = w.r2 + y.njobs;
    w.flag = w.beta + (long)y.ntgt * y.KM; w.slot = w.flag + 4;
}

PLSPM_HD int moderation_target_of(const ModDesc& d, int lv) {
    const int* tgt = d.list(MO_TGT);
    for (int g = 0; g < d.lay.ntgt; ++g) if (tgt[g] == lv) return g;
    return -1;
}
PLSPM_HD int moderation_pred_pos(const ModDesc& d, int j, int lv) {
    const int *po = d.list(MO_PRED_OFF), *pi = d.list(MO_PRED_IDX);
    for (int r = po[j]; r < po[j + 1]; ++r) if (pi[r] == lv) return r - po[j];
    return 0;
}

// w.tot and w.rcn are filled in;  n: the rows of the data set (the sum of the multiplicities);  rec: its bootstrap record (pitch R + 2);  out: the record (pitch W + 2)
template <class Ex>
PLSPM_HD void moderation_record(Ex& ex, const ModDesc& d, ModWs& w, double n, const double* rec, int R, double* out) {
    const ModLayout& y = d.lay;
    const int T = y.T, nl = y.nl, KM = y.KM, W = moderation_width(y);
    const int *po = d.list(MO_PRED_OFF), *pi = d.list(MO_PRED_IDX), *slot = d.list(MO_SLOT), *tgt = d.list(MO_TGT), *toff = d.list(MO_TGT_OFF), *tterms = d.list(MO_TGT_TERMS),
              *tjob = d.list(MO_TGT_JOB), *te = d.list(MO_TGT_E), *sbase = d.list(MO_SUM_BASE), *cross = d.list(MO_CROSS);
    const double inv_n = 1.0 / n;
    ex.par(T > 4 ? T : 4, [&](int t) {
        if (t < 4) w.flag[t] = 0.0;
        if (t < T) {
            const double m1 = w.tot[sbase[t]] * inv_n, m2 = w.tot[sbase[t] + 1] * inv_n, var = m2 - m1 * m1;
            w.zm[t] = m1;
            w.zs[t] = (var > 1e-9 * m2) ? sqrt(var) : ((var == var) ? 0.0 : var);
        }
    });
    // the extended correlation matrices: one lane per entry
    ex.par(te[y.ntgt], [&](int e) {
        int g = 0;
        while (e >= te[g + 1]) ++g;
        const int j = tgt[g], k = po[j + 1] - po[j], m = toff[g + 1] - toff[g], D = k + m + 1;
        const int r = (e - te[g]) / D, c = (e - te[g]) - r * D;
        const int tr = (r >= k && r < k + m) ? tterms[toff[g] + r - k] : -1, tc = (c >= k && c < k + m) ? tterms[toff[g] + c - k] : -1;
        const int lr = r < k ? pi[po[j] + r] : j, lc = c < k ? pi[po[j] + c] : j;
        double v;
        if (r == c) v = 1.0;
        else if (tr < 0 && tc < 0) v = w.rcn[slot[lr] * nl + slot[lc]];
        else if (tr >= 0 && tc >= 0) {
            const int lo = tr < tc ? tr : tc, hi = tr < tc ? tc : tr;
            v = (w.tot[cross[lo * T + hi]] * inv_n - w.zm[tr] * w.zm[tc]) / (w.zs[tr] * w.zs[tc]);
        } else {
            const int t = tr >= 0 ? tr : tc, pos = tr >= 0 ? c : r;      // (the LV's place among the regressors is its place in the term's sums: predecessors, then the target)
            v = (w.tot[sbase[t] + 2 + (pos < k ? pos : k)] * inv_n) / w.zs[t];
        }
        w.E[e] = v;
    });
    // the regressions: one lane per job
    const long slot_doubles = moderation_job_doubles(KM);
    ex.par(y.njobs, [&](int job) {
        const int g = d.list(MO_JOB_TGT)[job], drop = d.list(MO_JOB_DROP)[job];
        const int j = tgt[g], k = po[j + 1] - po[j], m = toff[g + 1] - toff[g], D = k + m + 1;
        double* scratch = w.slot + job * slot_doubles;
        double* x = scratch + regression_scratch_doubles(KM);
        int* idx = (int*)(x + KM);
        int kk = 0;
        for (int r = 0; r < k + m; ++r) if (r != k + drop || drop < 0) idx[kk++] = r;
        const double* E = w.E + te[g];
        bool finite = true;                      // (a product without variance: its correlations are not numbers, and neither is anything regressed on them)
        for (int r = 0; r < kk; ++r) {
            for (int c = 0; c < kk; ++c) finite = finite && isfinite(E[idx[r] * D + idx[c]]);
            finite = finite && isfinite(E[idx[r] * D + D - 1]);
        }
        if (!finite) for (int r = 0; r < kk; ++r) x[r] = __builtin_nan("");
        else if (!spd_solve<Ex::kcap>(E, D, idx, kk, D - 1, x, scratch)) w.flag[0] = 1.0;
        double s = 0.0;
        for (int r = 0; r < kk; ++r) s += x[r] * E[idx[r] * D + D - 1];
        w.r2[job] = s;
        if (drop < 0) for (int r = 0; r < kk; ++r) w.beta[g * KM + r] = x[r];
    });
    // the record: one lane per value
    const double* direct = rec + y.P + y.L + y.n_eff;
    ex.par(W, [&](int e) {
        double v;
        if (e < y.n_dir) {
            const int to = d.list(MO_DIR_TO)[e], g = moderation_target_of(d, to);
            v = g >= 0 ? w.beta[g * KM + moderation_pred_pos(d, to, d.list(MO_DIR_FROM)[e])] : direct[d.list(MO_DIR_EFF)[e]];
        } else if (e < y.n_dir + 4 * T) {
            const int what = (e - y.n_dir) / T, t = (e - y.n_dir) - what * T;
            const int j = d.list(MO_TERM_J)[t], g = moderation_target_of(d, j), k = po[j + 1] - po[j];
            int q = 0;
            while (tterms[toff[g] + q] != t) ++q;
            const double inter = w.beta[g * KM + k + q], full = w.r2[tjob[g]];
            const double main = w.beta[g * KM + moderation_pred_pos(d, j, d.list(MO_TERM_A)[t])];
            v = what == 0 ? inter : what == 1 ? (full - w.r2[tjob[g] + 1 + q]) / (1.0 - full) : what == 2 ? main - inter : main + inter;
        } else {
            const int l = e - y.n_dir - 4 * T, g = moderation_target_of(d, l);
            v = g >= 0 ? w.r2[tjob[g]] : rec[y.P + l];
        }
        if (!isfinite(v)) w.flag[1] = 1.0;
        out[e] = v;
    });
    ex.one([&]() {
        out[W] = (double)(w.flag[0] != 0.0 ? ST_SINGULAR : w.flag[1] != 0.0 ? ST_NONFINITE : ST_OK);
        out[W + 1] = rec[R + 1];
    });
}

// the executor of one host thread (tests/moderation_host): every index in ascending order
struct ModSerialExec {
    static constexpr int kcap = 8;
    template <class F> void par(int n, F f) { for (int i = 0; i < n; ++i) f(i); }
    template <class F> void one(F f) { f(); }
};

}  // namespace plspm
