// ipma_core.h -- importance-performance map analysis (IPMA): the lists of a handle, the plan of a launch and the record of one data set as ONE
// portable function the device kernel (kernels_ipma.h, one wave per problem) and a stand-alone host program (tests/ipma_host) both run.  Free of the HIP runtime.
// The definitions are this project's, after Ringle & Sarstedt (2016); equality with SmartPLS's numbers is not claimed.
//
// One data set: its moment matrix M of the P mean-shifted columns (row / column P the column sums, (P, P) the row count n), the shifts d_p, its bootstrap record
//     weights w [P] | r2 [L] | total [n_eff] | direct [n_eff] | loadings lambda [P]
// and per MV fixed bounds lo_p < hi_p, range_p = hi_p - lo_p (the same for every replicate).
//     mu_p, s_p     kernels_moments.h mv_stats, operation for operation (population sd; exactly 0 for a column that is constant in the data set, by its threshold)
//     r_pq          fma(-mu_p, mu_q, M_pq / n) * (1/s_p * 1/s_q), r_pp = 1, as kernels_assess.h has it
//     m_p           fma(M_pP, 1 / n, d_p) = d_p + mu_p in one rounding, the raw mean;   mvperf_p = 100 (m_p - lo_p) / range_p, the mean of the rescaled indicator x~_p = 100 (x_p - lo_p) / range_p
//     v_p           w_p s_p;  t_p = sum_{q in block(p)} r_pq v_q, q ascending, one fma per term from 0
//     n_l           sum_{p in l} v_p t_p = v_l' R_ll v_l, p ascending, one fma per term from 0;   f_l = 1 / sqrt(n_l): v f is plspm.quality's v, t f its u
//     sigma_l       -1 when sum_{p in l} (t_p lambda_p) < 0 (rounded products, p ascending, plain adds from 0), else +1: plspm.quality's sign rule (f_l > 0 does not
//                   change the sign)
//     a_p           ((sigma_l (v_p f_l)) (range_p (1/s_p))) / 100: the coefficient of x~_p in the standardised score y_l;   A_l = sum_{p in l} a_p, p ascending, plain adds from 0
//     weight_r_p    a_p / A_l: the rescaled weights, 1 in sum per block (exactly 1 for a single item)
//     perf_l        sum_{p in l} weight_r_p mvperf_p, p ascending, one fma per term from 0: the mean of Y_l = sum weight_r_p x~_p
//     sd_l          1 / A_l: Y_l - perf_l = y_l / A_l and y_l has population variance 1 (negative when A_l is)
//     total_u[e]    (total[e] A_i) / A_j for the effect pair e = (i -> j) of plspm_effect_pairs;  direct_u[e] likewise: the rescaling is a diagonal similarity of the
//                   path matrix, so it carries through to the total effects
//     mvimp[t][p]   weight_r_p total_u(l -> target t), l = the LV of p; 0 where the model has no effect pair l -> t, and 0 for the target's own block
// Record, width W = 2 L + 2 n_eff + 2 P + n_t P:
//     perf [L] | sd [L] | total_u [n_eff] | direct_u [n_eff] | weight_r [P] | mvperf [P] | mvimp [n_t x P]  | status | iterations
// MVs in device order, targets in ascending LV order.  Status: ST_NONFINITE when any value is not finite (a column that is constant in the data set: 0 * inf);
// otherwise ST_INADMISSIBLE (4, as plsc_core.h) when some weight_r_p < 0 -- an importance-performance map needs non-negative rescaled weights, or a performance
// can leave [0, 100]; the values stand under both.  Non-finite wins.
//
// One wave's LDS slice (ipma_wave_doubles):
//     1/s [P] | mu [P] | v, later weight_r [P] | t [P] | range / s, later a [P] | mvperf [P] | t lambda [P] | A [L] | sigma [L] | total_u [n_eff] | flags [kIpmaTail]
// Execution model: `ex.lanes(f)` runs f(lane) for the 64 lanes of a group and ends with the group's hand-over; between two hand-overs a lane reads only what an
// earlier phase wrote or what it wrote itself (the flags apart, which every writer sets to the same value).  Mom: `double operator()(int p, int q) const`.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <math.h>
#include <string>
#include <vector>
#include "solver_core.h"
#include "solver_route.h"         // kMaxLds
#include "plsc_core.h"            // ST_INADMISSIBLE

namespace plspm {

constexpr int kIpmaTail = 2;      // the flags: a non-finite value | a negative rescaled weight
constexpr int kIpmaRows = 8;      // rows of a block whose loads are in flight together while a lane forms t_p (kernels_assess.h ASSESS_ROWS, tetrad_core.h kTetradRows)

// ---- the plan
struct IpmaShape { int P, L, n_eff, n_t; };
PLSPM_HD long ipma_width(const IpmaShape& s) { return 2L * s.L + 2L * s.n_eff + 2L * s.P + (long)s.n_t * s.P; }
PLSPM_HD long ipma_wave_doubles(const IpmaShape& s) { return 7L * s.P + 2L * s.L + s.n_eff + kIpmaTail; }
// waves: 4, 2 or 1 per workgroup, the largest count whose slices fit kMaxLds (as tetrad_plan); one wave per problem; stride: the record pitch W + 2.
// refused: one wave's slice does not fit.
struct IpmaPlan { int waves; long wave_doubles; size_t lds; long grid; long stride; bool refused; };
inline IpmaPlan ipma_plan(const IpmaShape& s, long nb) {
    IpmaPlan p{};
    const long cap = (long)(kMaxLds / sizeof(double));
    p.wave_doubles = ipma_wave_doubles(s);
    int waves = 4;
    while (waves >= 1 && waves * p.wave_doubles > cap) waves >>= 1;
    p.refused = waves == 0;
    p.waves = waves < 1 ? 1 : waves;
    p.lds = (size_t)p.waves * p.wave_doubles * sizeof(double);
    p.grid = (nb + p.waves - 1) / p.waves;
    p.stride = ipma_width(s) + 2;
    return p;
}
inline const char* ipma_refusal() { return "the statistics of one replicate need more than 160 KiB of LDS"; }

// ---- the lists: what plspm_ipma_enable builds once (and tests/ipma_host)
// lvof [P]; targets [n_t], ascending; eff_of [L x L]: the effect pair of i -> j at i * L + j, or -1
struct IpmaBuild { std::vector<int> lvof, targets, eff_of; int n_t = 0; };

// mask [L] or null (every LV with a predecessor -- an LV that is the end of an effect pair).  0, or 1 with the reason in `why` (an argument error).
inline int ipma_build(int L, const int* boff, int n_eff, const int* eff_from, const int* eff_to, const unsigned char* mask, IpmaBuild& ib, std::string& why) {
    const int P = boff[L];
    ib.lvof.assign((size_t)P, 0);
    for (int l = 0; l < L; ++l) for (int p = boff[l]; p < boff[l + 1]; ++p) ib.lvof[p] = l;
    ib.eff_of.assign((size_t)L * L, -1);
    std::vector<char> has_pred((size_t)L, 0);
    for (int e = 0; e < n_eff; ++e) { ib.eff_of[(size_t)eff_from[e] * L + eff_to[e]] = e; has_pred[eff_to[e]] = 1; }
    ib.targets.clear();
    for (int l = 0; l < L; ++l) {
        if (mask && mask[l] && !has_pred[l]) { why = "LV " + std::to_string(l) + " has no predecessor: nothing has an effect on it"; return 1; }
        if (mask ? mask[l] != 0 : has_pred[l] != 0) ib.targets.push_back(l);
    }
    ib.n_t = (int)ib.targets.size();
    if (!ib.n_t) { why = mask ? "the mask names no LV" : "no LV has a predecessor: there is no target"; return 1; }
    return 0;
}

// the bounds: finite, lo_p < hi_p.  0, or 1 with the MV in `why`.
inline int ipma_check_bounds(int P, const double* lo, const double* hi, std::string& why) {
    for (int p = 0; p < P; ++p)
        if (!isfinite(lo[p]) || !isfinite(hi[p]) || !(lo[p] < hi[p])) { why = "MV " + std::to_string(p) + ": the bounds must be finite with lo < hi"; return 1; }
    return 0;
}

// ---- the arithmetic
// kernels_moments.h mv_stats, operation for operation
struct IpmaMv { double mean, sd; };
template <class Mom> PLSPM_HD IpmaMv ipma_mv_stats(const Mom& mom, int p, int P, double inv_n) {
    const double m = mom(p, P) * inv_n, m2 = mom(p, p) * inv_n, var = fma(-m, m, m2);
    const bool varies = var > 1e-9 * m2;
    return {m, varies ? sqrt(var) : ((var == var) ? 0.0 : var)};
}

struct IpmaDescs {
    int P, L, n_eff, n_t;
    const int* boff; const int* lvof; const int* targets; const int* eff_of; const int* eff_from; const int* eff_to;
    const double* shift; const double* lo; const double* hi;
};

// rec: the data set's bootstrap record (weights at 0, total at P + L, direct at P + L + n_eff, loadings at P + L + 2 n_eff);  slice: ipma_wave_doubles doubles;
// out: the record, pitch W + 2;  iterations: the bootstrap record's, passed through
template <class Ex, class Mom>
PLSPM_HD void ipma_record(Ex& ex, const IpmaDescs& d, const Mom& mom, const double* rec, double* slice, double iterations, double* out) {
    const int P = d.P, L = d.L, ne = d.n_eff;
    double* const isd = slice;
    double* const mu = isd + P;
    double* const v = mu + P;            // v_p; from phase 3 weight_r_p
    double* const t = v + P;
    double* const a = t + P;             // range_p / s_p; from phase 3 a_p
    double* const mvp = a + P;
    double* const tl = mvp + P;
    double* const A = tl + P;
    double* const sg = A + L;
    double* const tu = sg + L;
    double* const flag = tu + ne;
    const double* const total = rec + P + L;
    const double* const direct = total + ne;
    const double* const lam = direct + ne;
    double* const o_perf = out;
    double* const o_sd = o_perf + L;
    double* const o_total = o_sd + L;
    double* const o_direct = o_total + ne;
    double* const o_weight = o_direct + ne;
    double* const o_mvperf = o_weight + P;
    double* const o_mvimp = o_mvperf + P;
    const long W = 2L * L + 2L * ne + 2L * P + (long)d.n_t * P;
    const double inv_n = 1.0 / mom(P, P);
    // phase 1: lanes over the MVs -- the statistics, v, range / s and the indicator's performance
    ex.lanes([&](int lane) {
        for (int p = lane; p < P; p += 64) {
            const IpmaMv mv = ipma_mv_stats(mom, p, P, inv_n);
            const double is = 1.0 / mv.sd, lo = d.lo[p], range = d.hi[p] - lo;
            const double raw = fma(mom(p, P), inv_n, d.shift[p]);      // (an explicit fma: the same operation wherever this is compiled, whatever the contraction setting)
            const double perf = 100.0 * (raw - lo) / range;
            isd[p] = is; mu[p] = mv.mean; v[p] = rec[p] * mv.sd; a[p] = range * is; mvp[p] = perf;
            o_mvperf[p] = perf;
        }
        if (lane == 0) { flag[0] = 0.0; flag[1] = 0.0; }
    });
    // phase 2: lane p forms t_p over its own block: column p of the diagonal block, the loads of kIpmaRows rows in flight together
    ex.lanes([&](int lane) {
        for (int p = lane; p < P; p += 64) {
            const int l = d.lvof[p], b0 = d.boff[l], b1 = d.boff[l + 1];
            const double mup = mu[p], isp = isd[p], lp = lam[p];
            double tp = 0.0;
            for (int q0 = b0; q0 < b1; q0 += kIpmaRows) {
                double mm[kIpmaRows];
#pragma unroll
                for (int u = 0; u < kIpmaRows; ++u) { const int q = q0 + u < b1 ? q0 + u : b1 - 1; mm[u] = mom(q, p); }
#pragma unroll
                for (int u = 0; u < kIpmaRows; ++u) {
                    const int q = q0 + u;
                    if (q < b1) {
                        const double r = (q == p) ? 1.0 : fma(-mu[q], mup, mm[u] * inv_n) * (isd[q] * isp);
                        tp = fma(v[q], r, tp);
                    }
                }
            }
            t[p] = tp; tl[p] = tp * lp;
        }
    });
    // phase 3: lanes over the LVs -- the block norm, the sign, a_p and A_l, then the rescaled weights, the performance and the sd; a lane owns its block's entries
    ex.lanes([&](int lane) {
        bool bad = false;
        for (int l = lane; l < L; l += 64) {
            const int b0 = d.boff[l], b1 = d.boff[l + 1];
            double norm = 0.0, su = 0.0;
            for (int p = b0; p < b1; ++p) { norm = fma(v[p], t[p], norm); su += tl[p]; }
            const double f = 1.0 / sqrt(norm), sigma = (su < 0.0) ? -1.0 : 1.0;
            double Al = 0.0;
            for (int p = b0; p < b1; ++p) { const double ap = ((sigma * (v[p] * f)) * a[p]) / 100.0; a[p] = ap; Al += ap; }
            double perf = 0.0;
            for (int p = b0; p < b1; ++p) { const double wr = a[p] / Al; v[p] = wr; perf = fma(wr, mvp[p], perf); }
            const double sd = 1.0 / Al;
            A[l] = Al; sg[l] = sigma;
            o_perf[l] = perf; o_sd[l] = sd;
            bad = bad || !isfinite(perf) || !isfinite(sd);
        }
        if (bad) flag[0] = 1.0;
    });
    // phase 4: lanes over the effect pairs -- the unstandardised effects; lanes over the MVs -- the rescaled weights to the record, the flags
    ex.lanes([&](int lane) {
        bool bad = false, negative = false;
        for (int e = lane; e < ne; e += 64) {
            const double Ai = A[d.eff_from[e]], Aj = A[d.eff_to[e]];
            const double te = (total[e] * Ai) / Aj, de = (direct[e] * Ai) / Aj;
            tu[e] = te; o_total[e] = te; o_direct[e] = de;
            bad = bad || !isfinite(te) || !isfinite(de);
        }
        for (int p = lane; p < P; p += 64) {
            const double wr = v[p];
            o_weight[p] = wr;
            bad = bad || !isfinite(wr) || !isfinite(mvp[p]);
            negative = negative || wr < 0.0;
        }
        if (bad) flag[0] = 1.0;
        if (negative) flag[1] = 1.0;
    });
    // phase 5: lanes over (target, MV) -- the indicator importances, a target's row along the lanes
    ex.lanes([&](int lane) {
        bool bad = false;
        for (int k = 0; k < d.n_t; ++k) {
            const int target = d.targets[k];
            for (int p = lane; p < P; p += 64) {
                const int e = d.eff_of[(long)d.lvof[p] * L + target];
                const double imp = e < 0 ? 0.0 : v[p] * tu[e];
                o_mvimp[(long)k * P + p] = imp;
                bad = bad || !isfinite(imp);
            }
        }
        if (bad) flag[0] = 1.0;
    });
    ex.lanes([&](int lane) {
        if (lane == 0) { out[W] = (double)(flag[0] != 0.0 ? (int)ST_NONFINITE : flag[1] != 0.0 ? (int)ST_INADMISSIBLE : (int)ST_OK); out[W + 1] = iterations; }
    });
}

// the executor of one host thread (tests/ipma_host): the lanes one behind the other
struct IpmaSerialExec {
    template <class F> void lanes(F f) { for (int lane = 0; lane < 64; ++lane) f(lane); }
};

}  // namespace plspm
