// nm_route.h -- which route a non-metric batch takes (stop-rule pass, step kernel, one-launch forms) and the sizes that follow from it: a pure function of
// the model's shape, the call's inputs and the options, read by the planner (batch_route.h) and the runner (plspm_nonmetric.hip).
// Free of the HIP runtime: the CPU tests compile it (tests/hostemu).
#pragma once
#include <stddef.h>
#include "solver_nmg.h"
#include "solver_nmx.h"
#include "solver_route.h"

namespace nmw {

constexpr int LMAX_MAX = 8, CMAX_MAX = 16, CPL8 = 8;      // LVs (the kernel is instantiated for LMAX = 2, 4, 6, 8), categories per MV (CMAX = 8; 16: ten-point items -- the reference's own
                                                         // mobi / ECSI example data -- at one wave per SIMD), columns per lane

// LDS of one problem of the wave step (kernels_nmw.h; doubles): c | tq | mean | mzown (each QP = Q + 1 rounded up to 8), then the small arrays, then c_old (QP)
PLSPM_HD long lds_doubles(int Q, int Pm, int L, int kmax) {
    const long QP = (Q + 1 + 7) & ~7L;
    const long step = 3L * L * L + 6L * L + 2L * Pm + (long)L * plspm::regression_scratch_doubles(kmax) + 8 + 16;
    const long fin = plspm::workspace_small_doubles(Pm, L, kmax, 0) + Pm;           // the fused finish: MV-level workspace of finish_problem + one row of the MV moment matrix
    return 4 * QP + (step > fin ? step : fin) + QP;             // (+ QP, round 6: the old score map beside the new one for the step's own bound)
}

}  // namespace nmw

namespace plspm {

// What the decision reads from a handle (host_internal.h plan_shape).  An attached second stage of a HOC pair streams its first stage's rows: P1, N, kb and
// src_cat_pure are the first stage's there (P1 == P otherwise); kb = widest block of the block map the stop-rule pass uses (boff, or lv_cols when attached).
struct NmShape {
    int P, P1, Pm, L, kmax, n_chol, n_eff, nedge, cmax, kmv, kb, max_iter;
    long N;
    int nmx_K;
    bool nonmetric, categorical, cat_pure, src_cat_pure, all_mode_a, attached, has_stage2, has_ind, codes_tables;
};
// One call: counts8 = the int8 row multiplicities of the digit-plane Gram are at hand; lists_dcnt = (row,count) lists AND dense uint16 histograms are;
// counts16_ready = the Gram wrote the uint16 count matrices itself; finish = the records are written (false: the first stage of a HOC pair)
struct NmCall { long nproblems; bool counts8, lists_dcnt, counts16_ready, finish; };
struct NmOptions { int conv_pass, conv_gy, nm_k16, nm_wave, nm_codes, nm_mfma, nm_subset, nm_cat_one, nm_cpl, nm_c10, nm_fast_lds, nm_wave16, nm_direct16; };

enum NmPlanError { NM_PLAN_OK = 0, NM_PLAN_COUNTS8_WITHOUT_DENSE = 1, NM_PLAN_COUNTS16_WITHOUT_WAVE = 2, NM_PLAN_WORKSPACE = 3 };

struct NmPlan {
    NmCall call;
    int error;                   // NmPlanError: the first of the refused states, in the order of the enum
    // the stop-rule pass: dense (64 replicates' coefficient tile in LDS, whole or one LV block at a time) on fp64 columns / category codes / as an int8 matrix
    // product; else the gathering pass over (row,count) lists or all rows
    bool dense, dense_whole, use_codes, use_mfma, flag_from_list;
    // the step: uint16 count matrices, one wave per problem, the step's own bound with a lower-bound pass on row chunks, the whole batch in one launch + verification
    bool k16, wave_step, bound_ok, sub_pass, one_launch;
    bool cpl6, c10;
    int step_lmax, step_cmax, step_cpl;      // nmw_step_kernel<LMAX, CMAX, ., ., CPL>
    // the planner's questions about the handle: a Scale.NUM / RAW batch as one launch + verification (run_nonmetric_wave); the int8 Gram writes the uint16 counts
    bool num_one, direct16;
    int kb, KS, tpc, nparts, nsub, cat_fast, table_rows, ngroups, ld16;
    long ntiles16, ng16, st_doubles;
    size_t dense_lds, codes_lds, wave_lds, lds;
    size_t verify_bytes_per_rep;             // score maps + verification tables of the one-launch form that runs (0: none does)
};

// doubles of per-problem solver state (NmState head + what its solver keeps behind it)
PLSPM_HD long nm_state_doubles_of(const NmShape& s) {
    return s.categorical ? nmg_state_doubles(s.P, s.Pm, s.L, s.cmax, s.kmv) : s.nmx_K > 0 ? nmx_state_doubles(s.P, s.L, s.n_chol, s.nmx_K) : nm_state_doubles(s.P, s.L, s.n_chol);
}

// LDS footprint of the dense stop-rule pass (nm_conv_dense_kernel): the coefficient tile of 64 replicates whole, or one LV block at a time; 0 when neither fits
// or the option forbids the pass (conv_pass 1: never dense; 2 forces the blocked variant: tests)
PLSPM_HD size_t nm_dense_lds(const NmShape& s, int conv_pass, bool* whole) {
    const size_t tile = (size_t)(2 * s.P1 + 2 * s.L + 1) * 64 * sizeof(double);
    const bool w = tile <= kMaxLds && conv_pass != 2;
    const size_t use = w ? tile : (size_t)(2 * s.kb + 2) * 64 * sizeof(double);
    if (whole) *whole = w;
    return (use <= kMaxLds && conv_pass != 1) ? use : 0;
}

// the integer scratch of a verification (plspm_nonmetric.hip VerifyScratch): steps | force | fixlist per replicate, vb | vj | fb | fj | vneed per slot of a round, counters
PLSPM_HD size_t nm_verify_ints(long nb, int slots_per_rep) { return (size_t)(3 * nb + 5 * nb * slots_per_rep + 16); }
static constexpr int kNumVerifySlots = 4, kCatVerifySlots = 8;      // steps verified per round and replicate: Scale.NUM / RAW (three iterations is the rule), categorical (six to nine)

PLSPM_HD NmPlan nm_plan(const NmShape& s, const NmCall& c, const NmOptions& o) {
    NmPlan p{};
    p.call = c;
    const bool cat = s.categorical, nmx = s.nmx_K > 0;
    const int P = s.P, L = s.L;
    p.kb = s.kb;
    p.st_doubles = nm_state_doubles_of(s);
    p.ntiles16 = (s.N + 15) / 16;
    p.table_rows = 2 * s.P1 + 2 * L + 1;
    p.ngroups = (int)((c.nproblems + 63) / 64);
    p.ng16 = (c.nproblems + 15) / 16;
    // bootstrap: the dense pass when the replicates' row multiplicities are at hand (the Gram's int8 counts or resample_kernel's uint16 histograms) and the
    // coefficient tile fits LDS; otherwise (and for a single fit) the gathering pass
    p.dense_lds = nm_dense_lds(s, o.conv_pass, &p.dense_whole);
    p.dense = p.dense_lds != 0 && (c.counts8 || c.lists_dcnt);
    p.flag_from_list = p.dense && !s.attached;      // (the list kernel of the dense pass counts the live problems and writes the count to the pinned flag itself)
    const long gather_parts = (s.N + 1023) / 1024, gather_cap = c.nproblems == 1 ? 1024 : 8;
    p.nparts = p.dense ? (int)p.ntiles16 : (int)(gather_parts < 1 ? 1 : gather_parts > gather_cap ? gather_cap : gather_parts);
    // all-indicator categorical data on the dense pass with the int8 counts: the pass on category codes (one block's coefficients + the zero slot + the two constants) ...
    p.codes_lds = (size_t)(2 * (s.kb + 1) + 2) * 64 * sizeof(double);
    p.use_codes = p.dense && c.counts8 && s.src_cat_pure && (s.attached || cat) && s.codes_tables && !nmx && o.nm_codes != 0 && s.kb < 65535 && p.codes_lds <= kMaxLds;
    // ... and as an exact int8 matrix product: blocks of at most 128 columns (KS k-steps of 64), row chunks of `tpc` tiles -- enough waves to fill the device at the
    // batch's first passes (option conv_gy n: n x 256 waves aimed at)
    p.use_mfma = p.use_codes && s.kb <= 128 && o.nm_mfma != 0;
    p.KS = s.kb > 64 ? 2 : 1;
    if (p.use_mfma) {
        const long waves = o.conv_gy > 0 ? (long)o.conv_gy * 256 : 8192;
        long want = (waves + p.ng16 - 1) / p.ng16;
        if (want > (p.ntiles16 + 7) / 8) want = (p.ntiles16 + 7) / 8;
        if (want < 1) want = 1;
        p.tpc = (int)((p.ntiles16 + want - 1) / want);
        p.nparts = (int)((p.ntiles16 + p.tpc - 1) / p.tpc);
    }
    // the wave step (kernels_nmw.h): all-indicator models of at most 65,535 rows (uint16 counts) whose blocks are all Mode A, at most 64 MVs of at most 16
    // categories, 8 LVs and 511 indicator columns
    p.ld16 = (P + 1 + 7) & ~7;
    p.k16 = cat && s.cat_pure && s.N <= 65535 && o.nm_k16 != 0;
    p.wave_lds = (size_t)nmw::lds_doubles(P, s.Pm, L, s.kmax) * sizeof(double);
    p.wave_step = p.k16 && !nmx && o.nm_wave != 0 && s.all_mode_a && s.Pm <= 64 && L <= nmw::LMAX_MAX && s.cmax <= nmw::CMAX_MAX && P + 1 <= 512 && p.wave_lds <= kMaxLds;
    // the step's own bound + a lower-bound pass on the first row chunks: the int8-product pass only, not a stage of a HOC pair; launch by launch from 1,024 rows on
    // (below, a pass is a few row chunks and a launch floor either way), the one-launch form always
    p.bound_ok = p.use_mfma && !s.attached && o.nm_subset != 0 && p.wave_step;
    p.one_launch = p.bound_ok && c.counts8 && o.nm_cat_one != 0 && c.nproblems <= 0x7fffffffL;
    p.sub_pass = p.bound_ok && (s.N >= 1024 || p.one_launch);
    p.nsub = p.sub_pass ? (o.nm_subset > 1 ? o.nm_subset : 1) : 0;      // the safety factor of the rows a problem asks for; 0: every pass over all rows
    p.direct16 = o.nm_direct16 != 0 && !s.attached && !s.has_stage2 && p.wave_step;
    p.num_one = c.counts8 && o.nm_wave16 != 0 && s.nonmetric && !cat && !s.has_ind && !nmx && !s.attached && !s.has_stage2 && s.N <= 0x7fffffffL && p.dense_lds != 0 &&
                nm_wave_route(RouteShape{P, L, s.kmax, s.n_chol, s.n_eff, s.nedge, nullptr}) != ROUTE_NONE;
    // the step kernel: LMAX 2 / 4 / 6 / 8 LVs x at most 8 categories per MV (two waves per SIMD), 10 (nine- and ten-point items, two waves, six columns per lane
    // only) or 16 (one wave per SIMD).  Six columns per lane where they cover the model -- at most 383 aug columns of items with at most 13 categories (the finish
    // files an MV's columns from at most three neighbouring lanes); option nm_cpl 8: eight per lane, 6: six wherever the layout allows (probes).
    // (not for 7 / 8 LVs with items of 11 ... 13 categories: nmw_step_kernel<8, 16, false, false, 6> -- the launch-by-launch form without the step's own bound, i.e. every
    //  single FIT of such a model -- returns NaN inner weights under the PATH scheme and faults on the fit's one-problem buffers, while the same source with SUB, with eight columns
    //  per lane or with LMAX 6 is right (found by the large categorical fuzz, tests/fuzz_cases.make_cat_big_case seeds 34 / 124 / 133 / ...; centroid and factorial runs of the same
    //  binary are right too: DESIGN 6).  That class keeps eight columns per lane in every form.)
    p.cpl6 = s.cmax <= 13 && P + 1 <= 6 * 64 && o.nm_cpl != 8 && (o.nm_cpl == 6 || !(s.cmax > 10 && L > 6));
    p.c10 = s.cmax > 8 && s.cmax <= 10 && p.cpl6 && o.nm_c10 != 0;
    p.step_lmax = L <= 2 ? 2 : L <= 4 ? 4 : L <= 6 ? 6 : 8;
    p.step_cmax = p.c10 ? 10 : s.cmax <= 8 ? 8 : 16;
    p.step_cpl = p.cpl6 ? 6 : 8;
    // the launch-by-launch solvers (nm_kernel / nmx_kernel / nmg_kernel): workspace + descriptors; categorical problems keep the small arrays of the iteration
    // in LDS too when they fit beside the workspaces
    p.lds = (size_t)workspace_small_doubles(cat ? s.Pm : P, L, s.kmax, s.n_chol) * sizeof(double) + desc_lds_bytes(P, L, s.n_eff, s.nedge);
    if (cat) p.lds += (size_t)workspace_small_doubles(s.Pm, L, s.kmax, 0) * sizeof(double);
    const bool lds_ok = p.lds <= kMaxLds;
    const size_t cat_fast_bytes = cat ? (size_t)((nmg_fast_doubles(P, s.Pm, L, s.cmax, s.kmv) + 1) & ~1L) * sizeof(double) : 0;
    p.cat_fast = (cat && o.nm_fast_lds != 0 && p.lds + cat_fast_bytes <= kMaxLds) ? 1 : 0;
    if (p.cat_fast) p.lds += cat_fast_bytes;
    // per replicate: a score map per step; per slot of a round the coefficient table row (NUM / RAW) or the digit planes (categorical) + 64 bytes of lists and sums
    const size_t maps = (size_t)(s.max_iter + 2) * (P + L + 1) * sizeof(double);
    p.verify_bytes_per_rep = p.num_one ? maps + kNumVerifySlots * ((size_t)p.table_rows + 8) * sizeof(double)
                           : p.one_launch ? maps + kCatVerifySlots * ((size_t)L * 2 * 7 * 2 * 64 + 64) : 0;
    p.error = (c.counts8 && !p.dense) ? NM_PLAN_COUNTS8_WITHOUT_DENSE : (c.counts16_ready && !p.wave_step) ? NM_PLAN_COUNTS16_WITHOUT_WAVE : !lds_ok ? NM_PLAN_WORKSPACE : NM_PLAN_OK;
    return p;
}

}  // namespace plspm
