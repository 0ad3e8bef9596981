// batch_route.h -- the plan of one call of the batch driver (plspm_bootstrap.hip plspm_detail_bootstrap): which Gram, which solver arrangement, which scratch
// buffers at which strides, how many problems per pass -- and what a pass may still revise of it.  Pure functions of what the handle fixes (BatchShape), the options
// (BatchOptions) and the call (BatchKind); the predicates about the int8 route that the entry points ask (gram_i8_closed, choose_gram_path, nm_counts8_possible)
// live here too.  Free of the HIP runtime: the CPU tests compile it (tests/hostemu).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include "gram_route.h"
#include "nm_route.h"
#include "solver_route.h"

namespace plspm {

inline int i8_kblocks(long N) { return (int)((N + 127) / 128) * 2; }      // k-blocks of 64 rows, an even number
inline long i8_pair_count(int Pg) { const long C = Pg + 1; return C * (C + 1) / 2; }      // pair products of the uploaded columns + the ones column

static constexpr size_t kZsBudget = (size_t)24 << 30;       // digit planes of one data set: at most 24 GiB of the 288 GiB
static constexpr long kI8RowBound = 1L << 24;               // int32 accumulators: |sum_i c_bi d_is| <= 128 sum_i c_bi = 128 N < 2^31
static constexpr long kLdsHistRows = 65535;                 // rows of one LDS histogram of 16-bit counters (N * 2 bytes <= 128 KB)

// What the handle fixes.  R: the record pitch (plspm_row_stride); T: 16-column tiles of the Gram of the Pg = P + n_ind uploaded columns; nm: the non-metric shape
// (filled for non-metric handles only), nm2: the attached second stage's when the handle is the first stage of a HOC pair.
struct BatchShape {
    long N;
    int P, Pg, T, L, R, n_ind;
    bool nonmetric, has_stage1, has_stage2, micom_on, plain_metric;
    RouteShape route;
    NmShape nm, nm2;
};
// The options the plan reads (plspm_model_set_option).  nm / nm2: the non-metric options of the handle and of its second stage (each stage reads its own);
// aux_stream: the second stream of "resample_aux" exists.
struct BatchOptions {
    int gram_path, i8_min_batch, i8_slices, nm_counts8, resample_aux, i8_shape, i8_sched, solver_wave, solver_quad, solver_rows, boot_pass;
    NmOptions nm, nm2;
    bool aux_stream;
};
// One call.  own_counts: the kind launches its own count kernel (model.h brings_counts); pairs: problems 2p / 2p + 1 are the two sides of one split (a permutation
// call); stratified: draws inside a group; explicit_idx: the resample rows come with the call; moments: the moments seam (no solver); rows_out: the caller brought
// the record buffer (a sub-batch, a group's shard, the jackknife).
struct BatchKind { int64_t B; bool own_counts, pairs, stratified, explicit_idx, moments, rows_out; };

// ---- the int8 route: pure predicates of shape and options
// A non-metric bootstrap with on-device draws can take its stop-rule passes' row multiplicities from the int8 counts the digit-plane Gram consumed: no second
// resample kernel, no (row,count) lists, no uint16 histograms.  Needs the counts in 16-row pieces on the main stream and a dense stop-rule pass that fits LDS
// (both stages of a HOC pair); "nm_counts8" 0 keeps the lists (A/B).
inline bool nm_counts8_possible(const BatchShape& s, const BatchOptions& o) {
    return s.nonmetric && o.nm_counts8 != 0 && o.resample_aux == 0 && !o.aux_stream && o.i8_shape == 16 && s.nm.nmx_K == 0 && nm_dense_lds(s.nm, o.nm.conv_pass, nullptr) != 0 &&
           (!s.has_stage2 || nm_dense_lds(s.nm2, o.nm2.conv_pass, nullptr) != 0);
}
// The int8 route is closed for the resident data at `slices` digit planes (0: the automatic count, budgeted as seven) -- whatever the options would prefer.
// Every model's replicates start from the moment matrix of the uploaded columns, so only the data decide: an attached second stage has none of its own; the int32
// accumulators bound N; a non-metric model beyond one 16-bit histogram window has dense multiplicities only as the Gram's int8 counts; the planes have a budget.
inline bool gram_i8_closed(const BatchShape& s, const BatchOptions& o, int slices) {
    if (s.has_stage1 || s.N >= kI8RowBound || s.N < 2) return true;
    if (s.nonmetric && s.N > kLdsHistRows && !nm_counts8_possible(s, o)) return true;
    const size_t zs_bytes = (size_t)(i8_kblocks(s.N) + I8_SLACK_KB) * (size_t)(((i8_pair_count(s.Pg) + 31) / 32) * 2 * (slices ? slices : 7)) * 1024;
    return zs_bytes > kZsBudget;
}
// ... and the policy on top: 1 = fp64 MFMA on the (row,count) lists, 2 = int8 digit planes.  "gram_path" 1 / 2 decides where the route is open, else batches of
// "i8_min_batch" replicates and more take it.
inline int choose_gram_path(const BatchShape& s, const BatchOptions& o, int64_t B) {
    if (o.gram_path == 1 || gram_i8_closed(s, o, o.i8_slices)) return 1;
    return (o.gram_path == 2 || B >= o.i8_min_batch) ? 2 : 1;
}
// The route of the calls that bring their own counts: open at the seven planes at least such a call cuts (their counts add up to less than N), whatever the policy says.
inline bool gram_counts_route_open(const BatchShape& s, const BatchOptions& o) { return !gram_i8_closed(s, o, std::max(o.i8_slices, 7)); }

// The call's launches may raise the device error word (index out of range / multiplicity above 127 / stream-K wait expired): explicit indices, draws inside a
// group, the persistent Gram -- and data sets of fewer than 128 rows, which cannot exceed a multiplicity of 127 but take the short-N launch forms that share
// the word with the index check.  A Philox call on the tiled launch neither raises nor needs to clear it.
inline bool batch_may_raise(long N, int i8_sched, bool explicit_idx, bool stratified) { return explicit_idx || stratified || i8_sched != 0 || N < 128; }
// plspm_bootstrap() may cut the call into sub-batches whose records download behind the next one's kernels: metric models (the non-metric iteration makes host round
// trips as it is) whose launches cannot raise the error word (every sub-batch clears it at its start, which would wipe the bits of the one before).
inline bool batch_sub_batches_ok(bool nonmetric, bool raises) { return !nonmetric && !raises; }

// ---- the plan of a call
struct BatchPlan {
    bool nonmetric, hoc, moments;      // of the shape and the call, for batch_chunk: a non-metric handle; the first stage of a HOC pair; the moments seam
    int gpath;                   // 1 fp64 MFMA on (row,count) lists, 2 int8 digit planes; a kind that brings its own counts: 2 (its caller asked gram_counts_route_open)
    int plane_floor;             // digit planes at least (prepare_zs): 7 for the kinds that bring their own counts, 0 the handle's own choice
    bool lds_hist;               // the resample histogram fits LDS; beyond, a global scratch slice per replicate
    bool counts8_plan;           // the non-metric stop rule reads the Gram's int8 counts (explicit indices within one window keep lists + uint16 histograms: they need the lists anyway)
    bool want_dcnt;              // dense uint16 histograms beside the lists for the dense stop-rule pass (LDS-histogram path only)
    SolverRoute route;           // the metric solver on dense moment matrices (solver_route.h), ROUTE_LDS where none takes the model
    bool rows_solver;            // ... and it runs: int8 Gram, no missing-value indicators, metric, not the moments seam
    NmPlan nm;                   // the non-metric route as the call's passes will take it with the int8 counts the call expects (zero for metric handles)
    bool nm_wave;                // a Scale.NUM / RAW batch as one solver launch on dense moment matrices + verification (needs the int8 counts)
    bool dense;                  // the int8 Gram writes dense [(Pg+1) x cov_ld(Pg)] matrices instead of tile-packed ones
    bool need_lists;             // (row,count) lists: the fp64 Gram walks them (explicit indices may fall back to it), so do the stop-rule passes without int8 counts
    bool need_ghist;             // the global-scratch histogram serves the lists only (the int8 route on Philox draws never builds them)
    bool cat_one;                // the categorical batch in one launch: it lasts as long as its slowest replicate, so every further pass repeats that tail
    bool want16;                 // all-indicator categorical models on the wave step: the int8 product writes the uint16 count matrices the step streams (no fp64 slots)
    bool micom;                  // MICOM records: a permutation call on a plain metric handle into the handle's own records
    bool raises;                 // batch_may_raise
    long ent_stride, dcnt_stride, psize, gk16_stride;      // entries per list; uint16 counters per histogram; doubles per tile-packed matrix; uint16 per count matrix
    int micom_stride;            // doubles per MICOM record
    size_t kpad;                 // bytes of one problem's int8 counts
    // bytes per problem of the scratch a pass holds.  The budget of the moment matrices is deliberately the larger of the two layouts whatever the call writes
    // (gram_budget_bytes >= gram_bytes): the pass size never depended on the layout, and it stays so.  The int8 counts are reserved by the Gram's own plan
    // (gram_route.h cd_bytes, padded to whole tile rows); the verification scratch by the one-launch runners.
    size_t ent_bytes, gram_budget_bytes, gram_bytes, ghist_bytes, dcnt_bytes, counts_bytes, verify_bytes;
    size_t nent_bytes, gk16_bytes;      // ... and outside the budget: the list lengths, the uint16 count matrices (+ 64 bytes per buffer)
    size_t per_rep;              // ent + gram_budget + ghist + dcnt + counts + verify
    size_t budget;               // 2 GiB of scratch per pass; 16 GiB of the 288 for the one-launch categorical batch
    int64_t chunk, passes;       // problems per pass (whole 256-problem tiles on the int8 route; "boot_pass" caps it: test seam), and the passes
};

inline BatchPlan batch_plan(const BatchShape& s, const BatchOptions& o, const BatchKind& c) {
    BatchPlan p{};
    const long N = s.N;
    const int64_t B = c.B;
    p.nonmetric = s.nonmetric; p.hoc = s.nonmetric && s.has_stage2; p.moments = c.moments;
    p.lds_hist = N <= kLdsHistRows;
    p.gpath = c.own_counts ? 2 : choose_gram_path(s, o, B);
    p.plane_floor = c.own_counts ? 7 : 0;
    p.counts8_plan = p.gpath == 2 && (!c.explicit_idx || !p.lds_hist) && nm_counts8_possible(s, o);
    p.want_dcnt = s.nonmetric && p.lds_hist && !p.counts8_plan;
    p.route = metric_batch_route(s.route, o.solver_wave, o.solver_quad, o.solver_rows);
    p.rows_solver = p.gpath == 2 && p.route != ROUTE_LDS && !s.n_ind && !s.nonmetric && !c.moments;
    if (s.nonmetric) p.nm = nm_plan(s.nm, NmCall{(long)B, p.counts8_plan, false, false, true}, o.nm);
    p.nm_wave = p.gpath == 2 && !c.moments && p.nm.num_one;
    p.dense = p.rows_solver || p.nm_wave;
    p.need_lists = p.gpath == 1 || c.explicit_idx || (s.nonmetric && !p.counts8_plan);
    p.need_ghist = !p.lds_hist && p.need_lists;
    p.cat_one = p.nm.one_launch;
    p.want16 = p.gpath == 2 && s.nonmetric && !c.moments && p.nm.direct16;
    p.micom = s.micom_on && c.pairs && s.plain_metric && !c.rows_out;
    p.raises = batch_may_raise(N, o.i8_sched, c.explicit_idx, c.stratified);
    p.ent_stride = ((N + 3) & ~3L) + 4;
    p.dcnt_stride = (N + 15) & ~15L;
    p.psize = packed_size(s.T);
    p.gk16_stride = (long)(s.P + 1) * ((s.P + 1 + 7) & ~7);
    p.micom_stride = 3 * s.L + 2;
    p.kpad = (size_t)i8_kblocks(N) * 64;
    p.ent_bytes = p.need_lists ? (size_t)p.ent_stride * 8 : 0;      // (int2 entries)
    p.nent_bytes = p.need_lists ? sizeof(int) : 0;
    p.gram_budget_bytes = (size_t)std::max<long>(p.psize, cov_doubles(s.Pg)) * sizeof(double);
    p.gram_bytes = (size_t)std::max<long>(p.psize, p.dense ? cov_doubles(s.Pg) : 0) * sizeof(double);
    p.ghist_bytes = p.need_ghist ? (size_t)N * sizeof(unsigned) : 0;
    p.dcnt_bytes = p.want_dcnt ? (size_t)p.dcnt_stride * sizeof(unsigned short) : 0;
    p.counts_bytes = p.gpath == 2 ? p.kpad : 0;
    p.verify_bytes = (p.nm_wave || p.cat_one) ? p.nm.verify_bytes_per_rep : 0;
    p.gk16_bytes = p.want16 ? (size_t)p.gk16_stride * sizeof(unsigned short) : 0;
    p.per_rep = p.ent_bytes + p.gram_budget_bytes + p.ghist_bytes + p.dcnt_bytes + p.counts_bytes + p.verify_bytes;
    p.budget = (size_t)(p.cat_one ? 16ull : 2ull) << 30;
    p.chunk = std::max<int64_t>(1, std::min<int64_t>(B, (int64_t)(p.budget / p.per_rep)));
    if (p.gpath == 2 && p.chunk < B) p.chunk = std::max<int64_t>(256, p.chunk & ~(int64_t)255);
    if (o.boot_pass > 0 && o.boot_pass < p.chunk) p.chunk = o.boot_pass;
    p.passes = (B + p.chunk - 1) / p.chunk;
    return p;
}

// ---- what a pass revises: a pass whose explicit indices carried a multiplicity above 127 fell back to the fp64 Gram and has no usable int8 counts
// HOC: the two-stage estimation of a hierarchical-construct pair; NM_WAVE: a Scale.NUM / RAW pass in one solver launch; NONMETRIC: every other non-metric form;
// METRIC: the batch solver, then the derived chain and MICOM; MOMENTS: the moments seam, no solver
enum BatchSolve { BATCH_SOLVE_MOMENTS = 0, BATCH_SOLVE_HOC = 1, BATCH_SOLVE_NM_WAVE = 2, BATCH_SOLVE_NONMETRIC = 3, BATCH_SOLVE_METRIC = 4 };
struct BatchChunk {
    bool f64_gram;               // the pass's moment matrices come from the fp64 Gram on lists (tile-packed)
    bool counts8;                // the int8 counts the Gram consumed are there for the stop rule
    bool build_lists;            // the list resample runs: the same draws as the int8 counts
    bool lists;                  // ... and the non-metric solver reads them
    bool dense_solver;           // the metric solver (and what follows it) reads dense moment matrices
    SolverRoute route;           // ... as this route; ROUTE_LDS on tile-packed ones
    int solve;                   // BatchSolve
    NmCall call, call2;          // the non-metric call of the pass; HOC: of stage 1 (no records) and of stage 2
};
inline BatchChunk batch_chunk(const BatchPlan& p, int64_t nb, bool fell_back, bool wrote16) {
    BatchChunk k{};
    k.f64_gram = p.gpath == 1 || fell_back;
    k.counts8 = p.counts8_plan && !k.f64_gram;
    k.build_lists = k.f64_gram || (p.nonmetric && !k.counts8);
    k.lists = p.need_lists && !k.counts8;
    k.dense_solver = p.rows_solver && !k.f64_gram;
    k.route = k.dense_solver ? p.route : ROUTE_LDS;
    const bool lists_dcnt = k.lists && p.want_dcnt;      // (the uint16 histograms come with the lists where the plan wants them)
    k.solve = p.moments ? BATCH_SOLVE_MOMENTS : !p.nonmetric ? BATCH_SOLVE_METRIC : p.hoc ? BATCH_SOLVE_HOC : (p.nm_wave && k.counts8) ? BATCH_SOLVE_NM_WAVE : BATCH_SOLVE_NONMETRIC;
    switch (k.solve) {
        case BATCH_SOLVE_HOC: k.call = NmCall{(long)nb, k.counts8, lists_dcnt, false, false}; k.call2 = NmCall{(long)nb, k.counts8, lists_dcnt, false, true}; break;
        case BATCH_SOLVE_NM_WAVE: k.call = NmCall{(long)nb, true, false, false, true}; break;
        case BATCH_SOLVE_NONMETRIC: k.call = NmCall{(long)nb, k.counts8, lists_dcnt, wrote16, true}; break;
        default: break;
    }
    return k;
}

}  // namespace plspm
