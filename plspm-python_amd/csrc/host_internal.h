// host_internal.h -- what the translation units of libplspm_hip.so share on the HOST side (round 4: the former one-file host is split by
// concern so that the units compile side by side): plspm_hip.hip (allocator, handles, options as options.h tabulates them, upload, staging),
// plspm_fit.hip (fp64 Gram, metric solvers, the single fit phase by phase as fit_route.h plans it, operator seam), plspm_nonmetric.hip (the
// non-metric iteration), plspm_gram_i8.hip (digit planes + the int8 Gram of bootstrap batches), plspm_bootstrap.hip (batch driver phase by phase
// as batch_route.h plans it, record download, summaries), plspm_derived.hip (the records derived from a plain bootstrap's replicates, stage by stage as derived_route.h tabulates and plans them),
// plspm_group.cpp (multi-GPU groups); the units of one call kind each are listed further down.  Every device kernel lives in
// exactly one unit's headers; the functions below are the seams between them.  Nothing here is part of the C-ABI (include/plspm_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/plspm_hip_test.h"
#include "solver_core.h"
#include "solver_nmg.h"
#include "solver_hoc.h"
#include "solver_nmx.h"
#include "solver_ops.h"
#include "solver_wave.h"
#include "solver_quad.h"
#include "solver_wave16.h"
#include "solver_route.h"
#include "nm_route.h"
#include "batch_route.h"
#include "fit_route.h"

using namespace plspm;

typedef double d4 __attribute__((ext_vector_type(4)));
__host__ __device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }

#include "model.h"

inline RouteShape route_shape(const plspm_model* m) { return {m->P, m->L, m->kmax, m->n_chol, m->n_eff, (int)m->pred_idx.size(), m->boff.data()}; }
// nm_route.h: the shape, the options and the plan of a non-metric call on this handle (an attached second stage streams its first stage's data)
inline NmShape plan_shape(const plspm_model* m) {
    const plspm_model* src = m->stage1 ? m->stage1 : m;
    const std::vector<int>& blocks = m->stage1 ? m->lv_cols : m->boff;
    NmShape s{};
    s.P = m->P; s.P1 = src->P; s.Pm = m->Pm; s.L = m->L; s.kmax = m->kmax; s.n_chol = m->n_chol; s.n_eff = m->n_eff; s.nedge = (int)m->pred_idx.size();
    s.cmax = m->cmax; s.kmv = m->kmv; s.max_iter = m->max_iter; s.N = src->N; s.nmx_K = m->nmx_K;
    s.kb = 1;
    for (int l = 0; l < m->L; ++l) s.kb = std::max(s.kb, blocks[l + 1] - blocks[l]);
    s.nonmetric = m->nonmetric != 0; s.categorical = m->categorical != 0; s.cat_pure = m->cat_pure; s.src_cat_pure = src->categorical && src->cat_pure;
    s.all_mode_a = std::all_of(m->mode.begin(), m->mode.end(), [](int mode) { return mode == PLSPM_MODE_A; });
    s.attached = m->stage1 != nullptr; s.has_stage2 = m->stage2 != nullptr; s.has_ind = m->n_ind != 0;
    s.codes_tables = m->stage1 ? (m->d_mv_base2 && m->d_lmv2_off) : (m->d_mv_base && m->d_lmv_off);
    return s;
}
inline NmOptions nm_options(const plspm_model* m) {
    const plspm_model::Tune& t = m->tune;
    return {t.conv_pass, t.conv_gy, t.nm_k16, t.nm_wave, t.nm_codes, t.nm_mfma, t.nm_subset, t.nm_cat_one, t.nm_cpl, t.nm_c10, t.nm_fast_lds, t.nm_wave16, t.nm_direct16};
}
inline NmPlan plan_nonmetric(const plspm_model* m, const NmCall& call) { return nm_plan(plan_shape(m), call, nm_options(m)); }
// batch_route.h: the shape, the options and the kind of a batch call on this handle, and its predicates about the int8 route asked of a handle
inline BatchShape batch_shape(const plspm_model* m) {
    BatchShape s{};
    s.N = m->N; s.P = m->P; s.Pg = m->Pg; s.T = m->T; s.L = m->L; s.R = plspm_row_stride(m); s.n_ind = m->n_ind;
    s.nonmetric = m->nonmetric != 0; s.has_stage1 = m->stage1 != nullptr; s.has_stage2 = m->stage2 != nullptr; s.micom_on = m->micom_on; s.plain_metric = plain_metric(m);
    s.route = route_shape(m);
    if (m->nonmetric) { s.nm = plan_shape(m); if (m->stage2) s.nm2 = plan_shape(m->stage2); }
    return s;
}
inline BatchOptions batch_options(const plspm_model* m) {
    const plspm_model::Tune& t = m->tune;
    return {t.gram_path, t.i8_min_batch, t.i8_slices, t.nm_counts8, t.resample_aux, t.i8_shape, t.i8_sched, t.solver_wave, t.solver_quad, t.solver_rows, t.boot_pass,
            nm_options(m), m->stage2 ? nm_options(m->stage2) : NmOptions{}, m->aux != nullptr};
}
inline BatchKind batch_kind(const BatchCall& c) {
    return {c.B, brings_counts(c), pairs_problems(c), c.kind == BatchCall::STRATIFIED, c.d_idx != nullptr, c.moments_out != nullptr, c.rows_out != nullptr};
}
// fit_route.h: the shape of a single fit on this handle
inline FitShape fit_shape(const plspm_model* m) {
    return {(long)m->N, m->P, m->categorical ? m->Pm : m->P, m->L, m->n_eff, m->PA, m->T, m->kmax, m->n_chol, (int)m->pred_idx.size(), m->categorical != 0};
}
inline bool gram_i8_closed(const plspm_model* m, int slices) { return gram_i8_closed(batch_shape(m), batch_options(m), slices); }
inline int choose_gram_path(const plspm_model* m, int64_t B) { return choose_gram_path(batch_shape(m), batch_options(m), B); }
inline bool gram_counts_route_open(const plspm_model* m) { return gram_counts_route_open(batch_shape(m), batch_options(m)); }
inline bool may_raise(const plspm_model* m, const BatchCall& c) { return batch_may_raise(m->N, m->tune.i8_sched, c.d_idx != nullptr, c.kind == BatchCall::STRATIFIED); }
inline size_t nm_state_doubles_of(const plspm_model* m) { return (size_t)nm_state_doubles_of(plan_shape(m)); }
// Dynamic LDS beyond the 64 KiB default needs an explicit opt-in per kernel.
inline int allow_lds(plspm_model* m, const void* fn, size_t bytes) {
    if (bytes > kMaxLds) return fail(m, PLSPM_E_LIMIT, "kernel needs more than 160 KiB of LDS");
    if (bytes > 48 * 1024) {
        // (a kernel with static LDS of its own can be refused below 160 KiB of dynamic LDS: the same limit, the same code -- found by the many-LV fuzz, a 34-LV / 179-MV model)
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(m, PLSPM_E_LIMIT, "kernel needs " + std::to_string(bytes) + " bytes of dynamic LDS beside its static share: more than the device grants (" + hipGetErrorString(e) + ")");
        }
    }
    return 0;
}

// where a solver launch writes: per-problem strides; null base pointers are skipped
struct SolverOut {
    double* row; long row_stride;
    int* status; int* iters;
    long long* marks;
    FitOutputs fit;     // single-fit extras (problem 0 only)
};

// the device pointers an enqueue-only entry point hands back (any of the three may be null)
inline void hand_out(const plspm_model::Buf& rows, const plspm_model::Buf& status, const plspm_model::Buf& iters, void** d_out, void** d_status, void** d_iters) {
    if (d_out) *d_out = rows.p;
    if (d_status) *d_status = status.p;
    if (d_iters) *d_iters = iters.p;
}

// ---- plspm_hip.hip
ModelDesc make_desc(const plspm_model* m);
HocDesc make_hoc_desc(const plspm_model* m2);
void set_geometry(plspm_model* m);
static constexpr size_t kPinHalf = (size_t)8 << 20;       // two halves of the handle's pinned staging area: the host copy of chunk k+1 overlaps the DMA of chunk k
int pin_ready(plspm_model* m);

// ---- plspm_fit.hip
// moment matrix of ALL uploaded rows -> m->gram (dense fp64 MFMA Gram over row chunks + fixed-order reduce)
int dense_moments(plspm_model* m);
// fp64 MFMA Gram of `nproblems` replicates over their (row,count) lists -> tile-packed matrices at `out`
int launch_gram_lists(plspm_model* m, long nproblems, const int2* ent, const int* nent, long ent_stride, double* out);
int run_impute(plspm_model* m, long nproblems, const double* Min, const double** Mp, long* mp_stride);
int launch_solver(plspm_model* m, long nproblems, const double* Mp, long mp_stride, const SolverOut& so, int threads);
// the full sample as ONE solver problem (the one plspm_fit solves): the moments of all uploaded rows, tile-packed, into m->gram; its record at `record`, its status and
// iteration count at status_iters[0] and [1]
int solve_full_sample(plspm_model* m, double* record, int* status_iters);
// the metric solver of a bootstrap batch: `route` as metric_batch_route chose it when the int8 Gram wrote dense matrices, else ROUTE_LDS
// stop: an event the launch may signal on completion (the dense solvers do, and set *stop_taken; plspm_fit.hip launch_signalling), or null
int launch_batch_solver(plspm_model* m, long nb, SolverRoute route, const SolverOut& so, hipEvent_t stop, bool* stop_taken);
// Scale.NUM / RAW non-metric bootstrap batches as ONE solver launch (round 6; solver_wave16.h NM; nm_route.h num_one says whether the model has such a kernel)
// (dense moment matrices at m->gram; maps / steps as kernels_solver.h solver_nmwave_kernel takes them; force + live: the replay of `nb` listed replicates)
int launch_nm_wave_solver(plspm_model* m, long nb, const SolverOut& so, double* maps, long maps_stride, int* steps, const int* force, const int* live);
// What a non-metric solve reads of its problems.  Mp: their packed scatter matrices (unless the Gram wrote the uint16 counts); ent / nent: their (row,count) lists
// or null; cd8 / cd8_MT: the int8 row multiplicities the digit-plane Gram consumed or null; threads per problem of the launch-by-launch kernels
struct NmInputs { const double* Mp; long mp_stride; const int2* ent; const int* nent; long ent_stride; const void* cd8; int cd8_MT; int threads; };
// plspm_nonmetric.hip: the non-metric solve of pl.call.nproblems problems as `pl` (plan_nonmetric) routes it
int run_nonmetric(plspm_model* m, const NmPlan& pl, const NmInputs& in, const SolverOut& so_in);
// second-stage moments of a HOC pair by congruence with the first stage's score maps: m->gram (stage 1) -> m2->gram
int run_hoc_moments(plspm_model* m, plspm_model* m2, long nb);

// ---- plspm_gram_i8.hip
static inline long i8_pairs(const plspm_model* m) { return i8_pair_count(m->Pg); }
int prepare_zs_stats(plspm_model* m);
int prepare_zs(plspm_model* m, int floor = 0);      // floor: at least this many digit planes (0: the handle's own choice)
// What one pass through the int8 Gram leaves.  fallback: an explicit index list carried a multiplicity above 127 -- nothing was multiplied, the caller takes the
// fp64 Gram for these problems; counts / counts_MT: the dense int8 multiplicities in 16-row pieces (null: another layout); wrote16: the products left as uint16 at out16
struct GramI8Result { bool fallback; const void* counts; int counts_MT; bool wrote16; };
// problems [b0, b0 + nb) of `call`: their counts (drawn, or the kind's own count kernel) and the product.  out16 (may be null): where an all-indicator data set's
// products -- co-occurrence counts -- may leave as uint16 [nb][C][ld16], upper triangle, instead of fp64 slots at `out`
int run_gram_i8(plspm_model* m, const BatchCall& call, int64_t nb, int64_t b0, double* out, bool dense, unsigned short* out16, GramI8Result* res);
// plspm_nonmetric.hip: a Scale.NUM / RAW batch as one solver launch + verification (pl.num_one); reads in.cd8 / in.cd8_MT and the dense moment matrices at m->gram
int run_nonmetric_wave(plspm_model* m, const NmPlan& pl, const NmInputs& in, const SolverOut& so);

// ---- plspm_derived.hip: the records derived from a plain metric bootstrap's replicates behind its solver -- assessment, structural assessment, PLSc, model fit,
// geodesic discrepancy: the stages of derived_route.h's table --, as the batch driver sees them.  `runs` is the call's value: the stages that run, one bit each
// (derived_route.h stage_bit); zero: nothing to do.
// Once per call: *runs = the enabled stages and what they read (derived_route.h derived_plan), or zero unless this is a plain call on a plain metric handle, no moments
// seam, whose owner takes the records: a call into the handle's own `rows` does (and the running stages' record buffers are reserved here for call.B replicates), a
// sub-batch of plspm_bootstrap() does (call.chain_off; that function reserved them for the whole call with this same function), a group's shard does not.  A stage
// whose one wave the LDS does not hold is refused here, before anything of the call runs (PLSPM_E_LIMIT).
int derived_begin(plspm_model* m, const BatchCall& call, int* runs);
// Once per chunk, behind its solver: the running stages' launches on `nb` problems whose records start at position `pos` of the record buffers.  gram: their moment
// matrices (dense: [(P+1) x cov_ld(P)] upper triangles; else tile-packed); rows: their bootstrap records, status included (pitch row_stride).
int derived_launch(plspm_model* m, int runs, long nb, int64_t pos, bool dense, const double* gram, const double* rows, long row_stride);
// The owner of the record buffers, behind the last chunk: B records of every stage that ran are valid.
void derived_commit(plspm_model* m, int runs, int64_t B);

// ---- plspm_moderation.hip: the moderation records of a plain metric bootstrap's replicates, beside the derived chain's three calls and by the same rule.
// Once per call: *runs = 1 when the handle's switch is on and the call's owner takes the records (derived_begin's rule), else 0; the record buffer is reserved for
// call.B replicates by a call of its own.  A shape the plan refuses is refused here, before anything of the call runs (PLSPM_E_LIMIT).
int moderation_begin(plspm_model* m, const BatchCall& call, int* runs);
// Once per pass, behind derived_launch: `nb` problems whose records start at position `pos` of the record buffer and whose draws are those of replicates rep0 ..
// of `seed` (the two differ under rep_offset), or the explicit rows at d_idx [nb][N]; gram / rows as derived_launch takes them.
int moderation_launch(plspm_model* m, int runs, long nb, int64_t pos, int64_t rep0, uint64_t seed, const int32_t* d_idx, bool dense, const double* gram, const double* rows,
                      long row_stride);
void moderation_commit(plspm_model* m, int runs, int64_t B);

// ---- plspm_tetrad.hip: the tetrad records of a plain metric bootstrap's replicates, beside the moderation's three calls and by the same rule.
// Once per call: *runs = 1 when the handle's switch is on and the call's owner takes the records (derived_begin's rule), else 0; the record buffer is reserved for
// call.B replicates by a call of its own.  Lists whose one wave the LDS does not hold are refused here, before anything of the call runs (PLSPM_E_LIMIT).
int tetrad_begin(plspm_model* m, const BatchCall& call, int* runs);
// Once per pass, behind moderation_launch: `nb` problems whose records start at position `pos` of the record buffer; gram / rows as derived_launch takes them.
int tetrad_launch(plspm_model* m, int runs, long nb, int64_t pos, bool dense, const double* gram, const double* rows, long row_stride);
void tetrad_commit(plspm_model* m, int runs, int64_t B);

// ---- plspm_ipma.hip: the importance-performance records of a plain metric bootstrap's replicates, beside the tetrad's three calls and by the same
// rule: *runs = 1 when the handle's switch is on and the call's owner takes the records, else 0; a slice the LDS does not hold is refused in ipma_begin.
int ipma_begin(plspm_model* m, const BatchCall& call, int* runs);
// Once per pass, behind tetrad_launch: `nb` problems whose records start at position `pos` of the record buffer; gram / rows as derived_launch takes them.
int ipma_launch(plspm_model* m, int runs, long nb, int64_t pos, bool dense, const double* gram, const double* rows, long row_stride);
void ipma_commit(plspm_model* m, int runs, int64_t B);

// ---- plspm_bootstrap.hip: side records -- a buffer of records [count x (width + 2)] (values | status | iterations) beside the bootstrap records, valid while
// `count` is non-zero: the records of every stage of plspm_derived.hip, the MICOM records of a permutation call.  One description, and the entry points all share.
// plain_only: the entry points refuse any other handle kind behind their argument check (MICOM; the assessment answers "no records" there).  none / differs /
// range / method: the kind's whole messages behind "<who>" -- no records, B is not the count, a fetch past the count, a method the intervals do not take
struct SideRecords { const plspm_model::Buf& buf; int64_t count; int width; bool plain_only; const char *none, *differs, *range, *method; };
int side_state(plspm_model* m, const SideRecords& s, int64_t B, const char* who);       // records there, and B of them
int side_fetch(plspm_model* m, const SideRecords& s, int64_t first, int64_t count, double* out, int32_t* status, const char* who);
int side_summary(plspm_model* m, const SideRecords& s, int64_t B, const double* original, double* summary, int64_t* n_used, const char* who);
int side_intervals(plspm_model* m, const SideRecords& s, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used, const char* who);

// ---- plspm_bootstrap.hip: the calls that bring their own count rows to the int8 Gram (permutation, stratified bootstrap, cross-validation, jackknife).  What their
// entry points refuse alike, in two steps around the entry point's own argument checks (which read the uploaded N and come before the device is touched):
int counts_call_scope(plspm_model* m, const char* who, int64_t min_rows = 2);       // data uploaded (PLSPM_E_STATE), a plain metric handle (PLSPM_E_ARG)
int counts_route_scope(plspm_model* m, const char* who);       // the 16x16x64 layout (PLSPM_E_ARG), hipSetDevice, the int8 route open at seven planes (PLSPM_E_LIMIT)
// the (key, row) pairs of the N rows of repetition `rep` of a key stream (philox.h permute_quad / cv_quad), in row order: what the host mirrors of rank_select.h order
template <class Quad>
inline std::vector<std::pair<uint32_t, uint32_t>> row_keys(Quad quad, uint64_t seed, int64_t rep, int64_t N) {
    std::vector<std::pair<uint32_t, uint32_t>> key((size_t)N);
    for (int64_t q = 0; q < (N + 3) / 4; ++q) {
        const auto u = quad(seed, (uint64_t)rep, (uint32_t)q);
        for (int j = 0; j < 4; ++j) if (4 * q + j < N) key[(size_t)(4 * q + j)] = {u.v[j], (uint32_t)(4 * q + j)};
    }
    return key;
}

// ---- plspm_permute.hip (two-group permutation test)
// One call's splits: permutation rep_offset + p has problem 2p = group a (n1 rows), 2p + 1 = the other N - n1 rows; `d_member` [B][N] bytes 0/1
// (explicit memberships, tests) or null (on-device splits from the Philox keys, kernels_permute.h).
struct PermSpec { uint64_t seed; int64_t rep_offset; int64_t n1; const uint8_t* d_member; };
// run_gram_i8 on a permutation call: the 0/1 counts of problems [prob0, prob0 + nb) (prob0, nb even) of the call's splits `ps` into `cd`, layout of
// resample_i8_kernel (MT count tiles, KB k-blocks)
int launch_perm_counts(plspm_model* m, const PermSpec& ps, int64_t nb, int64_t prob0, int MT, int KB, void* cd);
// One call's stratified resamples: resample rep_offset + p has problem 2p = n_a draws from group a's rows, 2p + 1 = n_b draws from group b's;
// `d_rows` [N] = group a's rows then group b's, ascending; `d_draws` [B][N] explicit rows (tests) or null (Philox draws, kernels_strat.h).
struct StratSpec { uint64_t seed; int64_t rep_offset; int64_t n_a; const int32_t* d_rows; const int32_t* d_draws; };
// run_gram_i8 on a stratified call: the counts of problems [prob0, prob0 + nb) (prob0, nb even) of the call's draws `ss` into `cd`, same layout
int launch_strat_counts(plspm_model* m, const StratSpec& ss, int64_t nb, int64_t prob0, int MT, int KB, void* cd);

// ---- plspm_cv.hip (k-fold cross-validation: out-of-sample prediction)
// One call's folds: problem r * k + f = the rows of repetition rep_offset + r outside fold f; `d_fold` [reps][N] fold ids (drawn on the device from
// the Philox keys or uploaded, kernels_cv.h) -- ready on the handle's stream before plspm_detail_bootstrap runs.
struct CvSpec { int64_t reps; int k; const uint8_t* d_fold; };
// run_gram_i8 on a cross-validation call: the 0/1 counts of problems [prob0, prob0 + nb) of the call's folds `cs` into `cd`, layout of resample_i8_kernel
int launch_cv_counts(plspm_model* m, const CvSpec& cs, int64_t nb, int64_t prob0, int MT, int KB, void* cd);

// ---- plspm_jackknife.hip (delete-one / delete-a-group jackknife)
// One call's problems: problem g of G leaves out the rows i with i % G == g.
struct JackSpec { int64_t G; };
// run_gram_i8 on a jackknife call: the 0/1 counts of problems [prob0, prob0 + nb) of the call's groups `js` into `cd`, layout of resample_i8_kernel
int launch_jack_counts(plspm_model* m, const JackSpec& js, int64_t nb, int64_t prob0, int MT, int KB, void* cd);

// ---- plspm_rebus.hip (REBUS-PLS: response-based unit segmentation)
// One round's problems: problem k of K is the model on the rows whose label is k; `d_label` [N] ints below K, on the device.
struct RebusSpec { int K; const int* d_label; };
// run_gram_i8 on a REBUS call: the 0/1 counts of problems [prob0, prob0 + nb) of the round's classes `rs` into `cd`, layout of resample_i8_kernel
int launch_rebus_counts(plspm_model* m, const RebusSpec& rs, int64_t nb, int64_t prob0, int MT, int KB, void* cd);

// ---- plspm_micom.hip (MICOM: measurement invariance of composite models on a permutation call's splits)
// the pooled inputs of the resident rows (u [P], the diagonal blocks of R_0) into m->micom_pool, once per upload; overwrites m->gram
int micom_prepare(plspm_model* m);
// MICOM records of `nperm` permutations: problems 2p / 2p + 1 at `gram` (dense: [(P+1) x cov_ld(P)] upper triangles; else tile-packed) and `rows` (pitch
// plspm_row_stride) -> out [nperm x (3 L + 2)].  One wave per permutation (kernels_micom.h).
int launch_micom(plspm_model* m, long nperm, bool dense, const double* gram, const double* rows, double* out);
