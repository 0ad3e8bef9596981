// plspm_derived.hip -- host side, part 10: the records derived from a plain bootstrap's replicates.  One chain of per-replicate kernels behind the metric
// solver, each stage reading the replicate's moment matrix, its bootstrap record and the record the stage before it wrote:
//     assessment (plspm_assess_*)  ->  consistent PLS (plspm_plsc_*, 5o)  ->  model fit (plspm_modelfit_*, 5p)  ->  geodesic discrepancy (plspm_geodesic_*, 5q)
//                                                \->  structural-model assessment (plspm_structural_*, 5r)
// A call runs the chain to the depth of the deepest stage that is enabled; the structural stage is a branch off the assessment: it needs depth 1 and nothing else, runs
// whether or not the deeper stages do, and touches no record of theirs.  The batch driver carries one opaque int per call: the depth, and kBranchStructural for the
// branch (chain_depth / chain_branch below take it apart).  The batch driver (plspm_bootstrap.hip) sees three calls -- derived_begin,
// derived_launch, derived_commit (host_internal.h) --; the full-sample records (plspm_*_fit) are the same chain on one problem.
// Kernels: kernels_assess.h, kernels_plsc.h, kernels_modelfit.h, kernels_geodesic.h (their shared opening: kernels_moments.h), kernels_structural.h.
#include "wave_launch.h"

#include "wave_ops.h"
#include "kernels_assess.h"
#include "kernels_plsc.h"
#include "kernels_modelfit.h"
#include "kernels_geodesic.h"
#include "kernels_structural.h"

static int assess_width(const plspm_model* m) { return 4 * m->L + 3 * (m->L * (m->L - 1) / 2); }
static int plsc_width(const plspm_model* m) { return plspm_row_width(m) + m->L * (m->L - 1) / 2; }
static int modelfit_width(const plspm_model*) { return MODELFIT_WIDTH; }
static int geodesic_width(const plspm_model*) { return GEODESIC_WIDTH; }
static int structural_width(const plspm_model* m) { return m->structural_listed ? 2 * (int)m->struct_dir_from.size() + (int)m->struct_chain_off.size() - 1 : 0; }

// The stages in chain order, then the branch: the replicates' records [count x (width + 2)].  A further stage is a row here, a launcher and its place in chain_launch.
constexpr int kStages = 5, kStructural = 4;                     // stages 0 .. 3 are the chain (depth 1 .. 4), kStructural the branch off stage 0
constexpr int kBranchStructural = 8;                            // the call's opaque chain value: depth | kBranchStructural
static inline int chain_depth(int chain) { return chain & (kBranchStructural - 1); }
static inline bool chain_branch(int chain) { return (chain & kBranchStructural) != 0; }
static const struct Stage { plspm_model::Buf plspm_model::*rows; int64_t plspm_model::*count; int (*width)(const plspm_model*); } kStage[kStages] = {
    {&plspm_model::assess_rows, &plspm_model::assess_B, assess_width},
    {&plspm_model::plsc_rows, &plspm_model::plsc_B, plsc_width},
    {&plspm_model::modelfit_rows, &plspm_model::modelfit_B, modelfit_width},
    {&plspm_model::geodesic_rows, &plspm_model::geodesic_B, geodesic_width},
    {&plspm_model::structural_rows, &plspm_model::structural_B, structural_width},
};
static inline int stage_stride(const plspm_model* m, int s) { return kStage[s].width(m) + 2; }

// ---- the launchers: `nb` problems, their moment matrices `mom` (dense, or tile-packed), their bootstrap records at `rows` (row_stride 0: one problem).  One wave per problem.
static void print_assess_clocks(const long long* h) {
    fprintf(stderr, "[plspm assess clocks] per-MV values %lld  diagonal blocks %lld  block pairs %lld  total %lld\n", h[1] - h[0], h[2] - h[1], h[3] - h[2], h[3] - h[0]);
}
static void print_plsc_clocks(const long long* h) {
    fprintf(stderr, "[plspm plsc clocks] per-MV values %lld  rc %lld  regressions and effects %lld  stores %lld  total %lld\n", h[9] - h[8], h[10] - h[9], h[11] - h[10], h[12] - h[11],
            h[12] - h[8]);
}
static void print_modelfit_clocks(const long long* h) {
    fprintf(stderr, "[plspm modelfit clocks] per-MV values %lld  implied construct correlations %lld  residual sweep %lld  stores %lld  total %lld\n", h[1] - h[0], h[2] - h[1],
            h[3] - h[2], h[4] - h[3], h[4] - h[0]);
}
static void print_structural_clocks(const long long* h) {
    fprintf(stderr, "[plspm structural clocks] rc and chain products %lld  R2 per LV %lld  drop-one solves %lld  status %lld  total %lld\n", h[1] - h[0], h[2] - h[1], h[3] - h[2], h[4] - h[3],
            h[4] - h[0]);
}
static void print_geodesic_clocks(const long long* h) {      // (reduction, tridiagonalisation and bisection: the saturated and the estimated model together)
    fprintf(stderr, "[plspm geodesic clocks] per-MV values and implied construct correlations %lld  Cholesky %lld  reduction %lld  tridiagonalisation %lld  bisection %lld  stores %lld  total %lld\n",
            h[1] - h[0], h[2] - h[1], (h[3] - h[2]) + (h[6] - h[5]), (h[4] - h[3]) + (h[7] - h[6]), (h[5] - h[4]) + (h[8] - h[7]), h[9] - h[8], h[9] - h[0]);
}

// -> out [nb x (A + 2)]; side: null, or [nb x 3 L] for the PLSc kernel (kernels_assess.h)
static int launch_assess(plspm_model* m, long nb, bool dense, const MomentLayout& mom, const double* rows, long row_stride, double* out, double* side) {
    AssessArgs a{};
    a.mom = mom;
    a.L = m->L; a.R = plspm_row_width(m);
    a.boff = m->d_boff; a.lvof = m->d_lvof; a.mode = m->d_mode;
    a.rows = rows; a.row_stride = row_stride; a.out = out; a.nb = nb; a.side = side;
    return launch_wave_per_problem(m, dense ? assess_kernel<true> : assess_kernel<false>, a, nb, ASSESS_WAVES, assess_wave_doubles(m->P, m->L), &a.marks, 4, print_assess_clocks);
}

// the assessment records `assess` and the side output `side` that launch_assess wrote -> out [nb x (W + 2)] (kernels_plsc.h)
static int launch_plsc(plspm_model* m, long nb, bool dense, const MomentLayout& mom, const double* rows, long row_stride, const double* assess, const double* side, double* out) {
    PlscArgs a{};
    a.mom = mom;
    a.R = plspm_row_width(m); a.A = assess_width(m);
    a.md = make_desc(m);
    a.factor = (const unsigned char*)m->plsc_mask.p;
    a.rows = rows; a.row_stride = row_stride; a.assess = assess; a.side = side; a.out = out; a.nb = nb;
    return launch_wave_per_problem(m, dense ? plsc_kernel<true> : plsc_kernel<false>, a, nb, PLSC_WAVES, plsc_ws_doubles(m->P, m->L, m->kmax), &a.marks, 16, print_plsc_clocks);
}

// the PLSc records `plsc` that launch_plsc wrote -> out [nb x 6] (kernels_modelfit.h)
static int launch_modelfit(plspm_model* m, long nb, bool dense, const MomentLayout& mom, const double* rows, long row_stride, const double* plsc, double* out) {
    ModelfitArgs a{};
    a.mom = mom;
    a.R = plspm_row_width(m);
    a.md = make_desc(m);
    a.factor = (const unsigned char*)m->plsc_mask.p;
    a.rows = rows; a.row_stride = row_stride; a.plsc = plsc; a.out = out; a.nb = nb;
    return launch_wave_per_problem(m, dense ? modelfit_kernel<true> : modelfit_kernel<false>, a, nb, MODELFIT_WAVES, modelfit_ws_doubles(m->P, m->L), &a.marks, 8, print_modelfit_clocks);
}

// the PLSc records `plsc` and the model-fit records `modelfit` before it -> out [nb x 4] (kernels_geodesic.h).  A wave's LDS slice grows with P^2: four waves per
// workgroup where four slices fit, fewer beyond that, down to one.
static int launch_geodesic(plspm_model* m, long nb, bool dense, const MomentLayout& mom, const double* rows, long row_stride, const double* plsc, const double* modelfit, double* out) {
    GeodesicArgs a{};
    a.mom = mom;
    a.R = plspm_row_width(m);
    a.md = make_desc(m);
    a.factor = (const unsigned char*)m->plsc_mask.p;
    a.rows = rows; a.row_stride = row_stride; a.plsc = plsc; a.modelfit = modelfit; a.out = out; a.nb = nb;
    const long doubles = geodesic_ws_doubles(m->P, m->L);
    const int waves = (int)std::max<long>(1, std::min<long>(GEODESIC_WAVES, (long)(kMaxLds / sizeof(double)) / doubles));
    return launch_wave_per_problem(m, dense ? geodesic_kernel<true> : geodesic_kernel<false>, a, nb, waves, doubles, &a.marks, 16, print_geodesic_clocks);
}

// One wave's slots of regression scratch and the waves of a workgroup: a slot per index in flight (LVs, then direct paths), 64 at the most, fewer where the LDS does not
// hold them beside four waves' rc; fewer waves where four slices with one slot each do not fit.  false: one wave with one slot needs more than 160 KiB.
static bool structural_geometry(const plspm_model* m, int* waves, int* nslots) {
    const long cap = (long)(kMaxLds / sizeof(double)), slot = std::max<long>(1, structural_slot_doubles(m->kmax));
    const long want = std::max<long>(1, std::min<long>(64, std::max<long>(m->L, (long)m->struct_dir_from.size())));
    for (int w = STRUCTURAL_WAVES; w >= 1; w >>= 1) {
        const long fit = (cap / w - structural_ws_doubles(m->L, m->kmax, 0)) / slot;
        if (fit >= 1) { *waves = w; *nslots = (int)std::min(want, fit); return true; }
    }
    return false;
}

// the assessment records `assess` that launch_assess wrote -> out [nb x (S + 2)] (kernels_structural.h).  No moment matrix: one kernel for both layouts.
static int launch_structural(plspm_model* m, long nb, const double* rows, long row_stride, const double* assess, double* out) {
    StructuralArgs a{};
    a.R = plspm_row_width(m); a.A = assess_width(m);
    a.md = make_desc(m);
    const int n_dir = (int)m->struct_dir_from.size(), n_spec = (int)m->struct_chain_off.size() - 1;
    const int* d = (const int*)m->structural_desc.p;
    a.sd = StructDesc{n_dir, n_spec, d, d + n_dir, d + 2 * n_dir, d + 2 * n_dir + n_spec + 1};
    if (!structural_geometry(m, &a.waves, &a.nslots)) return fail(m, PLSPM_E_LIMIT, "structural assessment: rc and one regression slot of one replicate need more than 160 KiB of LDS");
    a.rows = rows; a.row_stride = row_stride; a.assess = assess; a.out = out; a.nb = nb;
    return launch_wave_per_problem(m, structural_kernel, a, nb, a.waves, structural_ws_doubles(m->L, m->kmax, a.nslots), &a.marks, 8, print_structural_clocks);
}

// The chain to `depth` on `nb` problems: stage s writes out[s] and reads out[s - 1]; `side` [nb x 3 L] takes the assessment's hand-over to PLSc (depth >= 2); the
// structural branch (out[kStructural] not null) reads out[0] and runs behind the assessment, before the deeper stages.
static int chain_launch(plspm_model* m, int depth, long nb, bool dense, const double* gram, const double* rows, long row_stride, double* const* out, double* side) {
    const MomentLayout mom = moment_layout(m, dense, gram);
    int rc;
    if ((rc = launch_assess(m, nb, dense, mom, rows, row_stride, out[0], depth >= 2 ? side : nullptr))) return rc;
    if (out[kStructural] && (rc = launch_structural(m, nb, rows, row_stride, out[0], out[kStructural]))) return rc;
    if (depth >= 2 && (rc = launch_plsc(m, nb, dense, mom, rows, row_stride, out[0], side, out[1]))) return rc;
    if (depth >= 3 && (rc = launch_modelfit(m, nb, dense, mom, rows, row_stride, out[1], out[2]))) return rc;
    if (depth >= 4 && (rc = launch_geodesic(m, nb, dense, mom, rows, row_stride, out[1], out[2], out[3]))) return rc;
    return 0;
}

// ---- the batch driver's three calls (host_internal.h)
int derived_begin(plspm_model* m, const BatchCall& call, int* depth) {
    *depth = 0;
    const bool own = !call.rows_out;
    if (!(own || call.chain_off >= 0) || !plain_metric(m) || call.kind != BatchCall::PLAIN || call.moments_out) return 0;
    const bool branch = m->structural_on;
    const int d = m->geodesic_on ? 4 : (m->modelfit_on ? 3 : (m->plsc_on ? 2 : ((m->assess_on || branch) ? 1 : 0)));
    if (d >= 4 && geodesic_ws_doubles(m->P, m->L) * sizeof(double) > kMaxLds)      // (refused before anything of the call runs; launch_geodesic's allow_lds says the same)
        return fail(m, PLSPM_E_LIMIT, "geodesic discrepancy: the two P x P triangles of one replicate need more than 160 KiB of LDS");
    for (int s = 0; own && s < d; ++s)
        if (int rc = ensure(m, m->*kStage[s].rows, (size_t)call.B * stage_stride(m, s) * sizeof(double))) return rc;
    if (own && branch)
        if (int rc = ensure(m, m->structural_rows, (size_t)call.B * stage_stride(m, kStructural) * sizeof(double))) return rc;
    *depth = d | (branch ? kBranchStructural : 0);
    return 0;
}

int derived_launch(plspm_model* m, int chain, long nb, int64_t pos, bool dense, const double* gram, const double* rows, long row_stride) {
    const int depth = chain_depth(chain);
    if (!depth) return 0;
    if (depth >= 2)      // (the assessment's side output lasts for one pass)
        if (int rc = ensure(m, m->plsc_side, (size_t)nb * 3 * m->L * sizeof(double))) return rc;
    double* out[kStages] = {};
    for (int s = 0; s < depth; ++s) out[s] = (double*)(m->*kStage[s].rows).p + pos * stage_stride(m, s);
    if (chain_branch(chain)) out[kStructural] = (double*)m->structural_rows.p + pos * stage_stride(m, kStructural);
    return chain_launch(m, depth, nb, dense, gram, rows, row_stride, out, (double*)m->plsc_side.p);
}

void derived_commit(plspm_model* m, int chain, int64_t B) {
    for (int s = 0; s < chain_depth(chain); ++s) m->*kStage[s].count = B;
    if (chain_branch(chain)) m->structural_B = B;
}

// ---- the factor mask of PLSc and model fit
// the default factor mask: every Mode-A block of two items or more
static std::vector<uint8_t> plsc_default_mask(const plspm_model* m) {
    std::vector<uint8_t> f((size_t)m->L);
    for (int l = 0; l < m->L; ++l) f[l] = (m->mode[l] == PLSPM_MODE_A && m->boff[l + 1] - m->boff[l] >= 2) ? 1 : 0;
    return f;
}

// the mask the PLSc kernel reads: on the device, behind whatever the stream still runs with the mask before it
static int plsc_set_mask(plspm_model* m, const std::vector<uint8_t>& f) {
    HIPCHK(m, hipSetDevice(m->device));
    if (int rc = ensure(m, m->plsc_mask, (size_t)m->L)) return rc;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(m->plsc_mask.p, f.data(), (size_t)m->L, hipMemcpyHostToDevice));
    m->plsc_factor = f;
    return 0;
}

// the handle's one factor mask from an entry point's argument (plspm_plsc_enable, plspm_modelfit_enable, plspm_geodesic_enable): checked against what can be a factor, then set
static int plsc_take_mask(plspm_model* m, const uint8_t* factor, const std::string& who) {
    std::vector<uint8_t> f = plsc_default_mask(m);
    for (int l = 0; l < m->L; ++l) {
        if (factor[l] > 1) return fail(m, PLSPM_E_ARG, who + ": the factor mask holds 0 or 1 per latent variable");
        if (factor[l] && !f[l]) return fail(m, PLSPM_E_ARG, who + ": latent variable " + std::to_string(l) + " cannot be a common factor (Mode B, or a single item)");
        f[l] = factor[l];
    }
    return plsc_set_mask(m, f);
}

// The full-sample record of stage `depth` (plspm_assess_fit, plspm_plsc_fit, plspm_modelfit_fit, plspm_geodesic_fit), or of the structural branch behind depth 1
// (plspm_structural_fit): the chain of a replicate on the moments of all uploaded rows and plspm_fit's solver problem, from depth 2 on with the handle's mask (the
// default mask if none was ever set).  h: that stage's record [width + 2].
static int chain_full_sample(plspm_model* m, int depth, std::vector<double>& h, const std::string& who, bool branch = false) {
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, who + ": plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)");
    if (!m->d_Xa || m->N < 2) return fail(m, PLSPM_E_STATE, who + ": no data uploaded");
    HIPCHK(m, hipSetDevice(m->device));
    int rc;
    if (depth >= 2 && m->plsc_factor.empty() && (rc = plsc_set_mask(m, plsc_default_mask(m)))) return rc;
    // [record RS | the stages' records, width + 2 each | side 3 L | status, iterations (int)]
    size_t doubles = (size_t)plspm_row_stride(m) + 3 * (size_t)m->L;
    for (int s = 0; s < depth; ++s) doubles += (size_t)stage_stride(m, s);
    if (branch) doubles += (size_t)stage_stride(m, kStructural);
    if ((rc = ensure(m, m->derived_fit, doubles * sizeof(double) + 2 * sizeof(int)))) return rc;
    double* const rec = (double*)m->derived_fit.p;
    double* out[kStages] = {};
    double* next = rec + plspm_row_stride(m);
    for (int s = 0; s < depth; ++s) { out[s] = next; next += stage_stride(m, s); }
    if (branch) { out[kStructural] = next; next += stage_stride(m, kStructural); }
    const int last = branch ? kStructural : depth - 1;
    if ((rc = solve_full_sample(m, rec, (int*)(next + 3 * m->L)))) return rc;      // (its moments: tile-packed, in m->gram)
    if ((rc = chain_launch(m, depth, 1, false, (const double*)m->gram.p, rec, 0, out, next))) return rc;
    HIPCHK(m, hipGetLastError());
    h.resize((size_t)stage_stride(m, last));
    HIPCHK(m, hipMemcpyAsync(h.data(), out[last], h.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return 0;
}

// ---- measurement-model assessment: per-replicate records [alpha | rho_a | rho_c | ave | htmt | htmt2 | lv_cor | status | iterations]
static SideRecords assess_records(const plspm_model* m) {
    return {m->assess_rows, m->assess_B, assess_width(m), false,
            ": no assessment records on this handle (plspm_assess_enable, then a plain bootstrap; an upload or a later call replaced them)",
            ": B differs from the last assessed bootstrap on this handle", ": range exceeds the last assessed bootstrap's replicates",
            ": method must be 0 (percentile), 1 (basic) or 2 (bc); the jackknife writes no assessment records, so there is no bca"};
}

extern "C" {

int plspm_assess_enable(plspm_model_t* m, int32_t on) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_assess_enable: no handle");
    if (on && !plain_metric(m)) return fail(m, PLSPM_E_ARG, "plspm_assess_enable: plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)");
    m->assess_on = on != 0;
    return 0;
}

int32_t plspm_assess_width(const plspm_model_t* m) { return m ? assess_width(m) : 0; }

int plspm_assess_fit(plspm_model_t* m, double* out, int32_t* status) {
    if (!m || !out) return fail(m, PLSPM_E_ARG, "plspm_assess_fit: bad arguments");
    std::vector<double> h;
    if (int rc = chain_full_sample(m, 1, h, "plspm_assess_fit")) return rc;
    const int A = assess_width(m);
    std::copy(h.begin(), h.begin() + A, out);
    if (status) *status = (h[A] == h[A]) ? (int32_t)h[A] : -1;
    return 0;
}

int plspm_assess_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) {
    return m ? side_fetch(m, assess_records(m), first, count, out, status, "plspm_assess_fetch") : fail(m, PLSPM_E_ARG, "plspm_assess_fetch: bad arguments");
}

int plspm_assess_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) {
    return m ? side_summary(m, assess_records(m), B, original, summary, n_used, "plspm_assess_summary") : fail(m, PLSPM_E_ARG, "plspm_assess_summary: bad arguments (1 <= B <= 2^30)");
}

int plspm_assess_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return m ? side_intervals(m, assess_records(m), B, original, method, level, out, n_used, "plspm_assess_intervals") : fail(m, PLSPM_E_ARG, "plspm_assess_intervals: bad arguments (1 <= B <= 2^30)");
}

}  // extern "C"

// ---- consistent PLS: per-replicate records [weights | r2 | total | direct | loadings | lv_cor_c | status | iterations]
static SideRecords plsc_records(const plspm_model* m) {
    return {m->plsc_rows, m->plsc_B, plsc_width(m), false,
            ": no PLSc records on this handle (plspm_plsc_enable, then a plain bootstrap; an upload or a later call replaced them)",
            ": B differs from the last PLSc bootstrap on this handle", ": range exceeds the last PLSc bootstrap's replicates",
            ": method must be 0 (percentile), 1 (basic) or 2 (bc); the jackknife writes no PLSc records, so there is no bca"};
}

extern "C" {

int plspm_plsc_enable(plspm_model_t* m, int32_t on, const uint8_t* factor) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_plsc_enable: no handle");
    if (!on) { m->plsc_on = false; return 0; }
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, "plspm_plsc_enable: plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)");
    if (int rc = factor ? plsc_take_mask(m, factor, "plspm_plsc_enable") : plsc_set_mask(m, plsc_default_mask(m))) return rc;
    m->plsc_on = true;
    return 0;
}

int32_t plspm_plsc_width(const plspm_model_t* m) { return m ? plsc_width(m) : 0; }

int plspm_plsc_fit(plspm_model_t* m, double* out, int32_t* status) {
    if (!m || !out) return fail(m, PLSPM_E_ARG, "plspm_plsc_fit: bad arguments");
    std::vector<double> h;
    if (int rc = chain_full_sample(m, 2, h, "plspm_plsc_fit")) return rc;
    const int W = plsc_width(m);
    std::copy(h.begin(), h.begin() + W, out);
    if (status) *status = (h[W] == h[W]) ? (int32_t)h[W] : -1;
    return 0;
}

int plspm_plsc_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) {
    return m ? side_fetch(m, plsc_records(m), first, count, out, status, "plspm_plsc_fetch") : fail(m, PLSPM_E_ARG, "plspm_plsc_fetch: bad arguments");
}

int plspm_plsc_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) {
    return m ? side_summary(m, plsc_records(m), B, original, summary, n_used, "plspm_plsc_summary") : fail(m, PLSPM_E_ARG, "plspm_plsc_summary: bad arguments (1 <= B <= 2^30)");
}

int plspm_plsc_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return m ? side_intervals(m, plsc_records(m), B, original, method, level, out, n_used, "plspm_plsc_intervals") : fail(m, PLSPM_E_ARG, "plspm_plsc_intervals: bad arguments (1 <= B <= 2^30)");
}

}  // extern "C"

// plspm_modelfit_enable, plspm_geodesic_enable: the stage's switch, and the handle's one factor mask (NULL keeps it)
static int enable_keeping_mask(plspm_model* m, int32_t on, const uint8_t* factor, bool plspm_model::*flag, const std::string& who) {
    if (!m) return fail(m, PLSPM_E_ARG, who + ": no handle");
    if (!on) { m->*flag = false; return 0; }
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, who + ": plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)");
    if (factor) { if (int rc = plsc_take_mask(m, factor, who)) return rc; }
    else if (m->plsc_factor.empty()) { if (int rc = plsc_set_mask(m, plsc_default_mask(m))) return rc; }      // (NULL keeps the handle's mask)
    m->*flag = true;
    return 0;
}

// ---- model fit: per-replicate records [srmr_sat | d_uls_sat | srmr_est | d_uls_est | status | iterations]
static SideRecords modelfit_records(const plspm_model* m) {
    return {m->modelfit_rows, m->modelfit_B, MODELFIT_WIDTH, true,
            ": no model-fit records on this handle (plspm_modelfit_enable, then a plain bootstrap; an upload or a later call replaced them)",
            ": B differs from the last model-fit bootstrap on this handle", ": range exceeds the last model-fit bootstrap's replicates",
            ": method must be 0 (percentile), 1 (basic) or 2 (bc); the jackknife writes no model-fit records, so there is no bca"};
}

extern "C" {

int plspm_modelfit_enable(plspm_model_t* m, int32_t on, const uint8_t* factor) { return enable_keeping_mask(m, on, factor, &plspm_model::modelfit_on, "plspm_modelfit_enable"); }

int32_t plspm_modelfit_width(const plspm_model_t* m) { return m ? MODELFIT_WIDTH : 0; }

int plspm_modelfit_fit(plspm_model_t* m, double* out, int32_t* status) {
    if (!m || !out) return fail(m, PLSPM_E_ARG, "plspm_modelfit_fit: bad arguments");
    std::vector<double> h;
    if (int rc = chain_full_sample(m, 3, h, "plspm_modelfit_fit")) return rc;
    std::copy(h.begin(), h.begin() + MODELFIT_WIDTH, out);
    if (status) *status = (int32_t)h[MODELFIT_WIDTH];
    return 0;
}

int plspm_modelfit_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) {
    return m ? side_fetch(m, modelfit_records(m), first, count, out, status, "plspm_modelfit_fetch") : fail(m, PLSPM_E_ARG, "plspm_modelfit_fetch: bad arguments");
}

int plspm_modelfit_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) {
    return m ? side_summary(m, modelfit_records(m), B, original, summary, n_used, "plspm_modelfit_summary") : fail(m, PLSPM_E_ARG, "plspm_modelfit_summary: bad arguments (1 <= B <= 2^30)");
}

int plspm_modelfit_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return m ? side_intervals(m, modelfit_records(m), B, original, method, level, out, n_used, "plspm_modelfit_intervals") : fail(m, PLSPM_E_ARG, "plspm_modelfit_intervals: bad arguments (1 <= B <= 2^30)");
}

}  // extern "C"

// ---- geodesic discrepancy: per-replicate records [d_g_sat | d_g_est | status | iterations]
static SideRecords geodesic_records(const plspm_model* m) {
    return {m->geodesic_rows, m->geodesic_B, GEODESIC_WIDTH, true,
            ": no geodesic records on this handle (plspm_geodesic_enable, then a plain bootstrap; an upload or a later call replaced them)",
            ": B differs from the last geodesic bootstrap on this handle", ": range exceeds the last geodesic bootstrap's replicates",
            ": method must be 0 (percentile), 1 (basic) or 2 (bc); the jackknife writes no geodesic records, so there is no bca"};
}

extern "C" {

int plspm_geodesic_enable(plspm_model_t* m, int32_t on, const uint8_t* factor) { return enable_keeping_mask(m, on, factor, &plspm_model::geodesic_on, "plspm_geodesic_enable"); }

int32_t plspm_geodesic_width(const plspm_model_t* m) { return m ? GEODESIC_WIDTH : 0; }

int plspm_geodesic_fit(plspm_model_t* m, double* out, int32_t* status) {
    if (!m || !out) return fail(m, PLSPM_E_ARG, "plspm_geodesic_fit: bad arguments");
    std::vector<double> h;
    if (int rc = chain_full_sample(m, 4, h, "plspm_geodesic_fit")) return rc;
    std::copy(h.begin(), h.begin() + GEODESIC_WIDTH, out);
    if (status) *status = (int32_t)h[GEODESIC_WIDTH];
    return 0;
}

int plspm_geodesic_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) {
    return m ? side_fetch(m, geodesic_records(m), first, count, out, status, "plspm_geodesic_fetch") : fail(m, PLSPM_E_ARG, "plspm_geodesic_fetch: bad arguments");
}

int plspm_geodesic_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) {
    return m ? side_summary(m, geodesic_records(m), B, original, summary, n_used, "plspm_geodesic_summary") : fail(m, PLSPM_E_ARG, "plspm_geodesic_summary: bad arguments (1 <= B <= 2^30)");
}

int plspm_geodesic_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return m ? side_intervals(m, geodesic_records(m), B, original, method, level, out, n_used, "plspm_geodesic_intervals") : fail(m, PLSPM_E_ARG, "plspm_geodesic_intervals: bad arguments (1 <= B <= 2^30)");
}

}  // extern "C"

// ---- structural-model assessment: per-replicate records [f2 | vif | specific | status | iterations]
constexpr long kStructuralMaxChains = 4096;

// The direct paths (effect pairs with a path of their own, in pair order) and the chains (pair order, then lexicographic by node sequence) of the handle's path matrix,
// once per handle: on the host for plspm_structural_paths, on the device as structural_core.h StructDesc reads them.  The chains are counted first, by dynamic
// programming over the DAG (the LV order is a topological one: the path matrix is strictly lower triangular), and only enumerated when there are few enough.
static int structural_list(plspm_model* m, const std::string& who) {
    if (m->structural_listed) return 0;
    const int L = m->L;
    std::vector<int> eff_of((size_t)L * L, -1);
    for (int e = 0; e < m->n_eff; ++e) eff_of[(size_t)m->eff_to[e] * L + m->eff_from[e]] = e;
    const double kSat = 1e15;                                      // (counts saturate far above the cap and far below where a double stops counting)
    double n_spec = 0.0;
    std::vector<double> paths((size_t)L);
    for (int f = 0; f < L; ++f) {                                  // paths[t]: directed paths f -> ... -> t
        std::fill(paths.begin(), paths.end(), 0.0);
        for (int t = f + 1; t < L; ++t) {
            double s = 0.0;
            for (int r = m->pred_off[t]; r < m->pred_off[t + 1]; ++r) s += m->pred_idx[r] == f ? 1.0 : paths[m->pred_idx[r]];
            paths[t] = std::min(s, kSat);
            n_spec = std::min(n_spec + paths[t] - (m->C[(size_t)t * L + f] ? 1.0 : 0.0), kSat);
        }
    }
    if (n_spec > (double)kStructuralMaxChains)
        return fail(m, PLSPM_E_LIMIT, who + ": the path model has " + (n_spec >= kSat ? std::string("more than 10^15") : std::to_string((long long)n_spec)) +
                                          " specific indirect effects, more than the " + std::to_string(kStructuralMaxChains) + " a record holds");
    std::vector<int> dir_from, dir_to, chain_off{0}, nodes, chain_eff;
    std::vector<std::vector<int>> by_target((size_t)L);            // the chains from one f, per target: node sequences back to back, each lexicographic as the walk finds them
    std::vector<int> walk;
    for (int f = 0; f < L; ++f) {
        for (auto& v : by_target) v.clear();
        walk.assign(1, f);
        std::vector<int> next(1, 0);                               // depth-first over the successors in ascending order: next[d] = position in the successor list of walk[d]
        while (!walk.empty()) {
            const int u = walk.back(), d = (int)walk.size() - 1;
            if (next[d] < m->succ_off[u + 1] - m->succ_off[u]) {
                const int s = m->succ_idx[m->succ_off[u] + next[d]++];
                walk.push_back(s); next.push_back(0);
                if (walk.size() >= 3) { auto& v = by_target[s]; v.push_back((int)walk.size()); v.insert(v.end(), walk.begin(), walk.end()); }
            } else { walk.pop_back(); next.pop_back(); }
        }
        for (int t = 0; t < L; ++t) {
            if (f != t && m->C[(size_t)t * L + f]) { dir_from.push_back(f); dir_to.push_back(t); }
            const auto& v = by_target[t];
            for (size_t p = 0; p < v.size(); p += (size_t)v[p] + 1) {
                const int len = v[p];
                for (int r = 0; r < len; ++r) {
                    nodes.push_back(v[p + 1 + r]);
                    chain_eff.push_back(r + 1 < len ? eff_of[(size_t)v[p + 2 + r] * L + v[p + 1 + r]] : 0);
                }
                chain_off.push_back((int)nodes.size());
            }
        }
    }
    if ((double)(chain_off.size() - 1) != n_spec) return fail(m, PLSPM_E_STATE, who + ": the chain count and the enumeration disagree");
    std::vector<int> blob(dir_from);
    blob.insert(blob.end(), dir_to.begin(), dir_to.end());
    blob.insert(blob.end(), chain_off.begin(), chain_off.end());
    blob.insert(blob.end(), chain_eff.begin(), chain_eff.end());
    HIPCHK(m, hipSetDevice(m->device));
    if (int rc = ensure(m, m->structural_desc, std::max<size_t>(blob.size(), 1) * sizeof(int))) return rc;
    HIPCHK(m, hipMemcpy(m->structural_desc.p, blob.data(), blob.size() * sizeof(int), hipMemcpyHostToDevice));
    m->struct_dir_from = dir_from; m->struct_dir_to = dir_to; m->struct_chain_off = chain_off; m->struct_chain_nodes = nodes;
    m->structural_listed = true;
    int waves, nslots;
    if (!structural_geometry(m, &waves, &nslots)) {
        m->structural_listed = false;
        return fail(m, PLSPM_E_LIMIT, who + ": rc and one regression slot of one replicate need more than 160 KiB of LDS");
    }
    return 0;
}

static SideRecords structural_records(const plspm_model* m) {
    return {m->structural_rows, m->structural_B, structural_width(m), true,
            ": no structural records on this handle (plspm_structural_enable, then a plain bootstrap; an upload or a later call replaced them)",
            ": B differs from the last structural bootstrap on this handle", ": range exceeds the last structural bootstrap's replicates",
            ": method must be 0 (percentile), 1 (basic) or 2 (bc); the jackknife writes no structural records, so there is no bca"};
}

extern "C" {

int plspm_structural_enable(plspm_model_t* m, int32_t on) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_structural_enable: no handle");
    if (!on) { m->structural_on = false; return 0; }
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, "plspm_structural_enable: plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)");
    if (int rc = structural_list(m, "plspm_structural_enable")) return rc;
    m->structural_on = true;
    return 0;
}

int32_t plspm_structural_width(const plspm_model_t* m) { return m ? structural_width(m) : 0; }

int plspm_structural_paths(plspm_model_t* m, int32_t* n_dir, int32_t* dir_from, int32_t* dir_to, int32_t* n_spec, int32_t* chain_off, int32_t* chain_nodes) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_structural_paths: no handle");
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, "plspm_structural_paths: plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)");
    if (int rc = structural_list(m, "plspm_structural_paths")) return rc;
    if (n_dir) *n_dir = (int32_t)m->struct_dir_from.size();
    if (n_spec) *n_spec = (int32_t)m->struct_chain_off.size() - 1;
    if (dir_from) std::copy(m->struct_dir_from.begin(), m->struct_dir_from.end(), dir_from);
    if (dir_to) std::copy(m->struct_dir_to.begin(), m->struct_dir_to.end(), dir_to);
    if (chain_off) std::copy(m->struct_chain_off.begin(), m->struct_chain_off.end(), chain_off);
    if (chain_nodes) std::copy(m->struct_chain_nodes.begin(), m->struct_chain_nodes.end(), chain_nodes);
    return 0;
}

int plspm_structural_fit(plspm_model_t* m, double* out, int32_t* status) {
    if (!m || !out) return fail(m, PLSPM_E_ARG, "plspm_structural_fit: bad arguments");
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, "plspm_structural_fit: plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)");
    if (int rc = structural_list(m, "plspm_structural_fit")) return rc;
    std::vector<double> h;
    if (int rc = chain_full_sample(m, 1, h, "plspm_structural_fit", true)) return rc;
    const int S = structural_width(m);
    std::copy(h.begin(), h.begin() + S, out);
    if (status) *status = (h[S] == h[S]) ? (int32_t)h[S] : -1;
    return 0;
}

int plspm_structural_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) {
    return m ? side_fetch(m, structural_records(m), first, count, out, status, "plspm_structural_fetch") : fail(m, PLSPM_E_ARG, "plspm_structural_fetch: bad arguments");
}

int plspm_structural_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) {
    return m ? side_summary(m, structural_records(m), B, original, summary, n_used, "plspm_structural_summary") : fail(m, PLSPM_E_ARG, "plspm_structural_summary: bad arguments (1 <= B <= 2^30)");
}

int plspm_structural_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return m ? side_intervals(m, structural_records(m), B, original, method, level, out, n_used, "plspm_structural_intervals") : fail(m, PLSPM_E_ARG, "plspm_structural_intervals: bad arguments (1 <= B <= 2^30)");
}

}  // extern "C"
