// plspm_derived.hip -- host side, part 10: the records derived from a plain bootstrap's replicates.  One chain of per-replicate kernels behind the metric
// solver, each stage reading the replicate's moment matrix, its bootstrap record and the record the stage before it wrote:
//     assessment (plspm_assess_*)  ->  consistent PLS (plspm_plsc_*, 5o)  ->  model fit (plspm_modelfit_*, 5p)  ->  geodesic discrepancy (plspm_geodesic_*, 5q)
// A call runs the chain to the depth of the deepest stage that is enabled.  The batch driver (plspm_bootstrap.hip) sees three calls -- derived_begin,
// derived_launch, derived_commit (host_internal.h) --; the full-sample records (plspm_*_fit) are the same chain on one problem.
// Kernels: kernels_assess.h, kernels_plsc.h, kernels_modelfit.h, kernels_geodesic.h (their shared opening: kernels_moments.h).
#include "wave_launch.h"

#include "wave_ops.h"
#include "kernels_assess.h"
#include "kernels_plsc.h"
#include "kernels_modelfit.h"
#include "kernels_geodesic.h"

static int assess_width(const plspm_model* m) { return 4 * m->L + 3 * (m->L * (m->L - 1) / 2); }
static int plsc_width(const plspm_model* m) { return plspm_row_width(m) + m->L * (m->L - 1) / 2; }
static int modelfit_width(const plspm_model*) { return MODELFIT_WIDTH; }
static int geodesic_width(const plspm_model*) { return GEODESIC_WIDTH; }

// The stages in chain order: the replicates' records [count x (width + 2)].  A further stage is a row here, a launcher and its place in chain_launch.
constexpr int kStages = 4;
static const struct Stage { plspm_model::Buf plspm_model::*rows; int64_t plspm_model::*count; int (*width)(const plspm_model*); } kStage[kStages] = {
    {&plspm_model::assess_rows, &plspm_model::assess_B, assess_width},
    {&plspm_model::plsc_rows, &plspm_model::plsc_B, plsc_width},
    {&plspm_model::modelfit_rows, &plspm_model::modelfit_B, modelfit_width},
    {&plspm_model::geodesic_rows, &plspm_model::geodesic_B, geodesic_width},
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

// The chain to `depth` on `nb` problems: stage s writes out[s] and reads out[s - 1]; `side` [nb x 3 L] takes the assessment's hand-over to PLSc (depth >= 2).
static int chain_launch(plspm_model* m, int depth, long nb, bool dense, const double* gram, const double* rows, long row_stride, double* const* out, double* side) {
    const MomentLayout mom = moment_layout(m, dense, gram);
    int rc;
    if ((rc = launch_assess(m, nb, dense, mom, rows, row_stride, out[0], depth >= 2 ? side : nullptr))) return rc;
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
    const int d = m->geodesic_on ? 4 : (m->modelfit_on ? 3 : (m->plsc_on ? 2 : (m->assess_on ? 1 : 0)));
    if (d >= 4 && geodesic_ws_doubles(m->P, m->L) * sizeof(double) > kMaxLds)      // (refused before anything of the call runs; launch_geodesic's allow_lds says the same)
        return fail(m, PLSPM_E_LIMIT, "geodesic discrepancy: the two P x P triangles of one replicate need more than 160 KiB of LDS");
    for (int s = 0; own && s < d; ++s)
        if (int rc = ensure(m, m->*kStage[s].rows, (size_t)call.B * stage_stride(m, s) * sizeof(double))) return rc;
    *depth = d;
    return 0;
}

int derived_launch(plspm_model* m, int depth, long nb, int64_t pos, bool dense, const double* gram, const double* rows, long row_stride) {
    if (!depth) return 0;
    if (depth >= 2)      // (the assessment's side output lasts for one pass)
        if (int rc = ensure(m, m->plsc_side, (size_t)nb * 3 * m->L * sizeof(double))) return rc;
    double* out[kStages];
    for (int s = 0; s < depth; ++s) out[s] = (double*)(m->*kStage[s].rows).p + pos * stage_stride(m, s);
    return chain_launch(m, depth, nb, dense, gram, rows, row_stride, out, (double*)m->plsc_side.p);
}

void derived_commit(plspm_model* m, int depth, int64_t B) {
    for (int s = 0; s < depth; ++s) m->*kStage[s].count = B;
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

// The full-sample record of stage `depth` (plspm_assess_fit, plspm_plsc_fit, plspm_modelfit_fit, plspm_geodesic_fit): the chain of a replicate on the moments of all uploaded rows and
// plspm_fit's solver problem, from depth 2 on with the handle's mask (the default mask if none was ever set).  h: that stage's record [width + 2].
static int chain_full_sample(plspm_model* m, int depth, std::vector<double>& h, const std::string& who) {
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, who + ": plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)");
    if (!m->d_Xa || m->N < 2) return fail(m, PLSPM_E_STATE, who + ": no data uploaded");
    HIPCHK(m, hipSetDevice(m->device));
    int rc;
    if (depth >= 2 && m->plsc_factor.empty() && (rc = plsc_set_mask(m, plsc_default_mask(m)))) return rc;
    // [record RS | the stages' records, width + 2 each | side 3 L | status, iterations (int)]
    size_t doubles = (size_t)plspm_row_stride(m) + 3 * (size_t)m->L;
    for (int s = 0; s < depth; ++s) doubles += (size_t)stage_stride(m, s);
    if ((rc = ensure(m, m->derived_fit, doubles * sizeof(double) + 2 * sizeof(int)))) return rc;
    double* const rec = (double*)m->derived_fit.p;
    double* out[kStages];
    double* next = rec + plspm_row_stride(m);
    for (int s = 0; s < depth; ++s) { out[s] = next; next += stage_stride(m, s); }
    if ((rc = solve_full_sample(m, rec, (int*)(next + 3 * m->L)))) return rc;      // (its moments: tile-packed, in m->gram)
    if ((rc = chain_launch(m, depth, 1, false, (const double*)m->gram.p, rec, 0, out, next))) return rc;
    HIPCHK(m, hipGetLastError());
    h.resize((size_t)stage_stride(m, depth - 1));
    HIPCHK(m, hipMemcpyAsync(h.data(), out[depth - 1], h.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
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
