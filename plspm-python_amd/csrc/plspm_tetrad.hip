// plspm_tetrad.hip -- host side, part 13: confirmatory tetrad analysis (CTA-PLS).  The tetrad lists of a handle (tetrad_core.h tetrad_build, at
// plspm_tetrad_enable), the one launch behind the metric solver of a plain bootstrap's pass (plspm_bootstrap.hip hooks it in beside the moderation's: tetrad_begin,
// tetrad_launch, tetrad_commit), the full-sample record -- the same kernel on one problem, on the moments solve_full_sample leaves in m->gram -- and the C-ABI entry
// points (plspm_tetrad_*).  Not a stage of derived_route.h's table: it reads no record of another stage, only the moment matrix.  Kernel: kernels_tetrad.h.
#include "wave_launch.h"

#include "kernels_tetrad.h"

static const char kTetPlainOnly[] = ": plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)";

static int tet_width(const plspm_model* m) { return m ? m->tet_n : 0; }
static TetradShape tet_shape(const plspm_model* m) { return {m->P, m->tet_tri, m->tet_n}; }

// `nb` problems: their moment matrices, their bootstrap records (status and iterations are read), where the tetrad records go
static int tet_launch(plspm_model* m, long nb, const MomentLayout& mom, bool dense, const double* rows, long row_stride, double* out) {
    const TetradPlan pl = tetrad_plan(tet_shape(m), nb);
    if (pl.refused) return fail(m, PLSPM_E_LIMIT, std::string("tetrad analysis: ") + tetrad_refusal());
    const char* const blob = (const char*)m->tet_desc.p;
    TetradArgs a{mom,
                 {m->L, m->tet_n, m->tet_matrix, m->d_boff, (const int*)(blob + (size_t)m->tet_n * sizeof(TetradDesc)), (const TetradDesc*)blob},
                 plspm_row_width(m), pl.waves, pl.wave_doubles, rows, row_stride, out, nb};
    return launch_wave_per_problem(m, dense ? tetrad_kernel<true> : tetrad_kernel<false>, a, pl.waves, pl.lds, pl.grid);
}

// ---- the batch driver's three calls (host_internal.h): the rule of derived_begin
int tetrad_begin(plspm_model* m, const BatchCall& call, int* runs) {
    *runs = 0;
    const bool own = !call.rows_out;
    if (!m->tet_on || !(own || call.chain_off >= 0) || !plain_metric(m) || call.kind != BatchCall::PLAIN || call.moments_out) return 0;
    if (tetrad_plan(tet_shape(m), 1).refused) return fail(m, PLSPM_E_LIMIT, std::string("tetrad analysis: ") + tetrad_refusal());      // (before anything of the call runs)
    if (own)
        if (int rc = ensure(m, m->tet_rows, (size_t)call.B * (m->tet_n + 2) * sizeof(double))) return rc;
    *runs = 1;
    return 0;
}

int tetrad_launch(plspm_model* m, int runs, long nb, int64_t pos, bool dense, const double* gram, const double* rows, long row_stride) {
    if (!runs) return 0;
    return tet_launch(m, nb, moment_layout(m, dense, gram), dense, rows, row_stride, (double*)m->tet_rows.p + pos * (m->tet_n + 2));
}

void tetrad_commit(plspm_model* m, int runs, int64_t B) {
    if (runs) m->tet_B = B;
}

static SideRecords tet_records(const plspm_model* m) {
    return {m->tet_rows, m->tet_B, tet_width(m), true,
            ": no tetrad records on this handle (plspm_tetrad_enable, then a plain bootstrap; an upload or a later call replaced them)",
            ": B differs from the last bootstrap with tetrads on this handle", ": range exceeds the replicates of the last bootstrap with tetrads",
            ": method must be 0 (percentile), 1 (basic) or 2 (bc); the jackknife writes no tetrad records, so there is no bca"};
}

extern "C" {

int plspm_tetrad_enable(plspm_model_t* m, int32_t on, const uint8_t* mask, int32_t set, int32_t matrix) {
    const std::string who = "plspm_tetrad_enable";
    if (!m) return fail(m, PLSPM_E_ARG, who + ": no handle");
    if (!on) { m->tet_on = false; return 0; }
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, who + kTetPlainOnly);
    if ((set != TETRAD_BASIS && set != TETRAD_ALL) || (matrix != TETRAD_CORRELATION && matrix != TETRAD_COVARIANCE))
        return fail(m, PLSPM_E_ARG, who + ": set must be 0 (basis) or 1 (all), matrix 0 (correlation) or 1 (covariance)");
    TetradBuild tb;
    std::string why;
    bool limit = false;
    if (tetrad_build(m->L, m->boff.data(), mask, set, tb, why, &limit)) return fail(m, limit ? PLSPM_E_LIMIT : PLSPM_E_ARG, who + ": " + why);
    if (tetrad_plan({m->P, tb.T_tri, tb.n_tet}, 1).refused) return fail(m, PLSPM_E_LIMIT, who + ": " + tetrad_refusal());
    HIPCHK(m, hipSetDevice(m->device));
    // one block: the descriptors, 8 bytes each, and behind them the triangles' offsets [L + 1]
    const size_t desc_bytes = tb.desc.size() * sizeof(TetradDesc), off_bytes = tb.tri_off.size() * sizeof(int);
    std::vector<char> blob(desc_bytes + off_bytes);
    memcpy(blob.data(), tb.desc.data(), desc_bytes);
    memcpy(blob.data() + desc_bytes, tb.tri_off.data(), off_bytes);
    if (int rc = ensure(m, m->tet_desc, blob.size())) return rc;
    HIPCHK(m, hipStreamSynchronize(m->stream));      // (nothing in flight reads the lists before them)
    HIPCHK(m, hipMemcpy(m->tet_desc.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    m->tet_set = set; m->tet_matrix = matrix; m->tet_n = tb.n_tet; m->tet_tri = tb.T_tri;
    m->tet_mask.assign((size_t)m->L, 0);
    for (int l = 0; l < m->L; ++l) m->tet_mask[l] = tb.tri_off[l + 1] != tb.tri_off[l];
    m->tet_block = std::move(tb.block); m->tet_items = std::move(tb.items);
    m->tet_B = 0;                                     // (records of other lists have another layout)
    m->tet_on = true;
    return 0;
}

int32_t plspm_tetrad_width(const plspm_model_t* m) { return tet_width(m); }

int plspm_tetrad_list(plspm_model_t* m, int32_t* n_tet, int32_t* block, int32_t* a, int32_t* b, int32_t* c, int32_t* d) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_tetrad_list: no handle");
    if (!m->tet_n) return fail(m, PLSPM_E_STATE, "plspm_tetrad_list: no tetrad lists on this handle (plspm_tetrad_enable)");
    if (n_tet) *n_tet = m->tet_n;
    int32_t* const item[4] = {a, b, c, d};
    for (int t = 0; t < m->tet_n; ++t) {
        if (block) block[t] = m->tet_block[t];
        for (int u = 0; u < 4; ++u) if (item[u]) item[u][t] = m->tet_items[4 * (size_t)t + u];
    }
    return 0;
}

int plspm_tetrad_fit(plspm_model_t* m, double* out, int32_t* status) {
    const std::string who = "plspm_tetrad_fit";
    if (!m || !out) return fail(m, PLSPM_E_ARG, who + ": bad arguments");
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, who + kTetPlainOnly);
    if (!m->tet_n) return fail(m, PLSPM_E_STATE, who + ": no tetrad lists on this handle (plspm_tetrad_enable)");
    if (!m->d_Xa || m->N < 2) return fail(m, PLSPM_E_STATE, who + ": no data uploaded");
    HIPCHK(m, hipSetDevice(m->device));
    // [the solver's record R + 2 | the tetrad record W + 2 | status, iterations (int)]
    const int RS = plspm_row_stride(m), W = tet_width(m);
    int rc;
    if ((rc = ensure(m, m->tet_fit, (size_t)(RS + W + 2) * sizeof(double) + 2 * sizeof(int)))) return rc;
    double* const rec = (double*)m->tet_fit.p;
    if ((rc = solve_full_sample(m, rec, (int*)(rec + RS + W + 2)))) return rc;      // (its moments: tile-packed, in m->gram)
    if ((rc = tet_launch(m, 1, moment_layout(m, false, (const double*)m->gram.p), false, rec, 0, rec + RS))) return rc;
    HIPCHK(m, hipGetLastError());
    std::vector<double> h((size_t)W + 2);
    HIPCHK(m, hipMemcpyAsync(h.data(), rec + RS, h.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    std::copy(h.begin(), h.begin() + W, out);
    if (status) *status = (h[W] == h[W]) ? (int32_t)h[W] : -1;
    return 0;
}

int plspm_tetrad_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) {
    return m ? side_fetch(m, tet_records(m), first, count, out, status, "plspm_tetrad_fetch") : fail(m, PLSPM_E_ARG, "plspm_tetrad_fetch: bad arguments");
}

int plspm_tetrad_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) {
    return m ? side_summary(m, tet_records(m), B, original, summary, n_used, "plspm_tetrad_summary") : fail(m, PLSPM_E_ARG, "plspm_tetrad_summary: bad arguments (1 <= B <= 2^30)");
}

int plspm_tetrad_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return m ? side_intervals(m, tet_records(m), B, original, method, level, out, n_used, "plspm_tetrad_intervals")
             : fail(m, PLSPM_E_ARG, "plspm_tetrad_intervals: bad arguments (1 <= B <= 2^30)");
}

}  // extern "C"
