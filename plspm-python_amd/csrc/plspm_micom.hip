// plspm_micom.hip -- host side, part 9: MICOM, the permutation test of measurement invariance of composite models.  The pooled inputs of the
// resident rows (once per upload), the launch of the per-permutation kernel behind a permutation batch's solver (plspm_bootstrap.hip hooks it in beside the
// chain of plspm_derived.hip), the counts on the records in HBM and the C-ABI entry points (plspm_micom_*).  Kernels: kernels_micom.h (its opening: kernels_moments.h).
#include "wave_launch.h"

#include "wave_ops.h"
#include "kernels_micom.h"

static inline int micom_width(const plspm_model* m) { return 3 * m->L; }
static inline int micom_largest_block(const plspm_model* m) {
    int kb = 1;
    for (int l = 0; l < m->L; ++l) kb = std::max(kb, m->boff[l + 1] - m->boff[l]);
    return kb;
}
static inline long micom_r0_doubles(const plspm_model* m) {
    long s = 0;
    for (int l = 0; l < m->L; ++l) { const long k = m->boff[l + 1] - m->boff[l]; s += k * k; }
    return s;
}

// m->micom_pool: [u P | s_0 P | R_0's diagonal blocks | the full-sample problem's record RS | its status, iterations (int)]
int micom_prepare(plspm_model* m) {
    if (m->micom_pool_valid) return 0;
    const int P = m->P, RS = plspm_row_stride(m);
    const long K2 = micom_r0_doubles(m);
    int rc;
    if ((rc = ensure(m, m->micom_pool, (size_t)(2L * P + K2 + RS) * sizeof(double) + 2 * sizeof(int)))) return rc;
    double* u = (double*)m->micom_pool.p;
    double *s0 = u + P, *r0 = s0 + P, *rec = r0 + K2;
    if ((rc = solve_full_sample(m, rec, (int*)(rec + RS)))) return rc;      // (its moments: tile-packed, in m->gram)
    hipLaunchKernelGGL(micom_pooled_kernel, dim3(1), dim3(64), 0, m->stream, (const double*)m->gram.p, m->T, P, m->L, (const int*)m->d_boff, (const double*)rec, plspm_row_width(m), u, s0, r0);
    HIPCHK(m, hipGetLastError());
    m->micom_pool_valid = true;
    return 0;
}

int launch_micom(plspm_model* m, long nperm, bool dense, const double* gram, const double* rows, double* out) {
    const int kb = micom_largest_block(m);
    MicomArgs a{};
    a.mom = moment_layout(m, dense, gram);
    a.L = m->L; a.R = plspm_row_width(m); a.kb = kb;
    a.boff = m->d_boff;
    a.rows = rows; a.row_stride = plspm_row_stride(m);
    a.u = (const double*)m->micom_pool.p; a.r0 = a.u + 2L * m->P;
    a.out = out; a.np = nperm;
    if (int rc = launch_wave_per_problem(m, dense ? micom_kernel<true> : micom_kernel<false>, a, MICOM_WAVES, (size_t)MICOM_WAVES * micom_wave_doubles(kb) * sizeof(double), (nperm + MICOM_WAVES - 1) / MICOM_WAVES)) return rc;
    m->last_micom_layout = dense ? 1 : 2;
    return 0;
}

// the handle's MICOM records as the entry points below share them with the assessment's (host_internal.h SideRecords)
static SideRecords micom_records(const plspm_model* m) {
    return {m->micom_rows, m->micom_B, micom_width(m), true,
            ": no MICOM records on this handle (plspm_micom_enable, then plspm_permutation_device; an upload or a later call replaced them)",
            ": B differs from the last MICOM permutation call on this handle", ": range exceeds the last MICOM permutation call's permutations",
            ": method must be 0 (percentile), 1 (basic) or 2 (bc)"};
}

extern "C" {

int plspm_micom_enable(plspm_model_t* m, int32_t on) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_micom_enable: no handle");
    if (on && !plain_metric(m)) return fail(m, PLSPM_E_ARG, "plspm_micom_enable: plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)");
    m->micom_on = on != 0;
    return 0;
}

int32_t plspm_micom_width(const plspm_model_t* m) { return m ? micom_width(m) : 0; }

int plspm_micom_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) {
    return m ? side_fetch(m, micom_records(m), first, count, out, status, "plspm_micom_fetch") : fail(m, PLSPM_E_ARG, "plspm_micom_fetch: bad arguments");
}

int plspm_micom_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) {
    return m ? side_summary(m, micom_records(m), B, original, summary, n_used, "plspm_micom_summary") : fail(m, PLSPM_E_ARG, "plspm_micom_summary: bad arguments (1 <= B <= 2^30)");
}

int plspm_micom_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return m ? side_intervals(m, micom_records(m), B, original, method, level, out, n_used, "plspm_micom_intervals") : fail(m, PLSPM_E_ARG, "plspm_micom_intervals: bad arguments (1 <= B <= 2^30)");
}

int plspm_micom_counts(plspm_model_t* m, int64_t B, const double* observed, int64_t* below, int64_t* exceed, int64_t* n_used) {
    if (!m || B < 1 || !observed || !below || !exceed) return fail(m, PLSPM_E_ARG, "plspm_micom_counts: bad arguments");
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, "plspm_micom_counts: plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)");
    int rc;
    if ((rc = side_state(m, micom_records(m), B, "plspm_micom_counts"))) return rc;
    HIPCHK(m, hipSetDevice(m->device));
    const int W = micom_width(m);
    // [observed W | below W | exceed W | valid records]
    if ((rc = ensure(m, m->micom_io, (size_t)(3 * W + 1) * sizeof(double)))) return rc;
    double* d_obs = (double*)m->micom_io.p;
    unsigned long long* d_cnt = (unsigned long long*)(d_obs + W);
    HIPCHK(m, hipMemcpyAsync(d_obs, observed, (size_t)W * sizeof(double), hipMemcpyHostToDevice, m->stream));
    {
        ProfScope ps(m, PLSPM_K_REDUCE);
        hipLaunchKernelGGL(micom_count_kernel, dim3((unsigned)W), dim3(MICOM_COUNT_NT), 0, m->stream, (const double*)m->micom_rows.p, (long)B, W, (const double*)d_obs, d_cnt, d_cnt + W,
                           d_cnt + 2 * W);
    }
    HIPCHK(m, hipGetLastError());
    std::vector<unsigned long long> h((size_t)2 * W + 1);
    HIPCHK(m, hipMemcpyAsync(h.data(), d_cnt, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    for (int j = 0; j < W; ++j) { below[j] = (int64_t)h[(size_t)j]; exceed[j] = (int64_t)h[(size_t)W + j]; }
    if (n_used) *n_used = (int64_t)h[(size_t)2 * W];
    return 0;
}

}  // extern "C"
