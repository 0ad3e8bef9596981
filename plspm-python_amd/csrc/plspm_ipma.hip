// plspm_ipma.hip -- host side, part 14: importance-performance map analysis (IPMA).  The lists and the bounds of a handle (ipma_core.h ipma_build,
// ipma_check_bounds, at plspm_ipma_enable), the one launch behind the metric solver of a plain bootstrap's pass (plspm_bootstrap.hip hooks it in beside the
// tetrad's: ipma_begin, ipma_launch, ipma_commit), the full-sample record -- the same kernel on one problem, on the moments solve_full_sample leaves in m->gram --
// and the C-ABI entry points (plspm_ipma_*).  Not a stage of derived_route.h's table: it reads no record of another stage, only the moment matrix and the
// bootstrap record.  Kernel: kernels_ipma.h.
#include "wave_launch.h"

#include "kernels_ipma.h"

static const char kIpmaPlainOnly[] = ": plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)";

static IpmaShape ipma_shape(const plspm_model* m) { return {m->P, m->L, m->n_eff, m->ipma_nt}; }
static int ipma_w(const plspm_model* m) { return (m && m->ipma_nt) ? (int)ipma_width(ipma_shape(m)) : 0; }

// `nb` problems: their moment matrices, their bootstrap records, where the IPMA records go
static int ipma_run(plspm_model* m, long nb, const MomentLayout& mom, bool dense, const double* rows, long row_stride, double* out) {
    const IpmaPlan pl = ipma_plan(ipma_shape(m), nb);
    if (pl.refused) return fail(m, PLSPM_E_LIMIT, std::string("importance-performance map: ") + ipma_refusal());
    const int* const ints = (const int*)m->ipma_ints.p;              // lvof [P] | targets [n_t] | eff_of [L x L]
    const double* const bounds = (const double*)m->ipma_bounds.p;    // lo [P] | hi [P]
    IpmaArgs a{mom,
               {m->P, m->L, m->n_eff, m->ipma_nt, m->d_boff, ints, ints + m->P, ints + m->P + m->ipma_nt, m->d_eff_from, m->d_eff_to, m->d_shift, bounds, bounds + m->P},
               plspm_row_width(m), pl.waves, pl.wave_doubles, pl.stride, rows, row_stride, out, nb};
    return launch_wave_per_problem(m, dense ? ipma_kernel<true> : ipma_kernel<false>, a, pl.waves, pl.lds, pl.grid);
}

// ---- the batch driver's three calls (host_internal.h): the rule of derived_begin
int ipma_begin(plspm_model* m, const BatchCall& call, int* runs) {
    *runs = 0;
    const bool own = !call.rows_out;
    if (!m->ipma_on || !(own || call.chain_off >= 0) || !plain_metric(m) || call.kind != BatchCall::PLAIN || call.moments_out) return 0;
    if (ipma_plan(ipma_shape(m), 1).refused) return fail(m, PLSPM_E_LIMIT, std::string("importance-performance map: ") + ipma_refusal());      // (before anything of the call runs)
    if (own)
        if (int rc = ensure(m, m->ipma_rows, (size_t)call.B * (ipma_w(m) + 2) * sizeof(double))) return rc;
    *runs = 1;
    return 0;
}

int ipma_launch(plspm_model* m, int runs, long nb, int64_t pos, bool dense, const double* gram, const double* rows, long row_stride) {
    if (!runs) return 0;
    return ipma_run(m, nb, moment_layout(m, dense, gram), dense, rows, row_stride, (double*)m->ipma_rows.p + pos * (ipma_w(m) + 2));
}

void ipma_commit(plspm_model* m, int runs, int64_t B) {
    if (runs) m->ipma_B = B;
}

static SideRecords ipma_records(const plspm_model* m) {
    return {m->ipma_rows, m->ipma_B, ipma_w(m), true,
            ": no importance-performance records on this handle (plspm_ipma_enable, then a plain bootstrap; an upload or a later call replaced them)",
            ": B differs from the last bootstrap with the importance-performance map on this handle",
            ": range exceeds the replicates of the last bootstrap with the importance-performance map",
            ": method must be 0 (percentile), 1 (basic) or 2 (bc); the jackknife writes no importance-performance records, so there is no bca"};
}

extern "C" {

int plspm_ipma_enable(plspm_model_t* m, int32_t on, const uint8_t* targets, const double* lo, const double* hi) {
    const std::string who = "plspm_ipma_enable";
    if (!m) return fail(m, PLSPM_E_ARG, who + ": no handle");
    if (!on) { m->ipma_on = false; return 0; }
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, who + kIpmaPlainOnly);
    if (!lo || !hi) return fail(m, PLSPM_E_ARG, who + ": the bounds lo [P] and hi [P] are required");
    std::string why;
    if (ipma_check_bounds(m->P, lo, hi, why)) return fail(m, PLSPM_E_ARG, who + ": " + why);
    IpmaBuild ib;
    if (ipma_build(m->L, m->boff.data(), m->n_eff, m->eff_from.data(), m->eff_to.data(), targets, ib, why)) return fail(m, PLSPM_E_ARG, who + ": " + why);
    if (ipma_plan({m->P, m->L, m->n_eff, ib.n_t}, 1).refused) return fail(m, PLSPM_E_LIMIT, who + ": " + ipma_refusal());
    HIPCHK(m, hipSetDevice(m->device));
    std::vector<int> ints(ib.lvof);
    ints.insert(ints.end(), ib.targets.begin(), ib.targets.end());
    ints.insert(ints.end(), ib.eff_of.begin(), ib.eff_of.end());
    std::vector<double> bounds(lo, lo + m->P);
    bounds.insert(bounds.end(), hi, hi + m->P);
    int rc;
    if ((rc = ensure(m, m->ipma_ints, ints.size() * sizeof(int))) || (rc = ensure(m, m->ipma_bounds, bounds.size() * sizeof(double)))) return rc;
    HIPCHK(m, hipStreamSynchronize(m->stream));      // (nothing in flight reads the lists before them)
    HIPCHK(m, hipMemcpy(m->ipma_ints.p, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(m, hipMemcpy(m->ipma_bounds.p, bounds.data(), bounds.size() * sizeof(double), hipMemcpyHostToDevice));
    m->ipma_targets = std::move(ib.targets);
    m->ipma_nt = ib.n_t;
    m->ipma_B = 0;                                    // (records of other targets have another layout, records of other bounds other values)
    m->ipma_on = true;
    return 0;
}

int32_t plspm_ipma_width(const plspm_model_t* m) { return ipma_w(m); }

int plspm_ipma_targets(plspm_model_t* m, int32_t* n_t, int32_t* lv) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_ipma_targets: no handle");
    if (!m->ipma_nt) return fail(m, PLSPM_E_STATE, "plspm_ipma_targets: no importance-performance map on this handle (plspm_ipma_enable)");
    if (n_t) *n_t = m->ipma_nt;
    if (lv) for (int k = 0; k < m->ipma_nt; ++k) lv[k] = m->ipma_targets[k];
    return 0;
}

int plspm_ipma_fit(plspm_model_t* m, double* out, int32_t* status) {
    const std::string who = "plspm_ipma_fit";
    if (!m || !out) return fail(m, PLSPM_E_ARG, who + ": bad arguments");
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, who + kIpmaPlainOnly);
    if (!m->ipma_nt) return fail(m, PLSPM_E_STATE, who + ": no importance-performance map on this handle (plspm_ipma_enable)");
    if (!m->d_Xa || m->N < 2) return fail(m, PLSPM_E_STATE, who + ": no data uploaded");
    HIPCHK(m, hipSetDevice(m->device));
    // [the solver's record R + 2 | the IPMA record W + 2 | status, iterations (int)]
    const int RS = plspm_row_stride(m), W = ipma_w(m);
    int rc;
    if ((rc = ensure(m, m->ipma_fit, (size_t)(RS + W + 2) * sizeof(double) + 2 * sizeof(int)))) return rc;
    double* const rec = (double*)m->ipma_fit.p;
    if ((rc = solve_full_sample(m, rec, (int*)(rec + RS + W + 2)))) return rc;      // (its moments: tile-packed, in m->gram)
    if ((rc = ipma_run(m, 1, moment_layout(m, false, (const double*)m->gram.p), false, rec, 0, rec + RS))) return rc;
    HIPCHK(m, hipGetLastError());
    std::vector<double> h((size_t)W + 2);
    HIPCHK(m, hipMemcpyAsync(h.data(), rec + RS, h.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    std::copy(h.begin(), h.begin() + W, out);
    if (status) *status = (h[W] == h[W]) ? (int32_t)h[W] : -1;
    return 0;
}

int plspm_ipma_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) {
    return m ? side_fetch(m, ipma_records(m), first, count, out, status, "plspm_ipma_fetch") : fail(m, PLSPM_E_ARG, "plspm_ipma_fetch: bad arguments");
}

int plspm_ipma_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) {
    return m ? side_summary(m, ipma_records(m), B, original, summary, n_used, "plspm_ipma_summary") : fail(m, PLSPM_E_ARG, "plspm_ipma_summary: bad arguments (1 <= B <= 2^30)");
}

int plspm_ipma_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return m ? side_intervals(m, ipma_records(m), B, original, method, level, out, n_used, "plspm_ipma_intervals")
             : fail(m, PLSPM_E_ARG, "plspm_ipma_intervals: bad arguments (1 <= B <= 2^30)");
}

}  // extern "C"
