// plspm_rebus.hip -- host side, part 15: REBUS-PLS, response-based unit segmentation.  A round is K local models -- problem k = the rows whose label is
// k, a 0/1 count row (kernels_rebus.h) through the bootstrap's int8 Gram (run_gram_i8) and batch solver, as the jackknife does it, records in buffers of their own --
// then one pass over all rows against the K fitted models and the assignment.  The driver is host-driven, one iteration per round: it reads back `changed`, the
// class sizes and the validity flags through pinned memory; the labels stay on the device.
#include "host_internal.h"

#include "wave_ops.h"
#include "kernels_rebus.h"

int launch_rebus_counts(plspm_model* m, const RebusSpec& rs, int64_t nb, int64_t prob0, int MT, int KB, void* cd) {
    hipLaunchKernelGGL(rebus_counts_kernel, count_rows_grid(nb, KB), dim3(COUNT_NT), 0, m->stream, (int)m->N, KB, MT, prob0, (int)nb, rs.d_label, (uint4*)cd);
    HIPCHK(m, hipGetLastError());
    return 0;
}

// the LVs that have predecessors, ascending
static std::vector<int> rebus_endo(const plspm_model* m) {
    std::vector<int> e;
    for (int l = 0; l < m->L; ++l) if (m->pred_off[l + 1] > m->pred_off[l]) e.push_back(l);
    return e;
}

// What the calls share once their arguments stand: the plan, the small tables on the device, the buffers of a round at K classes
struct RebusRun {
    plspm_model* m; int K, n_endo, PD, W; RebusPlan plan;
    const int *d_endo, *d_eff_of;
};
static int rebus_begin(plspm_model* m, int K, bool final_pass, bool store, const char* who, RebusRun* run) {
    const std::vector<int> endo = rebus_endo(m);
    const int P = m->P, L = m->L, ne = (int)endo.size();
    RebusRun& r = *run;
    r.m = m; r.K = K; r.n_endo = ne; r.PD = rebus_param_doubles(P, L, ne); r.W = P + ne;
    r.plan = rebus_plan(RebusShape{P, L, ne, K, (long)m->N}, m->tune.rebus_classes);
    if (r.plan.refused) return fail(m, PLSPM_E_LIMIT, std::string(who) + ": " + rebus_refusal());
    int rc;
    // small tables: [endo n_endo | eff_of n_endo x L]
    std::vector<int> tab((size_t)ne + (size_t)ne * L, -1);
    std::copy(endo.begin(), endo.end(), tab.begin());
    for (int jj = 0; jj < ne; ++jj) {
        const int j = endo[(size_t)jj];
        for (int e = m->pred_off[j]; e < m->pred_off[j + 1]; ++e) {
            int found = -1;
            for (int x = 0; x < m->n_eff; ++x) if (m->eff_from[x] == m->pred_idx[e] && m->eff_to[x] == j) found = x;
            if (found < 0) return fail(m, PLSPM_E_STATE, std::string(who) + ": a path of the model has no effect pair");
            tab[(size_t)ne + (size_t)jj * L + m->pred_idx[e]] = found;
        }
    }
    if ((rc = ensure(m, m->rebus_tab, tab.size() * sizeof(int)))) return rc;
    if ((rc = plspm_detail_h2d(m, m->rebus_tab.p, tab.data(), tab.size() * sizeof(int)))) return rc;
    r.d_endo = (const int*)m->rebus_tab.p; r.d_eff_of = r.d_endo + ne;
    const size_t N = (size_t)m->N, tiles = (size_t)r.plan.tiles;
    if ((rc = ensure(m, m->rebus_label, N * sizeof(int))) || (rc = ensure(m, m->rebus_rows, (size_t)K * plspm_row_stride(m) * sizeof(double))) ||
        (rc = ensure(m, m->rebus_mom, (size_t)K * r.plan.slices * (2 * P + 1) * sizeof(double))) || (rc = ensure(m, m->rebus_par, (size_t)K * r.PD * sizeof(double))) ||
        (rc = ensure(m, m->rebus_flags, (size_t)K * sizeof(int))) || (rc = ensure(m, m->rebus_ab, (size_t)2 * K * N * sizeof(double))) ||
        (rc = ensure(m, m->rebus_part, (size_t)2 * K * tiles * sizeof(double))))
        return rc;
    if (final_pass && ((rc = ensure(m, m->rebus_cm, N * K * sizeof(double))) || (rc = ensure(m, m->rebus_within_part, tiles * K * r.W * sizeof(double))) ||
                       (rc = ensure(m, m->rebus_within, (size_t)K * r.W * sizeof(double)))))
        return rc;
    if (store && (rc = ensure(m, m->rebus_resid, N * r.W * sizeof(double)))) return rc;
    if (!m->rebus_pin.p) HIPCHK(m, m->rebus_pin.reserve((size_t)(1 + 2 * kRebusMaxClasses) * sizeof(int)));
    return 0;
}

// One round on the labels as they are: the K local models, their moments and parameters, the row pass; then
//   mode 0: the assignment into the labels, counters at `ctr`;  mode 1 (final pass): CM and the members-only sums, no assignment;  mode 2: every residual (K = 1).
// Returns with the round's flags [K] (and, mode 0, changed | sizes [K]) in the pinned block: flags at [1 + K ..), counters at [0 .. K].
static int rebus_round(const RebusRun& r, int mode, int* d_ctr) {
    plspm_model* m = r.m;
    const int K = r.K, P = m->P, L = m->L, N = (int)m->N, RS = plspm_row_stride(m);
    const RebusPlan& pl = r.plan;
    int rc;
    const int* d_label = (const int*)m->rebus_label.p;
    const RebusSpec spec{K, d_label};
    BatchCall call;
    call.kind = BatchCall::REBUS; call.rebus = &spec; call.B = K;       // problem k = the rows of class k
    call.rows_out = (double*)m->rebus_rows.p; call.status_out = &m->rebus_status; call.iters_out = &m->rebus_iters;
    if ((rc = plspm_detail_bootstrap(m, call))) return rc;
    double* d_A = (double*)m->rebus_ab.p;
    double* d_B = d_A + (size_t)K * N;
    double* d_pA = (double*)m->rebus_part.p;
    double* d_pB = d_pA + (size_t)K * pl.tiles;
    {
        ProfScope ps(m, PLSPM_K_REDUCE);
        hipLaunchKernelGGL(rebus_moments_kernel, dim3((unsigned)K, (unsigned)pl.slices), dim3(256), 0, m->stream, (const double*)m->d_Xa, m->PA, P, N, pl.slice_rows, d_label,
                           (double*)m->rebus_mom.p);
        const RebusModel md{P, L, r.n_endo, m->n_eff, m->scaled, m->d_boff, m->d_lvof, r.d_endo, r.d_eff_of, m->d_shift};
        const size_t lds = ((size_t)4 * P + L) * sizeof(double);
        if ((rc = allow_lds(m, (const void*)rebus_compose_kernel, lds))) return rc;
        hipLaunchKernelGGL(rebus_compose_kernel, dim3((unsigned)K), dim3(64), lds, m->stream, md, (const double*)m->rebus_rows.p, RS, (const int*)m->rebus_status.p,
                           (const double*)m->rebus_mom.p, pl.slices, (double*)m->rebus_par.p, (int*)m->rebus_flags.p);
    }
    {
        auto kernel = mode == 0 ? rebus_residual_kernel<false, false> : (mode == 1 ? rebus_residual_kernel<true, false> : rebus_residual_kernel<false, true>);
        if ((rc = allow_lds(m, (const void*)kernel, (size_t)pl.lds_bytes))) return rc;
        ProfScope ps(m, PLSPM_K_REDUCE);
        hipLaunchKernelGGL(kernel, dim3((unsigned)pl.tiles), dim3(kRebusThreads), (size_t)pl.lds_bytes, m->stream, (const double*)m->d_Xa, m->PA, P, L, r.n_endo, N, K, pl.classes_per_load,
                           pl.xs, (const int*)m->d_boff, r.d_endo, (const double*)m->rebus_par.p, d_label, d_A, d_B, d_pA, d_pB, mode == 1 ? (double*)m->rebus_within_part.p : nullptr,
                           mode == 2 ? (double*)m->rebus_resid.p : nullptr);
        m->last_rebus_loads = pl.loads;
        if (mode == 1)
            hipLaunchKernelGGL(rebus_within_kernel, dim3((unsigned)K), dim3(256), 0, m->stream, (const double*)m->rebus_within_part.p, pl.tiles, K, r.W, (double*)m->rebus_within.p);
        if (mode != 2)
            hipLaunchKernelGGL(rebus_assign_kernel, dim3((unsigned)pl.assign_grid), dim3(kRebusThreads), 0, m->stream, N, K, pl.tiles, (const double*)d_A, (const double*)d_B,
                               (const double*)d_pA, (const double*)d_pB, (const int*)m->rebus_flags.p, mode == 0 ? 1 : 0, (int*)m->rebus_label.p,
                               mode == 1 ? (double*)m->rebus_cm.p : nullptr, d_ctr);
    }
    HIPCHK(m, hipGetLastError());
    int* pin = (int*)m->rebus_pin.p;
    if (mode == 0) HIPCHK(m, hipMemcpyAsync(pin, d_ctr, (size_t)(1 + K) * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipMemcpyAsync(pin + 1 + K, m->rebus_flags.p, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return 0;
}

static int rebus_scope(plspm_model* m, const char* who) {
    int rc;
    if ((rc = counts_call_scope(m, who))) return rc;
    if (!std::all_of(m->mode.begin(), m->mode.end(), [](int mode) { return mode == PLSPM_MODE_A; })) return fail(m, PLSPM_E_ARG, std::string(who) + ": every block must be Mode A");
    if (m->pred_idx.empty()) return fail(m, PLSPM_E_ARG, std::string(who) + ": the model has no path");
    return 0;
}

extern "C" {

int plspm_rebus_device(plspm_model_t* m, int32_t K, const int32_t* start, int32_t max_iter, double stop_crit, int64_t min_size, void** d_labels, void** d_cm) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_rebus_device: no handle");
    if (K < 1 || K > kRebusMaxClasses || !start || max_iter < 0 || max_iter > (1 << 20) || !(stop_crit >= 0.0) || min_size < 1)
        return fail(m, PLSPM_E_ARG, "plspm_rebus_device: bad arguments (1 <= K <= 16, start labels, 0 <= max_iter <= 2^20, stop_crit >= 0, min_size >= 1)");
    int rc;
    if ((rc = rebus_scope(m, "plspm_rebus_device"))) return rc;
    const int64_t N = m->N;
    std::vector<int> sizes((size_t)K, 0);
    for (int64_t i = 0; i < N; ++i) {
        if (start[i] < 0 || start[i] >= K) return fail(m, PLSPM_E_ARG, "plspm_rebus_device: a start label is not below K");
        ++sizes[(size_t)start[i]];
    }
    if ((rc = counts_route_scope(m, "plspm_rebus_device"))) return rc;
    m->rebus_K = 0;
    RebusRun run;
    if ((rc = rebus_begin(m, K, true, false, "plspm_rebus_device", &run))) return rc;
    const size_t ctr_bytes = ((size_t)max_iter + 1) * (1 + K) * sizeof(int);
    if ((rc = ensure(m, m->rebus_ctr, ctr_bytes))) return rc;
    HIPCHK(m, hipMemsetAsync(m->rebus_ctr.p, 0, ctr_bytes, m->stream));
    if ((rc = plspm_detail_h2d(m, m->rebus_label.p, start, (size_t)N * sizeof(int)))) return rc;
    const int* pin = (const int*)m->rebus_pin.p;
    auto small = [&]() { return std::any_of(sizes.begin(), sizes.end(), [&](int n) { return n < min_size; }); };
    auto invalid = [&]() { return std::any_of(pin + 1 + K, pin + 1 + 2 * K, [](int f) { return f == 0; }); };
    int status = -1, t = 0, iterations = 0;
    while (status < 0) {
        if (t == max_iter) { status = PLSPM_NOT_CONVERGED; iterations = t; break; }
        // iteration t + 1 on the labels of iteration t
        if (small()) { status = PLSPM_SINGULAR; iterations = t + 1; break; }
        if ((rc = rebus_round(run, 0, (int*)m->rebus_ctr.p + (size_t)t * (1 + K)))) return rc;
        if (invalid()) { status = PLSPM_SINGULAR; iterations = t + 1; break; }       // (the assignment left labels and counters alone)
        ++t;
        std::copy(pin + 1, pin + 1 + K, sizes.begin());
        if ((double)pin[0] / (double)N < stop_crit) { status = PLSPM_OK; iterations = t; }
    }
    // the final pass on the labels of iteration t: the reported local models, CM and the within-class sums
    if (status != PLSPM_SINGULAR) {
        if (small()) status = PLSPM_SINGULAR;
        else {
            if ((rc = rebus_round(run, 1, nullptr))) return rc;
            if (invalid()) status = PLSPM_SINGULAR;
        }
    }
    m->rebus_K = K; m->rebus_status_run = status; m->rebus_iters_run = iterations; m->rebus_hist = t; m->rebus_sizes = sizes;
    if (d_labels) *d_labels = m->rebus_label.p;
    if (d_cm) *d_cm = status == PLSPM_SINGULAR ? nullptr : m->rebus_cm.p;
    return 0;
}

int plspm_rebus_fetch(plspm_model_t* m, int32_t* labels, double* cm, double* records, int32_t* rec_status, int32_t* rec_iters, int64_t* sizes, double* within_e, double* within_f,
                      int32_t* run, int32_t* hist_changed, int32_t* hist_sizes) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_rebus_fetch: no handle");
    if (!m->rebus_K) return fail(m, PLSPM_E_STATE, "plspm_rebus_fetch: no REBUS run on this handle (no plspm_rebus_device yet, or an upload replaced the data)");
    HIPCHK(m, hipSetDevice(m->device));
    const int K = m->rebus_K, P = m->P, R = plspm_row_width(m), RS = plspm_row_stride(m), ne = (int)rebus_endo(m).size(), W = P + ne, H = m->rebus_hist;
    const size_t N = (size_t)m->N;
    const bool nan_out = m->rebus_status_run == PLSPM_SINGULAR;
    const double nan = __builtin_nan("");
    int rc;
    if (labels) HIPCHK(m, hipMemcpyAsync(labels, m->rebus_label.p, N * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    std::vector<int> ctr((size_t)H * (1 + K));
    if (H && (hist_changed || hist_sizes)) HIPCHK(m, hipMemcpyAsync(ctr.data(), m->rebus_ctr.p, ctr.size() * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    std::vector<double> wk((size_t)K * W);
    if (!nan_out) {
        if (cm) HIPCHK(m, hipMemcpyAsync(cm, m->rebus_cm.p, N * K * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        if (within_e || within_f) HIPCHK(m, hipMemcpyAsync(wk.data(), m->rebus_within.p, wk.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (!nan_out) {
        if ((records || rec_status || rec_iters) && (rc = plspm_detail_fetch_records(m, (const double*)m->rebus_rows.p, K, RS, records, rec_status, rec_iters))) return rc;
    } else {
        if (cm) std::fill(cm, cm + N * K, nan);
        if (records) std::fill(records, records + (size_t)K * R, nan);
        if (rec_status) std::fill(rec_status, rec_status + K, -1);
        if (rec_iters) std::fill(rec_iters, rec_iters + K, -1);
        std::fill(wk.begin(), wk.end(), nan);
    }
    for (int k = 0; k < K; ++k) {
        if (within_e) std::copy(wk.begin() + (size_t)k * W, wk.begin() + (size_t)k * W + P, within_e + (size_t)k * P);
        if (within_f) std::copy(wk.begin() + (size_t)k * W + P, wk.begin() + (size_t)(k + 1) * W, within_f + (size_t)k * ne);
        if (sizes) sizes[k] = m->rebus_sizes[(size_t)k];
    }
    if (run) { run[0] = m->rebus_status_run; run[1] = m->rebus_iters_run; run[2] = H; }
    for (int t = 0; t < H; ++t) {
        if (hist_changed) hist_changed[t] = ctr[(size_t)t * (1 + K)];
        if (hist_sizes) std::copy(ctr.begin() + (size_t)t * (1 + K) + 1, ctr.begin() + (size_t)(t + 1) * (1 + K), hist_sizes + (size_t)t * K);
    }
    return 0;
}

int plspm_rebus_residuals(plspm_model_t* m, double* out) {
    if (!m || !out) return fail(m, PLSPM_E_ARG, "plspm_rebus_residuals: bad arguments");
    int rc;
    if ((rc = rebus_scope(m, "plspm_rebus_residuals")) || (rc = counts_route_scope(m, "plspm_rebus_residuals"))) return rc;
    m->rebus_K = 0;                                           // (the round below overwrites a run's local records)
    RebusRun run;
    if ((rc = rebus_begin(m, 1, false, true, "plspm_rebus_residuals", &run))) return rc;
    HIPCHK(m, hipMemsetAsync(m->rebus_label.p, 0, (size_t)m->N * sizeof(int), m->stream));
    if ((rc = rebus_round(run, 2, nullptr))) return rc;
    HIPCHK(m, hipMemcpyAsync(out, m->rebus_resid.p, (size_t)m->N * run.W * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return 0;
}

}  // extern "C"
