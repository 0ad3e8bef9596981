// plspm_jackknife.hip -- host side, part 7: the jackknife.  Problem g of G leaves out the rows i with i % G == g (G = N: the ordinary leave-one-out
// jackknife; G < N: delete-a-group) and is problem g of the bootstrap's int8 route: a 0/1 count row (kernels_jack.h) through the same Gram
// (run_gram_i8) and batch solver, as the two-group tests and the cross-validation do it (plspm_permute.hip, plspm_cv.hip).  Records, status and
// iteration counts go into buffers of their own, so that the bootstrap whose BCa intervals ask for the acceleration keeps its records bit for bit.
#include "host_internal.h"

#include "wave_ops.h"
#include "kernels_jack.h"

int launch_jack_counts(plspm_model* m, const JackSpec& js, int64_t nb, int64_t prob0, int MT, int KB, void* cd) {
    hipLaunchKernelGGL(jack_counts_kernel, count_rows_grid(nb, KB), dim3(COUNT_NT), 0, m->stream, (int)m->N, KB, MT, (int)js.G, prob0, (int)nb, (uint4*)cd);
    HIPCHK(m, hipGetLastError());
    return 0;
}

// the last plspm_jackknife_device call's records are still on the handle, and they are G's
static int jack_state(plspm_model* m, int64_t G, const char* who) {
    if (!m->jack_G || !m->jack_rows.p) return fail(m, PLSPM_E_STATE, std::string(who) + ": no jackknife on this handle (no plspm_jackknife_device yet, or an upload replaced the data)");
    if (G != m->jack_G) return fail(m, PLSPM_E_ARG, std::string(who) + ": G is not the last plspm_jackknife_device call's");
    return 0;
}

extern "C" {

int plspm_jackknife_device(plspm_model_t* m, int64_t G, void** d_out, void** d_status, void** d_iters) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_jackknife_device: no handle");
    int rc;
    if ((rc = counts_call_scope(m, "plspm_jackknife_device"))) return rc;
    const int64_t N = m->N;
    if (G < 2 || G > N || N - (N + G - 1) / G < 4)
        return fail(m, PLSPM_E_ARG, "plspm_jackknife_device: bad G (2 <= G <= N, and every problem keeps at least four rows)");
    if ((rc = counts_route_scope(m, "plspm_jackknife_device"))) return rc;
    void_records(m, REC_JACK);
    if ((rc = ensure(m, m->jack_rows, (size_t)G * plspm_row_stride(m) * sizeof(double)))) return rc;
    const JackSpec spec{G};
    BatchCall call;
    call.kind = BatchCall::JACKKNIFE; call.jack = &spec; call.B = G;       // problem g = the rows i with i % G != g
    call.rows_out = (double*)m->jack_rows.p; call.status_out = &m->jack_status; call.iters_out = &m->jack_iters;
    if ((rc = plspm_detail_bootstrap(m, call))) return rc;
    m->jack_G = G;
    hand_out(m->jack_rows, m->jack_status, m->jack_iters, d_out, d_status, d_iters);
    return 0;
}

int plspm_jackknife_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status, int32_t* iters) {
    if (!m || first < 0 || count < 1) return fail(m, PLSPM_E_ARG, "plspm_jackknife_fetch: bad arguments");
    if (!m->jack_G || !m->jack_rows.p) return fail(m, PLSPM_E_STATE, "plspm_jackknife_fetch: no jackknife on this handle (no plspm_jackknife_device yet, or an upload replaced the data)");
    if (first + count > m->jack_G) return fail(m, PLSPM_E_ARG, "plspm_jackknife_fetch: range exceeds the last jackknife's problems");
    HIPCHK(m, hipSetDevice(m->device));
    const int RS = plspm_row_stride(m);
    return plspm_detail_fetch_records(m, (const double*)m->jack_rows.p + first * RS, count, RS, out, status, iters);
}

int plspm_jackknife_stats(plspm_model_t* m, int64_t G, double* mean, double* std_error, double* accel, int64_t* n_used) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_jackknife_stats: no handle");
    int rc;
    if ((rc = jack_state(m, G, "plspm_jackknife_stats"))) return rc;
    HIPCHK(m, hipSetDevice(m->device));
    const int R = plspm_row_width(m), RS = plspm_row_stride(m);
    // [mean R | std_error R | accel R | n_used]
    if ((rc = ensure(m, m->jack_io, (size_t)(3 * R + 1) * sizeof(double)))) return rc;
    double* d_out = (double*)m->jack_io.p;
    {
        ProfScope ps(m, PLSPM_K_REDUCE);
        hipLaunchKernelGGL(jack_stats_kernel, dim3((unsigned)R), dim3(JACK_NT), 0, m->stream, (const double*)m->jack_rows.p, (long)G, RS, R, d_out, (int*)(d_out + 3 * R));
    }
    HIPCHK(m, hipGetLastError());
    std::vector<double> h((size_t)3 * R + 1);
    HIPCHK(m, hipMemcpyAsync(h.data(), d_out, h.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (mean) std::copy(h.begin(), h.begin() + R, mean);
    if (std_error) std::copy(h.begin() + R, h.begin() + 2 * R, std_error);
    if (accel) std::copy(h.begin() + 2 * R, h.begin() + 3 * R, accel);
    if (n_used) { int n; memcpy(&n, &h[(size_t)3 * R], sizeof(int)); *n_used = n; }
    return 0;
}

}  // extern "C"
