// plspm_fimix.hip -- host side, part 9: FIMIX-PLS, the latent-class segmentation of the inner model.  A call's problems -- (K, an initial assignment of
// the rows) each -- are independent EM iterations on the scores the last fit left on the handle: one launch, one persistent workgroup per problem (kernels_fimix.h),
// as fimix_route.h plans it.  Records, status and iteration counts live in buffers of their own; nothing here reads or voids a bootstrap's records.
#include "host_internal.h"

#include "kernels_fimix.h"

// What the handle's path matrix fixes, host side: pred_off [L + 1] | pred_idx [n_dir] | endo [n_endo] | dir_of [n_dir] | ent [E] as one block of ints
struct FimixTables { FimixShape shape; std::vector<int> ints; size_t o_pred_idx, o_endo, o_dir_of, o_ent; };
static FimixTables fimix_tables(const plspm_model* m) {
    FimixTables t{};
    const int L = m->L, n_dir = (int)m->pred_idx.size();
    std::vector<int> endo, dir_of((size_t)n_dir, 0), ent((size_t)L * (L + 1) / 2);
    int kmax_pred = 0;
    for (int j = 0; j < L; ++j) {
        const int k = m->pred_off[j + 1] - m->pred_off[j];
        if (k) endo.push_back(j);
        kmax_pred = std::max(kmax_pred, k);
    }
    // direct paths from-major (the order of plspm_structural_paths): path d = (f, t); edge e of the predecessor lists is (pred_idx[e], its LV)
    int dpath = 0;
    for (int f = 0; f < L; ++f)
        for (int to = 0; to < L; ++to)
            for (int e = m->pred_off[to]; e < m->pred_off[to + 1]; ++e)
                if (m->pred_idx[e] == f) dir_of[(size_t)e] = dpath++;
    const int E = fimix_entries(L, m->pred_off.data(), m->pred_idx.data(), ent.data());
    ent.resize((size_t)E);
    t.shape = FimixShape{(long)m->N, L, n_dir, (int)endo.size(), kmax_pred, E};
    t.ints.assign(m->pred_off.begin(), m->pred_off.begin() + L + 1);
    t.o_pred_idx = t.ints.size(); t.ints.insert(t.ints.end(), m->pred_idx.begin(), m->pred_idx.end());
    t.o_endo = t.ints.size(); t.ints.insert(t.ints.end(), endo.begin(), endo.end());
    t.o_dir_of = t.ints.size(); t.ints.insert(t.ints.end(), dir_of.begin(), dir_of.end());
    t.o_ent = t.ints.size(); t.ints.insert(t.ints.end(), ent.begin(), ent.end());
    return t;
}
static FimixDesc fimix_desc(const FimixTables& t, const int* d_ints) {
    const FimixShape& s = t.shape;
    return FimixDesc{s.L, s.n_endo, s.n_dir, s.kmax_pred, s.E, d_ints, d_ints + t.o_pred_idx, d_ints + t.o_endo, d_ints + t.o_dir_of, d_ints + t.o_ent};
}

static int fimix_scope(plspm_model* m, const char* who) {
    if (m->stage1 || m->stage2) return fail(m, PLSPM_E_ARG, std::string(who) + ": plain metric models only (this handle is part of a two-stage pair)");
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, std::string(who) + ": plain metric models only (no non-metric scales, no missing values)");
    return 0;
}
static int fimix_state(plspm_model* m, const char* who) {
    if (!m->fimix_nprob || !m->fimix_rows.p) return fail(m, PLSPM_E_STATE, std::string(who) + ": no FIMIX problems on this handle (no plspm_fimix_device yet, or an upload replaced the data)");
    return 0;
}

extern "C" {

int plspm_fimix_starts(uint64_t seed, int64_t start, int64_t N, int32_t K, uint8_t* segment) {
    if (!segment || K < 1 || K > kFimixMaxK || N < 1 || N > 0x7fffffffLL || start < 0) return PLSPM_E_ARG;
    for (int64_t i = 0; i < N; ++i) segment[i] = (uint8_t)fimix_start_segment(seed, (uint64_t)start, (uint32_t)i, (uint32_t)K);
    return 0;
}

int32_t plspm_fimix_width(const plspm_model_t* m, int32_t kmax) {
    if (!m || kmax < 1 || kmax > kFimixMaxK) return 0;
    int n_endo = 0;
    for (int j = 0; j < m->L; ++j) n_endo += m->pred_off[j + 1] > m->pred_off[j];
    return fimix_record_width(kmax, (int)m->pred_idx.size(), n_endo);
}

int plspm_fimix_device(plspm_model_t* m, int64_t nprob, const int32_t* k_of, int32_t kmax, uint64_t seed, int64_t start_offset, const uint8_t* init, int32_t max_iter, double tol,
                       void** d_out, void** d_status, void** d_iters) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_fimix_device: no handle");
    if (nprob < 1 || nprob > ((int64_t)1 << 24) || !k_of || kmax < 1 || kmax > kFimixMaxK || max_iter < 1 || !(tol >= 0.0) || start_offset < 0 || start_offset > ((int64_t)1 << 61))
        return fail(m, PLSPM_E_ARG, "plspm_fimix_device: bad arguments (1 <= nprob <= 2^24, k_of, 1 <= kmax <= 16, max_iter >= 1, tol >= 0, start_offset >= 0)");
    for (int64_t p = 0; p < nprob; ++p)
        if (k_of[p] < 1 || k_of[p] > kmax) return fail(m, PLSPM_E_ARG, "plspm_fimix_device: every K lies in 1 .. kmax (kmax <= 16)");
    int rc;
    if ((rc = fimix_scope(m, "plspm_fimix_device"))) return rc;
    if (!m->d_Xa || m->N < 2 || !m->scores_valid || !m->scores.p)
        return fail(m, PLSPM_E_STATE, "plspm_fimix_device: the handle holds no scores of a fit on the rows now resident (plspm_fit with scores first)");
    if (m->pred_idx.empty()) return fail(m, PLSPM_E_ARG, "plspm_fimix_device: the model has no path");
    const int64_t N = m->N;
    if (init)
        for (int64_t p = 0; p < nprob; ++p)
            for (int64_t i = 0; i < N; ++i)
                if (init[p * N + i] >= k_of[p]) return fail(m, PLSPM_E_ARG, "plspm_fimix_device: an initial segment is not below its problem's K");
    const FimixTables tab = fimix_tables(m);
    const FimixPlan pl = fimix_plan(tab.shape, kmax);
    if (!pl.fits)
        return fail(m, PLSPM_E_LIMIT, "plspm_fimix_device: one problem's state (" + std::to_string(pl.lds_bytes) + " bytes: " + std::to_string(kmax) + " segments' moments of " +
                                          std::to_string(m->L) + " latent variables, parameters, one regression slot) exceeds 160 KiB of LDS");
    HIPCHK(m, hipSetDevice(m->device));
    m->fimix_nprob = 0;
    const int stride = pl.width + 2;
    if ((rc = ensure(m, m->fimix_rows, (size_t)nprob * stride * sizeof(double)))) return rc;
    if ((rc = ensure(m, m->fimix_status, (size_t)nprob * sizeof(int)))) return rc;
    if ((rc = ensure(m, m->fimix_iters, (size_t)nprob * sizeof(int)))) return rc;
    if ((rc = ensure(m, m->fimix_desc, tab.ints.size() * sizeof(int)))) return rc;
    if ((rc = ensure(m, m->fimix_k, (size_t)nprob * sizeof(int)))) return rc;
    if ((rc = plspm_detail_h2d(m, m->fimix_desc.p, tab.ints.data(), tab.ints.size() * sizeof(int)))) return rc;
    if ((rc = plspm_detail_h2d(m, m->fimix_k.p, k_of, (size_t)nprob * sizeof(int)))) return rc;
    if (init) {
        if ((rc = ensure(m, m->fimix_init, (size_t)nprob * N))) return rc;
        if ((rc = plspm_detail_h2d(m, m->fimix_init.p, init, (size_t)nprob * N))) return rc;
    }
    const FimixDesc d = fimix_desc(tab, (const int*)m->fimix_desc.p);
    if ((rc = allow_lds(m, (const void*)fimix_em_kernel, (size_t)pl.lds_bytes))) return rc;
    {
        ProfScope ps(m, PLSPM_K_SOLVER);
        hipLaunchKernelGGL(fimix_em_kernel, dim3((unsigned)nprob), dim3((unsigned)pl.threads), (size_t)pl.lds_bytes, m->stream, d, (const double*)m->scores.p, (long)N, (const int*)m->fimix_k.p, (int)kmax,
                           init ? (const unsigned char*)m->fimix_init.p : (const unsigned char*)nullptr, seed, start_offset, (int)max_iter, tol, pl.nslots, (double*)m->fimix_rows.p,
                           (int*)m->fimix_status.p, (int*)m->fimix_iters.p);
    }
    HIPCHK(m, hipGetLastError());
    m->fimix_nprob = nprob; m->fimix_kmax = kmax;
    m->fimix_k_of.assign(k_of, k_of + nprob);
    hand_out(m->fimix_rows, m->fimix_status, m->fimix_iters, d_out, d_status, d_iters);
    return 0;
}

int plspm_fimix_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status, int32_t* iters) {
    if (!m || first < 0 || count < 1) return fail(m, PLSPM_E_ARG, "plspm_fimix_fetch: bad arguments");
    int rc;
    if ((rc = fimix_state(m, "plspm_fimix_fetch"))) return rc;
    if (first + count > m->fimix_nprob) return fail(m, PLSPM_E_ARG, "plspm_fimix_fetch: range exceeds the last call's problems");
    HIPCHK(m, hipSetDevice(m->device));
    const int stride = plspm_fimix_width(m, m->fimix_kmax) + 2;
    return plspm_detail_fetch_records(m, (const double*)m->fimix_rows.p + first * stride, count, stride, out, status, iters);
}

int plspm_fimix_posteriors(plspm_model_t* m, int64_t problem, double* out) {
    if (!m || !out || problem < 0) return fail(m, PLSPM_E_ARG, "plspm_fimix_posteriors: bad arguments");
    int rc;
    if ((rc = fimix_state(m, "plspm_fimix_posteriors"))) return rc;
    if (problem >= m->fimix_nprob) return fail(m, PLSPM_E_ARG, "plspm_fimix_posteriors: not a problem of the last call");
    if (!m->scores_valid || !m->scores.p) return fail(m, PLSPM_E_STATE, "plspm_fimix_posteriors: the handle holds no scores");
    HIPCHK(m, hipSetDevice(m->device));
    const FimixTables tab = fimix_tables(m);
    const FimixDesc d = fimix_desc(tab, (const int*)m->fimix_desc.p);
    const int K = m->fimix_k_of[(size_t)problem], kmax = m->fimix_kmax, stride = fimix_record_width(kmax, d.n_dir, d.n_endo) + 2;
    const long N = (long)m->N;
    if ((rc = ensure(m, m->fimix_post, (size_t)N * K * sizeof(double)))) return rc;
    const size_t lds = ((size_t)fimix_param_doubles(d.L, d.n_dir, d.n_endo, 0) + (size_t)FIMIX_POST_NT * K) * sizeof(double);
    if ((rc = allow_lds(m, (const void*)fimix_posterior_kernel, lds))) return rc;
    {
        ProfScope ps(m, PLSPM_K_SCORES);
        hipLaunchKernelGGL(fimix_posterior_kernel, dim3((unsigned)((N + FIMIX_POST_NT - 1) / FIMIX_POST_NT)), dim3(FIMIX_POST_NT), lds, m->stream, d, (const double*)m->scores.p, N, K, kmax,
                           (const double*)m->fimix_rows.p + problem * stride, (double*)m->fimix_post.p);
    }
    HIPCHK(m, hipGetLastError());
    HIPCHK(m, hipMemcpyAsync(out, m->fimix_post.p, (size_t)N * K * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return 0;
}

}  // namespace extern "C"
