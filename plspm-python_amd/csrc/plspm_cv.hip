// plspm_cv.hip -- host side, part 6: repeated k-fold cross-validation for out-of-sample prediction (PLSpredict).  The training set of fold f of
// repetition r is problem r k + f of the bootstrap's int8 route: a 0/1 count row (kernels_cv.h) through the same Gram (run_gram_i8) and batch
// solver, as the two-group tests do it (plspm_permute.hip) -- the moments of a count row that is 1 on the training rows ARE the training moments,
// treatment and the `scaled` scalar included.  Behind the solver: the training moments of every problem in fp64 (full sample minus fold), the affine
// map x_hat = C [1; x_raw] of every problem's fit, and the errors of that map on the rows the problem did not see.
#include "host_internal.h"

#include "philox.h"
#include "wave_ops.h"
#include "kernels_cv.h"

int launch_cv_counts(plspm_model* m, const CvSpec& cs, int64_t nb, int64_t prob0, int MT, int KB, void* cd) {
    hipLaunchKernelGGL(cv_counts_kernel, count_rows_grid(nb, KB), dim3(COUNT_NT), 0, m->stream, (int)m->N, KB, MT, cs.k, prob0, (int)nb, cs.d_fold, (uint4*)cd);
    HIPCHK(m, hipGetLastError());
    return 0;
}

// the target indicators: the device columns of every LV that has a predecessor, ascending
static std::vector<int> cv_targets(const plspm_model* m) {
    std::vector<int> cols;
    for (int l = 0; l < m->L; ++l)
        if (m->pred_off[l + 1] > m->pred_off[l])
            for (int p = m->boff[l]; p < m->boff[l + 1]; ++p) cols.push_back(p);
    return cols;
}

// the last plspm_cv_device call's folds, moments and records are still on the handle, and they are (reps, k)'s
static int cv_state(plspm_model* m, int64_t reps, int32_t k, const char* who) {
    if (!m->cv_reps || !m->rows_B || !m->rows.p) return fail(m, PLSPM_E_STATE, std::string(who) + ": no cross-validation on this handle (a later call replaced it)");
    if (m->cv_reps != reps || m->cv_k != k || m->rows_B != reps * k) return fail(m, PLSPM_E_ARG, std::string(who) + ": reps / k are not the last plspm_cv_device call's");
    return 0;
}

extern "C" {

int plspm_cv_folds(uint64_t seed, int64_t rep, int64_t N, int32_t k, uint8_t* fold) {
    if (!fold || k < 2 || k > 256 || N < k || N > 0x7fffffffLL || rep < 0) return PLSPM_E_ARG;
    std::vector<std::pair<uint32_t, uint32_t>> key = row_keys(cv_quad, seed, rep, N);
    std::sort(key.begin(), key.end());
    for (int64_t j = 0; j < N; ++j) fold[key[(size_t)j].second] = (uint8_t)((j * k) / N);
    return 0;
}

int plspm_cv_targets(plspm_model_t* m, int32_t* cols) {
    if (!m) return 0;
    const std::vector<int> t = cv_targets(m);
    if (cols) std::copy(t.begin(), t.end(), cols);
    return (int)t.size();
}

int plspm_cv_device(plspm_model_t* m, int64_t reps, int32_t k, uint64_t seed, int64_t rep_offset, const uint8_t* fold, void** d_out, void** d_status, void** d_iters) {
    if (!m || reps < 1 || k < 2 || k > 256 || reps * k > ((int64_t)1 << 29) || rep_offset < 0 || rep_offset > ((int64_t)1 << 61))
        return fail(m, PLSPM_E_ARG, "plspm_cv_device: bad arguments (1 <= reps, 2 <= k <= 256, reps * k <= 2^29, rep_offset >= 0)");
    int rc;
    if ((rc = counts_call_scope(m, "plspm_cv_device"))) return rc;
    const int64_t N = m->N;
    if (!fold && (N < k || N - (N + k - 1) / k < 4)) return fail(m, PLSPM_E_ARG, "plspm_cv_device: every training set needs at least four rows (and every fold one)");
    if (fold) {
        // explicit fold ids (tests): every id below k, every fold non-empty, every training set of four rows at least
        std::vector<int64_t> size((size_t)k);
        for (int64_t r = 0; r < reps; ++r) {
            std::fill(size.begin(), size.end(), 0);
            for (int64_t i = 0; i < N; ++i) {
                const uint8_t f = fold[r * N + i];
                if (f >= k) return fail(m, PLSPM_E_ARG, "plspm_cv_device: a fold id is not below k");
                ++size[f];
            }
            for (int f = 0; f < k; ++f) {
                if (!size[(size_t)f]) return fail(m, PLSPM_E_ARG, "plspm_cv_device: a fold is empty");
                if (N - size[(size_t)f] < 4) return fail(m, PLSPM_E_ARG, "plspm_cv_device: every training set needs at least four rows");
            }
        }
    }
    if ((rc = counts_route_scope(m, "plspm_cv_device"))) return rc;
    void_records(m, REC_CV);
    const int C1 = m->P + 1;
    const long MS = (long)C1 * (C1 + 1) / 2;
    if ((rc = ensure(m, m->cv_fold, (size_t)reps * N))) return rc;
    if ((rc = ensure(m, m->cv_idx, (size_t)reps * N * sizeof(int)))) return rc;
    if ((rc = ensure(m, m->cv_off, (size_t)reps * (k + 1) * sizeof(int)))) return rc;
    if ((rc = ensure(m, m->cv_mom, (size_t)reps * k * MS * sizeof(double)))) return rc;
    uint8_t* d_fold = (uint8_t*)m->cv_fold.p;
    if (fold) {
        if ((rc = plspm_detail_h2d(m, d_fold, fold, (size_t)reps * N))) return rc;
    } else {
        if ((rc = ensure(m, m->cv_thr, (size_t)reps * (k - 1) * sizeof(uint2)))) return rc;
        // the keys in LDS after the first radix pass while they fit 48 KB; beyond that every pass draws them again
        const bool cache = N <= RANK_CACHE_ROWS;
        const size_t lds = cache ? (size_t)N * sizeof(unsigned) : 0;
        if ((rc = allow_lds(m, (const void*)cv_threshold_kernel, lds))) return rc;
        ProfScope ps(m, PLSPM_K_RESAMPLE);
        hipLaunchKernelGGL(cv_threshold_kernel, dim3((unsigned)reps, (unsigned)(k - 1)), dim3(RANK_NT), lds, m->stream, (int)N, k, seed, rep_offset, cache ? 1 : 0, (uint2*)m->cv_thr.p);
        hipLaunchKernelGGL(cv_assign_kernel, dim3((unsigned)reps, (unsigned)((N + 4 * CV_NT - 1) / (4 * CV_NT))), dim3(CV_NT), 0, m->stream, (int)N, k, seed, rep_offset,
                           (const uint2*)m->cv_thr.p, d_fold);
    }
    {
        ProfScope ps(m, PLSPM_K_RESAMPLE);
        hipLaunchKernelGGL(cv_order_kernel, dim3((unsigned)reps, (unsigned)k), dim3(RANK_NT), 0, m->stream, (int)N, k, (const uint8_t*)d_fold, (int*)m->cv_idx.p, (int*)m->cv_off.p);
    }
    HIPCHK(m, hipGetLastError());
    const CvSpec spec{reps, k, d_fold};
    BatchCall call;
    call.kind = BatchCall::CROSS_VALIDATION; call.cv = &spec; call.B = reps * k;       // problem r k + f = the rows of repetition rep_offset + r outside fold f
    if ((rc = plspm_detail_bootstrap(m, call))) return rc;
    {
        ProfScope ps(m, PLSPM_K_REDUCE);
        hipLaunchKernelGGL(cv_fold_moments_kernel, dim3((unsigned)(reps * k)), dim3(CV_NT), 0, m->stream, (const double*)m->d_Xa, m->PA, C1, (int)N, k, (const int*)m->cv_idx.p,
                           (const int*)m->cv_off.p, (double*)m->cv_mom.p, MS);
        hipLaunchKernelGGL(cv_train_moments_kernel, dim3((unsigned)reps), dim3(CV_NT), 0, m->stream, k, (double*)m->cv_mom.p, MS);
    }
    HIPCHK(m, hipGetLastError());
    m->cv_reps = reps; m->cv_k = k;
    hand_out(m->rows, m->status, m->iters, d_out, d_status, d_iters);
    return 0;
}

int plspm_cv_fold_ids(plspm_model_t* m, int64_t reps, int32_t k, uint8_t* fold, int32_t* order, int32_t* offsets) {
    if (!m) return PLSPM_E_ARG;
    int rc;
    if ((rc = cv_state(m, reps, k, "plspm_cv_fold_ids"))) return rc;
    HIPCHK(m, hipSetDevice(m->device));
    if (fold) HIPCHK(m, hipMemcpyAsync(fold, m->cv_fold.p, (size_t)reps * m->N, hipMemcpyDeviceToHost, m->stream));
    if (order) HIPCHK(m, hipMemcpyAsync(order, m->cv_idx.p, (size_t)reps * m->N * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    if (offsets) HIPCHK(m, hipMemcpyAsync(offsets, m->cv_off.p, (size_t)reps * (k + 1) * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return 0;
}

int plspm_cv_moments(plspm_model_t* m, int64_t reps, int32_t k, double* n_train, double* mean, double* cross) {
    if (!m) return PLSPM_E_ARG;
    int rc;
    if ((rc = cv_state(m, reps, k, "plspm_cv_moments"))) return rc;
    HIPCHK(m, hipSetDevice(m->device));
    const int P = m->P, C1 = P + 1;
    const long MS = (long)C1 * (C1 + 1) / 2, PS = (long)P * (P + 1) / 2;
    std::vector<double> shift((size_t)P);
    HIPCHK(m, hipMemcpyAsync(shift.data(), m->d_shift, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    // a slab of problems at a time (at most ~64 MB on the host)
    const int64_t nprob = reps * k, slab = std::max<int64_t>(1, std::min<int64_t>(nprob, (int64_t)((size_t)(64 << 20) / ((size_t)MS * sizeof(double)))));
    std::vector<double> h((size_t)slab * MS);
    for (int64_t q0 = 0; q0 < nprob; q0 += slab) {
        const int64_t nq = std::min(slab, nprob - q0);
        HIPCHK(m, hipMemcpyAsync(h.data(), (const double*)m->cv_mom.p + q0 * MS, (size_t)nq * MS * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(m, hipStreamSynchronize(m->stream));
        for (int64_t q = 0; q < nq; ++q) {
            const double* M = h.data() + q * MS;
            const double n = M[cv_tri(C1, P, P)], inv_n = 1.0 / n;
            if (n_train) n_train[q0 + q] = n;
            if (mean) for (int p = 0; p < P; ++p) mean[(q0 + q) * P + p] = M[cv_tri(C1, p, P)] * inv_n + shift[(size_t)p];
            if (cross) {
                double* out = cross + (q0 + q) * PS;
                for (int p = 0; p < P; ++p)
                    for (int pp = p; pp < P; ++pp) out[cv_tri(P, p, pp)] = M[cv_tri(C1, p, pp)] - (M[cv_tri(C1, p, P)] * M[cv_tri(C1, pp, P)]) * inv_n;
            }
        }
    }
    return 0;
}

int plspm_cv_predict(plspm_model_t* m, int64_t reps, int32_t k, int32_t technique, const double* coef, double* sse, double* sae, double* sst, int64_t* rows, double* pred_sum,
                     int32_t* pred_cnt) {
    if (!m || technique < 0 || technique > 1 || !sse || !sae || !sst || !rows || (pred_sum == nullptr) != (pred_cnt == nullptr))
        return fail(m, PLSPM_E_ARG, "plspm_cv_predict: bad arguments (technique 0 / 1; sse, sae, sst, rows required; pred_sum and pred_cnt together)");
    int rc;
    if ((rc = counts_call_scope(m, "plspm_cv_predict"))) return rc;
    if ((rc = cv_state(m, reps, k, "plspm_cv_predict"))) return rc;
    const std::vector<int> tcol = cv_targets(m);
    const int P = m->P, L = m->L, T = (int)tcol.size(), C1 = P + 1, N = (int)m->N;
    if (!T) return fail(m, PLSPM_E_ARG, "plspm_cv_predict: the model has no endogenous latent variable");
    HIPCHK(m, hipSetDevice(m->device));
    const int64_t nprob = reps * k;
    const long MS = (long)C1 * (C1 + 1) / 2;
    // row groups per workgroup: the most whose tile fits the LDS beside the matrix, with a thread per (row group, four targets)
    int nrg = 0;
    for (int cand : {16, 8, 4})
        if ((CV_NT / cand) * 4 >= T && cv_apply_lds(P, T, cand) <= kMaxLds) { nrg = cand; break; }
    if (!nrg) return fail(m, PLSPM_E_LIMIT, "plspm_cv_predict: the coefficient matrix of " + std::to_string(T) + " targets x " + std::to_string(C1) + " columns does not fit (at most 256 targets; 160 KiB of LDS)");
    // small tables: [edge_eff n_edges | tcol T]
    const int n_edges = (int)m->pred_idx.size();
    std::vector<int> tab((size_t)n_edges + T);
    for (int j = 0; j < L; ++j)
        for (int e = m->pred_off[j]; e < m->pred_off[j + 1]; ++e) {
            int found = -1;
            for (int x = 0; x < m->n_eff; ++x) if (m->eff_from[x] == m->pred_idx[e] && m->eff_to[x] == j) found = x;
            if (found < 0) return fail(m, PLSPM_E_STATE, "plspm_cv_predict: a path of the model has no effect pair");
            tab[(size_t)e] = found;
        }
    std::copy(tcol.begin(), tcol.end(), tab.begin() + n_edges);
    if ((rc = ensure(m, m->cv_tab, tab.size() * sizeof(int)))) return rc;
    if ((rc = plspm_detail_h2d(m, m->cv_tab.p, tab.data(), tab.size() * sizeof(int)))) return rc;
    const int* d_edge_eff = (const int*)m->cv_tab.p;
    const int* d_tcol = d_edge_eff + n_edges;
    const size_t coef_bytes = (size_t)nprob * T * C1 * sizeof(double);
    if ((rc = ensure(m, m->cv_coef, coef_bytes))) return rc;
    // [sse | sae | sst] nprob x T doubles, rows nprob
    const size_t io_doubles = (size_t)3 * nprob * T;
    if ((rc = ensure(m, m->cv_io, io_doubles * sizeof(double) + (size_t)nprob * sizeof(long long)))) return rc;
    double* d_sse = (double*)m->cv_io.p;
    double* d_sae = d_sse + (size_t)nprob * T;
    double* d_sst = d_sae + (size_t)nprob * T;
    long long* d_rows = (long long*)(d_sst + (size_t)nprob * T);
    double* d_psum = nullptr;
    int* d_pcnt = nullptr;
    if (pred_sum) {
        const size_t bytes = (size_t)N * T * sizeof(double) + (size_t)N * sizeof(int);
        if ((rc = ensure(m, m->cv_pred, bytes))) return rc;
        d_psum = (double*)m->cv_pred.p;
        d_pcnt = (int*)(d_psum + (size_t)N * T);
        HIPCHK(m, hipMemsetAsync(m->cv_pred.p, 0, bytes, m->stream));
    }
    if (coef) {
        if ((rc = plspm_detail_h2d(m, m->cv_coef.p, coef, coef_bytes))) return rc;
    } else {
        CvModel md{P, L, T, m->n_eff, m->scaled, technique, m->d_lvof, m->d_boff, m->d_pred_off, m->d_pred_idx, d_edge_eff, d_tcol, m->d_shift};
        const size_t lds = ((size_t)3 * P + L + (size_t)L * L) * sizeof(double);
        if ((rc = allow_lds(m, (const void*)cv_compose_kernel, lds))) return rc;
        ProfScope ps(m, PLSPM_K_REDUCE);
        hipLaunchKernelGGL(cv_compose_kernel, dim3((unsigned)nprob), dim3(64), lds, m->stream, md, (const double*)m->rows.p, plspm_row_stride(m), (const int*)m->status.p,
                           (const double*)m->cv_mom.p, MS, (double*)m->cv_coef.p);
    }
    {
        const size_t lds = cv_apply_lds(P, T, nrg);
        if ((rc = allow_lds(m, (const void*)cv_apply_kernel, lds))) return rc;
        ProfScope ps(m, PLSPM_K_REDUCE);
        hipLaunchKernelGGL(cv_apply_kernel, dim3((unsigned)nprob), dim3(CV_NT), lds, m->stream, (const double*)m->d_Xa, m->PA, P, T, N, k, nrg, (const int*)m->cv_idx.p,
                           (const int*)m->cv_off.p, d_tcol, (const double*)m->d_shift, (const double*)m->cv_coef.p, (const double*)m->cv_mom.p, MS, d_sse, d_sae, d_sst, d_rows, d_psum, d_pcnt);
    }
    HIPCHK(m, hipGetLastError());
    const size_t nt = (size_t)nprob * T;
    HIPCHK(m, hipMemcpyAsync(sse, d_sse, nt * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipMemcpyAsync(sae, d_sae, nt * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipMemcpyAsync(sst, d_sst, nt * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    static_assert(sizeof(long long) == sizeof(int64_t), "rows are copied as they are");
    HIPCHK(m, hipMemcpyAsync(rows, d_rows, (size_t)nprob * sizeof(int64_t), hipMemcpyDeviceToHost, m->stream));
    if (pred_sum) {
        HIPCHK(m, hipMemcpyAsync(pred_sum, d_psum, (size_t)N * T * sizeof(double), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(m, hipMemcpyAsync(pred_cnt, d_pcnt, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    }
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return 0;
}

}  // extern "C"
