// plspm_fit.hip -- host side, part 2: the fp64 MFMA Gram launches, the metric solvers, the single fit (plspm_fit, phase by phase as fit_route.h plans it) and the
// operator seam (plspm_op_*).  Kernels: kernels_gram.h, kernels_solver.h, kernels_scores.h.  (The non-metric iteration: plspm_nonmetric.hip.)
#include "host_internal.h"
#include <hip/hip_ext.h>

#include "wave_ops.h"
#include "device_exec.h"
#include "kernels_gram.h"
#include "kernels_solver.h"
#include "kernels_scores.h"

// ------------------------------------------------------------------------------------------------ launch helpers
template <bool DENSE>
static int launch_gram(plspm_model* m, long nproblems, int nchunks, const int2* ent, const int* nent, long ent_stride, double* out) {
    const dim3 grid(nchunks, (unsigned)nproblems);
    const long N = m->N;
    hipStream_t s = m->stream;
#define ROWS(TT)                                                                                                         \
    {                                                                                                                    \
        const size_t lds = std::max<size_t>(2 * (size_t)TileIdx<TT>::NTILE * 256 * sizeof(double), (size_t)m->tune.gram_lds_kb * 1024); \
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)gram_rows_kernel<TT, DENSE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL((gram_rows_kernel<TT, DENSE>), grid, dim3(256), lds, s, m->d_Xa, N, ent, nent, ent_stride, out); \
    }
#define WIDE(TT, NWV, NWP)                                                                                                     \
    hipLaunchKernelGGL((gram_wide_kernel<TT, NWV, NWP, DENSE>), dim3(nchunks, (unsigned)nproblems, NWV / NWP), dim3(NWP * 64), 0, s, m->d_Xa, N, ent, \
                       nent, ent_stride, out);
    switch (m->T) {
        case 2: ROWS(2) break;
        case 4: ROWS(4) break;
        case 5: WIDE(5, 4, 4) break;
        case 6: WIDE(6, 4, 4) break;
        case 7: WIDE(7, 4, 4) break;
        case 9: WIDE(9, 4, 4) break;
        case 11: WIDE(11, 4, 4) break;
        case 13: {
            // (configs[4]: the dense walk on a ring of row buffers -- kernels_gram.h gram_walk_dense_ring; option wide_ring 0: the two-stage ping-pong)
            const int ring = !DENSE ? 0 : m->tune.wide_ring == 4 ? 4 : m->tune.wide_ring >= 5 ? 6 : 0;
            const auto k = ring == 4 ? gram_wide_kernel<13, 4, 4, DENSE, DENSE ? 4 : 0> : ring == 6 ? gram_wide_kernel<13, 4, 4, DENSE, DENSE ? 6 : 0> : gram_wide_kernel<13, 4, 4, DENSE>;
            hipLaunchKernelGGL(k, dim3(nchunks, (unsigned)nproblems, 1), dim3(256), 0, s, m->d_Xa, N, ent, nent, ent_stride, out);
        } break;
        case 15: WIDE(15, 4, 4) break;
        case 8: WIDE(8, 4, 4) break;
        case 10: WIDE(10, 4, 4) break;
        case 12: WIDE(12, 4, 4) break;
        case 14: {
            const int sel = m->tune.wide_nw;        // measured on 1M x 200: NW=4 0.99 ms, 8: 1.12 ms, 16 (two workgroups per walk): 1.37 ms
            if (sel == 4) WIDE(14, 4, 4) else if (sel == 16) WIDE(14, 16, 8) else WIDE(14, 8, 8)
        } break;
        case 16: WIDE(16, 16, 8) break;
        default: {
            if (m->T < 18 || (m->T & 1)) return fail(m, PLSPM_E_LIMIT, "unsupported tile count");
            const int TB = (m->T + 3) / 4, nsb = TB * (TB + 1) / 2;
            hipLaunchKernelGGL((gram_block_kernel<DENSE>), dim3(nchunks, (unsigned)nproblems, (nsb + 3) / 4), dim3(256), 0, s, m->d_Xa, N, m->T, ent, nent, ent_stride, out);
        } break;
    }
#undef ROWS
#undef WIDE
    HIPCHK(m, hipGetLastError());
    return 0;
}

// Missing-data models: collapse the aug Gram(s) at `Min` into mean-imputed P-column moments; returns the matrix the solver reads.
int run_impute(plspm_model* m, long nproblems, const double* Min, const double** Mp, long* mp_stride) {
    *Mp = Min; *mp_stride = packed_size(m->T);
    if (!m->n_ind) return 0;
    const long out_stride = packed_size(m->Ts);
    int rc = ensure(m, m->gram2, (size_t)nproblems * out_stride * sizeof(double));
    if (rc) return rc;
    ProfScope ps(m, PLSPM_K_REDUCE);
    hipLaunchKernelGGL(impute_kernel, dim3((unsigned)nproblems), dim3(256), (size_t)m->P * sizeof(double), m->stream, m->P, m->Pg, m->T, m->Ts, m->d_ind_of, Min,
                       packed_size(m->T), (double*)m->gram2.p, out_stride);
    *Mp = (const double*)m->gram2.p; *mp_stride = out_stride;
    return 0;
}

int launch_solver(plspm_model* m, long nproblems, const double* Mp, long mp_stride, const SolverOut& so, int threads) {
    const SolverLds pl = solver_lds(route_shape(m), nproblems);      // (solver_route.h: what of the workspace lives in LDS)
    int rc;
    if (!pl.s_in_lds && (rc = ensure(m, m->gS, (size_t)nproblems * pl.s_bytes))) return rc;
    if (!pl.small_in_lds && (rc = ensure(m, m->gsmall, (size_t)nproblems * pl.small_bytes))) return rc;
    const auto k = pl.s_in_lds ? solver_kernel<true, true> : pl.small_in_lds ? solver_kernel<false, true> : solver_kernel<false, false>;
    if ((rc = allow_lds(m, (const void*)k, pl.lds))) return rc;
    hipLaunchKernelGGL(k, dim3((unsigned)nproblems), dim3(threads), pl.lds, m->stream, make_desc(m), Mp, mp_stride, so, (double*)m->gS.p, (double*)m->gsmall.p);
    HIPCHK(m, hipGetLastError());
    return 0;
}

// The full sample's metric solve behind dense_moments(): the single fit's and solve_full_sample's.
static int solve_metric_moments(plspm_model* m, const SolverOut& so) {
    const double* Mp; long mp_stride;
    if (int rc = run_impute(m, 1, (const double*)m->gram.p, &Mp, &mp_stride)) return rc;
    ProfScope ps(m, PLSPM_K_SOLVER);
    return launch_solver(m, 1, Mp, mp_stride, so, 256);
}


// Moment matrix of ALL uploaded rows (single fit, operator seam): the dense MFMA Gram split over row chunks + the fixed-order
// reduce -> m->gram (tile-packed, of the shifted columns + ones).
int dense_moments(plspm_model* m) {
    const long psize = packed_size(m->T);
    const int nchunks = fit_gram_chunks(m->N, m->T, m->tune.fit_chunks);      // (fit_route.h: the row chunks, one workgroup each)
    int rc;
    if ((rc = ensure(m, m->gram_partial, (size_t)nchunks * psize * sizeof(double)))) return rc;
    if ((rc = ensure(m, m->gram, (size_t)psize * sizeof(double)))) return rc;
    {
        ProfScope ps(m, PLSPM_K_GRAM);
        if ((rc = launch_gram<true>(m, 1, nchunks, nullptr, nullptr, 0, (double*)m->gram_partial.p))) return rc;
    }
    {
        ProfScope ps(m, PLSPM_K_REDUCE);
        hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)((psize + 255) / 256)), dim3(256), 0, m->stream, (const double*)m->gram_partial.p, nchunks, psize,
                           (double*)m->gram.p);
    }
    HIPCHK(m, hipGetLastError());
    return 0;
}

int solve_full_sample(plspm_model* m, double* record, int* status_iters) {
    int rc;
    if ((rc = dense_moments(m))) return rc;
    SolverOut so{};
    so.row = record; so.row_stride = 0; so.status = status_iters; so.iters = status_iters + 1;
    return solve_metric_moments(m, so);
}

int launch_gram_lists(plspm_model* m, long nproblems, const int2* ent, const int* nent, long ent_stride, double* out) {
    return launch_gram<false>(m, nproblems, 1, ent, nent, ent_stride, out);
}

int run_hoc_moments(plspm_model* m, plspm_model* m2, long nb) {
    const long psize = packed_size(m->T), psize2 = packed_size(m2->Ts);
    int rc;
    if ((rc = ensure(m, m2->gram, (size_t)nb * psize2 * sizeof(double)))) return rc;
    const HocDesc hd = make_hoc_desc(m2);
    const size_t vlds = std::max<size_t>(1, (size_t)hd.nh * (hd.P1 + 1)) * sizeof(double);
    if ((rc = allow_lds(m, (const void*)hoc_moments_kernel, vlds))) return rc;
    ProfScope ps(m, PLSPM_K_REDUCE);
    hipLaunchKernelGGL(hoc_moments_kernel, dim3((unsigned)nb), dim3(256), vlds, m->stream, hd, (const double*)m->gram.p, psize, (const double*)m->nmstate.p,
                       (long)nm_state_doubles_of(m), (double*)m2->gram.p, psize2);
    HIPCHK(m, hipGetLastError());
    return 0;
}

template <int LMAX>
static int launch_nm_wave(plspm_model* m, long nb, const SolverOut& so, double* maps, long maps_stride, int* steps, const int* force, const int* live) {
    const size_t lds = (size_t)(wave16_ws_doubles<LMAX>(m->L, m->kmax, m->n_chol) + 64) * sizeof(double);
    auto k = (LMAX < 32 && m->n_chol > 0) ? solver_nmwave_kernel<LMAX, LMAX < 32> : solver_nmwave_kernel<LMAX, false>;      // (17 .. 32 LVs: all Mode A)
    if (int rc = allow_lds(m, (const void*)k, lds)) return rc;
    hipLaunchKernelGGL(k, dim3((unsigned)nb), dim3(64), lds, m->stream, make_desc(m), (const double*)m->gram.p, (long)cov_doubles(m->Pg), so, maps, maps_stride, steps, force, live, std::ldexp(1.0, m->tune.nm_bound_shift));
    return 0;
}

int launch_nm_wave_solver(plspm_model* m, long nb, const SolverOut& so, double* maps, long maps_stride, int* steps, const int* force, const int* live) {
    const SolverRoute route = nm_wave_route(route_shape(m));      // (callers asked the plan: nm_route.h num_one)
    ProfScope ps(m, PLSPM_K_SOLVER);
    const int rc = route == ROUTE_NM_WAVE_8 ? launch_nm_wave<8>(m, nb, so, maps, maps_stride, steps, force, live)
                 : route == ROUTE_NM_WAVE_16 ? launch_nm_wave<16>(m, nb, so, maps, maps_stride, steps, force, live)
                 : route == ROUTE_NM_WAVE_32 ? launch_nm_wave<32>(m, nb, so, maps, maps_stride, steps, force, live) : fail(m, PLSPM_E_STATE, "no wave solver covers this model");
    if (!rc) m->last_solver = route;
    return rc;
}

// A dense solver launch that signals the caller's event `stop` (may be null; plspm_group.cpp: the `computed` event its collective waits for, BatchCall's
// stop_event; a separate hipEventRecord is one more packet the queue drains the device for, ~5 us of every step) and says so in *taken.  The rows / LDS
// solvers leave the event to their caller.
template <class K>
static int launch_signalling(plspm_model* m, K kernel, long nb, int threads, size_t lds, const SolverOut& so, hipEvent_t stop, bool* taken) {
    if (int rc = allow_lds(m, (const void*)kernel, lds)) return rc;
    ProfScope ps(m, PLSPM_K_SOLVER);
    if (stop) *taken = true;
    hipExtLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(threads), lds, m->stream, nullptr, stop, 0, make_desc(m), (const double*)m->gram.p, (long)cov_doubles(m->Pg), so);
    return 0;
}

int launch_batch_solver(plspm_model* m, long nb, SolverRoute route, const SolverOut& so_in, hipEvent_t stop, bool* stop_taken) {
    SolverOut so = so_in;
    int rc = 0;
    const double* gram_buf = (const double*)m->gram.p;
    const bool modeb = m->n_chol > 0;
#ifdef PLSPM_DEBUG_MARKS      // phase clocks of one solver problem (make marks); never in the release library
    long long* d_marks = nullptr;
    HIPCHK(m, plspm_dmalloc((void**)&d_marks, 32 * sizeof(long long))); so.marks = d_marks;
#endif
    switch (route) {
        case ROUTE_WAVE16_8:      // (round 5: V in LDS, the product stream's second copy w V for the Q sums, a folded into E; Mode-B blocks: a second instantiation)
            rc = launch_signalling(m, modeb ? solver_wave16_kernel<8, true> : solver_wave16_kernel<8, false>, nb, 64, (size_t)wave16_ws_doubles<8>(m->L, m->kmax, m->n_chol) * sizeof(double), so, stop, stop_taken); break;
        case ROUTE_WAVE:          // (fixed lane roles, solver_wave.h; Mode-B blocks keep their inverses behind the workspace)
            rc = launch_signalling(m, modeb ? solver_wave_kernel<8, true> : solver_wave_kernel<8, false>, nb, 64, (size_t)wave_ws_doubles<8>(m->n_chol) * sizeof(double), so, stop, stop_taken); break;
        case ROUTE_WAVE16_16:     // (four matrix entries per pair lane)
            rc = launch_signalling(m, modeb ? solver_wave16_kernel<16, true> : solver_wave16_kernel<16, false>, nb, 64, (size_t)wave16_ws_doubles<16>(m->L, m->kmax, m->n_chol) * sizeof(double), so, stop, stop_taken); break;
        case ROUTE_WAVE16_32:     // (sixteen matrix entries per pair lane, three problems per CU)
            rc = launch_signalling(m, solver_wave16_kernel<32, false>, nb, 64, (size_t)wave16_ws_doubles<32>(m->L, m->kmax, 0) * sizeof(double), so, stop, stop_taken); break;
        case ROUTE_QUAD:
            rc = launch_signalling(m, solver_quad_kernel<16>, nb, 256, (size_t)quad_ws_doubles<16>(m->L, m->kmax) * sizeof(double), so, stop, stop_taken); break;
        case ROUTE_ROWS_SPLIT:    // (two threads per MV on either side of a block boundary, rows_split_block)
        case ROUTE_ROWS: {
            const bool split = route == ROUTE_ROWS_SPLIT;
            const size_t lds = desc_lds_bytes(m->P, m->L, m->n_eff, (int)m->pred_idx.size()) + (workspace_small_doubles(m->P, m->L, m->kmax, m->n_chol) + (split ? PLSPM_ROWS_SPLIT_STAGE_DOUBLES : 0)) * sizeof(double);
            auto k = split ? solver_rows_split_kernel : solver_rows_kernel;
            if ((rc = allow_lds(m, (const void*)k, lds))) return rc;
            ProfScope ps(m, PLSPM_K_SOLVER);
            hipLaunchKernelGGL(k, dim3((unsigned)nb), dim3(split ? 256 : 64), lds, m->stream, make_desc(m), gram_buf, (long)cov_doubles(m->Pg), so);
        } break;
        default: {                // ROUTE_LDS
            const double* Mp; long mp_stride;
            if ((rc = run_impute(m, nb, gram_buf, &Mp, &mp_stride))) return rc;
            ProfScope ps(m, PLSPM_K_SOLVER);
            rc = launch_solver(m, nb, Mp, mp_stride, so, m->tune.solver_threads);
        } break;
    }
    if (rc) return rc;
    m->last_solver = route;
    HIPCHK(m, hipGetLastError());
#ifdef PLSPM_DEBUG_MARKS
    {
        long long h[32];
        HIPCHK(m, hipStreamSynchronize(m->stream));
        HIPCHK(m, hipMemcpy(h, d_marks, sizeof(h), hipMemcpyDeviceToHost));
        if (route != ROUTE_LDS && route != ROUTE_ROWS && route != ROUTE_ROWS_SPLIT) {      // the wave / quad solvers' marks
            fprintf(stderr, "[plspm wave clocks] load %lld  treat %lld  init %lld  iterations %lld  finalize %lld  inner %lld  effects %lld  outputs %lld  total %lld\n",
                    h[1] - h[0], h[2] - h[1], h[3] - h[2], h[4] - h[3], h[5] - h[4], h[6] - h[5], h[7] - h[6], h[13] - h[7], h[13] - h[0]);
            fprintf(stderr, "[plspm wave last iterate] apply_cov %lld  a/G/E %lld  regress %lld  outer+conv %lld\n", h[9] - h[8], h[10] - h[9], h[11] - h[10], h[12] - h[11]);
            fprintf(stderr, "[plspm wave last apply_cov] seg_products+T %lld  sync %lld  Q %lld\n", h[17] - h[16], h[18] - h[17], h[19] - h[18]);
            if (m->n_chol > 0) fprintf(stderr, "[plspm wave Mode-B inverses] setup %lld  fill %lld  rows %lld  sweep %lld  store %lld  fallback test %lld  rest of init %lld\n", h[20] - h[2], h[21] - h[20], h[22] - h[21],
                                       h[23] - h[22], h[24] - h[23], h[25] - h[24], h[3] - h[25]);
        } else {
        fprintf(stderr, "[plspm solver clocks] cov %lld  chol+init %lld  iterate %lld  finalize %lld  inner %lld  effects %lld  outputs %lld  total %lld\n",
                h[1] - h[0], h[2] - h[1], h[3] - h[2], h[4] - h[3], h[5] - h[4], h[6] - h[5], h[7] - h[6], h[7] - h[0]);
        fprintf(stderr, "[plspm cov] sweep %lld  scale-factor %lld  centre+sd %lld\n", h[14] - h[0], h[15] - h[14], h[1] - h[15]);
        fprintf(stderr, "[plspm last iterate] apply_cov %lld  a+G %lld  inner_weights %lld  outer %lld  conv+copy %lld\n", h[9] - h[8], h[10] - h[9],
                h[11] - h[10], h[12] - h[11], h[13] - h[12]);
        fprintf(stderr, "[plspm last apply_cov] block products %lld  Q %lld\n", h[17] - h[16], h[18] - h[17]);
        }
        plspm_dfree(d_marks);
    }
#endif
    return 0;
}

// ------------------------------------------------------------------------------------------------ the single fit, phase by phase as fit_route.h plans it
// The device result block as the plan lays it out, and where the solver writes into it.
static int fit_reserve(plspm_model* m, const FitPlan& pl, SolverOut* so) {
    if (int rc = ensure(m, m->fitout, pl.fit_bytes)) return rc;
    double* d = (double*)m->fitout.p;
    int* d_int = (int*)(d + pl.o_end);
    *so = SolverOut{};
    so->row = d + pl.o_row; so->row_stride = 0; so->status = d_int + FIT_INT_STATUS; so->iters = d_int + FIT_INT_ITERS;
    so->fit.weights = d + pl.o_w; so->fit.loadings = d + pl.o_ld; so->fit.crossloadings = d + pl.o_cl; so->fit.path_coef = d + pl.o_pc; so->fit.r2 = d + pl.o_r2;
    so->fit.lv_cov = d + pl.o_lc; so->fit.indirect = d + pl.o_ind; so->fit.score_w = d + pl.o_sw; so->fit.score_c = d + pl.o_sc;
    so->fit.cov = pl.call.want_cov ? d + pl.o_cov : nullptr; so->fit.mean = d + pl.o_mean; so->fit.sign = (int8_t*)(d_int + FIT_INT_SIGN);
    return 0;
}

// The one problem on the moments at m->gram.
static int fit_solve(plspm_model* m, const SolverOut& so) {
    if (!m->nonmetric) return solve_metric_moments(m, so);
    return run_nonmetric(m, plan_nonmetric(m, NmCall{1, false, false, false, true}), NmInputs{(const double*)m->gram.p, packed_size(m->T), nullptr, nullptr, 0, nullptr, 0, 256}, so);
}

// (tile rows, chunk class) of the plan -> the instantiation
typedef void (*ScoresFn)(const double*, long, int, int, int, const int*, const double*, const double*, double*);
static ScoresFn scores_fn(int tile_rows, int cls) {
    static const ScoresFn table[2][5] = {{scores_kernel<16, 2>, scores_kernel<16, 4>, scores_kernel<16, 6>, scores_kernel<16, 8>, scores_kernel<16, 0>},
                                         {scores_kernel<32, 2>, scores_kernel<32, 4>, scores_kernel<32, 6>, scores_kernel<32, 8>, scores_kernel<32, 0>}};
    return table[tile_rows == 32][cls ? cls / 2 - 1 : 4];
}

// Scores of all rows -> m->scores, from the score map the solver left in the block.
static int fit_scores(plspm_model* m, const FitPlan& pl) {
    const ScoresLaunch& k = pl.scores;
    const double* d = (const double*)m->fitout.p;
    int rc;
    if ((rc = ensure(m, m->scores, pl.score_bytes))) return rc;
    const ScoresFn fn = scores_fn(k.tile_rows, k.cls);
    if ((rc = allow_lds(m, (const void*)fn, k.lds))) return rc;
    ProfScope ps(m, PLSPM_K_SCORES);
    hipLaunchKernelGGL(fn, dim3(k.grid), dim3(256), k.lds, m->stream, (const double*)m->d_Xa, (long)m->N, m->PA, m->P, m->L, (const int*)m->d_boff, d + pl.o_sw, d + pl.o_sc, (double*)m->scores.p);
    if (m->nmx_K) {                                     // the incomplete rows' scores are not affine in the columns: take them from the state
        const int P = m->P, L = m->L;
        const double* Yn = (const double*)m->nmstate.p + nm_state_doubles(P, L, m->n_chol) + m->nmx_K + 2L * P + (long)m->nmx_K * P + (long)m->nmx_K * L;
        hipLaunchKernelGGL(patch_scores_kernel, dim3((unsigned)m->nmx_K), dim3(64), 0, m->stream, (double*)m->scores.p, L, (const int*)m->d_rowid, Yn);
    }
    return 0;
}

// ONE device->host copy of the whole result block into the pinned staging block (15 separate small copies cost more than the four kernels of a 10k x 60 fit);
// small score matrices ride it too, large ones go to the caller's array.  Returns with the stream drained.
static int fit_download(plspm_model* m, const FitPlan& pl, double* scores_out) {
    HIPCHK(m, m->h_stage.reserve(pl.stage_need));
    char* hs = (char*)m->h_stage.p;
    const double* d = (const double*)m->fitout.p;
    HIPCHK(m, hipMemcpyAsync(hs, d, pl.block_bytes, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipMemcpyAsync(hs + (size_t)pl.o_end * sizeof(double), d + pl.o_end, pl.tail_bytes, hipMemcpyDeviceToHost, m->stream));
    if (pl.stage_scores) HIPCHK(m, hipMemcpyAsync(hs + pl.fit_bytes, m->scores.p, pl.score_bytes, hipMemcpyDeviceToHost, m->stream));
    else if (pl.call.want_scores) HIPCHK(m, hipMemcpyAsync(scores_out, m->scores.p, pl.score_bytes, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return 0;
}

// The pinned copy -> the caller's arrays (any may be null).
static void fit_scatter(const plspm_model* m, const FitPlan& pl, const plspm_fit_result_t* out) {
    const char* hs = (const char*)m->h_stage.p;
    if (pl.stage_scores) memcpy(out->scores, hs + pl.fit_bytes, pl.score_bytes);
    const double* h = (const double*)hs;
    const int* h_int = (const int*)(h + pl.o_end);
    auto put = [&](void* dst, const void* src, size_t bytes) { if (dst) memcpy(dst, src, bytes); };
    const int P = m->P, L = m->L, ne = m->n_eff, Po = pl.Po;
    put(out->weights, h + pl.o_w, sizeof(double) * Po);
    put(out->loadings, h + pl.o_ld, sizeof(double) * Po);
    put(out->crossloadings, h + pl.o_cl, sizeof(double) * Po * L);
    put(out->path_coef, h + pl.o_pc, sizeof(double) * L * L);
    put(out->r2, h + pl.o_r2, sizeof(double) * L);
    put(out->lv_cov, h + pl.o_lc, sizeof(double) * L * L);
    put(out->total, h + pl.h_total, sizeof(double) * ne);
    put(out->direct, h + pl.h_direct, sizeof(double) * ne);
    put(out->indirect, h + pl.o_ind, sizeof(double) * ne);
    put(out->cov, h + pl.o_cov, sizeof(double) * Po * Po);
    if (m->categorical) { if (out->mean) memset(out->mean, 0, sizeof(double) * Po); }
    else put(out->mean, h + pl.o_mean, sizeof(double) * P);
    put(out->sign, h_int + FIT_INT_SIGN, (size_t)L);
    put(out->iterations, h_int + FIT_INT_ITERS, sizeof(int));
    put(out->status, h_int + FIT_INT_STATUS, sizeof(int));
}

extern "C" {

int plspm_fit(plspm_model_t* m, const plspm_fit_result_t* out) {
    if (!m || !out) return PLSPM_E_ARG;
    if (!m->d_Xa || m->N < 2) return fail(m, PLSPM_E_STATE, "plspm_fit: no data uploaded");
    HIPCHK(m, hipSetDevice(m->device));
    const FitPlan pl = fit_plan(fit_shape(m), FitCall{out->scores != nullptr, out->cov != nullptr}, FitOptions{m->tune.fit_chunks, m->tune.scores_tile});
    SolverOut so;
    int rc;
    if ((rc = fit_reserve(m, pl, &so)) || (rc = dense_moments(m)) || (rc = fit_solve(m, so))) return rc;
    if (pl.call.want_scores && (rc = fit_scores(m, pl))) return rc;
    HIPCHK(m, hipGetLastError());
    if (pl.call.want_scores) m->scores_valid = true;      // (plspm_fimix_device reads them where they are)
    if ((rc = fit_download(m, pl, out->scores))) return rc;
    // plspm_bootstrap_prepare ran before this fit: its column statistics are on the host now, so the digit planes are cut (enqueue only)
    // while the caller unpacks the fit -- the first bootstrap call finds them ready.  (A failure here is reported by that call, which retries.)
    if (m->zs_stats_ready && !m->zs_valid) { const std::string keep = m->error; if (prepare_zs(m)) { (void)hipGetLastError(); m->error = keep; } }
    fit_scatter(m, pl, out);
    return 0;
}


// ---- operator seam (solver_ops.h): the reference's Scheme / Mode plug-ins, one call = upload + MFMA Gram + one small kernel ----
int plspm_op_inner_weights(int32_t device_id, int32_t scheme, int32_t L, const uint8_t* path, const double* y, int64_t N, double* E) {
    g_create_error.clear();
    if (!path || !y || !E || L < 1 || L > 64 || N < 2) return fail(nullptr, PLSPM_E_ARG, "plspm_op_inner_weights: bad arguments (1 <= L <= 64, N >= 2)");
    std::vector<int32_t> boff(L + 1), mode(L, PLSPM_MODE_A);
    for (int l = 0; l <= L; ++l) boff[l] = l;                       // every LV's "block" is its own score column
    plspm_model* m = plspm_model_create(L, L, boff.data(), path, mode.data(), scheme, 0, 1, 1.0, device_id);
    if (!m) return PLSPM_E_ARG;                                     // text in plspm_last_error(NULL)
    auto done = [&](int rc) { if (rc) g_create_error = m->error; plspm_model_destroy(m); return rc; };
    int rc;
    if ((rc = plspm_upload(m, y, N, L, 0, nullptr)) || (rc = dense_moments(m))) return done(rc);
    if ((rc = ensure(m, m->fitout, sizeof(double) * (size_t)L * L))) return done(rc);
    const size_t lds = (size_t)workspace_small_doubles(L, L, m->kmax, m->n_chol) * sizeof(double) + desc_lds_bytes(L, L, m->n_eff, (int)m->pred_idx.size());
    if ((rc = allow_lds(m, (const void*)op_inner_kernel, lds))) return done(rc);
    hipLaunchKernelGGL(op_inner_kernel, dim3(1), dim3(256), lds, m->stream, make_desc(m), (const double*)m->gram.p, (double*)m->fitout.p);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(E, m->fitout.p, sizeof(double) * (size_t)L * L, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipStreamSynchronize(m->stream) != hipSuccess)
        return done(fail(m, PLSPM_E_STATE, "plspm_op_inner_weights: launch / copy failed"));
    return done(0);
}

int plspm_op_outer_weights(int32_t device_id, int32_t mode, const double* Xk, const double* z, int64_t N, int32_t k, double* w) {
    g_create_error.clear();
    if (!Xk || !z || !w || k < 1 || k > 1020 || N < 2 || (mode != PLSPM_MODE_A && mode != PLSPM_MODE_B))
        return fail(nullptr, PLSPM_E_ARG, "plspm_op_outer_weights: bad arguments (1 <= k <= 1020, N >= 2)");
    const int P = k + 1;                                            // [X_k | z]
    const int32_t boff[2] = {0, P}, modes[1] = {PLSPM_MODE_A};
    const uint8_t path[1] = {0};
    plspm_model* m = plspm_model_create(P, 1, boff, path, modes, PLSPM_SCHEME_CENTROID, 0, 1, 1.0, device_id);
    if (!m) return PLSPM_E_ARG;
    auto done = [&](int rc) { if (rc) g_create_error = m->error; plspm_model_destroy(m); return rc; };
    std::vector<double> both;                                       // the two host arrays side by side (one upload, one Gram)
    try { both.resize((size_t)N * P); } catch (...) { return done(fail(m, PLSPM_E_STATE, "out of host memory")); }
    for (int64_t i = 0; i < N; ++i) { memcpy(&both[(size_t)i * P], Xk + (size_t)i * k, sizeof(double) * k); both[(size_t)i * P + k] = z[i]; }
    int rc;
    if ((rc = plspm_upload(m, both.data(), N, P, 0, nullptr)) || (rc = dense_moments(m))) return done(rc);
    const size_t kk = (size_t)k * k;
    if ((rc = ensure(m, m->fitout, sizeof(double) * (3 * kk + 1 + k)))) return done(rc);
    double* scratch = (double*)m->fitout.p;
    double* d_w = scratch + 3 * kk + 1;
    hipLaunchKernelGGL(op_outer_kernel, dim3(1), dim3(256), 0, m->stream, (int)mode, (int)k, m->T, (const double*)m->gram.p, (const double*)m->d_shift, scratch, d_w);
    double flag = 0.0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(w, d_w, sizeof(double) * k, hipMemcpyDeviceToHost, m->stream) != hipSuccess ||
        hipMemcpyAsync(&flag, scratch + 3 * kk, sizeof(double), hipMemcpyDeviceToHost, m->stream) != hipSuccess || hipStreamSynchronize(m->stream) != hipSuccess)
        return done(fail(m, PLSPM_E_STATE, "plspm_op_outer_weights: launch / copy failed"));
    if (flag == 0.0) return done(fail(m, PLSPM_SINGULAR, "plspm_op_outer_weights: the Mode-B least squares did not converge"));
    return done(0);
}

int plspm_op_outer_weights_nonmetric(int32_t device_id, int32_t mode, const double* Xk, const uint8_t* present, const double* z, int64_t N, int32_t k,
                                     double correction, double* w, double* Y) {
    g_create_error.clear();
    if (!Xk || !z || !w || !Y || k < 1 || k > 1020 || N < 2 || (mode != PLSPM_MODE_A && mode != PLSPM_MODE_B))
        return fail(nullptr, PLSPM_E_ARG, "plspm_op_outer_weights_nonmetric: bad arguments (1 <= k <= 1020, N >= 2)");
    if (mode == PLSPM_MODE_B && present) return fail(nullptr, PLSPM_E_ARG, "plspm_op_outer_weights_nonmetric: Mode B takes no missing values (mode.py:55-56)");
    int rc;
    // Mode B: the least-squares weights of z on the block (minimum norm when rank deficient), as the metric operator computes them
    if (mode == PLSPM_MODE_B && (rc = plspm_op_outer_weights(device_id, PLSPM_MODE_B, Xk, z, N, k, w))) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev) return fail(nullptr, PLSPM_E_STATE, "plspm_op_outer_weights_nonmetric: no such HIP device");
    if (hipSetDevice(device_id) != hipSuccess) return fail(nullptr, PLSPM_E_STATE, "hipSetDevice failed");
    const size_t nx = (size_t)N * k;
    const size_t bytes = sizeof(double) * (nx + 2 * (size_t)N + k) + (present ? nx : 0);
    void* base = nullptr;
    hipStream_t st = nullptr;
    if (plspm_dmalloc(&base, bytes) != hipSuccess) return fail(nullptr, PLSPM_E_STATE, "plspm_op_outer_weights_nonmetric: out of device memory");
    auto done = [&](int code, const char* why) { if (st) { hipStreamSynchronize(st); plspm_stream_release(st); } plspm_dfree(base); return code ? fail(nullptr, code, why) : 0; };
    if (plspm_stream_acquire(&st) != hipSuccess) return done(PLSPM_E_STATE, "plspm_op_outer_weights_nonmetric: no stream");
    double* d_X = (double*)base; double* d_z = d_X + nx; double* d_Y = d_z + N; double* d_w = d_Y + N;
    unsigned char* d_m = present ? (unsigned char*)(d_w + k) : nullptr;
    bool ok = hipMemcpyAsync(d_X, Xk, sizeof(double) * nx, hipMemcpyHostToDevice, st) == hipSuccess &&
              hipMemcpyAsync(d_z, z, sizeof(double) * N, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok && present) ok = hipMemcpyAsync(d_m, present, nx, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok && mode == PLSPM_MODE_B) ok = hipMemcpyAsync(d_w, w, sizeof(double) * k, hipMemcpyHostToDevice, st) == hipSuccess;
    if (!ok) return done(PLSPM_E_STATE, "plspm_op_outer_weights_nonmetric: upload failed");
    hipLaunchKernelGGL(op_nm_outer_kernel, dim3(1), dim3(1024), 0, st, mode == PLSPM_MODE_B ? 1 : 0, (long)N, (int)k, (const double*)d_X, (const unsigned char*)d_m, (const double*)d_z,
                       correction, d_w, d_Y);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(w, d_w, sizeof(double) * k, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(Y, d_Y, sizeof(double) * N, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return done(PLSPM_E_STATE, "plspm_op_outer_weights_nonmetric: launch / copy failed");
    return done(0, "");
}

}  // extern "C"
