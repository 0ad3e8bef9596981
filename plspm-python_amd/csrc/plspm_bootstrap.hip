// plspm_bootstrap.hip -- host side, part 4: the batch driver of every call kind, phase by phase as batch_route.h plans it (check -> plan -> digit planes -> reserve ->
// void records, begin the derived chain -> error word -> per pass: Gram, lists, one of four solver arrangements -> commit), its C-ABI entry points, the record download, the device summaries and the confidence intervals,
// and what the entry points of every kind of side records share (host_internal.h SideRecords).
// Kernels: kernels_resample.h, kernels_summary.h, kernels_intervals.h.
#include "host_internal.h"

#include "philox.h"
#include "wave_ops.h"
#include "kernels_resample.h"
#include "kernels_summary.h"
#include "kernels_intervals.h"

// dense [C x C] symmetric moment matrix of every replicate out of the tile-packed one (plspm_bootstrap_moments)
__global__ void __launch_bounds__(256) moments_unpack_kernel(const double* __restrict__ gram, long psize, int T, int C, double* __restrict__ out) {
    const double* g = gram + (long)blockIdx.x * psize;
    double* o = out + (long)blockIdx.x * C * C;
    for (int e = threadIdx.x; e < C * C; e += 256) { const int p = e / C, q = e - p * C; o[e] = g[packed_index(T, p, q)]; }
}

// ------------------------------------------------------------------------------------------------ the batch driver, phase by phase
// batch_route.h decides -- batch_plan once per call, batch_chunk once per pass; the phases below only carry it out.
// What the phases of one call share
struct BatchRun {
    plspm_model* m;
    BatchCall& call;
    BatchShape shape; BatchOptions opts; BatchPlan plan;
    int R;                                               // record pitch
    int chain; int64_t chain_base;                       // the derived records (plspm_derived.hip): the stages that run, position of the call's first record
    int mod;                                             // the moderation records (plspm_moderation.hip): non-zero when they are written, from the same position
    int tet;                                             // the tetrad records (plspm_tetrad.hip): likewise
    int ipma;                                            // the importance-performance records (plspm_ipma.hip): likewise
    double* rows_out; plspm_model::Buf *status_buf, *iters_buf;
};
// ... and of one pass: problems [b0, b0 + nb), what the int8 Gram left, what batch_chunk made of it, where the solver writes
struct BatchPass { int64_t b0, nb; GramI8Result gram; BatchChunk k; SolverOut so; };

static int batch_check(plspm_model* m, const BatchCall& call) {
    if (!m || call.B < 1 || call.rep_offset < 0 || call.B > ((int64_t)1 << 30)) return fail(m, PLSPM_E_ARG, "plspm_bootstrap: bad arguments (1 <= B <= 2^30, rep_offset >= 0)");
    if (!m->d_Xa || m->N < 2) return fail(m, PLSPM_E_STATE, "plspm_bootstrap: no data uploaded");
    // (run_gram_i8 hands a count kernel rep_offset + b0 as its first problem)
    if (brings_counts(call) && (call.rep_offset || call.d_idx)) return fail(m, PLSPM_E_ARG, "plspm_bootstrap: a call that brings its own counts takes no offset or indices");
    return 0;
}

// reserve: per pass, chunk x the bytes per problem that entered the plan's per_rep; per call, the records
static int batch_reserve(BatchRun& r) {
    plspm_model* m = r.m;
    const BatchPlan& p = r.plan;
    const size_t chunk = (size_t)p.chunk, B = (size_t)r.call.B;
    int rc;
    if ((rc = ensure(m, m->ent, chunk * p.ent_bytes)) || (rc = ensure(m, m->nent, chunk * p.nent_bytes)) || (rc = ensure(m, m->gram, chunk * p.gram_bytes)) ||
        (rc = ensure(m, m->ghist, chunk * p.ghist_bytes)) || (rc = ensure(m, m->dcnt, chunk * p.dcnt_bytes)))
        return rc;
    if (p.want16 && (rc = ensure(m, m->gK16, chunk * p.gk16_bytes + 64))) return rc;
    m->dcnt_stride = p.dcnt_stride;
    if (p.micom && (rc = ensure(m, m->micom_rows, (B / 2) * p.micom_stride * sizeof(double)))) return rc;
    if (!r.call.rows_out && (rc = ensure(m, m->rows, B * r.R * sizeof(double)))) return rc;
    r.rows_out = r.call.rows_out ? r.call.rows_out : (double*)m->rows.p;
    r.status_buf = r.call.status_out ? r.call.status_out : &m->status;
    r.iters_buf = r.call.iters_out ? r.call.iters_out : &m->iters;
    if ((rc = ensure(m, *r.status_buf, B * sizeof(int))) || (rc = ensure(m, *r.iters_buf, B * sizeof(int)))) return rc;
    const void* err_before = m->err.p;
    if ((rc = ensure(m, m->err, sizeof(int)))) return rc;
    if (m->err.p != err_before) m->err_clean = false;
    return 0;
}

// The error word is cleared only in front of a call that may raise it (batch_route.h batch_may_raise), or behind one that could have: the 4-byte memset is a kernel
// of its own on the stream, ~8 us with its gaps, 1.5 % of a 5,000-replicate step
static int batch_error_word(BatchRun& r) {
    plspm_model* m = r.m;
    if (!m->err_clean || r.plan.raises) HIPCHK(m, hipMemsetAsync(m->err.p, 0, sizeof(int), m->stream));
    m->err_clean = !r.plan.raises;
    return 0;
}

// (row,count) lists (+ dense uint16 histograms where the plan wants them) of a pass: the same draws as the int8 counts
static int launch_resample_lists(BatchRun& r, const BatchPass& ps) {
    plspm_model* m = r.m;
    const BatchPlan& p = r.plan;
    const int N = (int)m->N;
    const int32_t* const d_idx = r.call.d_idx ? r.call.d_idx + ps.b0 * m->N : nullptr;
    const int64_t rep0 = r.call.rep_offset + ps.b0;
    if (!p.lds_hist) {
        ProfScope prof(m, PLSPM_K_RESAMPLE);
        hipLaunchKernelGGL(resample_global_kernel, dim3((unsigned)ps.nb), dim3(256), 0, m->stream, N, d_idx, r.call.seed, rep0, (unsigned*)m->ghist.p, (int2*)m->ent.p, (int*)m->nent.p,
                           p.ent_stride, (int*)m->err.p);
        return 0;
    }
    const size_t hist_bytes = (size_t)((m->N + 1) / 2) * sizeof(unsigned);
    if (int rc = allow_lds(m, (const void*)resample_kernel, hist_bytes)) return rc;
    ProfScope prof(m, PLSPM_K_RESAMPLE);
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)ps.nb), dim3(256), hist_bytes, m->stream, N, d_idx, r.call.seed, rep0, (int2*)m->ent.p, (int*)m->nent.p, p.ent_stride, (int*)m->err.p,
                       p.want_dcnt ? (unsigned short*)m->dcnt.p : (unsigned short*)nullptr, p.dcnt_stride);
    return 0;
}

// Gram + lists of a pass: the int8 product where the call takes it, the list resample where something reads lists, the fp64 Gram on them where the pass has no other
static int batch_gram(BatchRun& r, BatchPass& ps) {
    plspm_model* m = r.m;
    const BatchPlan& p = r.plan;
    int rc;
    ps.gram = GramI8Result{};
    if (p.gpath == 2 && (rc = run_gram_i8(m, r.call, ps.nb, ps.b0, (double*)m->gram.p, p.dense, p.want16 ? (unsigned short*)m->gK16.p : nullptr, &ps.gram))) return rc;
    ps.k = batch_chunk(p, ps.nb, ps.gram.fallback, ps.gram.wrote16);
    if (ps.k.build_lists && (rc = launch_resample_lists(r, ps))) return rc;
    if (ps.k.f64_gram) {
        ProfScope prof(m, PLSPM_K_GRAM);
        if ((rc = launch_gram_lists(m, ps.nb, (const int2*)m->ent.p, (const int*)m->nent.p, p.ent_stride, (double*)m->gram.p))) return rc;
    }
    return 0;
}

// Threads per problem of the launch-by-launch non-metric kernels unless the handle's "nm_threads" says otherwise (each stage of a HOC pair reads its own): 128 for
// the stages of a pair, else by model width (measured: 60 columns 0.60 / 0.64 / 0.81 ms with 64 / 128 / 256 threads; 300 indicator columns 21.0 / 13.5 / 10.0 ms)
static int nm_threads_of(const plspm_model* h, bool hoc_stage) {
    if (h->tune.nm_threads > 0) return h->tune.nm_threads;
    return hoc_stage ? 128 : (h->P > 128 ? 256 : (h->P > 64 ? 128 : 64));
}
// what a non-metric solve on handle `h` reads of the pass: h's moment matrices, the first stage's lists and int8 counts
static NmInputs nm_inputs(const BatchRun& r, const BatchPass& ps, const plspm_model* h, long mp_stride, bool hoc_stage) {
    const plspm_model* m = r.m;
    const bool lists = ps.k.lists, c8 = ps.k.counts8;
    return NmInputs{(const double*)h->gram.p, mp_stride, lists ? (const int2*)m->ent.p : nullptr, lists ? (const int*)m->nent.p : nullptr, r.plan.ent_stride,
                    c8 ? ps.gram.counts : nullptr, c8 ? ps.gram.counts_MT : 0, nm_threads_of(h, hoc_stage)};
}

// plspm_bootstrap_moments (test seam): the problems' moment matrices, dense, no solver
static int solve_moments(BatchRun& r, const BatchPass& ps) {
    plspm_model* m = r.m;
    const int C = m->Pg + 1;
    hipLaunchKernelGGL(moments_unpack_kernel, dim3((unsigned)ps.nb), dim3(256), 0, m->stream, (const double*)m->gram.p, r.plan.psize, m->T, C, r.call.moments_out + ps.b0 * C * C);
    return 0;
}
// two-stage HOC estimation per problem (solver_hoc.h): stage 1 to convergence (no report), stage-2 moments by congruence, stage 2 on the second handle's descriptors
// with the convergence pass streaming THIS handle's data
static int solve_hoc(BatchRun& r, const BatchPass& ps) {
    plspm_model* m = r.m;
    plspm_model* m2 = m->stage2;
    int rc;
    if ((rc = run_nonmetric(m, nm_plan(r.shape.nm, ps.k.call, r.opts.nm), nm_inputs(r, ps, m, r.plan.psize, true), SolverOut{}))) return rc;
    if ((rc = run_hoc_moments(m, m2, ps.nb))) return rc;
    rc = run_nonmetric(m2, nm_plan(r.shape.nm2, ps.k.call2, r.opts.nm2), nm_inputs(r, ps, m2, packed_size(m2->Ts), true), ps.so);
    return rc ? fail(m, rc, "second stage: " + m2->error) : 0;
}
static int solve_nm_wave(BatchRun& r, const BatchPass& ps) {
    return run_nonmetric_wave(r.m, nm_plan(r.shape.nm, ps.k.call, r.opts.nm), nm_inputs(r, ps, r.m, r.plan.psize, false), ps.so);
}
static int solve_nonmetric(BatchRun& r, const BatchPass& ps) {
    r.m->last_nm_wave16 = 0;
    return run_nonmetric(r.m, nm_plan(r.shape.nm, ps.k.call, r.opts.nm), nm_inputs(r, ps, r.m, r.plan.psize, false), ps.so);
}
// the metric batch solver, and behind it what reads the pass's moment matrices while they are still in m->gram -- dense where a dense solver read them, tile-packed
// for the LDS solver (fp64 Gram, int8 passes that fell back): the derived chain, MICOM
static int solve_metric(BatchRun& r, const BatchPass& ps) {
    plspm_model* m = r.m;
    const bool dense = ps.k.dense_solver, last = ps.b0 + ps.nb >= r.call.B;
    const double* gram = (const double*)m->gram.p;
    int rc;
    // (only the last pass's solver launch may signal the caller's event)
    if ((rc = launch_batch_solver(m, ps.nb, ps.k.route, ps.so, last ? r.call.stop_event : nullptr, &r.call.stop_taken))) return rc;
    if ((rc = derived_launch(m, r.chain, ps.nb, r.chain_base + ps.b0, dense, gram, ps.so.row, r.R))) return rc;
    if ((rc = moderation_launch(m, r.mod, ps.nb, r.chain_base + ps.b0, r.call.rep_offset + ps.b0, r.call.seed, r.call.d_idx ? r.call.d_idx + ps.b0 * m->N : nullptr, dense, gram, ps.so.row,
                                r.R)))
        return rc;
    if ((rc = tetrad_launch(m, r.tet, ps.nb, r.chain_base + ps.b0, dense, gram, ps.so.row, r.R))) return rc;
    if ((rc = ipma_launch(m, r.ipma, ps.nb, r.chain_base + ps.b0, dense, gram, ps.so.row, r.R))) return rc;
    // (a pass holds whole 256-problem tiles: the pairs stay together, and the pass that starts at problem b0 starts at permutation b0 / 2)
    if (r.plan.micom) return launch_micom(m, ps.nb / 2, dense, gram, ps.so.row, (double*)m->micom_rows.p + (ps.b0 / 2) * r.plan.micom_stride);
    return 0;
}
static int batch_solve(BatchRun& r, BatchPass& ps) {
    ps.so = SolverOut{};
    ps.so.row = r.rows_out + ps.b0 * r.R; ps.so.row_stride = r.R; ps.so.status = (int*)r.status_buf->p + ps.b0; ps.so.iters = (int*)r.iters_buf->p + ps.b0;
    switch (ps.k.solve) {
        case BATCH_SOLVE_MOMENTS: return solve_moments(r, ps);
        case BATCH_SOLVE_HOC: return solve_hoc(r, ps);
        case BATCH_SOLVE_NM_WAVE: return solve_nm_wave(r, ps);
        case BATCH_SOLVE_NONMETRIC: return solve_nonmetric(r, ps);
        default: return solve_metric(r, ps);
    }
}

static void batch_commit(BatchRun& r) {
    plspm_model* m = r.m;
    if (r.rows_out == (double*)m->rows.p) m->rows_B = r.call.B;
    if (!r.call.rows_out) { derived_commit(m, r.chain, r.call.B); moderation_commit(m, r.mod, r.call.B); tetrad_commit(m, r.tet, r.call.B); ipma_commit(m, r.ipma, r.call.B); }
    if (r.plan.micom) m->micom_B = r.call.B / 2;
}

int plspm_detail_bootstrap(plspm_model* m, BatchCall& call) {
    call.stop_taken = false;
    int rc;
    if ((rc = batch_check(m, call))) return rc;
    HIPCHK(m, hipSetDevice(m->device));
    BatchRun r{m, call, batch_shape(m), batch_options(m)};
    r.plan = batch_plan(r.shape, r.opts, batch_kind(call));
    r.R = r.shape.R;
    m->last_gram_path = r.plan.gpath; m->last_boot_passes = (int)r.plan.passes;
    if (r.plan.gpath == 2 && (rc = prepare_zs(m, r.plan.plane_floor))) return rc;
    if ((rc = batch_reserve(r))) return rc;
    // Whatever replaces the handle's bootstrap records voids the cross-validation, assessment and MICOM records that went with them (or whose status / iteration
    // buffers are reused); a jackknife call writes into buffers of its own, and whatever the handle holds survives it.
    void_records(m, call);
    // The derived records of a plain bootstrap: a call of its own (rows_out null) sizes their buffers and starts at record 0; a sub-batch of plspm_bootstrap()
    // writes from its position in that call (call.chain_off; the buffers are plspm_bootstrap's).
    if ((rc = derived_begin(m, call, &r.chain)) || (rc = moderation_begin(m, call, &r.mod)) || (rc = tetrad_begin(m, call, &r.tet)) || (rc = ipma_begin(m, call, &r.ipma))) return rc;
    r.chain_base = call.rows_out ? call.chain_off : 0;
    if ((rc = batch_error_word(r))) return rc;
    for (int64_t b0 = 0; b0 < call.B; b0 += r.plan.chunk) {
        BatchPass ps{b0, std::min<int64_t>(r.plan.chunk, call.B - b0)};
        if ((rc = batch_gram(r, ps)) || (rc = batch_solve(r, ps))) return rc;
    }
    HIPCHK(m, hipGetLastError());
    batch_commit(r);
    return 0;
}


static int fetch_segments(plspm_model* m, hipStream_t cs, const double* d_records, int32_t stride, const FetchSeg* segs, int nsegs, int64_t B_total, double* out, int32_t* status,
                          int32_t* iters);

// explicit resample rows [B][N] of a host entry point (may be null) -> m->idx
static int upload_idx(plspm_model* m, const int32_t* idx, int64_t B, const int32_t** d_idx) {
    if (!idx) return 0;
    const size_t bytes = (size_t)B * m->N * sizeof(int32_t);
    if (int rc = ensure(m, m->idx, bytes)) return rc;
    *d_idx = (const int32_t*)m->idx.p;
    return plspm_detail_h2d(m, m->idx.p, idx, bytes);
}

extern "C" {

int plspm_bootstrap_device(plspm_model_t* m, int64_t B, uint64_t seed, int64_t rep_offset, const int32_t* d_idx, void** d_out, void** d_status,
                           void** d_iters) {
    BatchCall call;
    call.B = B; call.seed = seed; call.rep_offset = rep_offset; call.d_idx = d_idx;
    int rc = plspm_detail_bootstrap(m, call);
    if (rc) return rc;
    hand_out(m->rows, m->status, m->iters, d_out, d_status, d_iters);
    return 0;
}

int plspm_bootstrap(plspm_model_t* m, int64_t B, uint64_t seed, int64_t rep_offset, const int32_t* idx, double* out, int32_t* status, int32_t* iters) {
    if (!m || !out || B < 1 || B > ((int64_t)1 << 30)) return fail(m, PLSPM_E_ARG, "plspm_bootstrap: bad arguments");
    if (!m->d_Xa) return fail(m, PLSPM_E_STATE, "plspm_bootstrap: no data uploaded");
    HIPCHK(m, hipSetDevice(m->device));
    const int32_t* d_idx = nullptr;
    int rc;
    if ((rc = upload_idx(m, idx, B, &d_idx))) return rc;
    // The call as SUB-BATCHES (round 5): the records of sub-batch k cross PCIe on a copy stream of the handle's own
    // -- and are unpacked into the caller's buffers -- while the kernels of sub-batch k + 1 run; only the last, smallest sub-batch's download is
    // exposed.  Metric models on Philox draws (explicit index lists and the non-metric iteration make host round trips inside the call as
    // it is).  The records of a replicate do not depend on the sub-batch it travels in (exact integer Gram, per-replicate solver).
    const int RS = plspm_row_stride(m);
    int64_t parts[kBootChunksMax];
    int nparts = 1;
    parts[0] = B;
    // (a call whose launches may raise the device error word -- the driver's own test -- clears that word at the start of every sub-batch, which would wipe
    //  the bits of the sub-batch before: such calls run as one batch, one memset, one read; batch_route.h batch_sub_batches_ok)
    BatchCall call;
    call.B = B; call.seed = seed; call.d_idx = d_idx;
    if (batch_sub_batches_ok(m->nonmetric != 0, may_raise(m, call)))
        nparts = plspm_detail_chunk_plan(B, (int64_t)RS * (int64_t)sizeof(double), m->tune.boot_chunks, m->tune.boot_ratio, parts, m->tune.boot_align > 0 ? m->tune.boot_align : plspm_detail_round_units(m));
    if (nparts > 1) {
        if (!m->dl) HIPCHK(m, plspm_stream_acquire(&m->dl));
        for (int k = 0; k < nparts; ++k)
            if (!m->ev_part[k]) HIPCHK(m, hipEventCreateWithFlags(&m->ev_part[k], hipEventDisableTiming));
    }
    void_records(m, REC_ROWS | REC_ASSESS | REC_PLSC);
    if ((rc = ensure(m, m->rows, (size_t)B * RS * sizeof(double)))) return rc;
    double* const rows = (double*)m->rows.p;
    // the derived records follow the sub-batches: one buffer per stage for the whole call, every part writes from its first replicate's position (call.chain_off)
    int chain = 0, mod = 0, tet = 0, ipma = 0;
    if ((rc = derived_begin(m, call, &chain)) || (rc = moderation_begin(m, call, &mod)) || (rc = tetrad_begin(m, call, &tet)) || (rc = ipma_begin(m, call, &ipma))) return rc;
    int* h_err = (int*)m->h_flag + 10;                   // (+8: plspm_bootstrap_fetch, +9: run_gram_i8's look at the multiplicity flag of an explicit index list)
    h_err[0] = h_err[1] = 0;
    FetchSeg segs[kBootChunksMax];
    int64_t b0 = 0;
    for (int k = 0; k < nparts; ++k) {
        call.B = parts[k]; call.rep_offset = rep_offset + b0; call.d_idx = d_idx ? d_idx + b0 * m->N : nullptr;
        call.rows_out = rows + b0 * RS; call.chain_off = (chain || mod || tet || ipma) ? b0 : -1;
        if ((rc = plspm_detail_bootstrap(m, call))) return rc;
        if (k == nparts - 1) {
            // ONE error word, read with the last sub-batch: copied behind the last kernel, in front of the event its download waits for
            HIPCHK(m, hipMemcpyAsync(h_err, m->err.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));
            if (m->err2.p) HIPCHK(m, hipMemcpyAsync(h_err + 1, m->err2.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));      // (experiments build: counts drawn on a second stream)
        }
        segs[k].b0 = b0; segs[k].nb = parts[k]; segs[k].ready = nullptr;
        if (nparts > 1) { HIPCHK(m, hipEventRecord(m->ev_part[k], m->stream)); segs[k].ready = m->ev_part[k]; }
        b0 += parts[k];
    }
    rc = fetch_segments(m, nparts > 1 ? m->dl : m->stream, rows, RS, segs, nparts, B, out, status, iters);
    if (nparts > 1) HIPCHK(m, hipStreamSynchronize(m->stream));      // (done already: the last download waited for the last kernel; keeps the handle's invariants simple)
    if (rc) return rc;
    m->rows_B = B;
    derived_commit(m, chain, B);
    moderation_commit(m, mod, B);
    tetrad_commit(m, tet, B);
    ipma_commit(m, ipma, B);
    if (h_err[0] & 4) return fail(m, PLSPM_E_STATE, "plspm_bootstrap: the persistent Gram gave up waiting for a partial tile (device shared with a long-running kernel?); set_option i8_sched 0");
    if (h_err[0] & 1) return fail(m, PLSPM_E_ARG, "plspm_bootstrap: resample index outside [0, N)");
    if ((h_err[0] & 2) || h_err[1]) return fail(m, PLSPM_E_LIMIT, "plspm_bootstrap: a resample multiplicity exceeded 127 on the int8 Gram path (set_option gram_path 1)");
    if (h_err[0]) return fail(m, PLSPM_E_STATE, "plspm_bootstrap: the device reported error bits " + std::to_string(h_err[0]));
    return 0;
}

int plspm_bootstrap_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status, int32_t* iters) {
    if (!m || first < 0 || count < 1) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_fetch: bad arguments");
    if (!m->rows_B || !m->rows.p) return fail(m, PLSPM_E_STATE, "plspm_bootstrap_fetch: no bootstrap records on this handle (a later call replaced them)");
    if (first + count > m->rows_B) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_fetch: range exceeds the last bootstrap's replicates");
    HIPCHK(m, hipSetDevice(m->device));
    const int RS = plspm_row_stride(m);
    int rc = plspm_detail_fetch_records(m, (const double*)m->rows.p + first * RS, count, RS, out, status, iters);
    if (rc) return rc;
    if (m->sk_epoch && m->err.p) {          // the persistent Gram's bounded wait (its tiles are NaN / status 3 then; say why)
        int* h_err = (int*)m->h_flag + 8;
        HIPCHK(m, hipMemcpyAsync(h_err, m->err.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));
        HIPCHK(m, hipStreamSynchronize(m->stream));
        if (*h_err & 4) return fail(m, PLSPM_E_STATE, "plspm_bootstrap_fetch: the persistent Gram gave up waiting for a partial tile (device shared with a long-running kernel?); set_option i8_sched 0");
    }
    return 0;
}

int plspm_bootstrap_store(plspm_model_t* m, const double* records, int64_t B) {
    if (!m || !records || B < 1 || B > ((int64_t)1 << 30)) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_store: bad arguments");
    HIPCHK(m, hipSetDevice(m->device));
    const size_t bytes = (size_t)B * plspm_row_stride(m) * sizeof(double);
    void_records(m, REC_ROWS | REC_MICOM);
    int rc;
    if ((rc = ensure(m, m->rows, bytes))) return rc;
    if ((rc = plspm_detail_h2d(m, m->rows.p, records, bytes))) return rc;
    m->rows_B = B;
    return 0;
}

int plspm_bootstrap_summary(plspm_model_t* m, const void* d_rows, int64_t B, int32_t stride, const double* original, double* summary, int64_t* n_used) {
    if (!m || !original || !summary || B < 1 || B > ((int64_t)1 << 30)) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_summary: bad arguments (1 <= B <= 2^30)");
    const double* rows = (const double*)d_rows;
    if (!rows) {
        // the handle's own records: exactly the replicates of the last plspm_bootstrap(_device) call (the buffer is never shared
        // with another result, and a different B would read stale or foreign memory as records)
        if (!m->rows_B || !m->rows.p) return fail(m, PLSPM_E_STATE, "plspm_bootstrap_summary: no bootstrap result on this handle");
        if (B != m->rows_B) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_summary: B differs from the last bootstrap on this handle");
        rows = (const double*)m->rows.p;
        stride = plspm_row_stride(m);
    }
    return plspm_detail_summary(m, rows, B, stride, plspm_row_width(m), original, summary, n_used);
}

int plspm_bootstrap_intervals(plspm_model_t* m, const void* d_rows, int64_t B, int32_t stride, const double* original, const double* accel, int32_t method, double level,
                              double* out, int64_t* n_used) {
    if (!m || !original || !out || B < 1 || B > ((int64_t)1 << 30)) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_intervals: bad arguments (1 <= B <= 2^30)");
    if (method < CI_PERCENTILE || method > CI_BCA) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_intervals: method must be 0 (percentile), 1 (basic), 2 (bc) or 3 (bca)");
    if (!(level > 0.0 && level < 1.0)) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_intervals: level must lie strictly between 0 and 1");
    if (method == CI_BCA && !accel) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_intervals: the bca method needs the acceleration of every column (plspm_jackknife_stats)");
    const double* rows = (const double*)d_rows;
    if (!rows) {
        // the handle's own records, as plspm_bootstrap_summary takes them
        if (!m->rows_B || !m->rows.p) return fail(m, PLSPM_E_STATE, "plspm_bootstrap_intervals: no bootstrap result on this handle");
        if (B != m->rows_B) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_intervals: B differs from the last bootstrap on this handle");
        rows = (const double*)m->rows.p;
        stride = plspm_row_stride(m);
    }
    return plspm_detail_intervals(m, rows, B, stride, plspm_row_width(m), original, accel, method, level, out, n_used);
}

}  // extern "C"

// Unpacking of downloaded records (strided pinned staging -> the caller's pageable rows / status / iterations) by a small resident crew:
// one thread needs ~0.3 ms for the 6.3 MB of 5,000 records, more than their four DMA chunks take (plspm_bootstrap: 0.84 ms per call against
// 0.53 on the device; 0.76 with the crew -- what is left is the device -> host copy itself, ~30 GB/s at this size on a copy-only stream or
// behind the kernels, into coherent or non-coherent pinned memory alike).  Three helper threads, started on first use and leaked with the
// process (like the memory cache): asleep on a condition variable between downloads, woken when a download starts -- the first chunk's
// DMA covers the wake-up -- and spinning on a sequence number only while that download lasts, so that handing them a chunk costs no
// system call.
namespace {
struct UnpackCrew {
    static constexpr int kHelpers = 3;
    std::mutex session;                                   // one download at a time uses the crew (handles may live on different threads)
    std::mutex mu;
    std::condition_variable cv;
    bool started = false, broken = false;
    std::atomic<int> active{0};                           // a download is running: helpers spin instead of sleeping
    std::atomic<uint64_t> seq{0};
    std::atomic<int> done{0};
    void (*fn)(void*, int, int) = nullptr;
    void* arg = nullptr;
    void helper(int t) {
        uint64_t seen = 0;
        for (;;) {
            { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return active.load(std::memory_order_acquire) > 0; }); }
            int idle = 0;
            while (active.load(std::memory_order_acquire) > 0) {
                const uint64_t s = seq.load(std::memory_order_acquire);
                if (s != seen) { seen = s; fn(arg, t, kHelpers + 1); done.fetch_add(1, std::memory_order_release); idle = 0; }
                else if (++idle > 4000) std::this_thread::yield();
            }
        }
    }
    bool begin() {
        session.lock();
        if (!started) {
            started = true;
            broken = std::thread::hardware_concurrency() < 8;
            if (!broken) {
                try { for (int t = 1; t <= kHelpers; ++t) std::thread([this, t]() { helper(t); }).detach(); }
                catch (...) { broken = true; }            // (helpers that did start sleep for ever: the crew is never activated)
            }
        }
        if (broken) { session.unlock(); return false; }
        { std::lock_guard<std::mutex> lk(mu); active.store(1, std::memory_order_release); }
        cv.notify_all();
        return true;
    }
    void run(void (*f)(void*, int, int), void* a) {       // f(a, t, T) on the caller (t = 0) and the helpers (t = 1 .. kHelpers); returns when all are done
        fn = f; arg = a;
        done.store(0, std::memory_order_relaxed);
        seq.fetch_add(1, std::memory_order_release);
        f(a, 0, kHelpers + 1);
        while (done.load(std::memory_order_acquire) < kHelpers) std::this_thread::yield();
    }
    void end() { active.store(0, std::memory_order_release); session.unlock(); }
};
UnpackCrew& unpack_crew() { static UnpackCrew* c = new UnpackCrew(); return *c; }      // leaked on purpose (must outlive every static destructor)
}  // namespace

// Record exchange of a group whose handles all live on ONE device (tests and single-GPU runs of the multi-GPU path; real multi-GPU
// groups use ncclAllGather): one launch copies every send buffer into its slot of every receive buffer -- the same G x G block copies the
// peer-to-peer route issues one by one (64 hipMemcpyAsync + 64 event waits at eight handles: 0.35 ms of host time).
struct GatherLocalArgs { const double* send[PLSPM_GATHER_LOCAL_MAX]; double* recv[PLSPM_GATHER_LOCAL_MAX]; };
template <typename T>      // double2 when a record block is a whole number of 16-byte pieces
__global__ void __launch_bounds__(256) gather_local_kernel(GatherLocalArgs a, long n) {
    const T* __restrict__ src = reinterpret_cast<const T*>(a.send[blockIdx.y]);
    T* __restrict__ dst = reinterpret_cast<T*>(a.recv[blockIdx.z]) + (long)blockIdx.y * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = src[i];
}
int plspm_detail_gather_local(hipStream_t stream, int n, const double* const* send, double* const* recv, size_t doubles, int ndst) {
    if (n < 1 || n > PLSPM_GATHER_LOCAL_MAX || ndst < 1 || ndst > n) return PLSPM_E_ARG;
    GatherLocalArgs a;
    for (int i = 0; i < n; ++i) { a.send[i] = send[i]; a.recv[i] = recv[i]; }
    for (int i = n; i < PLSPM_GATHER_LOCAL_MAX; ++i) { a.send[i] = nullptr; a.recv[i] = nullptr; }
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>((doubles + 2047) / 2048, 512));
    if (doubles % 2 == 0) hipLaunchKernelGGL(gather_local_kernel<double2>, dim3(gx, (unsigned)n, (unsigned)ndst), dim3(256), 0, stream, a, (long)(doubles / 2));
    else hipLaunchKernelGGL(gather_local_kernel<double>, dim3(gx, (unsigned)n, (unsigned)ndst), dim3(256), 0, stream, a, (long)doubles);
    return hipGetLastError() == hipSuccess ? 0 : PLSPM_E_STATE;
}

// Host copy of device records, segment by segment: segment k = records [b0, b0 + nb) of `d_records`, downloaded on `cs` once its `ready` event
// (may be null) has fired on the device side -- the copy stream waits, not the host.  Pieces of at most half the staging area -- and of at
// most a quarter of all records, so that the host's unpacking of one piece runs beside the DMA of the next even when everything would fit a
// single piece (5,000 x 158 records = 6.3 MB).
static int fetch_segments(plspm_model* m, hipStream_t cs, const double* d_records, int32_t stride, const FetchSeg* segs, int nsegs, int64_t B_total, double* out, int32_t* status,
                          int32_t* iters) {
    const int R = stride - 2;
    int rc = pin_ready(m);
    if (rc) return rc;
    int64_t per = std::max<int64_t>(1, (int64_t)(kPinHalf / ((size_t)stride * sizeof(double))));
    per = std::min<int64_t>(per, std::max<int64_t>(256, (B_total + 3) / 4));
    struct Job { const double* rec; int64_t b0, nb; int32_t stride, R; double* out; int32_t* status; int32_t* iters; };
    auto unpack_part = [](void* a, int t, int T) {
        const Job& j = *(const Job*)a;
        const int64_t lo = j.nb * t / T, hi = j.nb * (t + 1) / T;
        const double* rec = j.rec + lo * j.stride;
        for (int64_t b = lo; b < hi; ++b, rec += j.stride) {
            if (j.out) memcpy(j.out + (j.b0 + b) * j.R, rec, (size_t)j.R * sizeof(double));
            if (j.status) j.status[j.b0 + b] = (rec[j.R] == rec[j.R]) ? (int32_t)rec[j.R] : -1;      // NaN marks the padding records of a ragged shard
            if (j.iters) j.iters[j.b0 + b] = (rec[j.R + 1] == rec[j.R + 1]) ? (int32_t)rec[j.R + 1] : 0;
        }
    };
    // the crew from a megabyte of records on (smaller downloads are done before a helper has woken up)
    struct Session { bool on = false; ~Session() { if (on) unpack_crew().end(); } } crew;
    if ((size_t)B_total * stride * sizeof(double) >= ((size_t)1 << 20)) crew.on = unpack_crew().begin();
    auto unpack = [&](int h, int64_t b0, int64_t nb) {
        Job j{(const double*)((const char*)m->h_pin.p + h * kPinHalf), b0, nb, stride, R, out, status, iters};
        if (crew.on) unpack_crew().run(unpack_part, &j); else unpack_part(&j, 0, 1);
    };
    int64_t prev_b0 = 0, prev_nb = 0;
    int k = 0;
    for (int sg = 0; sg < nsegs; ++sg) {
        if (segs[sg].ready) HIPCHK(m, hipStreamWaitEvent(cs, segs[sg].ready, 0));
        for (int64_t b0 = segs[sg].b0; b0 < segs[sg].b0 + segs[sg].nb; b0 += per, ++k) {
            const int h = k & 1;
            const int64_t nb = std::min<int64_t>(per, segs[sg].b0 + segs[sg].nb - b0);
            // (half h was unpacked before the piece before this one was waited for: free)
            HIPCHK(m, hipMemcpyAsync((char*)m->h_pin.p + h * kPinHalf, d_records + b0 * stride, (size_t)nb * stride * sizeof(double), hipMemcpyDeviceToHost, cs));
            HIPCHK(m, hipEventRecord(m->ev_pin[h], cs));
            if (prev_nb) { HIPCHK(m, hipEventSynchronize(m->ev_pin[h ^ 1])); unpack(h ^ 1, prev_b0, prev_nb); }
            prev_b0 = b0; prev_nb = nb;
        }
    }
    if (prev_nb) { HIPCHK(m, hipEventSynchronize(m->ev_pin[(k - 1) & 1])); unpack((k - 1) & 1, prev_b0, prev_nb); }
    return 0;
}

int plspm_detail_fetch_records(plspm_model* m, const double* d_records, int64_t B, int32_t stride, double* out, int32_t* status, int32_t* iters) {
    const FetchSeg seg{0, B, nullptr};
    return fetch_segments(m, m->stream, d_records, stride, &seg, 1, B, out, status, iters);
}

int plspm_detail_summary(plspm_model* m, const double* rows, int64_t B, int32_t stride, int32_t ncols, const double* original, double* summary, int64_t* n_used) {
    HIPCHK(m, hipSetDevice(m->device));
    const int R = ncols;
    if (stride < R + 1) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_summary: stride must cover the status column");
    const int npad = (int)((B + 1) & ~(int64_t)1);                   // values per column (no padding needed: nothing is sorted)
    const bool in_lds = (size_t)npad * sizeof(double) <= (size_t)128 * 1024;
    int rc;
    if ((rc = pin_ready(m))) return rc;
    if ((size_t)R * 7 * sizeof(double) + 64 > m->h_pin.cap) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_summary: record too wide for the staging area");
    if (!in_lds && (rc = ensure(m, m->sum_buf, (size_t)R * npad * sizeof(double)))) return rc;
    // [original R | summary 6R | n_used] in the handle's pinned staging area, read and written by the kernel itself (R + 6R + 1 words
    // across the host link): no copy engine operation in front of or behind the kernel, whose scheduling gaps cost more than the bytes
    double* h_io = (double*)m->h_pin.p;
    memcpy(h_io, original, sizeof(double) * R);
    // the records column-major first (values + status: R + 1 columns of B, one small tiled transpose): read in place, every value of a
    // column costs the summary workgroup a 128-byte line of its own (2 x B L1 fills per column were 40 % of the kernel)
    const long cols_ld = (long)((B + 63) & ~(int64_t)63);
    if ((rc = ensure(m, m->cols, (size_t)(R + 1) * cols_ld * sizeof(double)))) return rc;
    const double* cols = (const double*)m->cols.p;
    hipLaunchKernelGGL(records_transpose_kernel, dim3((unsigned)((B + 63) / 64), (unsigned)((R + 1 + 63) / 64)), dim3(256), 0, m->stream, rows, (long)B, (int)stride, R + 1, (double*)m->cols.p,
                       cols_ld);
    double* h_out = h_io + R;
    int* h_used = (int*)(h_out + (size_t)R * 6);
    if (in_lds) {
        const size_t lds = (size_t)npad * sizeof(double);
        if ((rc = allow_lds(m, (const void*)summary_kernel<true>, lds))) return rc;
        hipLaunchKernelGGL((summary_kernel<true>), dim3(R), dim3(SUM_NT), lds, m->stream, cols, cols_ld, (long)B, R, (const double*)h_io, (double*)nullptr, npad, h_out, h_used);
    } else {
        hipLaunchKernelGGL((summary_kernel<false>), dim3(R), dim3(SUM_NT), 0, m->stream, cols, cols_ld, (long)B, R, (const double*)h_io, (double*)m->sum_buf.p, npad, h_out, h_used);
    }
    HIPCHK(m, hipGetLastError());
    HIPCHK(m, hipStreamSynchronize(m->stream));
    memcpy(summary, h_io + R, sizeof(double) * R * 6);
    if (n_used) *n_used = *(const int*)(h_io + R + (size_t)R * 6);
#ifdef PLSPM_DEBUG_MARKS
    {
        long long h[16];
        HIPCHK(m, hipMemcpyFromSymbol(h, HIP_SYMBOL(g_summary_marks), sizeof(h)));
        fprintf(stderr, "[plspm summary clocks] compaction %lld  mean+var %lld  select %lld  successors %lld  total %lld\n", h[1] - h[0], h[2] - h[1], h[3] - h[2], h[4] - h[3], h[4] - h[0]);
    }
#endif
    return 0;
}

// The nominal levels of a two-sided interval, alpha = (1 - level) / 2 and 1 - alpha = (1 + level) / 2, rounded to twelve decimals: 1 - 0.95 is not 0.05 in
// binary, and the percentile interval at level 0.95 has to interpolate at exactly the summary's 0.025 and 0.975 (plspm.bootstrap._ci_levels is the same rule).
static void ci_levels(double level, double* lo, double* hi) {
    *lo = nearbyint((1.0 - level) * 0.5 * 1e12) / 1e12;
    *hi = nearbyint((1.0 + level) * 0.5 * 1e12) / 1e12;
}

int plspm_detail_intervals(plspm_model* m, const double* rows, int64_t B, int32_t stride, int32_t ncols, const double* original, const double* accel, int32_t method, double level,
                           double* out, int64_t* n_used) {
    HIPCHK(m, hipSetDevice(m->device));
    const int R = ncols;
    if (stride < R + 1) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_intervals: stride must cover the status column");
    const int npad = (int)((B + 1) & ~(int64_t)1);
    const bool in_lds = npad <= CI_LDS_VALUES;
    int rc;
    if ((rc = pin_ready(m))) return rc;
    if ((size_t)R * 8 * sizeof(double) + 64 > m->h_pin.cap) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_intervals: record too wide for the staging area");
    if (!in_lds && (rc = ensure(m, m->sum_buf, (size_t)R * npad * sizeof(double)))) return rc;
    // [original R | accel R | intervals 6R | n_used] in the handle's pinned staging area, read and written by the kernel itself (plspm_detail_summary)
    double* h_io = (double*)m->h_pin.p;
    memcpy(h_io, original, sizeof(double) * R);
    if (accel) memcpy(h_io + R, accel, sizeof(double) * R);
    const long cols_ld = (long)((B + 63) & ~(int64_t)63);
    if ((rc = ensure(m, m->cols, (size_t)(R + 1) * cols_ld * sizeof(double)))) return rc;
    const double* cols = (const double*)m->cols.p;
    hipLaunchKernelGGL(records_transpose_kernel, dim3((unsigned)((B + 63) / 64), (unsigned)((R + 1 + 63) / 64)), dim3(256), 0, m->stream, rows, (long)B, (int)stride, R + 1, (double*)m->cols.p,
                       cols_ld);
    double* h_out = h_io + 2 * (size_t)R;
    int* h_used = (int*)(h_out + (size_t)R * 6);
    double a_lo, a_hi;
    ci_levels(level, &a_lo, &a_hi);
    if (in_lds) {
        const size_t lds = (size_t)npad * sizeof(double);
        if ((rc = allow_lds(m, (const void*)intervals_kernel<true>, lds))) return rc;
        hipLaunchKernelGGL((intervals_kernel<true>), dim3(R), dim3(SUM_NT), lds, m->stream, cols, cols_ld, (long)B, R, (const double*)h_io, (const double*)(h_io + R), (int)method, a_lo, a_hi,
                           (double*)nullptr, npad, h_out, h_used);
    } else {
        hipLaunchKernelGGL((intervals_kernel<false>), dim3(R), dim3(SUM_NT), 0, m->stream, cols, cols_ld, (long)B, R, (const double*)h_io, (const double*)(h_io + R), (int)method, a_lo, a_hi,
                           (double*)m->sum_buf.p, npad, h_out, h_used);
    }
    HIPCHK(m, hipGetLastError());
    HIPCHK(m, hipStreamSynchronize(m->stream));
    memcpy(out, h_out, sizeof(double) * R * 6);
    if (n_used) *n_used = *(const int*)h_used;
    return 0;
}

extern "C" {

int plspm_bootstrap_moments(plspm_model_t* m, int64_t B, uint64_t seed, int64_t rep_offset, const int32_t* idx, double* out) {
    if (!m || !out || B < 1) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_moments: bad arguments");
    if (!m->d_Xa) return fail(m, PLSPM_E_STATE, "plspm_bootstrap_moments: no data uploaded");
    if (m->stage1) return fail(m, PLSPM_E_ARG, "plspm_bootstrap_moments: not on an attached second stage");
    HIPCHK(m, hipSetDevice(m->device));
    const int32_t* d_idx = nullptr;
    int rc;
    if ((rc = upload_idx(m, idx, B, &d_idx))) return rc;
    const size_t C = (size_t)m->Pg + 1, bytes = (size_t)B * C * C * sizeof(double);
    double* d_out = nullptr;
    HIPCHK(m, plspm_dmalloc((void**)&d_out, bytes));
    BatchCall call;
    call.B = B; call.seed = seed; call.rep_offset = rep_offset; call.d_idx = d_idx; call.moments_out = d_out;
    rc = plspm_detail_bootstrap(m, call);
    if (!rc) {
        hipError_t e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, m->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
        if (e != hipSuccess) rc = fail(m, -(int)e, std::string("plspm_bootstrap_moments: ") + hipGetErrorString(e));
    } else hipStreamSynchronize(m->stream);
    plspm_dfree(d_out);
    void_records(m, REC_ROWS);      // (the driver left B in rows_B for records it never wrote; a call it refused for its arguments voids them too, as ever)
    return rc;
}

}  // extern "C"

// ---- the calls that bring their own count rows (host_internal.h): what their entry points refuse alike, in two steps around their own argument checks
int counts_call_scope(plspm_model* m, const char* who, int64_t min_rows) {
    if (!m->d_Xa || m->N < min_rows) return fail(m, PLSPM_E_STATE, std::string(who) + ": no data uploaded");
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, std::string(who) + ": plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)");
    return 0;
}
int counts_route_scope(plspm_model* m, const char* who) {
    if (m->tune.i8_shape != 16) return fail(m, PLSPM_E_ARG, std::string(who) + ": needs the 16x16x64 layout of the int8 Gram (i8_shape 16)");
    HIPCHK(m, hipSetDevice(m->device));
    // the int8 route whatever "gram_path" / "i8_min_batch" say (the dense 0/1 counts are what it reads; they add up to less than N, and the statistics are differences
    // of nearly equal estimates: seven digit planes at least), unless the route itself is closed at the seven planes such a call cuts
    if (!gram_counts_route_open(m)) return fail(m, PLSPM_E_LIMIT, std::string(who) + ": the int8 Gram route is closed for this data set (N >= 2^24, or digit planes above their 24 GiB budget)");
    return 0;
}

// ---- side records (host_internal.h SideRecords): the state check, the fetch, the summary and the intervals that the entry points of plspm_derived.hip and plspm_micom_* share
int side_state(plspm_model* m, const SideRecords& s, int64_t B, const char* who) {
    if (!s.count || !s.buf.p) return fail(m, PLSPM_E_STATE, std::string(who) + s.none);
    if (B != s.count) return fail(m, PLSPM_E_ARG, std::string(who) + s.differs);
    return 0;
}
static int side_scope(plspm_model* m, const SideRecords& s, const char* who) {
    return s.plain_only && !plain_metric(m) ? fail(m, PLSPM_E_ARG, std::string(who) + ": plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)") : 0;
}
int side_fetch(plspm_model* m, const SideRecords& s, int64_t first, int64_t count, double* out, int32_t* status, const char* who) {
    if (first < 0 || count < 1) return fail(m, PLSPM_E_ARG, std::string(who) + ": bad arguments");
    if (int rc = side_scope(m, s, who)) return rc;
    if (!s.count || !s.buf.p) return fail(m, PLSPM_E_STATE, std::string(who) + s.none);
    if (first + count > s.count) return fail(m, PLSPM_E_ARG, std::string(who) + s.range);
    HIPCHK(m, hipSetDevice(m->device));
    return plspm_detail_fetch_records(m, (const double*)s.buf.p + first * (s.width + 2), count, s.width + 2, out, status, nullptr);
}
int side_summary(plspm_model* m, const SideRecords& s, int64_t B, const double* original, double* summary, int64_t* n_used, const char* who) {
    if (!original || !summary || B < 1 || B > ((int64_t)1 << 30)) return fail(m, PLSPM_E_ARG, std::string(who) + ": bad arguments (1 <= B <= 2^30)");
    int rc;
    if ((rc = side_scope(m, s, who)) || (rc = side_state(m, s, B, who))) return rc;
    return plspm_detail_summary(m, (const double*)s.buf.p, B, s.width + 2, s.width, original, summary, n_used);
}
int side_intervals(plspm_model* m, const SideRecords& s, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used, const char* who) {
    if (!original || !out || B < 1 || B > ((int64_t)1 << 30)) return fail(m, PLSPM_E_ARG, std::string(who) + ": bad arguments (1 <= B <= 2^30)");
    if (int rc = side_scope(m, s, who)) return rc;
    if (method < CI_PERCENTILE || method >= CI_BCA) return fail(m, PLSPM_E_ARG, std::string(who) + s.method);
    if (!(level > 0.0 && level < 1.0)) return fail(m, PLSPM_E_ARG, std::string(who) + ": level must lie strictly between 0 and 1");
    if (int rc = side_state(m, s, B, who)) return rc;
    return plspm_detail_intervals(m, (const double*)s.buf.p, B, s.width + 2, s.width, original, nullptr, method, level, out, n_used);
}
