// plspm_moderation.hip -- host side, part 12: moderation analysis by the two-stage approach.  The terms' lists of a handle (moderation_core.h
// moderation_build, at plspm_moderation_enable), the four launches behind the metric solver of a plain bootstrap's pass (plspm_bootstrap.hip hooks them in behind
// the chain of plspm_derived.hip: moderation_begin, moderation_launch, moderation_commit), the full-sample record -- the same kernels on one problem with every
// multiplicity 1 -- and the C-ABI entry points (plspm_moderation_*).  Not a stage of derived_route.h's table: the row pass reads the resident rows and the
// replicates' draws, which that chain does not carry.  Kernels: kernels_moderation.h (its opening: kernels_moments.h).
#include "wave_launch.h"

#include "philox.h"
#include "wave_ops.h"
#include "kernels_moderation.h"

static const char kModPlainOnly[] = ": plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)";

static ModDesc mod_desc(const plspm_model* m) { return ModDesc{m->mod_lay, (const int*)m->mod_desc.p}; }
static int mod_width(const plspm_model* m) { return (m && m->mod_lay.T) ? moderation_width(m->mod_lay) : 0; }

// What one launch of the four kernels works on: `nb` problems whose counts are the draws of replicates rep0 .. (or the explicit rows at d_idx, or all ones), their
// moment matrices and bootstrap records, and where the moderation records go.
struct ModCall { long nb; const int32_t* d_idx; uint64_t seed; int64_t rep0; bool ones; MomentLayout mom; bool dense; const double* rows; long row_stride; double* out; };

template <int NACC>
static int launch_rows(plspm_model* m, const ModPlan& pl, const ModRowsArgs& a, long groups) {
    auto k = pl.table_in_lds ? moderation_rows_kernel<NACC, true> : moderation_rows_kernel<NACC, false>;
    if (int rc = allow_lds(m, (const void*)k, pl.rows_lds)) return rc;
    ProfScope ps(m, PLSPM_K_MOD_ROWS);
    hipLaunchKernelGGL(k, dim3((unsigned)((pl.row_blocks + kModRowsWaves - 1) / kModRowsWaves), (unsigned)groups), dim3(64 * kModRowsWaves), pl.rows_lds, m->stream, a);
    return 0;
}

static int mod_launch(plspm_model* m, const ModCall& c) {
    const ModLayout& y = m->mod_lay;
    const long N = (long)m->N;
    const ModPlan pl = moderation_plan(y, m->mod_e_total, N);
    if (pl.refused) return fail(m, PLSPM_E_LIMIT, std::string("moderation: ") + moderation_refusal(pl.refused));
    const long groups = (c.nb + 63) / 64, nbpad = groups * 64, ntab = y.ncoef + y.nl;
    int rc;
    if ((rc = ensure(m, m->mod_cnt, (size_t)groups * N * 64 * sizeof(unsigned short))) || (rc = ensure(m, m->mod_table, (size_t)groups * ntab * 64 * sizeof(double))) ||
        (rc = ensure(m, m->mod_rc, (size_t)c.nb * y.nl * y.nl * sizeof(double))) || (rc = ensure(m, m->mod_partial, (size_t)pl.row_blocks * y.nsums * nbpad * sizeof(double))))
        return rc;
    const ModDesc d = mod_desc(m);
    {
        ModCountsArgs a{(int)N, c.nb, c.d_idx, c.seed, c.rep0, c.ones ? 1 : 0, (unsigned short*)m->mod_cnt.p};
        if ((rc = allow_lds(m, (const void*)moderation_counts_kernel, pl.counts_lds))) return rc;
        ProfScope ps(m, PLSPM_K_MOD_COUNTS);
        hipLaunchKernelGGL(moderation_counts_kernel, dim3((unsigned)c.nb), dim3(256), pl.counts_lds, m->stream, a);
    }
    {
        ModPrepareArgs a{c.mom, d, plspm_row_width(m), m->d_boff, c.rows, c.row_stride, (double*)m->mod_table.p, (double*)m->mod_rc.p, c.nb};
        auto k = c.dense ? moderation_prepare_kernel<true> : moderation_prepare_kernel<false>;
        if ((rc = allow_lds(m, (const void*)k, pl.prepare_lds))) return rc;
        ProfScope ps(m, PLSPM_K_MOD_PREPARE);
        hipLaunchKernelGGL(k, dim3((unsigned)((c.nb + kModPrepareWaves - 1) / kModPrepareWaves)), dim3(64 * kModPrepareWaves), pl.prepare_lds, m->stream, a);
    }
    {
        ModRowsArgs a{m->d_Xa, (int)N, m->PA, d, m->d_boff, (const unsigned short*)m->mod_cnt.p, (const double*)m->mod_table.p, (double*)m->mod_partial.p, nbpad, pl.row_block, pl.row_blocks};
        rc = pl.nacc == 16 ? launch_rows<16>(m, pl, a, groups) : pl.nacc == 32 ? launch_rows<32>(m, pl, a, groups) : pl.nacc == 64 ? launch_rows<64>(m, pl, a, groups)
                                                                                                                                      : launch_rows<128>(m, pl, a, groups);
        if (rc) return rc;
    }
    {
        ModFinishArgs a{d, plspm_row_width(m), m->mod_e_total, pl.row_blocks, nbpad, (double)N, (const double*)m->mod_partial.p, (const double*)m->mod_rc.p, c.rows, c.row_stride, c.out, c.nb};
        if ((rc = allow_lds(m, (const void*)moderation_finish_kernel, pl.finish_lds))) return rc;
        ProfScope ps(m, PLSPM_K_MOD_FINISH);
        hipLaunchKernelGGL(moderation_finish_kernel, dim3((unsigned)c.nb), dim3(64), pl.finish_lds, m->stream, a);
    }
    return 0;
}

// ---- the batch driver's three calls (host_internal.h): the rule of derived_begin
int moderation_begin(plspm_model* m, const BatchCall& call, int* runs) {
    *runs = 0;
    const bool own = !call.rows_out;
    if (!m->mod_on || !(own || call.chain_off >= 0) || !plain_metric(m) || call.kind != BatchCall::PLAIN || call.moments_out) return 0;
    const ModPlan pl = moderation_plan(m->mod_lay, m->mod_e_total, (long)m->N);
    if (pl.refused) return fail(m, PLSPM_E_LIMIT, std::string("moderation: ") + moderation_refusal(pl.refused));      // (before anything of the call runs)
    if (own)
        if (int rc = ensure(m, m->mod_rows, (size_t)call.B * (pl.width + 2) * sizeof(double))) return rc;
    *runs = 1;
    return 0;
}

int moderation_launch(plspm_model* m, int runs, long nb, int64_t pos, int64_t rep0, uint64_t seed, const int32_t* d_idx, bool dense, const double* gram, const double* rows,
                      long row_stride) {
    if (!runs) return 0;
    ModCall c{nb, d_idx, seed, rep0, false, moment_layout(m, dense, gram), dense, rows, row_stride, (double*)m->mod_rows.p + pos * (mod_width(m) + 2)};
    return mod_launch(m, c);
}

void moderation_commit(plspm_model* m, int runs, int64_t B) {
    if (runs) m->mod_B = B;
}

static SideRecords mod_records(const plspm_model* m) {
    return {m->mod_rows, m->mod_B, mod_width(m), true,
            ": no moderation records on this handle (plspm_moderation_enable, then a plain bootstrap; an upload or a later call replaced them)",
            ": B differs from the last moderated bootstrap on this handle", ": range exceeds the last moderated bootstrap's replicates",
            ": method must be 0 (percentile), 1 (basic) or 2 (bc); the jackknife writes no moderation records, so there is no bca"};
}

extern "C" {

int plspm_moderation_enable(plspm_model_t* m, int32_t n_terms, const int32_t* predictor, const int32_t* moderator, const int32_t* target) {
    const std::string who = "plspm_moderation_enable";
    if (!m) return fail(m, PLSPM_E_ARG, who + ": no handle");
    if (n_terms == 0) { m->mod_on = false; return 0; }
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, who + kModPlainOnly);
    if (n_terms < 0 || !predictor || !moderator || !target) return fail(m, PLSPM_E_ARG, who + ": bad arguments");
    ModBuild mb;
    std::string why;
    if (moderation_build(m->L, m->P, m->boff.data(), m->C.data(), m->pred_off.data(), m->pred_idx.data(), m->n_eff, m->eff_from.data(), m->eff_to.data(), n_terms, predictor, moderator,
                         target, mb, why))
        return fail(m, PLSPM_E_ARG, who + ": " + why);
    const ModPlan pl = moderation_plan(mb.lay, mb.e_total, m->d_Xa ? (long)m->N : 0);
    if (pl.refused) return fail(m, PLSPM_E_LIMIT, who + ": " + moderation_refusal(pl.refused));
    HIPCHK(m, hipSetDevice(m->device));
    if (int rc = ensure(m, m->mod_desc, mb.blob.size() * sizeof(int))) return rc;
    HIPCHK(m, hipStreamSynchronize(m->stream));      // (nothing in flight reads the lists before them)
    HIPCHK(m, hipMemcpy(m->mod_desc.p, mb.blob.data(), mb.blob.size() * sizeof(int), hipMemcpyHostToDevice));
    m->mod_lay = mb.lay; m->mod_e_total = mb.e_total;
    m->mod_terms.assign(predictor, predictor + n_terms);
    m->mod_terms.insert(m->mod_terms.end(), moderator, moderator + n_terms);
    m->mod_terms.insert(m->mod_terms.end(), target, target + n_terms);
    m->mod_B = 0;                                     // (records of other terms have another layout)
    m->mod_on = true;
    return 0;
}

int32_t plspm_moderation_width(const plspm_model_t* m) { return mod_width(m); }

int plspm_moderation_fit(plspm_model_t* m, double* out, int32_t* status) {
    const std::string who = "plspm_moderation_fit";
    if (!m || !out) return fail(m, PLSPM_E_ARG, who + ": bad arguments");
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, who + kModPlainOnly);
    if (!m->mod_lay.T) return fail(m, PLSPM_E_STATE, who + ": no interaction terms on this handle (plspm_moderation_enable)");
    if (!m->d_Xa || m->N < 2) return fail(m, PLSPM_E_STATE, who + ": no data uploaded");
    HIPCHK(m, hipSetDevice(m->device));
    // [the solver's record R + 2 | the moderation record W + 2 | status, iterations (int)]
    const int RS = plspm_row_stride(m), W = mod_width(m);
    int rc;
    if ((rc = ensure(m, m->mod_fit, (size_t)(RS + W + 2) * sizeof(double) + 2 * sizeof(int)))) return rc;
    double* const rec = (double*)m->mod_fit.p;
    if ((rc = solve_full_sample(m, rec, (int*)(rec + RS + W + 2)))) return rc;      // (its moments: tile-packed, in m->gram)
    ModCall c{1, nullptr, 0, 0, true, moment_layout(m, false, (const double*)m->gram.p), false, rec, 0, rec + RS};
    if ((rc = mod_launch(m, c))) return rc;
    HIPCHK(m, hipGetLastError());
    std::vector<double> h((size_t)W + 2);
    HIPCHK(m, hipMemcpyAsync(h.data(), rec + RS, h.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    std::copy(h.begin(), h.begin() + W, out);
    if (status) *status = (h[W] == h[W]) ? (int32_t)h[W] : -1;
    return 0;
}

int plspm_moderation_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) {
    return m ? side_fetch(m, mod_records(m), first, count, out, status, "plspm_moderation_fetch") : fail(m, PLSPM_E_ARG, "plspm_moderation_fetch: bad arguments");
}

int plspm_moderation_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) {
    return m ? side_summary(m, mod_records(m), B, original, summary, n_used, "plspm_moderation_summary") : fail(m, PLSPM_E_ARG, "plspm_moderation_summary: bad arguments (1 <= B <= 2^30)");
}

int plspm_moderation_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return m ? side_intervals(m, mod_records(m), B, original, method, level, out, n_used, "plspm_moderation_intervals")
             : fail(m, PLSPM_E_ARG, "plspm_moderation_intervals: bad arguments (1 <= B <= 2^30)");
}

}  // extern "C"
