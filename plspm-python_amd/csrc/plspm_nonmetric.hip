// plspm_nonmetric.hip -- host side, part 2b: the non-metric iteration (Scale.NUM / RAW, ORD / NOM, incomplete rows, HOC second stages):
// prepare -> (step, stop-rule pass)* -> finish, the host reading one counter per iteration; or the whole batch in one launch + a verification.
// Which of these a call takes is decided in nm_route.h (NmPlan); this file carries the plan out.  Kernels: kernels_nonmetric.h, kernels_nmw.h, kernels_nmp.h.
#include "host_internal.h"

#include "wave_ops.h"
#include "device_exec.h"
#include "kernels_nonmetric.h"
#include "kernels_nmw.h"
#include "kernels_nmp.h"

namespace {

// The wave step's instantiation for the plan's (LMAX, CMAX, CPL): LMAX 2 / 4 / 6 / 8 LVs x (8 categories, six or eight columns per lane | 10, six | 16, six or eight),
// each as the launch-by-launch step (SUB: with the step's own bound) and as the one-launch form (SUB + ONE).  nm_plan holds the rule and its one exclusion.
using NmwStepFn = decltype(&nmw::nmw_step_kernel<2, 8, false, false, 6>);
template <bool SUB, bool ONE, int CMAX, int CPL> NmwStepFn nmw_step_lmax(int lmax) {
    return lmax == 2 ? nmw::nmw_step_kernel<2, CMAX, SUB, ONE, CPL> : lmax == 4 ? nmw::nmw_step_kernel<4, CMAX, SUB, ONE, CPL>
         : lmax == 6 ? nmw::nmw_step_kernel<6, CMAX, SUB, ONE, CPL> : nmw::nmw_step_kernel<8, CMAX, SUB, ONE, CPL>;
}
template <bool SUB, bool ONE> NmwStepFn nmw_step_of(const NmPlan& pl) {
    if (pl.step_cmax == 10) return nmw_step_lmax<SUB, ONE, 10, 6>(pl.step_lmax);
    if (pl.step_cmax == 8) return pl.step_cpl == 6 ? nmw_step_lmax<SUB, ONE, 8, 6>(pl.step_lmax) : nmw_step_lmax<SUB, ONE, 8, 8>(pl.step_lmax);
    return pl.step_cpl == 6 ? nmw_step_lmax<SUB, ONE, 16, 6>(pl.step_lmax) : nmw_step_lmax<SUB, ONE, 16, 8>(pl.step_lmax);
}
auto nm_dense_kernel_of(const NmPlan& pl, bool counts8) {
    return counts8 ? (pl.dense_whole ? nm_conv_dense_kernel<16, 8, false, true> : nm_conv_dense_kernel<16, 8, true, true>)
                   : (pl.dense_whole ? nm_conv_dense_kernel<16, 8, false, false> : nm_conv_dense_kernel<16, 8, true, false>);
}

// What the phases of one run_nonmetric call share
struct NmRun {
    plspm_model* m;
    plspm_model* src;            // an attached second stage streams its first stage's data (solver_hoc.h)
    const NmPlan& pl;
    long nproblems;
    const double* Mp; long mp_stride;
    SolverOut so;
    const int2* ent; const int* nent; long ent_stride;
    int threads;
    const void* cd8; int cd8_MT;
    ModelDesc md; CatDesc cd; ModelDesc mdm;
    bool cat, nmx;
    int fuse;                    // the finish of a problem runs inside the step launch that decides its stop
    double *gS, *gSm, *gst, *part;
    int* nact;
    const int *codes_base, *codes_lmv;      // a second HOC stage streams its first stage's rows under its own blocks and keeps its own code table
    size_t conv_lds; long ps_stride;
};

// Buffers, LDS opt-ins, the once-per-upload tables (tiled transpose, category codes, indicator bytes) and the report fields of a call
int nm_prepare(NmRun& r) {
    plspm_model* m = r.m; plspm_model* src = r.src;
    const NmPlan& pl = r.pl;
    const int P = m->P, L = m->L;
    const long N = src->N, nproblems = r.nproblems, ntiles16 = pl.ntiles16;
    int rc;
    if (pl.dense) {
        if ((rc = ensure(m, src->Xt, (size_t)ntiles16 * 16 * src->PA * sizeof(double)))) return rc;
        if ((rc = ensure(m, m->ctable, (size_t)pl.ngroups * pl.table_rows * 64 * sizeof(double)))) return rc;
        if ((rc = ensure(m, m->nmlist, 2 * ((size_t)nproblems + 1) * sizeof(int)))) return rc;      // [count | live problems] + [count | those that ask for the pass over all rows]
        if ((rc = allow_lds(m, (const void*)nm_dense_kernel_of(pl, pl.call.counts8), pl.dense_lds))) return rc;
        if (!src->Xt_valid) {
            hipLaunchKernelGGL(tile_transpose_kernel, dim3((unsigned)ntiles16), dim3(256), 0, m->stream, (const double*)src->d_Xa, N, src->PA, (double*)src->Xt.p);
            src->Xt_valid = true;
        }
    }
    if (pl.use_codes) {          // one table of 16 codes per (row tile, MV), built once per upload
        if ((rc = allow_lds(m, (const void*)nm_conv_codes_kernel<8>, pl.codes_lds))) return rc;
        if (!m->codes_valid) {
            if ((rc = ensure(m, m->codes, (size_t)ntiles16 * src->Pm * 16 * sizeof(unsigned short)))) return rc;
            const long total = ntiles16 * src->Pm * 16;
            hipLaunchKernelGGL(cat_codes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, m->stream, (const double*)src->d_Xa, N, src->PA, src->Pm, (const int*)src->d_mv_off,
                               r.codes_base, pl.kb, ntiles16, (unsigned short*)m->codes.p);
            m->codes_valid = true;
        }
    }
    if (pl.use_mfma) {           // indicator bytes x digit planes of the score maps (kernels_nmp.h)
        if (!m->ind8_valid) {
            if ((rc = ensure(m, m->ind8, (size_t)L * ntiles16 * pl.KS * 64 * sizeof(uint4)))) return rc;
            const long total = (long)L * ntiles16 * pl.KS * 64;
            hipLaunchKernelGGL(nmp::ind8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, m->stream, (const unsigned short*)m->codes.p, ntiles16, src->Pm, L, pl.KS, r.codes_lmv,
                               (uint4*)m->ind8.p);
            m->ind8_valid = true;
        }
        if ((rc = ensure(m, m->tab8, (size_t)pl.ng16 * L * 2 * nmp::S * pl.KS * 64 * sizeof(uint4)))) return rc;
        if ((rc = ensure(m, m->scl8, (size_t)pl.ng16 * L * 2 * 16 * sizeof(double2)))) return rc;
    }
    m->last_nm_codes = pl.use_codes ? 1 : 0;
    m->last_nm_problems = nproblems;
    m->last_nm_exact = 0;
    m->last_nm_mfma = pl.use_mfma ? 1 : 0;
    m->last_nm_wave = pl.wave_step ? 1 : 0;
    m->last_nm_direct16 = pl.call.counts16_ready ? 1 : 0;
    m->last_nm_one = pl.one_launch ? 1 : 0;
    if (r.cat && (rc = ensure(m, m->gSm, (size_t)nproblems * cov_doubles(m->Pm) * sizeof(double)))) return rc;
    if ((rc = ensure(m, m->nmstate, (size_t)nproblems * pl.st_doubles * sizeof(double)))) return rc;
    // the fp64 square of every problem (730 KB at 300 indicator columns): not for the wave step, which reads the uint16 counts only
    if (!pl.wave_step && (rc = ensure(m, m->gS, (size_t)nproblems * cov_doubles(P) * sizeof(double)))) return rc;
    if (pl.k16 && (rc = ensure(m, m->gK16, (size_t)nproblems * (P + 1) * pl.ld16 * sizeof(unsigned short) + 64))) return rc;      // (+ 64: the six-column lanes of the last row read a dword past it)
    if ((rc = ensure(m, m->nmpartial, (size_t)nproblems * pl.nparts * sizeof(double)))) return rc;
    if ((rc = ensure(m, m->nmactive, sizeof(int)))) return rc;
    if (r.cat) {
        if ((rc = allow_lds(m, (const void*)nmg_kernel<0>, pl.lds)) || (rc = allow_lds(m, (const void*)nmg_kernel<1>, pl.lds)) || (rc = allow_lds(m, (const void*)nmg_kernel<2>, pl.lds)) ||
            (rc = allow_lds(m, (const void*)nmg_kernel<3>, pl.lds)) || (rc = allow_lds(m, (const void*)nmg_kernel<4>, pl.lds)))
            return rc;
    } else if (r.nmx) {
        if ((rc = allow_lds(m, (const void*)nmx_kernel<0>, pl.lds)) || (rc = allow_lds(m, (const void*)nmx_kernel<1>, pl.lds)) || (rc = allow_lds(m, (const void*)nmx_kernel<2>, pl.lds)))
            return rc;
    } else if ((rc = allow_lds(m, (const void*)nm_kernel<0>, pl.lds)) || (rc = allow_lds(m, (const void*)nm_kernel<1>, pl.lds)) || (rc = allow_lds(m, (const void*)nm_kernel<2>, pl.lds)))
        return rc;
    r.conv_lds = ((size_t)SCORE_ROWS * (src->PA + 1) + 2 * (size_t)src->P + 2 * (size_t)L + SCORE_ROWS + 256) * sizeof(double) + (size_t)(L + 2) * sizeof(int);
    r.ps_stride = 8 + 4L * src->P + 2L * L;
    if (m->stage1 && (rc = ensure(m, m->pseudo, (size_t)nproblems * r.ps_stride * sizeof(double)))) return rc;
    if ((rc = allow_lds(m, (const void*)nm_conv_kernel, r.conv_lds))) return rc;
    const NmwStepFn step_kernel = pl.one_launch ? nmw_step_of<true, true>(pl) : pl.sub_pass ? nmw_step_of<true, false>(pl) : nmw_step_of<false, false>(pl);
    if (pl.wave_step && (rc = allow_lds(m, (const void*)step_kernel, pl.wave_lds))) return rc;
    r.gS = (double*)m->gS.p; r.gSm = (double*)m->gSm.p; r.gst = (double*)m->nmstate.p; r.part = (double*)m->nmpartial.p; r.nact = (int*)m->nmactive.p;
    return 0;
}

// the start of a wave-step batch: the uint16 counts + the initial state of the problems of `list` (null: all `count`)
void nm_launch_start16(const NmRun& r, long count, const int* list) {
    plspm_model* m = r.m;
    const NmPlan& pl = r.pl;
    if (pl.call.counts16_ready)      // the Gram wrote the upper triangles: mirror them, set the initial state (no packed fp64 matrix exists)
        hipLaunchKernelGGL(nmg_kernel<4>, dim3((unsigned)count), dim3(256), pl.lds, m->stream, r.md, r.cd, r.mdm, (const double*)nullptr, 0L, r.so, r.gS, r.gSm, r.gst, pl.st_doubles, (const double*)r.part,
                           pl.nparts, r.nact, 0, pl.cat_fast, (unsigned short*)m->gK16.p, pl.ld16, list);
    else
        hipLaunchKernelGGL(nmg_kernel<3>, dim3((unsigned)count), dim3(r.threads), pl.lds, m->stream, r.md, r.cd, r.mdm, r.Mp, r.mp_stride, r.so, r.gS, r.gSm, r.gst, pl.st_doubles, (const double*)r.part,
                           pl.nparts, r.nact, 0, pl.cat_fast, (unsigned short*)m->gK16.p, pl.ld16, list);
}

// The integer and sum scratch of a one-launch form's verification (Scale.NUM / RAW: run_nonmetric_wave; categorical: nm_run_one_launch), `slots` steps per round and replicate
struct VerifyScratch {
    long capV;                           // slots of a round
    int *steps, *force, *fixlist;        // per replicate: steps taken, the stop the exact pass moved it to, the replicates to replay
    int *vb, *vj, *fb, *fj, *vneed;      // per slot: (replicate, step) of the round / of what the lower bound left open, row chunks a slot asks for
    int* cnt;                            // [0] virtual problems of the round, [1] flagged, [2] replicates to replay
    double* vsum;
    int* h;                              // pinned: [0] most steps of a replicate, [1] flagged, [2] to replay, [3] a long round's slots did not fit
};
int verify_scratch(plspm_model* m, long nb, int slots, VerifyScratch& v) {
    int rc;
    v.capV = nb * slots;
    if ((rc = ensure(m, m->nmw_ints, nm_verify_ints(nb, slots) * sizeof(int)))) return rc;
    if ((rc = ensure(m, m->nmw_vsum, (size_t)v.capV * sizeof(double)))) return rc;
    int* ip = (int*)m->nmw_ints.p;
    v.steps = ip; ip += nb;
    v.force = ip; ip += nb;
    v.fixlist = ip; ip += nb;
    v.vb = ip; ip += v.capV;
    v.vj = ip; ip += v.capV;
    v.fb = ip; ip += v.capV;
    v.fj = ip; ip += v.capV;
    v.vneed = ip; ip += v.capV;
    v.cnt = ip;
    v.vsum = (double*)m->nmw_vsum.p;
    v.h = (int*)m->h_flag;
    m->last_nm_flagged = 0; m->last_nm_replayed = 0;
    return 0;
}
int verify_read(plspm_model* m) {        // the host reads what the round's kernels wrote to the pinned words
    HIPCHK(m, hipEventRecord(m->ev_flag, m->stream));
    HIPCHK(m, hipEventSynchronize(m->ev_flag));
    return 0;
}
// the replicates whose exact criterion was below the tolerance at a step they continued behind: listed for the replay with the reference's stop; *nreplay = how many
int verify_fix(plspm_model* m, const VerifyScratch& v, long nb, int* nreplay) {
    hipLaunchKernelGGL(nm_vfix_kernel, dim3(1), dim3(1024), 0, m->stream, (const int*)v.steps, (const int*)v.force, nb, v.fixlist, v.cnt + 2, v.h + 2);
    if (int rc = verify_read(m)) return rc;
    *nreplay = m->last_nm_replayed = v.h[2];
    return 0;
}

// ---- round 6: the whole batch in ONE solver launch + verification (kernels_nmw.h ONE; the categorical counterpart of run_nonmetric_wave) --------------------------------
// All-indicator, all-Mode-A models on the wave step with the int8 stop-rule product, not a stage of a HOC pair.  The solver iterates on its own upper bound and
// leaves every step's score map behind; the verification evaluates the criterion of every step a replicate continued behind on the row chunks that step asks for
// (a lower bound), the exact pass takes what that leaves open, a replicate whose exact criterion was below the tolerance is replayed with the reference's stop.
// (the first stage of a HOC pair too -- nothing to finish there: the final state is what the second stage's moments are composed from)
int nm_run_one_launch(NmRun& r) {
    plspm_model* m = r.m;
    const NmPlan& pl = r.pl;
    const int P = m->P, L = m->L, KS = pl.KS, nparts = pl.nparts;
    const long nproblems = r.nproblems, ntiles16 = pl.ntiles16;
    int rc;
    constexpr int JR = kCatVerifySlots;                  // steps verified per round (six to nine iterations is the rule: one round, one host read-back)
    const long capV = nproblems * JR, ng16V = (capV + 15) / 16;
    const long cstride = (long)(m->max_iter + 2) * P, kstride = (long)(m->max_iter + 2) * (L + 1);
    VerifyScratch v;
    if ((rc = ensure(m, m->nmw_maps, (size_t)nproblems * (cstride + kstride) * sizeof(double)))) return rc;
    if ((rc = verify_scratch(m, nproblems, JR, v))) return rc;
    if ((rc = ensure(m, m->tab8, (size_t)ng16V * L * 2 * nmp::S * KS * 64 * sizeof(uint4)))) return rc;
    if ((rc = ensure(m, m->scl8, (size_t)ng16V * L * 2 * 16 * sizeof(double2)))) return rc;
    double* cmaps = (double*)m->nmw_maps.p;
    double* kmaps = cmaps + nproblems * cstride;
    int* const h = v.h;
    const NmwStepFn one_kernel = nmw_step_of<true, true>(pl);
    auto pass_kernel = KS == 1 ? nmp::conv_mfma_kernel<4, 1> : nmp::conv_mfma_kernel<4, 2>;
    auto solve = [&](long count, const int* list, const int* forced) {
        ProfScope ps(m, PLSPM_K_SOLVER);
        nm_launch_start16(r, count, list);
        hipLaunchKernelGGL(one_kernel, dim3((unsigned)count), dim3(64), pl.wave_lds, m->stream, r.md, r.cd, r.mdm, r.so, r.gSm, r.gst, pl.st_doubles, (const double*)nullptr, nparts, r.nact,
                           (const unsigned short*)m->gK16.p, pl.ld16, r.fuse, list, pl.nsub, nmw::NmwMaps{forced ? nullptr : cmaps, cstride, forced ? nullptr : kmaps, kstride, v.steps, forced, std::ldexp(1.0, m->tune.nm_bound_shift)});
    };
    solve(nproblems, nullptr, nullptr);
    bool any_flagged = false;
    // (last session of round 6: behind the fourth round the replicates that are still iterating are the few that never converge -- 101 steps each, nine more rounds of four
    //  launches and a host read-back for a handful of slots -- so the fifth round takes JRB steps at once where their slots fit the buffers of a short round: the list
    //  kernel checks that itself and files nothing otherwise; option nm_vlong 0: short rounds only)
    constexpr int JRB = 72;
    bool long_ok = m->tune.nm_vlong != 0;
    for (int j0 = 1;;) {
        const bool long_round = long_ok && j0 > 4 * JR;
        const int jr = long_round ? JRB : JR;
        {
            ProfScope ps(m, PLSPM_K_SCORES);
            if (long_round)
                hipLaunchKernelGGL(nm_vlist_kernel<JRB>, dim3(1), dim3(1024), 0, m->stream, (const int*)v.steps, (long)nproblems, j0, v.vb, v.vj, v.cnt, v.vsum, v.force, h, (int)std::min<long>(capV, 0x7fffffffL));
            else
                hipLaunchKernelGGL(nm_vlist_kernel<JR>, dim3(1), dim3(1024), 0, m->stream, (const int*)v.steps, (long)nproblems, j0, v.vb, v.vj, v.cnt, v.vsum, v.force, h, 0);
            hipLaunchKernelGGL(nmp::planes_kernel, dim3((unsigned)(ng16V * 16)), dim3(64), 0, m->stream, (const double*)cmaps, cstride, P, L, KS, (const int*)m->d_boff, (const int*)v.vb,
                               (const int*)v.cnt, (uint4*)m->tab8.p, (double2*)m->scl8.p, (const int*)v.vj, (const double*)kmaps, kstride, v.vneed, m->tol, pl.nsub, nparts);
            hipLaunchKernelGGL(pass_kernel, dim3((unsigned)(nparts * ((ng16V + 3) / 4))), dim3(256), 0, m->stream, (const uint4*)m->ind8.p, ntiles16, L, (const unsigned*)r.cd8, (long)r.cd8_MT,
                               (const uint4*)m->tab8.p, (const double2*)m->scl8.p, (const int*)v.vb, (const int*)v.cnt, (double*)nullptr, nparts, pl.tpc, nparts, (const double*)nullptr, 0L,
                               (const int*)v.vneed, v.vsum, 1);
            hipLaunchKernelGGL(nm_vflag_kernel, dim3(1), dim3(1024), 0, m->stream, (const double*)v.vsum, (const int*)v.vb, (const int*)v.vj, (const int*)v.cnt, m->tol, v.fb, v.fj, v.cnt + 1, h + 1);
        }
        if ((rc = verify_read(m))) return rc;
        if (long_round && h[3] == 1) { long_ok = false; continue; }      // (too many slots: nothing was filed; the same steps again, eight at a time)
        const int most = h[0], flagged = h[1];
        if (flagged > 0) {
            ProfScope ps(m, PLSPM_K_SCORES);
            any_flagged = true;
            m->last_nm_flagged += flagged;
            const long ngf = ((long)flagged + 15) / 16;
            if ((rc = ensure(m, m->nmpartial, (size_t)std::max<long>(flagged, nproblems) * nparts * sizeof(double)))) return rc;
            hipLaunchKernelGGL(nmp::planes_kernel, dim3((unsigned)(ngf * 16)), dim3(64), 0, m->stream, (const double*)cmaps, cstride, P, L, KS, (const int*)m->d_boff, (const int*)v.fb,
                               (const int*)(v.cnt + 1), (uint4*)m->tab8.p, (double2*)m->scl8.p, (const int*)v.fj, (const double*)kmaps, kstride, (int*)nullptr, m->tol, 0, nparts);
            hipLaunchKernelGGL(pass_kernel, dim3((unsigned)(nparts * ((ngf + 3) / 4))), dim3(256), 0, m->stream, (const uint4*)m->ind8.p, ntiles16, L, (const unsigned*)r.cd8, (long)r.cd8_MT,
                               (const uint4*)m->tab8.p, (const double2*)m->scl8.p, (const int*)v.fb, (const int*)(v.cnt + 1), (double*)m->nmpartial.p, nparts, pl.tpc, nparts, (const double*)nullptr, 0L,
                               (const int*)nullptr, (double*)nullptr, 1);
            hipLaunchKernelGGL(nm_vcheck_kernel, dim3((unsigned)flagged), dim3(64), 0, m->stream, (const double*)m->nmpartial.p, nparts, (const int*)v.fb, (const int*)v.fj, (const int*)(v.cnt + 1),
                               m->tol, v.force);
        }
        if (j0 + jr > most - 1) break;
        j0 += jr;
    }
    int nreplay = 0;
    if (any_flagged && (rc = verify_fix(m, v, nproblems, &nreplay))) return rc;
    if (nreplay > 0) solve(nreplay, v.fixlist, v.force);
    HIPCHK(m, hipGetLastError());
    return 0;
}

// One launch-by-launch step of the problems of `live` (null: all of `lgrid`): the wave step (every step, the first one included, one wave per problem; the
// finish of a problem inside the launch that decides its stop), or the solver of the model's class (launch 0 = prepare + first step)
void nm_launch_step(const NmRun& r, int it, dim3 lgrid, const int* live, NmwStepFn wave_kernel) {
    plspm_model* m = r.m;
    const NmPlan& pl = r.pl;
    const int mode_op = it == 0 ? 0 : 1;
    ProfScope ps(m, PLSPM_K_SOLVER);
    if (pl.wave_step) {
        if (it == 0) nm_launch_start16(r, r.nproblems, nullptr);
        hipLaunchKernelGGL(wave_kernel, lgrid, dim3(64), pl.wave_lds, m->stream, r.md, r.cd, r.mdm, r.so, r.gSm, r.gst, pl.st_doubles, (const double*)r.part, pl.nparts, r.nact,
                           (const unsigned short*)m->gK16.p, pl.ld16, r.fuse, live, pl.nsub, nmw::NmwMaps{});
    } else if (r.cat) {
        auto k = mode_op == 0 ? nmg_kernel<0> : nmg_kernel<1>;
        hipLaunchKernelGGL(k, lgrid, dim3(r.threads), pl.lds, m->stream, r.md, r.cd, r.mdm, r.Mp, r.mp_stride, r.so, r.gS, r.gSm, r.gst, pl.st_doubles, (const double*)r.part, pl.nparts, r.nact, r.fuse,
                           pl.cat_fast, pl.k16 ? (unsigned short*)m->gK16.p : (unsigned short*)nullptr, pl.ld16, live);
    } else if (r.nmx) {
        auto k = mode_op == 0 ? nmx_kernel<0> : nmx_kernel<1>;
        const MissDesc xd{m->nmx_raw, m->nmx_K, m->d_Xk, m->d_Mk};
        hipLaunchKernelGGL(k, lgrid, dim3(r.threads), pl.lds, m->stream, r.md, xd, (const int*)m->d_rowid, r.Mp, r.mp_stride, r.so, r.gS, r.gst, pl.st_doubles, (const double*)r.part, pl.nparts,
                           r.nact, r.ent, r.nent, r.ent_stride, r.fuse, live);
    } else {
        auto k = mode_op == 0 ? nm_kernel<0> : nm_kernel<1>;
        hipLaunchKernelGGL(k, lgrid, dim3(r.threads), pl.lds, m->stream, r.md, r.Mp, r.mp_stride, r.so, r.gS, r.gst, (const double*)r.part, pl.nparts, r.nact, r.fuse, live);
    }
}

// The stop-rule pass behind a step: the criterion's partial sums of every live problem, as an int8 product, on category codes, dense, or gathering.  Enqueued
// BEFORE the host knows whether any problem is still active: finished problems / replicate groups return at once on the device.
int nm_stop_pass(NmRun& r, dim3 lgrid, const int* live) {
    plspm_model* m = r.m; plspm_model* src = r.src;
    const NmPlan& pl = r.pl;
    const int L = m->L, KS = pl.KS, nparts = pl.nparts;
    const long nproblems = r.nproblems, ntiles16 = pl.ntiles16;
    ProfScope ps(m, PLSPM_K_SCORES);
    const double* conv_state = r.gst;
    long conv_stride = pl.st_doubles;
    const int* conv_boff = m->d_boff;
    if (m->stage1) {
        hipLaunchKernelGGL(hoc_compose_kernel, lgrid, dim3(64), 0, m->stream, make_hoc_desc(m), (const double*)m->stage1->nmstate.p,
                           (long)nm_state_doubles_of(src), r.gst, pl.st_doubles, m->n_chol, (double*)m->pseudo.p, r.ps_stride, live);
        conv_state = (const double*)m->pseudo.p; conv_stride = r.ps_stride; conv_boff = m->d_lv_cols;
    }
    if (!pl.dense) {
        hipLaunchKernelGGL(nm_conv_kernel, dim3(nparts, (unsigned)nproblems), dim3(256), r.conv_lds, m->stream, src->d_Xa, (long)src->N, src->PA, src->P, L, 0, conv_boff, r.ent, r.nent,
                           r.ent_stride, conv_state, conv_stride, r.part);
        return 0;
    }
    int* live_list = (int*)m->nmlist.p;                            // [count | ids of the problems still iterating, in problem order]
    int* full_list = live_list + nproblems + 1;                    // [count | ids of the live problems that ask for the pass over all rows] (round 6)
    int* h_full = (int*)m->h_flag + 1;
    if (pl.sub_pass) *h_full = 0;
    hipLaunchKernelGGL(active_list_kernel, dim3(1), dim3(1024), 0, m->stream, conv_state, conv_stride, nproblems, live_list + 1, live_list,
                       pl.flag_from_list ? (int*)m->h_flag : (int*)nullptr, pl.sub_pass ? full_list + 1 : (int*)nullptr, pl.sub_pass ? full_list : (int*)nullptr,
                       (pl.sub_pass && pl.flag_from_list) ? h_full : (int*)nullptr);
    if (pl.flag_from_list) HIPCHK(m, hipEventRecord(m->ev_flag, m->stream));
    if (pl.use_mfma) {
        auto pass_kernel = KS == 1 ? nmp::conv_mfma_kernel<4, 1> : nmp::conv_mfma_kernel<4, 2>;
        auto product = [&](const int* list, long ng, const double* bound_state, long bound_stride) {      // digit planes of the listed problems' score maps x the indicator bytes
            hipLaunchKernelGGL(nmp::planes_kernel, dim3((unsigned)(ng * 16)), dim3(64), 0, m->stream, conv_state, conv_stride, src->P, L, KS, conv_boff, (const int*)(list + 1),
                               (const int*)list, (uint4*)m->tab8.p, (double2*)m->scl8.p, (const int*)nullptr, (const double*)nullptr, 0L, (int*)nullptr, 0.0, 0, 0);
            hipLaunchKernelGGL(pass_kernel, dim3((unsigned)(nparts * ((ng + 3) / 4))), dim3(256), 0, m->stream, (const uint4*)m->ind8.p, ntiles16, L, (const unsigned*)r.cd8,
                               (long)r.cd8_MT, (const uint4*)m->tab8.p, (const double2*)m->scl8.p, (const int*)(list + 1), (const int*)list, r.part, nparts, pl.tpc, nparts,
                               bound_state, bound_stride, (const int*)nullptr, (double*)nullptr, 0);
        };
        product(live_list, pl.ng16, pl.sub_pass ? conv_state : (const double*)nullptr, conv_stride);
        if (pl.sub_pass && pl.flag_from_list) {
            // the problems whose lower bound decided nothing (few, as a rule none): all row chunks, fixed-order sums -- the host knows their number
            // by now (the list kernel wrote it to pinned memory; the passes above run meanwhile)
            HIPCHK(m, hipEventSynchronize(m->ev_flag));
            const long nfull = *h_full;
            if (nfull > 0) {
                m->last_nm_exact += (int)nfull;
                product(full_list, (nfull + 15) / 16, nullptr, 0L);
            }
        }
        return 0;
    }
    hipLaunchKernelGGL(coef_table_kernel, dim3((unsigned)pl.ngroups, (unsigned)((pl.table_rows + 63) / 64)), dim3(256), 0, m->stream, conv_state, conv_stride, src->P, L,
                       (const int*)(live_list + 1), (const int*)live_list, (double*)m->ctable.p);
    const int gx = (int)((ntiles16 + 7) / 8);                      // row blocks of 128 rows (8 tiles: 8 x 16-row or 16 x 8-row waves)
    const int rbx = (gx + 7) / 8;                                  // row blocks per XCD
    // replicate slices: one group of 64 replicates per workgroup measured best (1.06 ms for three passes against 1.17 / 1.21 /
    // 1.28 with 12 / 6 / 13 slices): many small workgroups let the dispatcher balance the CUs
    const int gy = m->tune.conv_gy > 0 ? m->tune.conv_gy : pl.ngroups;
    const bool counts8 = pl.call.counts8;
    if (pl.use_codes)
        hipLaunchKernelGGL(nm_conv_codes_kernel<8>, dim3((unsigned)(8 * rbx * gy)), dim3(512), pl.codes_lds, m->stream, (const unsigned short*)m->codes.p, ntiles16, src->Pm, src->P, L,
                           conv_boff, r.codes_lmv, (const uint4*)r.cd8, (long)r.cd8_MT, (const double*)m->ctable.p, (const int*)(live_list + 1), (const int*)live_list, r.part, nparts, rbx, gy, pl.kb);
    else
        hipLaunchKernelGGL(nm_dense_kernel_of(pl, counts8), dim3((unsigned)(8 * rbx * gy)), dim3(512), pl.dense_lds, m->stream, (const double*)src->Xt.p, ntiles16, src->PA, src->P, L,
                           conv_boff, counts8 ? (const unsigned short*)r.cd8 : (const unsigned short*)src->dcnt.p, counts8 ? (long)r.cd8_MT : src->dcnt_stride,
                           (const double*)m->ctable.p, (const int*)(live_list + 1), (const int*)live_list, r.part, nparts, rbx, gy, pl.kb, 0);
    return 0;
}

// prepare -> (step, stop-rule pass)* -> finish.  The host only reads one counter per iteration (how many problems are still active).
int nm_run_steps(NmRun& r) {
    plspm_model* m = r.m;
    const NmPlan& pl = r.pl;
    const long nproblems = r.nproblems;
    const NmwStepFn wave_kernel = pl.sub_pass ? nmw_step_of<true, false>(pl) : nmw_step_of<false, false>(pl);
    // round 5 (second half): from the second step on, a launch of the dense route covers the problems that were still iterating after the previous step --
    // the list the previous stop-rule pass built and the count the host has just read -- instead of every problem of the batch: the late iterations of
    // a batch are a handful of stragglers (up to max_iter + 1 trips) among thousands of problems whose workgroups did nothing but find their flag cleared
    // (HOC on ordinal items: ~90 of ~100 trips per stage; 31 us per step launch, 79 us per compose launch at 5,000 problems)
    dim3 lgrid((unsigned)nproblems);
    const int* live = nullptr;
    // (round 6: a problem whose lower bound decided nothing sits one launch out while the pass over all rows runs for it -- at most once per step)
    for (int it = 0; it <= (pl.sub_pass ? 2 : 1) * (m->max_iter + 1); ++it) {
        if (it >= 1 && pl.dense && m->tune.nm_live != 0) {            // (*h_flag: the count behind the previous step == the length of the list its pass built)
            const long nlive = *m->h_flag;
            if (nlive >= 1 && nlive < nproblems) { lgrid = dim3((unsigned)nlive); live = (const int*)m->nmlist.p + 1; }
        }
        // (dense stop-rule pass: the list kernel of the pass counts the live problems anyway and writes the count to the pinned flag itself -- no
        //  counter to clear, no copy operation: two tiny launches and their gaps less per iteration, 35 of ~590 us at three iterations)
        if (!pl.flag_from_list) HIPCHK(m, hipMemsetAsync(r.nact, 0, sizeof(int), m->stream));
        nm_launch_step(r, it, lgrid, live, wave_kernel);
        // the 4-byte read-back of the counter overlaps with the pass instead of leaving the GPU idle for a host round trip per iteration
        if (!pl.flag_from_list) {
            HIPCHK(m, hipMemcpyAsync(m->h_flag, r.nact, sizeof(int), hipMemcpyDeviceToHost, m->stream));
            HIPCHK(m, hipEventRecord(m->ev_flag, m->stream));
        }
        if (int rc = nm_stop_pass(r, lgrid, live)) return rc;
        HIPCHK(m, hipEventSynchronize(m->ev_flag));
#ifdef PLSPM_DEBUG_MARKS
        if (r.cat && it == 1) {
            long long h[32];
            HIPCHK(m, hipStreamSynchronize(m->stream));
            HIPCHK(m, hipMemcpy(h, r.so.marks, sizeof(h), hipMemcpyDeviceToHost));
            fprintf(stderr, "[plspm nmg_step clocks] V=Mn.c %lld  YY+G %lld  inner weights %lld  MZ+a %lld  quantify(par) %lld  LV loop %lld  score map %lld  total %lld\n", h[21] - h[20],
                    h[22] - h[21], h[23] - h[22], h[24] - h[23], h[25] - h[24], h[26] - h[25], h[27] - h[26], h[27] - h[20]);
        }
#endif
        if (*m->h_flag == 0) break;
    }
    HIPCHK(m, hipGetLastError());
    return 0;
}

}  // namespace

int run_nonmetric(plspm_model* m, const NmPlan& pl, const NmInputs& in, const SolverOut& so_in) {
    if (pl.error == NM_PLAN_COUNTS8_WITHOUT_DENSE) return fail(m, PLSPM_E_STATE, "non-metric bootstrap: the dense stop-rule pass does not fit and no (row,count) lists were built");
    if (pl.error == NM_PLAN_COUNTS16_WITHOUT_WAVE) return fail(m, PLSPM_E_STATE, "non-metric solver: uint16 counts without the wave step");
    if (pl.error == NM_PLAN_WORKSPACE) return fail(m, PLSPM_E_LIMIT, "non-metric solver: workspace exceeds LDS");
    if (pl.call.counts8 != (in.cd8 != nullptr)) return fail(m, PLSPM_E_STATE, "non-metric solver: the plan and the call disagree about the int8 counts");
    NmRun r{m, m->stage1 ? m->stage1 : m, pl, pl.call.nproblems, in.Mp, in.mp_stride, so_in, in.ent, in.nent, in.ent_stride, in.threads, in.cd8, in.cd8_MT};
    r.cat = m->categorical != 0; r.nmx = m->nmx_K > 0;
    r.fuse = pl.call.finish ? 1 : 0;
    r.codes_base = m->stage1 ? m->d_mv_base2 : m->d_mv_base;
    r.codes_lmv = m->stage1 ? m->d_lmv2_off : m->d_lmv_off;
    if (int rc = nm_prepare(r)) return rc;
    r.md = make_desc(m);
    r.mdm = r.md;
    if (r.cat) {
        r.cd.Pm = m->Pm; r.cd.cmax = m->cmax; r.cd.kmv = m->kmv; r.cd.mv_off = m->d_mv_off; r.cd.mv_kind = m->d_mv_kind; r.cd.lmv_off = m->d_lmv_off;
        r.mdm.P = m->Pm; r.mdm.boff = m->d_lmv_off; r.mdm.lvof = m->d_mv_lv; r.mdm.chol_off = m->d_no_chol; r.mdm.n_chol = 0;      // shift: zeros (upload)
    }
#ifdef PLSPM_DEBUG_MARKS
    if (r.cat) HIPCHK(m, plspm_dmalloc((void**)&r.so.marks, 32 * sizeof(long long)));
#endif
    const int rc = pl.one_launch ? nm_run_one_launch(r) : nm_run_steps(r);
#ifdef PLSPM_DEBUG_MARKS
    if (r.cat) plspm_dfree(r.so.marks);
#endif
    return rc;
}

// Round 6: a bootstrap batch of a Scale.NUM / RAW model (no missing cells, at most 64 MVs and 16 LVs) on the int8 Gram route as ONE solver launch + a
// verification pass (kernels_solver.h solver_nmwave_kernel; kernels_nonmetric.h nm_vlist_kernel ...).  The legacy loop (run_nonmetric) launches one step
// kernel + one stop-rule pass over all rows per iteration, with a host round trip each: 0.435 ms of solver launches and 0.61 ms of passes per 5,000
// replicates of the headline's shape (profiles/r05_nonmetric_kernels.txt).  Here: 1 launch that iterates on the bound, then -- for the steps it continued
// behind -- an eighth of the rows (a lower bound of the criterion that only has to clear the tolerance), ONE host read-back, and the exact pass + replay for
// whatever the lower bound could not confirm (nothing, as a rule).  Dense moment matrices at m->gram; cd8 / cd8_MT: the int8 counts the Gram consumed.
int run_nonmetric_wave(plspm_model* m, const NmPlan& pl, const NmInputs& in, const SolverOut& so) {
    const void* const cd8 = in.cd8;
    const int cd8_MT = in.cd8_MT;
    const int P = m->P, L = m->L, W = P + L + 1;                 // a map: c_p | k_l | the bound of its step
    const long N = m->N, ntiles16 = pl.ntiles16, nb = pl.call.nproblems;
    int rc;
    if (!pl.dense_lds || !cd8) return fail(m, PLSPM_E_STATE, "non-metric wave route: no dense stop-rule pass / no int8 counts");
    constexpr int JR = kNumVerifySlots;                          // steps verified per round (three iterations -- two continued steps -- is the rule)
    const long maps_stride = (long)(m->max_iter + 2) * W;
    const int table_rows = pl.table_rows;
    VerifyScratch v;
    if ((rc = ensure(m, m->nmw_maps, (size_t)nb * maps_stride * sizeof(double)))) return rc;
    if ((rc = verify_scratch(m, nb, JR, v))) return rc;
    const long ngroupsV = (v.capV + 63) / 64;
    if ((rc = ensure(m, m->Xt, (size_t)ntiles16 * 16 * m->PA * sizeof(double)))) return rc;
    if ((rc = ensure(m, m->ctable, (size_t)ngroupsV * table_rows * 64 * sizeof(double)))) return rc;
    auto conv_kernel = nm_dense_kernel_of(pl, true);
    if ((rc = allow_lds(m, (const void*)conv_kernel, pl.dense_lds))) return rc;
    if (!m->Xt_valid) {
        hipLaunchKernelGGL(tile_transpose_kernel, dim3((unsigned)ntiles16), dim3(256), 0, m->stream, (const double*)m->d_Xa, N, m->PA, (double*)m->Xt.p);
        m->Xt_valid = true;
    }
    double* maps = (double*)m->nmw_maps.p;
    int* const h = v.h;
    m->last_nm_wave16 = 1; m->last_nm_problems = 0; m->last_nm_codes = 0; m->last_nm_mfma = 0; m->last_nm_wave = 0; m->last_nm_direct16 = 0;
    if ((rc = launch_nm_wave_solver(m, nb, so, maps, maps_stride, v.steps, nullptr, nullptr))) return rc;
    // the rows pass A looks at: per slot by the bound of its step (nm_vlist_kernel), at most the first eighth of the row blocks of 128 rows -- or, option
    // nm_verify_rows, that percentage for every slot
    const int nblocks_all = (int)((ntiles16 + 7) / 8);
    const int fixed_blocks = m->tune.nm_verify_rows > 0 ? (int)std::min<long>(nblocks_all, std::max<long>(1, ((long)nblocks_all * m->tune.nm_verify_rows + 99) / 100)) : 0;
    const int cap_blocks = fixed_blocks > 0 ? fixed_blocks : std::max(1, (nblocks_all + 7) / 8);
    const long nsub = std::min<long>(ntiles16, 8L * cap_blocks);
    const int gyV = (int)std::max<long>(1, (2 * nb + 63) / 64);
    const size_t verify_lds = ((size_t)table_rows * 64 + (size_t)8 * P * 16) * sizeof(double);
    if ((rc = allow_lds(m, (const void*)nm_verify_kernel, verify_lds))) return rc;
    bool any_flagged = false;
    for (int j0 = 1;; j0 += JR) {
        {
            ProfScope ps(m, PLSPM_K_SCORES);
            hipLaunchKernelGGL(nm_vlist_kernel<JR>, dim3(1), dim3(1024), 0, m->stream, (const int*)v.steps, nb, j0, v.vb, v.vj, v.cnt, v.vsum, v.force, h, 0);
            hipLaunchKernelGGL(nm_vtable_kernel, dim3((unsigned)ngroupsV, (unsigned)((table_rows + 63) / 64)), dim3(256), 0, m->stream, (const double*)maps, maps_stride, P, L, (const int*)v.vb,
                               (const int*)v.vj, (const int*)v.cnt, (double*)m->ctable.p, v.vneed, m->tol, nblocks_all, cap_blocks, fixed_blocks);
            hipLaunchKernelGGL(nm_verify_kernel, dim3((unsigned)(cap_blocks * gyV)), dim3(512), verify_lds, m->stream, (const double*)m->Xt.p, nsub, m->PA, P, L, (const int*)m->d_boff,
                               (const uint4*)cd8, (long)cd8_MT, (const double*)m->ctable.p, (const int*)v.vb, (const int*)v.cnt, (const int*)v.vneed, v.vsum, cap_blocks, gyV);
            hipLaunchKernelGGL(nm_vflag_kernel, dim3(1), dim3(1024), 0, m->stream, (const double*)v.vsum, (const int*)v.vb, (const int*)v.vj, (const int*)v.cnt, m->tol, v.fb, v.fj, v.cnt + 1, h + 1);
        }
        if ((rc = verify_read(m))) return rc;
        const int most = h[0], flagged = h[1];
        if (flagged > 0) {
            // the exact criterion of what the lower bound left open: all rows, fixed-order partial sums filed under the (virtual) slot; a value below the
            // tolerance moves that replicate's stop
            ProfScope ps(m, PLSPM_K_SCORES);
            any_flagged = true;
            m->last_nm_flagged += flagged;
            if ((rc = ensure(m, m->nmpartial, (size_t)flagged * ntiles16 * sizeof(double)))) return rc;
            hipLaunchKernelGGL(nm_vtable_kernel, dim3((unsigned)((flagged + 63) / 64), (unsigned)((table_rows + 63) / 64)), dim3(256), 0, m->stream, (const double*)maps, maps_stride, P, L,
                               (const int*)v.fb, (const int*)v.fj, (const int*)(v.cnt + 1), (double*)m->ctable.p, (int*)nullptr, m->tol, 0, 0, 0);
            const int gx = (int)((ntiles16 + 7) / 8), rbx = (gx + 7) / 8;
            hipLaunchKernelGGL(conv_kernel, dim3((unsigned)(8 * rbx * gyV)), dim3(512), pl.dense_lds, m->stream, (const double*)m->Xt.p, ntiles16, m->PA, P, L, (const int*)m->d_boff,
                               (const unsigned short*)cd8, (long)cd8_MT, (const double*)m->ctable.p, (const int*)v.fb, (const int*)(v.cnt + 1), (double*)m->nmpartial.p, (int)ntiles16, rbx, gyV, pl.kb, 1);
            hipLaunchKernelGGL(nm_vcheck_kernel, dim3((unsigned)flagged), dim3(64), 0, m->stream, (const double*)m->nmpartial.p, (int)ntiles16, (const int*)v.fb, (const int*)v.fj,
                               (const int*)(v.cnt + 1), m->tol, v.force);
        }
        if (j0 + JR > most - 1) break;                           // every step a replicate continued behind has been looked at
    }
    int nreplay = 0;
    if (any_flagged && (rc = verify_fix(m, v, nb, &nreplay))) return rc;
    if (nreplay > 0 && (rc = launch_nm_wave_solver(m, nreplay, so, nullptr, 0, nullptr, v.force, v.fixlist))) return rc;
    HIPCHK(m, hipGetLastError());
    return 0;
}

// include/plspm_hip_test.h
extern "C" int plspm_nonmetric_criteria(plspm_model_t* m, int64_t B, double* out) {
    if (!m || !out || B < 0) return PLSPM_E_ARG;
    const size_t st = nm_state_doubles_of(m);
    if (!m->nmstate.p || m->nmstate.cap < (size_t)B * st * sizeof(double) || !m->last_nm_problems || B > m->last_nm_problems) return fail(m, PLSPM_E_STATE, "plspm_nonmetric_criteria: no non-metric run of that many problems");
    hipSetDevice(m->device);
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy2D(out, sizeof(double), (const double*)m->nmstate.p + 4, st * sizeof(double), sizeof(double), (size_t)B, hipMemcpyDeviceToHost));
    return 0;
}
