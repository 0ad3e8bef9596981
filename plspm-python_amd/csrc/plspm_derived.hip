// plspm_derived.hip -- host side, part 10: the records derived from a plain bootstrap's replicates.  Per-replicate kernels behind the metric solver, each stage
// reading the replicate's moment matrix, its bootstrap record and the records of the stages derived_route.h's table says it reads:
//     assessment (plspm_assess_*)  ->  consistent PLS (plspm_plsc_*, 5o)  ->  model fit (plspm_modelfit_*, 5p)  ->  geodesic discrepancy (plspm_geodesic_*, 5q)
//                                                \->  structural-model assessment (plspm_structural_*, 5r)
// derived_route.h decides -- derived_plan once per call and per pass: the stages that run (the enabled ones and what they read), each one's record pitch, waves,
// LDS and grid, what the LDS refuses --; this unit only carries it out.  The batch driver (plspm_bootstrap.hip) carries the set of running stages as one int
// through three calls -- derived_begin, derived_launch, derived_commit (host_internal.h) --; the full-sample records (plspm_*_fit) are the same launches on one
// problem, laid out by derived_fit_layout.  The handle keeps a stage's switch, records and count in m->derived[stage] (model.h).
// A further stage is a row of kDerivedStage, a launcher in kLaunch, and a block of entry points at the end.
// Kernels: kernels_assess.h, kernels_plsc.h, kernels_modelfit.h, kernels_geodesic.h (their shared opening: kernels_moments.h), kernels_structural.h.
#include "wave_launch.h"

#include "wave_ops.h"
#include "kernels_assess.h"
#include "kernels_plsc.h"
#include "kernels_modelfit.h"
#include "kernels_geodesic.h"
#include "kernels_structural.h"

static_assert(kDerivedStage[STAGE_ASSESS].waves == ASSESS_WAVES && kDerivedStage[STAGE_STRUCTURAL].waves == STRUCTURAL_WAVES && kDerivedStage[STAGE_PLSC].waves == PLSC_WAVES &&
                  kDerivedStage[STAGE_MODELFIT].waves == MODELFIT_WAVES && kDerivedStage[STAGE_GEODESIC].waves == GEODESIC_WAVES,
              "derived_route.h plans the workgroups the kernels are compiled for");

static const char kPlainOnly[] = ": plain metric models only (no non-metric scales, no missing values, not part of a two-stage pair)";

static DerivedShape derived_shape(const plspm_model* m) {
    const bool listed = m->structural_listed;
    return {m->P, m->L, m->kmax, plspm_row_width(m), listed ? (int)m->struct_dir_from.size() : 0, listed ? (int)m->struct_chain_off.size() - 1 : 0};
}
static int derived_enabled(const plspm_model* m) {
    int on = 0;
    for (int s = 0; s < kDerivedStages; ++s) on |= m->derived[s].on ? stage_bit(s) : 0;
    return on;
}
static int stage_width(const plspm_model* m, int s) { return m ? kDerivedStage[s].width(derived_shape(m)) : 0; }      // (plspm_*_width of no handle: 0)

// ---- the launchers: the problems of one ChainCall -- their moment matrices `mom` (dense, or tile-packed), their bootstrap records at `rows` (row_stride 0: one
// problem), stage s's records at out[s] [nb x (width + 2)], `side`: null, or [nb x 3 L] for the assessment's hand-over to PLSc.  One wave per problem, as `pl` has it.
struct ChainCall { long nb; bool dense; MomentLayout mom; const double* rows; long row_stride; double* out[kDerivedStages]; double* side; };
// one stage's launch as the plan has it; nclocks / print: its phase clocks (wave_launch.h)
template <class Args>
static int launch_stage(plspm_model* m, void (*k)(Args), Args& a, const DerivedLaunch& g, int nclocks, void (*print)(const long long*)) {
    return launch_wave_per_problem(m, k, a, g.waves, g.lds, g.grid, &a.marks, nclocks, print);
}

static void print_assess_clocks(const long long* h) {
    fprintf(stderr, "[plspm assess clocks] per-MV values %lld  diagonal blocks %lld  block pairs %lld  total %lld\n", h[1] - h[0], h[2] - h[1], h[3] - h[2], h[3] - h[0]);
}
static void print_plsc_clocks(const long long* h) {
    fprintf(stderr, "[plspm plsc clocks] per-MV values %lld  rc %lld  regressions and effects %lld  stores %lld  total %lld\n", h[9] - h[8], h[10] - h[9], h[11] - h[10], h[12] - h[11],
            h[12] - h[8]);
}
static void print_modelfit_clocks(const long long* h) {
    fprintf(stderr, "[plspm modelfit clocks] per-MV values %lld  implied construct correlations %lld  residual sweep %lld  stores %lld  total %lld\n", h[1] - h[0], h[2] - h[1],
            h[3] - h[2], h[4] - h[3], h[4] - h[0]);
}
static void print_structural_clocks(const long long* h) {
    fprintf(stderr, "[plspm structural clocks] rc and chain products %lld  R2 per LV %lld  drop-one solves %lld  status %lld  total %lld\n", h[1] - h[0], h[2] - h[1], h[3] - h[2], h[4] - h[3],
            h[4] - h[0]);
}
static void print_geodesic_clocks(const long long* h) {      // (reduction, tridiagonalisation and bisection: the saturated and the estimated model together)
    fprintf(stderr, "[plspm geodesic clocks] per-MV values and implied construct correlations %lld  Cholesky %lld  reduction %lld  tridiagonalisation %lld  bisection %lld  stores %lld  total %lld\n",
            h[1] - h[0], h[2] - h[1], (h[3] - h[2]) + (h[6] - h[5]), (h[4] - h[3]) + (h[7] - h[6]), (h[5] - h[4]) + (h[8] - h[7]), h[9] - h[8], h[9] - h[0]);
}

// -> out [nb x (A + 2)], and the hand-over where PLSc runs (kernels_assess.h)
static int launch_assess(plspm_model* m, const DerivedPlan& pl, const ChainCall& c) {
    AssessArgs a{};
    a.mom = c.mom;
    a.L = m->L; a.R = plspm_row_width(m);
    a.boff = m->d_boff; a.lvof = m->d_lvof; a.mode = m->d_mode;
    a.rows = c.rows; a.row_stride = c.row_stride; a.out = c.out[STAGE_ASSESS]; a.nb = c.nb; a.side = c.side;
    return launch_stage(m, c.dense ? assess_kernel<true> : assess_kernel<false>, a, pl.stage[STAGE_ASSESS], 4, print_assess_clocks);
}

// the assessment records -> out [nb x (S + 2)] (kernels_structural.h).  No moment matrix: one kernel for both layouts.  The kernel is told its workgroup's waves
// and a wave's regression slots.
static int launch_structural(plspm_model* m, const DerivedPlan& pl, const ChainCall& c) {
    StructuralArgs a{};
    a.R = plspm_row_width(m); a.A = stage_width(m, STAGE_ASSESS);
    a.md = make_desc(m);
    const int n_dir = (int)m->struct_dir_from.size(), n_spec = (int)m->struct_chain_off.size() - 1;
    const int* d = (const int*)m->structural_desc.p;
    a.sd = StructDesc{n_dir, n_spec, d, d + n_dir, d + 2 * n_dir, d + 2 * n_dir + n_spec + 1};
    a.waves = pl.stage[STAGE_STRUCTURAL].waves; a.nslots = pl.nslots;
    a.rows = c.rows; a.row_stride = c.row_stride; a.assess = c.out[STAGE_ASSESS]; a.out = c.out[STAGE_STRUCTURAL]; a.nb = c.nb;
    return launch_stage(m, structural_kernel, a, pl.stage[STAGE_STRUCTURAL], 8, print_structural_clocks);
}

// the assessment records and the hand-over -> out [nb x (W + 2)] (kernels_plsc.h)
static int launch_plsc(plspm_model* m, const DerivedPlan& pl, const ChainCall& c) {
    PlscArgs a{};
    a.mom = c.mom;
    a.R = plspm_row_width(m); a.A = stage_width(m, STAGE_ASSESS);
    a.md = make_desc(m);
    a.factor = (const unsigned char*)m->plsc_mask.p;
    a.rows = c.rows; a.row_stride = c.row_stride; a.assess = c.out[STAGE_ASSESS]; a.side = c.side; a.out = c.out[STAGE_PLSC]; a.nb = c.nb;
    return launch_stage(m, c.dense ? plsc_kernel<true> : plsc_kernel<false>, a, pl.stage[STAGE_PLSC], 16, print_plsc_clocks);
}

// the PLSc records -> out [nb x 6] (kernels_modelfit.h)
static int launch_modelfit(plspm_model* m, const DerivedPlan& pl, const ChainCall& c) {
    ModelfitArgs a{};
    a.mom = c.mom;
    a.R = plspm_row_width(m);
    a.md = make_desc(m);
    a.factor = (const unsigned char*)m->plsc_mask.p;
    a.rows = c.rows; a.row_stride = c.row_stride; a.plsc = c.out[STAGE_PLSC]; a.out = c.out[STAGE_MODELFIT]; a.nb = c.nb;
    return launch_stage(m, c.dense ? modelfit_kernel<true> : modelfit_kernel<false>, a, pl.stage[STAGE_MODELFIT], 8, print_modelfit_clocks);
}

// the PLSc and the model-fit records -> out [nb x 4] (kernels_geodesic.h).  The kernel reads its workgroup's waves from the launch.
static int launch_geodesic(plspm_model* m, const DerivedPlan& pl, const ChainCall& c) {
    GeodesicArgs a{};
    a.mom = c.mom;
    a.R = plspm_row_width(m);
    a.md = make_desc(m);
    a.factor = (const unsigned char*)m->plsc_mask.p;
    a.rows = c.rows; a.row_stride = c.row_stride; a.plsc = c.out[STAGE_PLSC]; a.modelfit = c.out[STAGE_MODELFIT]; a.out = c.out[STAGE_GEODESIC]; a.nb = c.nb;
    return launch_stage(m, c.dense ? geodesic_kernel<true> : geodesic_kernel<false>, a, pl.stage[STAGE_GEODESIC], 16, print_geodesic_clocks);
}

static int (*const kLaunch[kDerivedStages])(plspm_model*, const DerivedPlan&, const ChainCall&) = {launch_assess, launch_structural, launch_plsc, launch_modelfit, launch_geodesic};

// the running stages' launches, in the table's order
static int chain_launch(plspm_model* m, const DerivedPlan& pl, const ChainCall& c) {
    int rc = 0;
    for (int s = 0; s < kDerivedStages && !rc; ++s)
        if (pl.runs & stage_bit(s)) rc = kLaunch[s](m, pl, c);
    return rc;
}

// ---- the batch driver's three calls (host_internal.h)
int derived_begin(plspm_model* m, const BatchCall& call, int* runs) {
    *runs = 0;
    const bool own = !call.rows_out;
    const int on = derived_enabled(m);
    if (!on || !(own || call.chain_off >= 0) || !plain_metric(m) || call.kind != BatchCall::PLAIN || call.moments_out) return 0;
    const DerivedPlan pl = derived_plan(derived_shape(m), on, (long)call.B);
    if (pl.refused >= 0)      // (before anything of the call runs)
        return fail(m, PLSPM_E_LIMIT, std::string(kDerivedStage[pl.refused].title) + ": " + kDerivedStage[pl.refused].lds_need);
    for (int s = 0; own && s < kDerivedStages; ++s)
        if (pl.runs & stage_bit(s))
            if (int rc = ensure(m, m->derived[s].rows, (size_t)call.B * pl.stage[s].stride * sizeof(double))) return rc;
    *runs = pl.runs;
    return 0;
}

int derived_launch(plspm_model* m, int runs, long nb, int64_t pos, bool dense, const double* gram, const double* rows, long row_stride) {
    if (!runs) return 0;
    const DerivedPlan pl = derived_plan(derived_shape(m), runs, nb);
    if (int rc = ensure(m, m->plsc_side, pl.side_bytes)) return rc;      // (the assessment's hand-over lasts for one pass)
    ChainCall c{nb, dense, moment_layout(m, dense, gram), rows, row_stride, {}, pl.side_bytes ? (double*)m->plsc_side.p : nullptr};
    for (int s = 0; s < kDerivedStages; ++s)
        if (pl.runs & stage_bit(s)) c.out[s] = (double*)m->derived[s].rows.p + pos * pl.stage[s].stride;
    return chain_launch(m, pl, c);
}

void derived_commit(plspm_model* m, int runs, int64_t B) {
    for (int s = 0; s < kDerivedStages; ++s)
        if (runs & stage_bit(s)) m->derived[s].B = B;
}

// ---- the factor mask of PLSc and model fit
// the default factor mask: every Mode-A block of two items or more
static std::vector<uint8_t> plsc_default_mask(const plspm_model* m) {
    std::vector<uint8_t> f((size_t)m->L);
    for (int l = 0; l < m->L; ++l) f[l] = (m->mode[l] == PLSPM_MODE_A && m->boff[l + 1] - m->boff[l] >= 2) ? 1 : 0;
    return f;
}

// the mask the PLSc kernel reads: on the device, behind whatever the stream still runs with the mask before it
static int plsc_set_mask(plspm_model* m, const std::vector<uint8_t>& f) {
    HIPCHK(m, hipSetDevice(m->device));
    if (int rc = ensure(m, m->plsc_mask, (size_t)m->L)) return rc;
    HIPCHK(m, hipStreamSynchronize(m->stream));
    HIPCHK(m, hipMemcpy(m->plsc_mask.p, f.data(), (size_t)m->L, hipMemcpyHostToDevice));
    m->plsc_factor = f;
    return 0;
}

// the handle's one factor mask from an entry point's argument (plspm_plsc_enable, plspm_modelfit_enable, plspm_geodesic_enable): checked against what can be a factor, then set
static int plsc_take_mask(plspm_model* m, const uint8_t* factor, const std::string& who) {
    std::vector<uint8_t> f = plsc_default_mask(m);
    for (int l = 0; l < m->L; ++l) {
        if (factor[l] > 1) return fail(m, PLSPM_E_ARG, who + ": the factor mask holds 0 or 1 per latent variable");
        if (factor[l] && !f[l]) return fail(m, PLSPM_E_ARG, who + ": latent variable " + std::to_string(l) + " cannot be a common factor (Mode B, or a single item)");
        f[l] = factor[l];
    }
    return plsc_set_mask(m, f);
}

// ---- structural-model assessment: the lists
constexpr long kStructuralMaxChains = 4096;

// The direct paths (effect pairs with a path of their own, in pair order) and the chains (pair order, then lexicographic by node sequence) of the handle's path matrix,
// once per handle: on the host for plspm_structural_paths, on the device as structural_core.h StructDesc reads them.  The chains are counted first, by dynamic
// programming over the DAG (the LV order is a topological one: the path matrix is strictly lower triangular), and only enumerated when there are few enough.
static int structural_list(plspm_model* m, const std::string& who) {
    if (m->structural_listed) return 0;
    const int L = m->L;
    std::vector<int> eff_of((size_t)L * L, -1);
    for (int e = 0; e < m->n_eff; ++e) eff_of[(size_t)m->eff_to[e] * L + m->eff_from[e]] = e;
    const double kSat = 1e15;                                      // (counts saturate far above the cap and far below where a double stops counting)
    double n_spec = 0.0;
    std::vector<double> paths((size_t)L);
    for (int f = 0; f < L; ++f) {                                  // paths[t]: directed paths f -> ... -> t
        std::fill(paths.begin(), paths.end(), 0.0);
        for (int t = f + 1; t < L; ++t) {
            double s = 0.0;
            for (int r = m->pred_off[t]; r < m->pred_off[t + 1]; ++r) s += m->pred_idx[r] == f ? 1.0 : paths[m->pred_idx[r]];
            paths[t] = std::min(s, kSat);
            n_spec = std::min(n_spec + paths[t] - (m->C[(size_t)t * L + f] ? 1.0 : 0.0), kSat);
        }
    }
    if (n_spec > (double)kStructuralMaxChains)
        return fail(m, PLSPM_E_LIMIT, who + ": the path model has " + (n_spec >= kSat ? std::string("more than 10^15") : std::to_string((long long)n_spec)) +
                                          " specific indirect effects, more than the " + std::to_string(kStructuralMaxChains) + " a record holds");
    std::vector<int> dir_from, dir_to, chain_off{0}, nodes, chain_eff;
    std::vector<std::vector<int>> by_target((size_t)L);            // the chains from one f, per target: node sequences back to back, each lexicographic as the walk finds them
    std::vector<int> walk;
    for (int f = 0; f < L; ++f) {
        for (auto& v : by_target) v.clear();
        walk.assign(1, f);
        std::vector<int> next(1, 0);                               // depth-first over the successors in ascending order: next[d] = position in the successor list of walk[d]
        while (!walk.empty()) {
            const int u = walk.back(), d = (int)walk.size() - 1;
            if (next[d] < m->succ_off[u + 1] - m->succ_off[u]) {
                const int s = m->succ_idx[m->succ_off[u] + next[d]++];
                walk.push_back(s); next.push_back(0);
                if (walk.size() >= 3) { auto& v = by_target[s]; v.push_back((int)walk.size()); v.insert(v.end(), walk.begin(), walk.end()); }
            } else { walk.pop_back(); next.pop_back(); }
        }
        for (int t = 0; t < L; ++t) {
            if (f != t && m->C[(size_t)t * L + f]) { dir_from.push_back(f); dir_to.push_back(t); }
            const auto& v = by_target[t];
            for (size_t p = 0; p < v.size(); p += (size_t)v[p] + 1) {
                const int len = v[p];
                for (int r = 0; r < len; ++r) {
                    nodes.push_back(v[p + 1 + r]);
                    chain_eff.push_back(r + 1 < len ? eff_of[(size_t)v[p + 2 + r] * L + v[p + 1 + r]] : 0);
                }
                chain_off.push_back((int)nodes.size());
            }
        }
    }
    if ((double)(chain_off.size() - 1) != n_spec) return fail(m, PLSPM_E_STATE, who + ": the chain count and the enumeration disagree");
    std::vector<int> blob(dir_from);
    blob.insert(blob.end(), dir_to.begin(), dir_to.end());
    blob.insert(blob.end(), chain_off.begin(), chain_off.end());
    blob.insert(blob.end(), chain_eff.begin(), chain_eff.end());
    HIPCHK(m, hipSetDevice(m->device));
    if (int rc = ensure(m, m->structural_desc, std::max<size_t>(blob.size(), 1) * sizeof(int))) return rc;
    HIPCHK(m, hipMemcpy(m->structural_desc.p, blob.data(), blob.size() * sizeof(int), hipMemcpyHostToDevice));
    m->struct_dir_from = dir_from; m->struct_dir_to = dir_to; m->struct_chain_off = chain_off; m->struct_chain_nodes = nodes;
    m->structural_listed = true;
    if (derived_plan(derived_shape(m), stage_bit(STAGE_STRUCTURAL), 1).refused == STAGE_STRUCTURAL) {
        m->structural_listed = false;
        return fail(m, PLSPM_E_LIMIT, who + ": " + kDerivedStage[STAGE_STRUCTURAL].lds_need);
    }
    return 0;
}

// ---- what the entry points of every stage share
// The full-sample record of stage `target` (plspm_*_fit): the launches of a replicate, for the stages `target` takes, on the moments of all uploaded rows and
// plspm_fit's solver problem; where PLSc runs, with the handle's mask (the default mask if none was ever set).  h: that stage's record [width + 2].
static int chain_full_sample(plspm_model* m, int target, std::vector<double>& h, const std::string& who) {
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, who + kPlainOnly);
    int rc;
    if (target == STAGE_STRUCTURAL && (rc = structural_list(m, who))) return rc;
    if (!m->d_Xa || m->N < 2) return fail(m, PLSPM_E_STATE, who + ": no data uploaded");
    HIPCHK(m, hipSetDevice(m->device));
    const DerivedFitLayout lay = derived_fit_layout(derived_shape(m), target);
    if ((lay.plan.runs & stage_bit(STAGE_PLSC)) && m->plsc_factor.empty() && (rc = plsc_set_mask(m, plsc_default_mask(m)))) return rc;
    if ((rc = ensure(m, m->derived_fit, lay.bytes))) return rc;
    double* const rec = (double*)m->derived_fit.p;
    ChainCall c{1, false, {}, rec, 0, {}, lay.plan.side_bytes ? rec + lay.o_side : nullptr};
    for (int s = 0; s < kDerivedStages; ++s)
        if (lay.o_stage[s] >= 0) c.out[s] = rec + lay.o_stage[s];
    if ((rc = solve_full_sample(m, rec, (int*)(rec + lay.o_ints)))) return rc;      // (its moments: tile-packed, in m->gram)
    c.mom = moment_layout(m, false, (const double*)m->gram.p);
    if ((rc = chain_launch(m, lay.plan, c))) return rc;
    HIPCHK(m, hipGetLastError());
    h.resize((size_t)lay.plan.stage[target].stride);
    HIPCHK(m, hipMemcpyAsync(h.data(), c.out[target], h.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    return 0;
}

// a stage's records as the side-record functions take them (host_internal.h SideRecords), its four messages from the table's two words
static SideRecords stage_records(const plspm_model* m, int s) {
    static const std::vector<std::string> msg = [] {
        std::vector<std::string> v;
        for (const DerivedStageRow& r : kDerivedStage) {
            const std::string noun = r.noun, last = r.last;
            v.push_back(": no " + noun + " records on this handle (plspm_" + r.api + "_enable, then a plain bootstrap; an upload or a later call replaced them)");
            v.push_back(": B differs from the last " + last + " bootstrap on this handle");
            v.push_back(": range exceeds the last " + last + " bootstrap's replicates");
            v.push_back(": method must be 0 (percentile), 1 (basic) or 2 (bc); the jackknife writes no " + noun + " records, so there is no bca");
        }
        return v;
    }();
    const plspm_model::DerivedRecords& d = m->derived[s];
    return {d.rows, d.B, stage_width(m, s), kDerivedStage[s].plain_only, msg[4 * s].c_str(), msg[4 * s + 1].c_str(), msg[4 * s + 2].c_str(), msg[4 * s + 3].c_str()};
}

// plspm_*_enable: the handle check, the off switch and the plain-metric refusal they share; `prepare`: what the stage needs on the handle before it is switched on
static int stage_enable(plspm_model* m, int s, int32_t on, const std::string& who, int (*prepare)(plspm_model*, const uint8_t*, const std::string&) = nullptr,
                        const uint8_t* factor = nullptr) {
    if (!m) return fail(m, PLSPM_E_ARG, who + ": no handle");
    if (!on) { m->derived[s].on = false; return 0; }
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, who + kPlainOnly);
    if (prepare) { if (int rc = prepare(m, factor, who)) return rc; }
    m->derived[s].on = true;
    return 0;
}
// plspm_plsc_enable: the handle's one factor mask is set whenever the stage is switched on (NULL: the default mask)
static int mask_set(plspm_model* m, const uint8_t* factor, const std::string& who) { return factor ? plsc_take_mask(m, factor, who) : plsc_set_mask(m, plsc_default_mask(m)); }
// plspm_modelfit_enable, plspm_geodesic_enable: NULL keeps the handle's mask
static int mask_keep(plspm_model* m, const uint8_t* factor, const std::string& who) {
    if (factor) return plsc_take_mask(m, factor, who);
    return m->plsc_factor.empty() ? plsc_set_mask(m, plsc_default_mask(m)) : 0;
}
static int lists_built(plspm_model* m, const uint8_t*, const std::string& who) { return structural_list(m, who); }

// (the status word of a record is an integer status as a double in every stage -- the solver's, or the stage's own --, never NaN; the guard keeps the cast defined
//  whatever a kernel may come to write)
static int stage_fit(plspm_model* m, int s, double* out, int32_t* status, const char* who) {
    if (!m || !out) return fail(m, PLSPM_E_ARG, std::string(who) + ": bad arguments");
    std::vector<double> h;
    if (int rc = chain_full_sample(m, s, h, who)) return rc;
    const size_t W = h.size() - 2;
    std::copy(h.begin(), h.begin() + W, out);
    if (status) *status = (h[W] == h[W]) ? (int32_t)h[W] : -1;
    return 0;
}
static int stage_fetch(plspm_model* m, int s, int64_t first, int64_t count, double* out, int32_t* status, const char* who) {
    return m ? side_fetch(m, stage_records(m, s), first, count, out, status, who) : fail(m, PLSPM_E_ARG, std::string(who) + ": bad arguments");
}
static int stage_summary(plspm_model* m, int s, int64_t B, const double* original, double* summary, int64_t* n_used, const char* who) {
    return m ? side_summary(m, stage_records(m, s), B, original, summary, n_used, who) : fail(m, PLSPM_E_ARG, std::string(who) + ": bad arguments (1 <= B <= 2^30)");
}
static int stage_intervals(plspm_model* m, int s, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used, const char* who) {
    return m ? side_intervals(m, stage_records(m, s), B, original, method, level, out, n_used, who) : fail(m, PLSPM_E_ARG, std::string(who) + ": bad arguments (1 <= B <= 2^30)");
}

extern "C" {

// ---- measurement-model assessment: per-replicate records [alpha | rho_a | rho_c | ave | htmt | htmt2 | lv_cor | status | iterations]
int plspm_assess_enable(plspm_model_t* m, int32_t on) { return stage_enable(m, STAGE_ASSESS, on, "plspm_assess_enable"); }
int32_t plspm_assess_width(const plspm_model_t* m) { return stage_width(m, STAGE_ASSESS); }
int plspm_assess_fit(plspm_model_t* m, double* out, int32_t* status) { return stage_fit(m, STAGE_ASSESS, out, status, "plspm_assess_fit"); }
int plspm_assess_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) { return stage_fetch(m, STAGE_ASSESS, first, count, out, status, "plspm_assess_fetch"); }
int plspm_assess_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) { return stage_summary(m, STAGE_ASSESS, B, original, summary, n_used, "plspm_assess_summary"); }
int plspm_assess_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return stage_intervals(m, STAGE_ASSESS, B, original, method, level, out, n_used, "plspm_assess_intervals");
}

// ---- consistent PLS: per-replicate records [weights | r2 | total | direct | loadings | lv_cor_c | status | iterations]
int plspm_plsc_enable(plspm_model_t* m, int32_t on, const uint8_t* factor) { return stage_enable(m, STAGE_PLSC, on, "plspm_plsc_enable", mask_set, factor); }
int32_t plspm_plsc_width(const plspm_model_t* m) { return stage_width(m, STAGE_PLSC); }
int plspm_plsc_fit(plspm_model_t* m, double* out, int32_t* status) { return stage_fit(m, STAGE_PLSC, out, status, "plspm_plsc_fit"); }
int plspm_plsc_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) { return stage_fetch(m, STAGE_PLSC, first, count, out, status, "plspm_plsc_fetch"); }
int plspm_plsc_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) { return stage_summary(m, STAGE_PLSC, B, original, summary, n_used, "plspm_plsc_summary"); }
int plspm_plsc_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return stage_intervals(m, STAGE_PLSC, B, original, method, level, out, n_used, "plspm_plsc_intervals");
}

// ---- model fit: per-replicate records [srmr_sat | d_uls_sat | srmr_est | d_uls_est | status | iterations]
int plspm_modelfit_enable(plspm_model_t* m, int32_t on, const uint8_t* factor) { return stage_enable(m, STAGE_MODELFIT, on, "plspm_modelfit_enable", mask_keep, factor); }
int32_t plspm_modelfit_width(const plspm_model_t* m) { return stage_width(m, STAGE_MODELFIT); }
int plspm_modelfit_fit(plspm_model_t* m, double* out, int32_t* status) { return stage_fit(m, STAGE_MODELFIT, out, status, "plspm_modelfit_fit"); }
int plspm_modelfit_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) { return stage_fetch(m, STAGE_MODELFIT, first, count, out, status, "plspm_modelfit_fetch"); }
int plspm_modelfit_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) { return stage_summary(m, STAGE_MODELFIT, B, original, summary, n_used, "plspm_modelfit_summary"); }
int plspm_modelfit_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return stage_intervals(m, STAGE_MODELFIT, B, original, method, level, out, n_used, "plspm_modelfit_intervals");
}

// ---- geodesic discrepancy: per-replicate records [d_g_sat | d_g_est | status | iterations]
int plspm_geodesic_enable(plspm_model_t* m, int32_t on, const uint8_t* factor) { return stage_enable(m, STAGE_GEODESIC, on, "plspm_geodesic_enable", mask_keep, factor); }
int32_t plspm_geodesic_width(const plspm_model_t* m) { return stage_width(m, STAGE_GEODESIC); }
int plspm_geodesic_fit(plspm_model_t* m, double* out, int32_t* status) { return stage_fit(m, STAGE_GEODESIC, out, status, "plspm_geodesic_fit"); }
int plspm_geodesic_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) { return stage_fetch(m, STAGE_GEODESIC, first, count, out, status, "plspm_geodesic_fetch"); }
int plspm_geodesic_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) { return stage_summary(m, STAGE_GEODESIC, B, original, summary, n_used, "plspm_geodesic_summary"); }
int plspm_geodesic_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return stage_intervals(m, STAGE_GEODESIC, B, original, method, level, out, n_used, "plspm_geodesic_intervals");
}

// ---- structural-model assessment: per-replicate records [f2 | vif | specific | status | iterations]
int plspm_structural_enable(plspm_model_t* m, int32_t on) { return stage_enable(m, STAGE_STRUCTURAL, on, "plspm_structural_enable", lists_built); }
int32_t plspm_structural_width(const plspm_model_t* m) { return stage_width(m, STAGE_STRUCTURAL); }
int plspm_structural_fit(plspm_model_t* m, double* out, int32_t* status) { return stage_fit(m, STAGE_STRUCTURAL, out, status, "plspm_structural_fit"); }
int plspm_structural_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status) { return stage_fetch(m, STAGE_STRUCTURAL, first, count, out, status, "plspm_structural_fetch"); }
int plspm_structural_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used) { return stage_summary(m, STAGE_STRUCTURAL, B, original, summary, n_used, "plspm_structural_summary"); }
int plspm_structural_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used) {
    return stage_intervals(m, STAGE_STRUCTURAL, B, original, method, level, out, n_used, "plspm_structural_intervals");
}

int plspm_structural_paths(plspm_model_t* m, int32_t* n_dir, int32_t* dir_from, int32_t* dir_to, int32_t* n_spec, int32_t* chain_off, int32_t* chain_nodes) {
    if (!m) return fail(m, PLSPM_E_ARG, "plspm_structural_paths: no handle");
    if (!plain_metric(m)) return fail(m, PLSPM_E_ARG, std::string("plspm_structural_paths") + kPlainOnly);
    if (int rc = structural_list(m, "plspm_structural_paths")) return rc;
    if (n_dir) *n_dir = (int32_t)m->struct_dir_from.size();
    if (n_spec) *n_spec = (int32_t)m->struct_chain_off.size() - 1;
    if (dir_from) std::copy(m->struct_dir_from.begin(), m->struct_dir_from.end(), dir_from);
    if (dir_to) std::copy(m->struct_dir_to.begin(), m->struct_dir_to.end(), dir_to);
    if (chain_off) std::copy(m->struct_chain_off.begin(), m->struct_chain_off.end(), chain_off);
    if (chain_nodes) std::copy(m->struct_chain_nodes.begin(), m->struct_chain_nodes.end(), chain_nodes);
    return 0;
}

}  // extern "C"
