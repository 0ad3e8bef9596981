// derived_route.h -- the records derived from a plain bootstrap's replicates (plspm_derived.hip): the stages as ONE table, and the plan of a call on it -- which stages
// run, each one's record pitch and launch geometry, the assessment's hand-over to PLSc, and which stage the LDS refuses.  Pure functions of what the handle fixes
// (DerivedShape), its switches and the number of problems.  Free of the HIP runtime: the CPU tests compile it (tests/hostemu).
#pragma once
#include <stddef.h>
#include <algorithm>
#include "geodesic_core.h"        // (and through it modelfit_core.h, plsc_core.h, solver_core.h: the wave workspaces)
#include "structural_core.h"
#include "solver_route.h"         // kMaxLds

namespace plspm {

// The stages, in the order of their launches on the stream: a stage reads records of stages before it only.
enum DerivedStage { STAGE_ASSESS, STAGE_STRUCTURAL, STAGE_PLSC, STAGE_MODELFIT, STAGE_GEODESIC, kDerivedStages };
constexpr int stage_bit(int s) { return 1 << s; }

// What the handle fixes.  R: the bootstrap record's width (plspm_row_width); n_dir / n_spec: the direct paths and specific indirect effects of the structural
// lists, zero while they are not built.
struct DerivedShape { int P, L, kmax, R, n_dir, n_spec; };

inline int assess_width(const DerivedShape& s) { return 4 * s.L + 3 * (s.L * (s.L - 1) / 2); }
inline int structural_width(const DerivedShape& s) { return 2 * s.n_dir + s.n_spec; }
inline int plsc_width(const DerivedShape& s) { return s.R + s.L * (s.L - 1) / 2; }
inline int modelfit_width(const DerivedShape&) { return MODELFIT_WIDTH; }
inline int geodesic_width(const DerivedShape&) { return GEODESIC_WIDTH; }
inline long assess_doubles(const DerivedShape& s) { return assess_wave_doubles(s.P, s.L); }
inline long structural_doubles(const DerivedShape& s) { return structural_ws_doubles(s.L, s.kmax, 0); }
inline long structural_slot(const DerivedShape& s) { return structural_slot_doubles(s.kmax); }
inline long plsc_doubles(const DerivedShape& s) { return plsc_ws_doubles(s.P, s.L, s.kmax); }
inline long modelfit_doubles(const DerivedShape& s) { return modelfit_ws_doubles(s.P, s.L); }
inline long geodesic_doubles(const DerivedShape& s) { return geodesic_ws_doubles(s.P, s.L); }

// One row per stage.  reads: the stages whose records its kernel reads -- they run whenever it does, and its records go when theirs go (model.h void_records).
// width: of a record, status and iterations behind it.  wave_doubles: one wave's LDS slice (the structural stage's without its regression slots, slot_doubles each).
// waves: per workgroup; min_waves below it: the kernel takes its workgroup's waves from the launch, which sizes the workgroup by the LDS.  plain_only: the entry
// points refuse any other handle kind behind their argument check (host_internal.h SideRecords).  api / noun / last: plspm_<api>_*, and the two words the
// messages of its entry points differ in ("no <noun> records", "the last <last> bootstrap").  title / lds_need: of a stage sized by the LDS, the refusal when one
// wave does not fit ("<title>: <lds_need>" from a batch call, "<entry point>: <lds_need>" from plspm_structural_enable); null for a stage of fixed waves.
struct DerivedStageRow {
    int reads;
    int (*width)(const DerivedShape&);
    long (*wave_doubles)(const DerivedShape&);
    long (*slot_doubles)(const DerivedShape&);
    int waves, min_waves;
    bool plain_only;
    const char *api, *noun, *last, *title, *lds_need;
};
constexpr DerivedStageRow kDerivedStage[kDerivedStages] = {
    {0, assess_width, assess_doubles, nullptr, 4, 4, false, "assess", "assessment", "assessed", nullptr, nullptr},
    {stage_bit(STAGE_ASSESS), structural_width, structural_doubles, structural_slot, 4, 1, true, "structural", "structural", "structural", "structural assessment",
     "rc and one regression slot of one replicate need more than 160 KiB of LDS"},
    {stage_bit(STAGE_ASSESS), plsc_width, plsc_doubles, nullptr, 4, 4, false, "plsc", "PLSc", "PLSc", nullptr, nullptr},
    {stage_bit(STAGE_PLSC), modelfit_width, modelfit_doubles, nullptr, 4, 4, true, "modelfit", "model-fit", "model-fit", nullptr, nullptr},
    {stage_bit(STAGE_MODELFIT) | stage_bit(STAGE_PLSC), geodesic_width, geodesic_doubles, nullptr, 4, 1, true, "geodesic", "geodesic", "geodesic", "geodesic discrepancy",
     "the two P x P triangles of one replicate need more than 160 KiB of LDS"},
};

// The stages that run when those of `enabled` are asked for: its closure over what they read (a row reads rows before it, so one descending sweep closes it).
constexpr int derived_closure(int enabled) {
    int runs = enabled & (stage_bit(kDerivedStages) - 1);
    for (int s = kDerivedStages - 1; s >= 0; --s)
        if (runs & stage_bit(s)) runs |= kDerivedStage[s].reads;
    return runs;
}

// One stage's launch: its records' pitch, `waves` waves of `wave_doubles` of LDS per workgroup, one wave per problem.
struct DerivedLaunch { int stride, waves; long wave_doubles; size_t lds; long grid; };
// The plan of `nb` problems.  runs: the stages that run, one bit each -- the value the batch driver carries through a call (zero: nothing to do).  stage[s]: set for
// the stages that run.  nslots: a structural wave's regression slots.  side_bytes: the assessment's hand-over to PLSc, [nb x 3 L] doubles, 0 unless PLSc runs.
// refused: -1, or the first stage in launch order of those sized by the LDS whose one wave needs more than 160 KiB (a stage of fixed waves is checked where it is
// launched: host_internal.h allow_lds).
struct DerivedPlan { int runs; DerivedLaunch stage[kDerivedStages]; int nslots; size_t side_bytes; int refused; };

inline DerivedPlan derived_plan(const DerivedShape& sh, int enabled, long nb) {
    DerivedPlan p{};
    p.runs = derived_closure(enabled); p.refused = -1;
    const long cap = (long)(kMaxLds / sizeof(double));
    for (int s = 0; s < kDerivedStages; ++s) {
        if (!(p.runs & stage_bit(s))) continue;
        const DerivedStageRow& row = kDerivedStage[s];
        DerivedLaunch& k = p.stage[s];
        long doubles = row.wave_doubles(sh);
        int waves = row.waves;
        if (row.slot_doubles) {
            // a slot per index in flight (LVs, then direct paths), 64 at the most, fewer where the LDS does not hold them beside four waves' share; half the
            // waves, and half again, where four slices with one slot each do not fit
            const long slot = std::max<long>(1, row.slot_doubles(sh)), want = std::max<long>(1, std::min<long>(64, std::max(sh.L, sh.n_dir)));
            long fit = 0;
            while (waves >= 1 && (fit = (cap / waves - doubles) / slot) < 1) waves >>= 1;
            if (!waves && p.refused < 0) p.refused = s;
            waves = std::max(waves, 1);
            p.nslots = (int)std::max<long>(1, std::min(want, fit));
            doubles += p.nslots * row.slot_doubles(sh);
        } else {
            waves = (int)std::max<long>(row.min_waves, std::min<long>(waves, cap / doubles));
            if (row.min_waves < row.waves && doubles > cap && p.refused < 0) p.refused = s;
        }
        k.stride = row.width(sh) + 2;
        k.waves = waves; k.wave_doubles = doubles;
        k.lds = (size_t)waves * doubles * sizeof(double);
        k.grid = (nb + waves - 1) / waves;
    }
    if (p.runs & stage_bit(STAGE_PLSC)) p.side_bytes = (size_t)nb * 3 * sh.L * sizeof(double);
    return p;
}

// The full-sample record of stage `target` (plspm_*_fit): the plan of one problem for the stages it takes, and where they write in the handle's block, in doubles:
// [the solver's record R + 2 | every running stage's record, in launch order | the hand-over 3 L, where PLSc runs | status, iterations (int)].  o_stage[s]: -1 for a
// stage that does not run.
struct DerivedFitLayout { DerivedPlan plan; long o_stage[kDerivedStages]; long o_side, o_ints; size_t bytes; };

inline DerivedFitLayout derived_fit_layout(const DerivedShape& sh, int target) {
    DerivedFitLayout f{};
    f.plan = derived_plan(sh, stage_bit(target), 1);
    long next = sh.R + 2;
    for (int s = 0; s < kDerivedStages; ++s) {
        f.o_stage[s] = (f.plan.runs & stage_bit(s)) ? next : -1;
        if (f.plan.runs & stage_bit(s)) next += f.plan.stage[s].stride;
    }
    f.o_side = next;
    f.o_ints = next + (long)(f.plan.side_bytes / sizeof(double));
    f.bytes = (size_t)f.o_ints * sizeof(double) + 2 * sizeof(int);
    return f;
}

}  // namespace plspm
