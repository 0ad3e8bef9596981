// options.h -- the integer options of a handle (plspm_model_set_option / plspm_model_get_option): their defaults (Tune), and ONE table that says for every option
// where it is kept, which values it takes, which of them exist in the experiments build only (make -C plspm-python_amd/csrc experiments) and what a change of it
// voids.  Adding an option is one field of Tune and one row of kOptions.  The read-only names (last_*, boot_round_units, build_experiments) need the handle and
// live in plspm_hip.hip.  Free of the HIP runtime: the CPU tests compile it (tests/hostemu).
#pragma once
#include <string.h>
#include "group_route.h"

namespace plspm {

// Validated by option_set, never read from the environment.
struct Tune {
    int wide_nw = 4;
    int fit_chunks = 0;
    int conv_pass = 0;
    int conv_gy = 0;
    int nm_threads = 0;
    int solver_threads = 128;
    int scores_tile = 0;
    int gram_lds_kb = 0;
    int gram_path = 0;           // 0 automatic | 1 fp64 MFMA on (row,count) lists | 2 int8 digit planes (batch_route.h choose_gram_path)
    int i8_slices = 0;           // digit planes of the int8 Gram (0: the automatic count)
    int i8_min_batch = 1;        // batches of this many replicates and more take the int8 route
    int i8_waves = 8;
    int i8_rt = 0;
    int i8_short = -1;           // option "i8_short_rows"
    int i8_cus = 0;
    int upload_direct = 0;       // 1: uploads beyond 64 MB leave through the runtime's own pageable path (plspm_upload)
    int i8_dma = 0;
    int i8_variant = -1;
    int solver_rows = 1;
    int solver_wave = 1;
    int solver_quad = 1;
    int nm_counts8 = 1;          // 0: the non-metric stop rule keeps the (row,count) lists (A/B; batch_route.h nm_counts8_possible)
    int nm_fast_lds = 1;
    int nm_k16 = 1;
    int nm_codes = 1;
    int i8_ind = 1;
    int i8_shape = 16;
    int resample_aux = 0;        // 1..3: the int8 counts are drawn on a second stream (1 lowest / 2 default / 3 highest priority; model.h)
    int i8_sched = 0;            // 1: the persistent ("stream-K") int8 Gram
    int i8_priv = 1;
    int boot_chunks = 0;         // sub-batches of plspm_bootstrap (0: automatic; plspm_detail_chunk_plan)
    int boot_ratio = 60;         // ... their sizes' ratio in percent
    int boot_align = 0;          // ... their alignment in replicates (0: whole rounds of the device)
    int i8_persist = 0;
    int i8_min_slices = 0;
    int i8_nostore = 0;
    int nm_wave = 1;
    int nm_live = 1;
    int nm_mfma = 1;
    int nm_direct16 = 1;
    int i8_nibbles = 1;
    int nm_wave16 = 1;           // 0: Scale.NUM / RAW batches on the per-iteration launches of rounds 1-5
    int nm_verify_rows = 0;      // percent of the rows the lower-bound pass reads (0: an eighth)
    int nm_bound_shift = 0;      // test seam: the solver's stop bound times 2^value (solver_wave16.h NmWaveIo)
    int wide_ring = 4;           // row buffers of the dense wide Gram's ring (0: two-stage ping-pong)
    int nm_subset = 4;           // categorical wave step: 0 every stop-rule pass over all rows (rounds 1-5) | n >= 1: the step stops on its own upper bound and its pass reads n tol / bound of the rows (lower bound)
    int nm_cat_one = 1;          // 0: the categorical wave step launch by launch (round 5 / the bound + row-subset form of round 6)
    int nm_cpl = 0;              // categorical wave step: 0 automatic (six aug columns per lane where they cover the model) | 8 eight per lane (round 5) | 6 six wherever the layout allows (probes: plspm_nonmetric.hip `cpl6`)
    int nm_c10 = 1;              // categorical wave step, items of nine / ten categories: 1 the ten-category instantiation (two waves per SIMD) | 0 the sixteen-category one
    int nm_vlong = 1;            // one-launch categorical batch, verification: 1 one long round for the stragglers behind the fourth short one
    int strat_rows = 0;
    int boot_pass = 0;           // test seam: cap on the replicates per pass (plspm_detail_bootstrap)
    int rebus_classes = 0;       // test seam: cap on the classes per LDS load of rebus_residual_kernel (0: as many as fit; rebus_route.h)
};

// The values an option takes: an integer in [v0, v1]; one of v0 .. v3; 0 or an integer in [v0, v1]; a multiple of 256 up to 2^30.
struct OptionValues { enum Kind { RANGE, ONE_OF, ZERO_OR_RANGE, PASS_CAP } kind; int v[4]; };
constexpr OptionValues in_range(int lo, int hi) { return {OptionValues::RANGE, {lo, hi, 0, 0}}; }
constexpr OptionValues one_of(int a, int b) { return {OptionValues::ONE_OF, {a, b, b, b}}; }
constexpr OptionValues one_of(int a, int b, int c) { return {OptionValues::ONE_OF, {a, b, c, c}}; }
constexpr OptionValues one_of(int a, int b, int c, int d) { return {OptionValues::ONE_OF, {a, b, c, d}}; }
constexpr OptionValues zero_or_range(int lo, int hi) { return {OptionValues::ZERO_OR_RANGE, {lo, hi, 0, 0}}; }
constexpr OptionValues pass_cap() { return {OptionValues::PASS_CAP, {0, 0, 0, 0}}; }
constexpr OptionValues kOnOff = in_range(0, 1);
// ... and which of them name a measured-neutral / slower kernel variant or a timing probe of the experiments build: none, every value but one, or one value.
struct OptionExperiments { enum Kind { NONE, ALL_BUT, ONLY } kind; int value; };
constexpr OptionExperiments kEverywhere = {OptionExperiments::NONE, 0};
constexpr OptionExperiments all_but(int v) { return {OptionExperiments::ALL_BUT, v}; }
constexpr OptionExperiments only(int v) { return {OptionExperiments::ONLY, v}; }
// What a CHANGE of the value voids on the handle (bits): the digit planes of the int8 Gram (zs_valid); their column statistics as well (zs_stats_ready).
enum OptionEffect : unsigned { OPTION_VOIDS_NOTHING = 0, OPTION_VOIDS_PLANES = 1, OPTION_VOIDS_STATS = 2, OPTION_VOIDS_PLANES_AND_STATS = 3 };

struct OptionRow { const char* name; int Tune::*field; OptionValues values; OptionExperiments experiments = kEverywhere; OptionEffect voids = OPTION_VOIDS_NOTHING; };
static constexpr OptionRow kOptions[] = {
    {"solver_threads", &Tune::solver_threads, one_of(64, 128, 256)},
    {"nm_threads", &Tune::nm_threads, one_of(0, 64, 128, 256)},
    {"fit_chunks", &Tune::fit_chunks, in_range(0, 65535)},
    {"wide_ring", &Tune::wide_ring, one_of(0, 4, 6)},
    {"wide_nw", &Tune::wide_nw, one_of(4, 8, 16)},
    {"conv_pass", &Tune::conv_pass, in_range(0, 2)},
    {"conv_gy", &Tune::conv_gy, in_range(0, 65535)},
    {"scores_tile", &Tune::scores_tile, one_of(0, 16, 32)},
    {"gram_lds_kb", &Tune::gram_lds_kb, in_range(0, 160)},
    {"gram_path", &Tune::gram_path, in_range(0, 2)},
    {"upload_direct", &Tune::upload_direct, kOnOff},
    {"solver_rows", &Tune::solver_rows, kOnOff},
    {"solver_wave", &Tune::solver_wave, in_range(0, 3)},
    {"solver_quad", &Tune::solver_quad, kOnOff},
    {"strat_rows", &Tune::strat_rows, in_range(0, 2)},
    // the int8 Gram of bootstrap batches
    {"i8_slices", &Tune::i8_slices, in_range(0, 8), kEverywhere, OPTION_VOIDS_PLANES},
    {"i8_min_slices", &Tune::i8_min_slices, zero_or_range(6, 8), kEverywhere, OPTION_VOIDS_PLANES_AND_STATS},
    {"i8_min_batch", &Tune::i8_min_batch, in_range(1, 0x7fffffff)},
    {"i8_ind", &Tune::i8_ind, kOnOff, kEverywhere, OPTION_VOIDS_PLANES},
    {"i8_shape", &Tune::i8_shape, one_of(16, 32), all_but(16), OPTION_VOIDS_PLANES},
    {"i8_waves", &Tune::i8_waves, one_of(4, 8), all_but(8)},
    {"i8_rt", &Tune::i8_rt, one_of(0, 16, 8, 20), only(8)},
    {"i8_short_rows", &Tune::i8_short, in_range(-1, 4096)},
    {"i8_cus", &Tune::i8_cus, zero_or_range(8, 4096)},
    {"i8_dma", &Tune::i8_dma, in_range(0, 2)},
    {"i8_nibbles", &Tune::i8_nibbles, in_range(0, 2)},
    {"i8_priv", &Tune::i8_priv, kOnOff},
    {"i8_persist", &Tune::i8_persist, kOnOff},
    {"i8_sched", &Tune::i8_sched, kOnOff, all_but(0)},
    {"i8_nostore", &Tune::i8_nostore, kOnOff, all_but(0)},
    {"i8_variant", &Tune::i8_variant, in_range(-1, 899), all_but(-1)},
    {"resample_aux", &Tune::resample_aux, in_range(0, 3), all_but(0)},
    // the non-metric iteration
    {"nm_fast_lds", &Tune::nm_fast_lds, kOnOff},
    {"nm_k16", &Tune::nm_k16, kOnOff},
    {"nm_codes", &Tune::nm_codes, kOnOff},
    {"nm_mfma", &Tune::nm_mfma, kOnOff},
    {"nm_direct16", &Tune::nm_direct16, kOnOff},
    {"nm_wave", &Tune::nm_wave, kOnOff},
    {"nm_live", &Tune::nm_live, kOnOff},
    {"nm_wave16", &Tune::nm_wave16, kOnOff},
    {"nm_subset", &Tune::nm_subset, in_range(0, 100)},
    {"nm_cpl", &Tune::nm_cpl, one_of(0, 8, 6)},
    {"nm_c10", &Tune::nm_c10, kOnOff},
    {"nm_vlong", &Tune::nm_vlong, kOnOff},
    {"nm_cat_one", &Tune::nm_cat_one, kOnOff},
    {"nm_bound_shift", &Tune::nm_bound_shift, in_range(0, 200)},
    {"nm_verify_rows", &Tune::nm_verify_rows, in_range(0, 100)},
    {"nm_counts8", &Tune::nm_counts8, kOnOff},
    // the sub-batches and passes of a bootstrap call
    {"boot_chunks", &Tune::boot_chunks, in_range(0, kBootChunksMax)},
    {"boot_ratio", &Tune::boot_ratio, in_range(10, 100)},
    {"boot_align", &Tune::boot_align, in_range(0, 1 << 20)},
    {"boot_pass", &Tune::boot_pass, pass_cap()},
};

// The seams of one call kind each, settable like the options above and outside their table: kOptions is what tests/golden/option_table.json records row by row.
static constexpr OptionRow kSeamOptions[] = {
    {"rebus_classes", &Tune::rebus_classes, in_range(0, 16)},
};

inline const OptionRow* option_find(const char* name) {
    for (const OptionRow& o : kOptions) if (!strcmp(o.name, name)) return &o;
    for (const OptionRow& o : kSeamOptions) if (!strcmp(o.name, name)) return &o;
    return nullptr;
}
inline bool option_takes(const OptionValues& s, int value) {
    switch (s.kind) {
        case OptionValues::RANGE: return value >= s.v[0] && value <= s.v[1];
        case OptionValues::ONE_OF: return value == s.v[0] || value == s.v[1] || value == s.v[2] || value == s.v[3];
        case OptionValues::ZERO_OR_RANGE: return value == 0 || (value >= s.v[0] && value <= s.v[1]);
        case OptionValues::PASS_CAP: return value >= 0 && value <= (1 << 30) && !(value & 255);
    }
    return false;
}
inline bool option_experimental(const OptionExperiments& e, int value) {
    return e.kind == OptionExperiments::ALL_BUT ? value != e.value : e.kind == OptionExperiments::ONLY && value == e.value;
}

// Set option `name` of `t`.  A refused call leaves `t` as it was; *effect (may be null): what the handle has to void -- nothing when the value is the one `t` held.
enum OptionResult { OPTION_OK = 0, OPTION_OUT_OF_RANGE, OPTION_EXPERIMENTS_ONLY, OPTION_UNKNOWN };
inline OptionResult option_set(Tune& t, const char* name, int value, bool experiments, OptionEffect* effect) {
    if (effect) *effect = OPTION_VOIDS_NOTHING;
    const OptionRow* o = option_find(name);
    if (!o) return OPTION_UNKNOWN;
    if (!option_takes(o->values, value)) return OPTION_OUT_OF_RANGE;
    if (!experiments && option_experimental(o->experiments, value)) return OPTION_EXPERIMENTS_ONLY;
    if (effect && value != t.*(o->field)) *effect = o->voids;
    t.*(o->field) = value;
    return OPTION_OK;
}
inline bool option_get(const Tune& t, const char* name, int* value) {
    const OptionRow* o = option_find(name);
    if (o) *value = t.*(o->field);
    return o != nullptr;
}

}  // namespace plspm
