// rebus_route.h -- the plan of one REBUS-PLS round (plspm_rebus.hip): the doubles of one class's parameters, the classes whose parameters one LDS load of the row
// pass holds, the row tile, the grids of the three kernels, the slices of the class-moment pass, and the refusal when one class's parameters do not fit.  A pure
// function of (P, L, n_endo, K, N) and the test-only cap "rebus_classes".  Free of the HIP runtime: tests/rebus_host compiles it.
#pragma once
#include "rebus_core.h"

namespace plspm {

constexpr long kRebusMaxLds = 160 * 1024;      // a workgroup's LDS (solver_route.h kMaxLds)
constexpr int kRebusThreads = 256;             // threads of a row-pass / assignment workgroup: four waves
constexpr int kRebusRows = 64;                 // rows of a tile: lane = row, so a wave works on one class at a time and reads its parameters as broadcasts
constexpr int kRebusMaxClasses = 16;
constexpr int kRebusSliceRows = 2048;          // rows of one slice of the class-moment pass
constexpr int kRebusMaxSlices = 64;

struct RebusShape { int P, L, n_endo, K; long N; };
struct RebusPlan {
    int param_doubles;       // of one class (rebus_core.h rebus_param_doubles)
    int xs;                  // pitch of a tile row in LDS, doubles: odd, so that the 64 lanes of a wave read 64 rows without a bank conflict
    long fixed_doubles;      // the tile [rows x xs] and a thread's scores [L x threads]
    int classes_per_load;    // classes whose parameters sit in LDS beside them (0: refused)
    int loads;               // LDS loads per tile: ceil(K / classes_per_load)
    int rows;                // of a tile
    long tiles;              // grid of the row pass
    long assign_grid;        // grid of the assignment: a thread per row
    int slices;              // of the class-moment pass: grid (K, slices)
    long slice_rows;
    long lds_bytes;          // of the row pass
    bool refused;            // one class's parameters do not fit beside the tile: PLSPM_E_LIMIT
};

inline RebusPlan rebus_plan(const RebusShape& s, int cap = 0) {
    RebusPlan p{};
    p.param_doubles = rebus_param_doubles(s.P, s.L, s.n_endo);
    p.xs = s.P | 1;
    p.rows = kRebusRows;
    p.fixed_doubles = (long)p.rows * p.xs + (long)s.L * kRebusThreads;
    const long room = kRebusMaxLds / (long)sizeof(double) - p.fixed_doubles;
    long fit = room > 0 ? room / p.param_doubles : 0;
    if (fit > s.K) fit = s.K;
    if (cap > 0 && fit > cap) fit = cap;
    p.classes_per_load = (int)fit;
    p.refused = fit < 1;
    p.loads = p.refused ? 0 : (s.K + p.classes_per_load - 1) / p.classes_per_load;
    p.tiles = (s.N + p.rows - 1) / p.rows;
    p.assign_grid = (s.N + kRebusThreads - 1) / kRebusThreads;
    long sl = (s.N + kRebusSliceRows - 1) / kRebusSliceRows;
    if (sl > kRebusMaxSlices) sl = kRebusMaxSlices;
    if (sl < 1) sl = 1;
    p.slices = (int)sl;
    p.slice_rows = ((s.N + sl - 1) / sl + 3) & ~3L;
    p.lds_bytes = (p.fixed_doubles + (long)p.classes_per_load * p.param_doubles) * (long)sizeof(double);
    return p;
}
inline const char* rebus_refusal() { return "one class's parameters do not fit a workgroup's 160 KiB of LDS beside a tile of 64 rows and the threads' scores"; }

}  // namespace plspm
