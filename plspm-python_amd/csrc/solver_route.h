// solver_route.h -- which solver kernel takes a bootstrap batch: a pure function of the model's shape and the solver options, read by the planner
// (plspm_bootstrap.hip: Gram layout, buffer sizes) and the launchers (plspm_fit.hip).  Free of the HIP runtime: the CPU tests compile it (tests/hostemu).
#pragma once
#include <stddef.h>
#include "solver_quad.h"
#include "solver_wave16.h"

namespace plspm {

// The values are what get_option("last_solver") reports.  LDS: solver_kernel (packed moment matrices, any model); ROWS: solver_rows_kernel (<= 64 MVs);
// WAVE: solver_wave_kernel<8> (the round-3 wave solver, option solver_wave 3); ROWS_SPLIT: solver_rows_split_kernel (65 .. 128 MVs); QUAD: solver_quad_kernel<16>
// (Mode-A models of 65 .. 128 MVs, <= 16 LVs); WAVE16_8 / 16 / 32: solver_wave16_kernel<8> (<= 8 LVs, the headline's class) / <16> (9 .. 16 LVs) / <32> (17 .. 32
// LVs, all Mode A); NM_WAVE_8 / 16 / 32: solver_nmwave_kernel<8 / 16 / 32>, a Scale.NUM / RAW batch in one launch.
enum SolverRoute { ROUTE_NONE = 0, ROUTE_LDS = 1, ROUTE_ROWS = 2, ROUTE_WAVE = 3, ROUTE_ROWS_SPLIT = 4, ROUTE_QUAD = 5, ROUTE_WAVE16_16 = 6, ROUTE_WAVE16_8 = 7,
                   ROUTE_WAVE16_32 = 8, ROUTE_NM_WAVE_8 = 9, ROUTE_NM_WAVE_16 = 10, ROUTE_NM_WAVE_32 = 11 };

static constexpr size_t kMaxLds = 160 * 1024;
// LDS of the model descriptors the LDS / rows solvers copy in
PLSPM_HD size_t desc_lds_bytes(int P, int L, int ne, int nedge) {
    const size_t T = ((size_t)P + 1 + 31) / 32 * 2, ntile = T * (T + 1) / 2;
    return (size_t)P * 8 + (3 * (size_t)(L + 1) + P + 2 * (size_t)L + 2 * (size_t)ne + 2 * (size_t)nedge + (ntile + 1) / 2 + 4) * 4 + (((size_t)L * L + 15) & ~(size_t)15) + 16;
}

// As plspm_model_create derives it: kmax = most predecessors of one LV, n_chol = doubles of the Mode-B factors, n_eff = effect pairs, nedge = path edges
struct RouteShape { int P, L, kmax, n_chol, n_eff, nedge; const int* boff; };

// Where solver_kernel (ROUTE_LDS, and the single fit) keeps its workspace: the small workspace goes in LDS behind the descriptors if it fits the budget -- all of a
// CU's LDS for one problem, 64 KiB for a batch (>= 2 workgroups per CU) -- and the covariance matrix S too if it then still fits; what does not lives in global
// scratch (s_bytes / small_bytes per problem).  lds: the launch's dynamic LDS.
struct SolverLds { bool s_in_lds, small_in_lds; size_t lds, s_bytes, small_bytes; };
PLSPM_HD SolverLds solver_lds(const RouteShape& s, long nproblems) {
    SolverLds k{};
    k.s_bytes = (size_t)cov_doubles(s.P) * sizeof(double);
    k.small_bytes = (size_t)workspace_small_doubles(s.P, s.L, s.kmax, s.n_chol) * sizeof(double);
    const size_t budget = nproblems == 1 ? kMaxLds : 64 * 1024;
    k.lds = desc_lds_bytes(s.P, s.L, s.n_eff, s.nedge);
    if (k.lds + k.small_bytes <= budget) { k.small_in_lds = true; k.lds += k.small_bytes; }
    if (k.small_in_lds && k.lds + k.s_bytes <= budget) { k.s_in_lds = true; k.lds += k.s_bytes; }
    return k;
}

// A metric batch's solver on the dense moment matrices the int8 Gram can write, or ROUTE_LDS (packed matrices) where no dense solver takes the model.  solver_wave:
// 0 none, 1 / 2 the wave16 form at <= 8 LVs, 3 the round-3 kernel there; solver_quad 0: split rows instead; solver_rows 0: no dense solver.  (A model of the
// <= 8 LV wave forms always passes the rows test below: at most 37 KB.)
PLSPM_HD SolverRoute metric_batch_route(const RouteShape& s, int solver_wave, int solver_quad, int solver_rows) {
    if (solver_rows == 0) return ROUTE_LDS;
    if ((solver_wave == 1 || solver_wave == 2) && s.L <= 8 && wave_solver_covers<8>(s.P, s.L, s.n_chol) && wave16_ws_doubles<8>(s.L, s.kmax, s.n_chol) * sizeof(double) <= 20 * 1024) return ROUTE_WAVE16_8;
    if (solver_wave != 0 && wave_solver_covers<8>(s.P, s.L, s.n_chol)) return ROUTE_WAVE;
    if (solver_wave != 0 && wave16_solver_covers<16>(s.P, s.L, s.n_chol, s.kmax)) return ROUTE_WAVE16_16;
    if (solver_wave != 0 && s.n_chol == 0 && wave16_solver_covers<32>(s.P, s.L, 0, s.kmax)) return ROUTE_WAVE16_32;
    if (solver_quad != 0 && quad_solver_covers<16>(s.P, s.L, s.n_chol, s.kmax, s.boff)) return ROUTE_QUAD;
    // the rows solvers hold their small workspace + descriptors in LDS: at least four problems per CU at <= 64 MVs, two in the split form
    const size_t rows_lds = desc_lds_bytes(s.P, s.L, s.n_eff, s.nedge) + (size_t)workspace_small_doubles(s.P, s.L, s.kmax, s.n_chol) * sizeof(double);
    if (s.P <= 64) return rows_lds <= kMaxLds / 4 ? ROUTE_ROWS : ROUTE_LDS;
    return s.P <= 128 && rows_split_block(s.boff, s.L, 64) > 0 && rows_lds + 4 * 16 * 66 * sizeof(double) <= kMaxLds / 2 ? ROUTE_ROWS_SPLIT : ROUTE_LDS;
}

// The one-launch form of a Scale.NUM / RAW batch, or ROUTE_NONE (per-iteration launches).  Its <= 8 LV form takes 64 doubles more than the metric one.
PLSPM_HD SolverRoute nm_wave_route(const RouteShape& s) {
    if (s.P < 1 || s.P > 64) return ROUTE_NONE;
    if (s.L <= 8) return (wave16_ws_doubles<8>(s.L, s.kmax, s.n_chol) + 64) * sizeof(double) <= 20 * 1024 && s.n_chol / 2 <= 16 * 66 ? ROUTE_NM_WAVE_8 : ROUTE_NONE;
    if (s.L <= 16) return wave16_solver_covers<16>(s.P, s.L, s.n_chol, s.kmax) ? ROUTE_NM_WAVE_16 : ROUTE_NONE;
    return s.n_chol == 0 && wave16_solver_covers<32>(s.P, s.L, 0, s.kmax) ? ROUTE_NM_WAVE_32 : ROUTE_NONE;      // (17 .. 32 LVs: all Mode A)
}

}  // namespace plspm
