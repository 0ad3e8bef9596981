// host_internal.h -- what the translation units of libplspm_hip.so share on the HOST side (round 4: the former one-file host is split by
// concern so that the units compile side by side): plspm_hip.hip (allocator, handles, options, upload, staging), plspm_fit.hip (fp64 Gram,
// solvers, non-metric iteration, single fit, operator seam), plspm_gram_i8.hip (digit planes + the int8 Gram of bootstrap batches),
// plspm_bootstrap.hip (bootstrap driver, record download, summaries), plspm_group.cpp (multi-GPU groups).  Every device kernel lives in
// exactly one unit's headers; the functions below are the seams between them.  Nothing here is part of the C-ABI (include/plspm_hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/plspm_hip_test.h"
#include "solver_core.h"
#include "solver_nmg.h"
#include "solver_hoc.h"
#include "solver_nmx.h"
#include "solver_ops.h"
#include "solver_wave.h"
#include "solver_quad.h"
#include "solver_wave16.h"
#include "solver_route.h"

using namespace plspm;

typedef double d4 __attribute__((ext_vector_type(4)));
__host__ __device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }

#include "model.h"

inline RouteShape route_shape(const plspm_model* m) { return {m->P, m->L, m->kmax, m->n_chol, m->n_eff, (int)m->pred_idx.size(), m->boff.data()}; }
// Dynamic LDS beyond the 64 KiB default needs an explicit opt-in per kernel.
inline int allow_lds(plspm_model* m, const void* fn, size_t bytes) {
    if (bytes > kMaxLds) return fail(m, PLSPM_E_LIMIT, "kernel needs more than 160 KiB of LDS");
    if (bytes > 48 * 1024) {
        // (a kernel with static LDS of its own can be refused below 160 KiB of dynamic LDS: the same limit, the same code -- found by the many-LV fuzz, a 34-LV / 179-MV model)
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(m, PLSPM_E_LIMIT, "kernel needs " + std::to_string(bytes) + " bytes of dynamic LDS beside its static share: more than the device grants (" + hipGetErrorString(e) + ")");
        }
    }
    return 0;
}

// where a solver launch writes: per-problem strides; null base pointers are skipped
struct SolverOut {
    double* row; long row_stride;
    int* status; int* iters;
    long long* marks;
    FitOutputs fit;     // single-fit extras (problem 0 only)
};

// ---- plspm_hip.hip
ModelDesc make_desc(const plspm_model* m);
HocDesc make_hoc_desc(const plspm_model* m2);
void set_geometry(plspm_model* m);
static constexpr size_t kPinHalf = (size_t)8 << 20;       // two halves of the handle's pinned staging area: the host copy of chunk k+1 overlaps the DMA of chunk k
int pin_ready(plspm_model* m);

// ---- plspm_fit.hip
// moment matrix of ALL uploaded rows -> m->gram (dense fp64 MFMA Gram over row chunks + fixed-order reduce)
int dense_moments(plspm_model* m);
// fp64 MFMA Gram of `nproblems` replicates over their (row,count) lists -> tile-packed matrices at `out`
int launch_gram_lists(plspm_model* m, long nproblems, const int2* ent, const int* nent, long ent_stride, double* out);
int run_impute(plspm_model* m, long nproblems, const double* Min, const double** Mp, long* mp_stride);
int launch_solver(plspm_model* m, long nproblems, const double* Mp, long mp_stride, const SolverOut& so, int threads);
// the metric solver of a bootstrap batch: `route` as metric_batch_route chose it when the int8 Gram wrote dense matrices, else ROUTE_LDS
int launch_batch_solver(plspm_model* m, long nb, SolverRoute route, const SolverOut& so);
// Scale.NUM / RAW non-metric bootstrap batches as ONE solver launch (round 6; solver_wave16.h NM): does this model have such a kernel, and the launch itself
// (dense moment matrices at m->gram; maps / steps as kernels_solver.h solver_nmwave_kernel takes them; force + live: the replay of `nb` listed replicates)
bool nm_wave_solver_covers(const plspm_model* m);
int launch_nm_wave_solver(plspm_model* m, long nb, const SolverOut& so, double* maps, long maps_stride, int* steps, const int* force, const int* live);
size_t nm_state_doubles_of(const plspm_model* m);
size_t nm_dense_lds(const plspm_model* m, bool* whole, int* kb_out);
int run_nonmetric(plspm_model* m, long nproblems, const double* Mp, long mp_stride, const SolverOut& so_in, const int2* ent, const int* nent, long ent_stride, int threads,
                  bool finish = true, const void* cd8 = nullptr, int cd8_MT = 0, bool counts16_ready = false);
// second-stage moments of a HOC pair by congruence with the first stage's score maps: m->gram (stage 1) -> m2->gram
int run_hoc_moments(plspm_model* m, plspm_model* m2, long nb);

// ---- plspm_gram_i8.hip
static inline int i8_kblocks(long N) { return (int)((N + 127) / 128) * 2; }      // k-blocks of 64 rows, an even number
static inline long i8_pairs(const plspm_model* m) { const long C = m->Pg + 1; return C * (C + 1) / 2; }
bool nm_counts8_possible(const plspm_model* m);
int choose_gram_path(const plspm_model* m, int64_t B);      // 1 fp64 MFMA on (row,count) lists, 2 int8 digit planes
int prepare_zs_stats(plspm_model* m);
int prepare_zs(plspm_model* m, int floor = 0);      // floor: at least this many digit planes (0: the handle's own choice)
int run_gram_i8(plspm_model* m, int64_t nb, uint64_t seed, int64_t rep0, const int32_t* d_idx, double* out, bool dense, bool* fallback, const void** counts = nullptr,
                int* counts_MT = nullptr, unsigned short* out16 = nullptr, bool* wrote16 = nullptr);
bool nm_wave_route_planned(const plspm_model* m);     // plspm_nonmetric.hip: Scale.NUM / RAW batches as one solver launch + verification (run_nonmetric_wave)
int run_nonmetric_wave(plspm_model* m, long nb, const SolverOut& so, const void* cd8, int cd8_MT);
bool nm_wave_step_planned(const plspm_model* m);      // plspm_nonmetric.hip: the categorical iteration of this handle runs one wave per problem (kernels_nmw.h)

// ---- plspm_permute.hip (two-group permutation test)
// One call's splits: permutation rep_offset + p has problem 2p = group a (n1 rows), 2p + 1 = the other N - n1 rows; `d_member` [B][N] bytes 0/1
// (explicit memberships, tests) or null (on-device splits from the Philox keys, kernels_permute.h).
struct PermSpec { uint64_t seed; int64_t rep_offset; int64_t n1; const uint8_t* d_member; };
// run_gram_i8 on a permutation call (m->perm set): the 0/1 counts of problems [prob0, prob0 + nb) (prob0, nb even) into `cd`, layout of
// resample_i8_kernel (MT count tiles, KB k-blocks)
int launch_perm_counts(plspm_model* m, int64_t nb, int64_t prob0, int MT, int KB, void* cd);
// One call's stratified resamples: resample rep_offset + p has problem 2p = n_a draws from group a's rows, 2p + 1 = n_b draws from group b's;
// `d_rows` [N] = group a's rows then group b's, ascending; `d_draws` [B][N] explicit rows (tests) or null (Philox draws, kernels_strat.h).
struct StratSpec { uint64_t seed; int64_t rep_offset; int64_t n_a; const int32_t* d_rows; const int32_t* d_draws; };
// run_gram_i8 on a stratified call (m->strat set): the counts of problems [prob0, prob0 + nb) (prob0, nb even) into `cd`, same layout
int launch_strat_counts(plspm_model* m, int64_t nb, int64_t prob0, int MT, int KB, void* cd);
