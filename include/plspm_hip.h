/*
 * plspm_hip.h -- C-ABI of libplspm_hip.so, the MI355X (gfx950) estimator backend for the PLS-PM
 * weight-solver + bootstrap hot path of GoogleCloudPlatform/plspm-python.
 *
 * The reference is pure Python and has no FFI of its own; this ABI is the seam a maintainer would bind
 * with ctypes in place of two internal call sites (paths relative to the reference repository):
 *
 *   (i)  WeightsCalculatorFactory.calculate(data, path)      plspm/weights.py:172-187
 *        called from Estimator.estimate                      plspm/estimator.py:39,52
 *        -> plspm_model_create + plspm_upload + plspm_fit
 *   (ii) Bootstrap.__init__ / BootstrapProcess.run           plspm/bootstrap.py:81-117, 45-73
 *        called from Plspm.__init__                          plspm/plspm.py:78-82
 *        -> plspm_bootstrap (replicates in [rep_offset, rep_offset + B) of one logical stream, so the
 *           result does not depend on how replicates are sharded over GPUs / processes)
 *        -> plspm_group_* : the fan-out over `processes` workers and the Queue merge (bootstrap.py:89-111)
 *           as replicate shards on several MI355X with ONE RCCL all-gather over xGMI at the end
 *
 * Conventions
 *   - plain C types only; all host buffers caller-allocated, row-major, IEEE fp64 unless noted.
 *   - "device column order": MVs grouped by LV in path-matrix order, blocks contiguous
 *     (block_offset[l] .. block_offset[l+1]); the caller supplies the map from its own columns.
 *   - every function returns 0 on success, > 0 for a numerical/argument condition, < 0 for a
 *     HIP runtime error; plspm_last_error() returns the text.  Nothing throws across the boundary.
 *   - one opaque handle per (model, device); handles are independent and may be used from different
 *     threads; a single handle is not re-entrant.
 *   - there is NO CPU fallback: without a usable HIP device plspm_model_create fails.
 */
#ifndef PLSPM_HIP_H
#define PLSPM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plspm_model plspm_model_t;

/* Scheme ids (reference plspm/scheme.py:57-63) and Mode ids (plspm/mode.py:64-69). */
enum { PLSPM_SCHEME_CENTROID = 0, PLSPM_SCHEME_FACTORIAL = 1, PLSPM_SCHEME_PATH = 2 };
enum { PLSPM_MODE_A = 0, PLSPM_MODE_B = 1 };
/* Per-problem status written by plspm_fit / plspm_bootstrap. */
enum {
    PLSPM_OK = 0,
    PLSPM_NOT_CONVERGED = 1, /* reference raises Exception("Could not converge ...") weights.py:185-186 */
    PLSPM_SINGULAR = 2,      /* a regression the reference cannot solve either (e.g. Mode B on a block with missing cells, mode.py:55-56) */
    PLSPM_NONFINITE = 3,     /* zero-variance MV or NaN input                                            */
    PLSPM_INADMISSIBLE = 4   /* PLSc, model-fit and geodesic records only (plspm_plsc_*, plspm_modelfit_*, plspm_geodesic_*; the last has causes of its own): a factor's rho_A is not positive and finite, or a corrected construct correlation is not below 1 in magnitude */
};
/* Argument errors returned by the API functions themselves. */
enum { PLSPM_E_ARG = 100, PLSPM_E_STATE = 101, PLSPM_E_LIMIT = 102 };

/* ABI version of this header; plspm_abi_version() of the loaded library must match. */
#define PLSPM_ABI_VERSION 4
int plspm_abi_version(void);

/* Number of HIP devices visible to the process (0 when there is none; never negative). */
int plspm_device_count(void);

/* The library keeps freed device / pinned-host blocks for re-use (a Plspm() call creates, fills and destroys a handle; without the
 * cache that is ~40 allocator round trips per call).  This hands every cached block back to the HIP runtime. */
int plspm_release_cached_memory(void);

/* Text of the last error on this handle (or of the last failed plspm_model_create when NULL). */
const char* plspm_last_error(const plspm_model_t* m);

/*
 * Options of a handle.  The defaults are the measured optima; tests and benches use the rest to force a route or a kernel form.  The library
 * reads NO environment variables.  Unknown keys / out-of-range values return PLSPM_E_ARG.
 *
 * Routes and precision
 *   "gram_path"       0 auto | 1 fp64 MFMA Gram over (row,count) lists | 2 int8 digit-plane Gram (exact integer product of the dense resample
 *                     multiplicities with the base-256 digit planes of the pair products x_p x_q).  Auto = 2 for every bootstrap whose planes
 *                     fit the memory budget and whose sums fit int32 (N < 2^24 rows): metric, mean-imputed, non-metric and categorical models,
 *                     on-device draws and explicit index lists alike (a chunk of an index list that carries a multiplicity above 127 takes
 *                     route 1); second stages of HOC pairs work on their first stage's matrices
 *   "i8_slices"       0 | 1 .. 8   digit planes per pair product.  0 (default) = automatic: 6 planes when every pair column of the uploaded data has
 *                     sum|z| >= 257 max|z| -- the worst-case error N 2^-47 max|z| of a replicate's sum is then below the a-priori bound N 2^-53 sum|z|
 *                     of an fp64 accumulation of the same terms, with a factor 4 to spare, even for a replicate that misses the column's largest
 *                     row -- else 7 (>= 54 significant bits of the column maximum), else -- sum|z| < 2 max|z|: one gross outlier row carries
 *                     the column, and a replicate without it sums products that are tiny against the scale of the planes -- 8; and never more
 *                     planes than carry anything: planes that are identically zero in the
 *                     seven-plane decomposition are dropped (0/1 indicator columns: ONE plane, bit-identical sums).  Read-only "last_i8_slices" /
 *                     "last_i8_ratio" report the choice and floor(min sum / max)
 *   "i8_min_slices"   0 (default) | 6 .. 8   the automatic choice, but never fewer planes (Plspm(precision="strict"): 7 -- the rate bench.py reports
 *                     as `value_strict`)
 *   "i8_min_batch"    auto mode takes the int8 route from this many replicates per call (default 1: always -- the route must not
 *                     depend on how a job is sharded, or shards of different size would differ in the last bits)
 * Int8 Gram kernels (all forms give bit-identical matrices: exact int32 sums)
 *   "i8_priv"         1 (default) | 0   six / seven planes: gram_i8p_kernel (round 4: four waves, count fragments straight from global memory into
 *                     registers, only the digit blocks through the LDS ring; tile rows of 320 / 256 replicates with six planes, 256 / 192 with
 *                     seven) or, 0, the round-3 gram_i8_kernel (eight waves, both operands through LDS: 9-10 % slower, kept as the A/B reference
 *                     and for the other plane counts).  Read-only "last_i8_priv"
 *   "i8_rt"           0 (default) | 16 | 20   count tiles (16 replicates each) per tall workgroup tile.  0 = automatic: the replicates are cut into
 *                     tall and short tile rows in ONE launch so that the machine's last round is as full as the others (list-scheduling model of
 *                     the 8 XCDs, tile costs measured per kernel: profiles/r04_i8_mix_calib.jsonl); 20 / 16 with six / seven planes: tall rows
 *                     only; 16 with six planes: the 256-replicate round-3 kernel.  Read-only "last_i8_rt" / "last_i8_short" / "last_i8_mt": tall
 *                     tile height, short rows and padded count tiles of the last launch
 *   "i8_cus"          0 (default: every CU of the device) | 8 ... the device's count: the tile-row cut is planned for that many CUs -- for launches
 *                     that share the chip with the kernels of a collective (a Gram workgroup needs a whole CU; bench.py tries a few values when it
 *                     runs more than one rank).  Results do not depend on it
 *   "i8_dma"          0 (auto) | 1 | 2   LDS-DMA form of the round-3 kernel: 1 global_load_lds_dwordx4 (64-bit base per block), 2 buffer_load_dwordx4
 *                     ... lds (per-workgroup descriptors + 32-bit offsets; auto takes it whenever an operand's walk stays below 4 GiB)
 *   "i8_ind"          1 (default) | 0   one-plane data run through the seven-plane main loop, the planes of a wave standing for seven pair groups
 *   "i8_nibbles"      1 (default) | 0 | 2   (round 5) Philox draws of data sets beyond 65,536 rows: 4-bit LDS counters (three workgroups per CU at 100,000
 *                     rows) with an exact overflow test -- sum of the counts == draws -- and an 8-bit second try for a replicate that fails it; 0: the
 *                     8-bit histogram of round 3; 2: every replicate through the second try (tests).  Same counts.  Read-only "last_i8_nibbles"
 * Solvers
 *   "solver_rows"     1 (default) | 0   bootstrap of metric models with at most 64 MVs on the int8 route: one wave per replicate with the
 *                     covariance columns in registers (solver_rows_kernel) instead of one workgroup with the covariance in LDS; models of
 *                     65 ... 128 MVs whose blocks divide into two runs of at most 64 MVs: four waves per replicate, two threads per MV
 *                     (solver_rows_split_kernel)
 *   "solver_wave"     1 (default) | 0 | 3   among those, models with at most 16 LVs (round 5; Mode-B blocks whose inverses fit 1,056 doubles) and all-Mode-A
 *                     models with at most 32: the
 *                     wave-native formulation (one wave per replicate with fixed lane roles, coalesced triangle load + LDS transpose:
 *                     solver_wave16_kernel<8> / <16>) instead of solver_rows_kernel; 3: models of at most 8 LVs on the round-3 / round-4
 *                     kernel (solver_wave_kernel<8>; A/B)
 *   "solver_quad"     1 (default) | 0   (round 5) Mode-A models of 65 ... 128 MVs and at most 16 LVs whose blocks divide into two runs of at most 64
 *                     MVs: the wave solver's fixed lane roles on four waves per replicate (solver_quad_kernel) instead of solver_rows_split_kernel
 *   "solver_threads"  64 | 128 | 256      threads per problem of the LDS solver (default 128)
 *   "nm_threads"      0 (by model width) | 64 | 128 | 256   threads per problem of the non-metric solvers
 *   "nm_live"         1 (default) | 0   (round 5) non-metric iteration on the dense stop-rule route: from the second step on, the step / compose launches cover the
 *                     problems still iterating after the previous step (the list that step's stop-rule pass built) instead of every problem of the batch
 *   "nm_counts8"      1 (default) | 0   non-metric bootstrap on the int8 route: the dense stop-rule pass takes the replicates' row
 *                     multiplicities from the int8 counts of the Gram (no second resample kernel / uint16 histograms / (row,count) lists)
 *   "nm_codes"        1 (default) | 0   all-indicator categorical models (every MV ORD / NOM), bootstrap on the int8 route: the dense
 *                     stop-rule pass adds the coefficient of the one column a row has set per MV (16 category codes per row tile and MV,
 *                     nm_conv_codes_kernel) instead of multiplying every 0/1 column through -- bit-identical partial sums, 2.3 x faster
 *                     passes on 300 indicator columns.  Read-only "last_nm_codes"
 *   "nm_mfma"         1 (default) | 0   (round 5) among those, LV blocks of at most 128 indicator columns: the stop-rule pass as an exact int8 matrix product --
 *                     indicator bytes of the rows x seven base-256 digit planes of the replicates' score maps (nmp::conv_mfma_kernel), the digits put
 *                     together again per (row, replicate); same decisions, criterion values equal to ~1e-12 relative, 2 x faster than the pass on
 *                     category codes.  Read-only "last_nm_mfma"
 *   "nm_wave"         1 (default) | 0   (round 5) all-indicator categorical models, every block Mode A, at most 64 MVs of at most 16 categories, 8 LVs,
 *                     511 indicator columns, 65,535 rows: the iteration as one wave per problem (nmw::nmw_step_kernel) instead of one workgroup
 *                     (nmg_kernel<1>); records equal to ~1e-13, equal iteration counts.  Read-only "last_nm_wave"
 *   "nm_c10"          1 (default) | 0   (round 6) among those, items of nine or ten categories (the reference's mobi / ECSI data): the ten-category instantiation
 *                     of the wave step, two waves per SIMD, instead of the sixteen-category one, which runs alone on its SIMD -- the same arithmetic, identical records
 *   "nm_vlong"        1 (default) | 0   (round 6) verification of the one-launch categorical batch: behind the fourth round of eight steps the replicates still
 *                     iterating are the few that never converge; their remaining steps (up to 72) are verified in ONE round where the slots fit, instead of
 *                     nine more rounds with a host read-back each -- the same slots, the same decisions
 *   "nm_direct16"     1 (default) | 0   (round 5) bootstrap of such models on the int8 route: the product writes the replicates' co-occurrence counts
 *                     as uint16 matrices itself (upper triangle; mirrored through LDS by nmg_kernel<4>) instead of fp64 moment matrices that a scatter
 *                     pass turns into the same integers -- bit-identical records.  Read-only "last_nm_direct16"
 *   "nm_fast_lds"     1 (default) | 0   categorical (ORD / NOM) solver: the small arrays of the iteration in LDS for the duration of a launch
 *   "nm_k16"          1 (default) | 0   all-indicator categorical models of at most 65,535 rows: uint16 copy of the count matrix for the
 *                     streaming product of every step (bit-identical steps, a quarter of the bytes)
 *   "conv_pass"       0 auto | 1 gathering stop-rule pass | 2 dense pass with block-staged coefficients (non-metric bootstrap)
 *   "conv_gy"         0 (default) .. 65535   replicate slices of the dense stop-rule pass (0: one replicate group per workgroup); matrix-product pass:
 *                     the waves it aims at, in units of 256 (0: 8,192)
 * Host-buffer bootstrap (plspm_bootstrap)
 *   "boot_chunks"     0 (default: automatic) | 1 .. 8   plspm_bootstrap() of a metric model on Philox draws runs as sub-batches: the records of
 *                     sub-batch k cross PCIe on a copy stream -- and are unpacked into the caller's buffers -- while the kernels of sub-batch
 *                     k + 1 run.  Automatic: one below 2 MiB of records, else three, sizes falling by "boot_ratio" percent (default 60: what
 *                     moving a record costs relative to computing it on the headline model), every one but the last a multiple of 64
 *                     replicates.  Records do not depend on it
 * Single fit / upload
 *   "fit_chunks"      0 (auto) .. 65535   row chunks (workgroups) of the single-fit Gram
 *   "wide_nw"         4 | 8 | 16          waves sharing one row walk in gram_wide_kernel<14>
 *   "scores_tile"     0 (by LDS footprint) | 16 | 32   rows per tile of the scores kernel
 *   "upload_direct"   0 (default) | 1   plspm_upload of more than 64 MB: 0 through the handle's pinned staging halves, filled by several host
 *                     threads; 1 the runtime's pageable copy (one staging thread: 13-52 GB/s depending on the host)
 * (Test seams and the option values of the experiments build: include/plspm_hip_test.h.)
 *
 * plspm_model_get_option reads a value back; the read-only keys "last_gram_path" (1 fp64 MFMA, 2 int8 digit planes), "last_i8_dma" (1 / 2) and "last_solver"
 * (1 LDS solver, 2 rows solver, 3 wave solver of round 3 / Mode-B blocks, 4 split rows solver, 5 quad solver, 6 / 7 / 8 wave solver for 9 ... 16 / at most 8 / 17 ... 32 LVs) tell what the last bootstrap call took.
 */
int plspm_model_set_option(plspm_model_t* m, const char* key, int32_t value);
int plspm_model_get_option(const plspm_model_t* m, const char* key, int32_t* value);

/*
 * Compile a model specification (reference Config + path matrix + Plspm kwargs, plspm/config.py:89-160,
 * plspm/plspm.py:35-67) into device descriptors.
 *   P, L           manifest / latent variable counts (1 <= L <= 64, L <= P <= 1022).  Metric handles fall back to global scratch
 *                  when a problem's workspace exceeds LDS; the non-metric / categorical / incomplete-rows solvers keep their
 *                  small workspace (about (7P + P L + 8 L^2 + L (2 k^2 + k) + 2 sum k_b^2) * 8 bytes, k = most predecessors of an
 *                  LV, k_b = Mode-B block sizes) in the 160 KiB of LDS and return PLSPM_E_LIMIT from plspm_fit / plspm_bootstrap
 *                  beyond that (P ~ 1000 with L = 6 still fits; L = 64 with P = 1022 does not)
 *   block_offset   [L+1] device-column ranges of the LV blocks
 *   path           [L*L] row-major 0/1, path[i*L+j] = 1 iff LV j -> LV i; must be strictly lower triangular
 *   mode           [L]   PLSPM_MODE_A / PLSPM_MODE_B per LV
 *   scheme         PLSPM_SCHEME_*
 *   scaled         Config(scaled=...) : divide the centred data by ONE global scalar (config.py:302-303)
 *   max_iter, tol  already clamped by the caller the way Plspm.__init__ does (plspm.py:54-56)
 *   device_id      HIP device ordinal
 * Returns NULL on failure (see plspm_last_error(NULL)).
 */
plspm_model_t* plspm_model_create(int32_t P, int32_t L, const int32_t* block_offset, const uint8_t* path, const int32_t* mode,
                                  int32_t scheme, int32_t scaled, int32_t max_iter, double tol, int32_t device_id);
void plspm_model_destroy(plspm_model_t* m);

/*
 * Non-metric data with Scale.NUM / Scale.RAW on every MV (reference _NonmetricWeights, plspm/weights.py:73-133 with
 * scale.py:22-39; `Config(default_scale=Scale.NUM)`): every MV is population-standardised (config.py:314), the stop rule is
 * sum (|Y_old| - |Y_new|)^2 over the LV scores (weights.py:120, evaluated by a streaming pass over the observations after
 * every iteration), weights are rescaled as weights.py:130-132 and there is no sign rule.  `scaled` of plspm_model_create is
 * ignored in this mode.  Scale.ORD / Scale.NOM need plspm_model_set_categorical below.
 */
int plspm_model_set_nonmetric(plspm_model_t* m, int32_t on);

/*
 * Non-metric data with Scale.ORD / Scale.NOM MVs (optimal scaling: scale.py:41-56 with util.py rank / dummy / list_to_dummy,
 * weights.py:96-118).  The handle's P device columns become AUGMENTED columns: a NUM / RAW MV keeps its one data column, an
 * ORD / NOM MV is uploaded as its 0/1 indicator columns, one per category in ascending value order (what util.dummy builds
 * per fit).  Pm logical MVs, grouped by LV in path order like the columns:
 *   mv_off   [Pm+1] aug-column range of every MV (mv_off[0] = 0, mv_off[Pm] = P; a range never crosses an LV block)
 *   mv_kind  [Pm]   PLSPM_MV_NUM (one column) / PLSPM_MV_ORD / PLSPM_MV_NOM
 * Every per-MV output (weights, loadings, crossloadings, cov, bootstrap rows) then has Pm entries instead of P; the score
 * map (scores = Xaug . score_w + score_c) stays on the aug columns.  `mean` is reported as zeros.  Implies set_nonmetric(1).
 * Call before plspm_upload.  Bootstrap replicates that miss a category re-rank the present ones (rank of a resampled
 * column, util.py rank).
 */
#define PLSPM_MV_NUM 0
#define PLSPM_MV_ORD 1
#define PLSPM_MV_NOM 2
int plspm_model_set_categorical(plspm_model_t* m, int32_t Pm, const int32_t* mv_off, const int32_t* mv_kind);

/*
 * Metric data with missing values (reference util.impute, plspm/util.py:61-68, applied by Config.treat, config.py:300 -- to
 * the full data for the fit and to every RESAMPLED data set in the bootstrap, bootstrap.py:57): n_ind of the P data columns
 * have NaNs.  The caller uploads P + n_ind columns: the data columns with every NaN replaced by that column's mean over its
 * present values, then one 0/1 column per incomplete data column marking its NaN cells.
 *   ind_of  [P]  upload column (in [P, P + n_ind)) of the indicator of data column p, or -1 when p is complete
 * The fit then sees the mean-imputed data; every bootstrap replicate is re-imputed with its own column means, on the moments
 * (solver_core.h impute_collapse) -- no per-replicate pass over the data.  A replicate in which some column lost all its
 * present cells reports PLSPM_NONFINITE.  Metric handles only; call before plspm_upload.  Limit: P + n_ind <= 1022.
 */
int plspm_model_set_missing(plspm_model_t* m, int32_t n_ind, const int32_t* ind_of);

/*
 * Two-stage estimation of higher order constructs in the bootstrap (reference Estimator.estimate, plspm/estimator.py:29-55, run
 * per resampled data set by bootstrap.py:57).  `first` is the stage-1 model (every HOC replaced by its constituent LVs,
 * estimator.py:60-74) and holds the data; `second` is the original path model whose HOC blocks have ONE column per
 * constituent LV -- that LV's stage-1 score (Scale.NUM, estimator.py:43-52) -- and takes no upload.  The stage-1 LV order
 * must be the stage-2 order with every HOC expanded in place:
 *   lv_first  [L2+1]  stage-2 LV l stands for the stage-1 LVs [lv_first[l], lv_first[l+1]): one LV with the same block
 *                     (an ordinary LV) or its constituents (a HOC)
 * After attaching, plspm_bootstrap* on `first` runs both stages per replicate -- the stage-2 moment matrix is a congruence of
 * the replicate's stage-1 Gram with the stage-1 score maps (solver_hoc.h), no second pass over the data -- and reports the
 * SECOND stage's rows (plspm_row_width(first) becomes the second stage's; effect pairs: plspm_effect_pairs(second)).
 * plspm_fit(first) still fits stage 1 alone.  Both handles: plspm_model_set_nonmetric(.., 1), same device.  Destroy in any order.
 */
int plspm_model_attach_second_stage(plspm_model_t* first, plspm_model_t* second, const int32_t* lv_first);

/*
 * Upload the filtered raw observation matrix (what Config.filter returns, config.py:247-285; no NaNs).
 *   X          host pointer, dense fp64, src_cols columns x N rows
 *   layout     0: row-major (element (i,c) at X[i*src_cols + c]);  1: column-major (X[c*N + i])
 *   col_index  [P] source column of every device column, or NULL for the identity
 * The matrix stays resident in HBM (shifted by its column means, padded, with a ones column) until the
 * next upload / destroy.
 */
int plspm_upload(plspm_model_t* m, const double* X, int64_t N, int32_t src_cols, int32_t layout, const int32_t* col_index);

/*
 * Non-metric (Scale.NUM) data with missing values (reference weights.py:88-98, mode.py:35-41, scale.py:27-30; pairwise-complete
 * loadings outer_model.py:26).  Call AFTER plspm_upload: K rows of the uploaded matrix have missing cells (their NaNs replaced by
 * any finite value before the upload); rows in which a whole LV block is missing must have been dropped (config.py:273-285).
 *   row_index  [K]    ascending row numbers
 *   present    [K*P]  1 = cell present, 0 = missing (device column order)
 *   raw_scale  1 for a Scale.RAW-only model: the MVs then keep the treated values (scale.py:38-39), which are scaled by
 *              sqrt((f-1)/f) / sqrt((N-1)/N) against Scale.NUM in a column with f < N present cells; 0 for Scale.NUM
 * The rows move into a side table and become all-zero rows of the resident matrix, so the Gram kernels see the complete rows only;
 * the solver adds the incomplete rows explicitly in every sum (solver_nmx.h), weighted by their bootstrap counts.  Mode B blocks
 * must be complete in the data set at hand (mode.py:55-56): otherwise the fit / replicate reports PLSPM_SINGULAR.
 * plspm_model_set_nonmetric(.., 1) handles only; not combinable with set_categorical / set_missing / a two-stage pair.
 */
int plspm_model_set_incomplete_rows(plspm_model_t* m, int32_t K, const int32_t* row_index, const uint8_t* present, int32_t raw_scale);

/* Number of (from,to) effect rows = ordered LV pairs joined by a directed path; from-major order
 * (reference inner_model.py:46-52).  from/to may be NULL. */
int32_t plspm_effect_pairs(const plspm_model_t* m, int32_t* from, int32_t* to);

/* Width R = 2P + L + 2*n_eff of one bootstrap row:  weights[P] | r2[L] | total[n_eff] | direct[n_eff] | loadings[P]
 * (device column order; the reference collects the same five vectors per replicate, bootstrap.py:58-64). */
int32_t plspm_row_width(const plspm_model_t* m);

/* Row pitch (in doubles) of the DEVICE result buffer of plspm_bootstrap_device: R + 2.  Columns R and R+1 of every
 * device row hold that replicate's status and iteration count as doubles, so that one collective moves everything. */
int32_t plspm_row_stride(const plspm_model_t* m);

/* Outputs of one fit; every pointer may be NULL. */
typedef struct plspm_fit_result {
    double* weights;       /* [P]    outer weights, never sign-flipped (weights.py:69)                      */
    double* loadings;      /* [P]    cor(x_p, score of own LV) after the sign rule (outer_model.py:27)      */
    double* crossloadings; /* [P*L]  cor(x_p, score_l)                    (outer_model.py:26)               */
    double* path_coef;     /* [L*L]  inner-model slopes, [i*L+j] = j -> i (inner_model.py:70)               */
    double* r2;            /* [L]    R^2 per LV, 0 for exogenous          (inner_model.py:71-72)            */
    double* lv_cov;        /* [L*L]  population covariance of the LV scores                                */
    double* total;         /* [n_eff] total effects                       (inner_model.py:45-52)            */
    double* direct;        /* [n_eff]                                                                       */
    double* indirect;      /* [n_eff]                                                                       */
    double* scores;        /* [N*L]  LV scores, row-major, sign-corrected (weights.py:60-68)               */
    double* cov;           /* [P*P]  population covariance of the treated data (device column order)       */
    double* mean;          /* [P]    raw column means                                                      */
    int8_t* sign;          /* [L]    the sign vector of weights.py:62-64                                   */
    int32_t* iterations;   /* [1]    value of the reference's iteration counter when the loop stopped      */
    int32_t* status;       /* [1]    PLSPM_OK / PLSPM_NOT_CONVERGED / ...                                  */
} plspm_fit_result_t;

/* One estimate on the uploaded data (Estimator.estimate, estimator.py:29-55, without higher-order constructs). */
int plspm_fit(plspm_model_t* m, const plspm_fit_result_t* out);

/*
 * B bootstrap replicates (the loop of BootstrapProcess.run, bootstrap.py:54-66).
 *   rep_offset  global id of the first replicate; replicate r draws its N row indices from a counter-based
 *               Philox4x32-10 stream keyed by (seed, r), so any sharding reproduces the same rows
 *   idx         NULL -> on-device RNG;  else [B*N] int32 explicit resample indices in [0, N) (parity testing:
 *               the reference draws np.random.randint(N, size=N), bootstrap.py:56)
 *   out         [B*R] host buffer, R = plspm_row_width();  status/iters [B] (may be NULL)
 * Replicates whose status != PLSPM_OK are the ones the reference silently drops (bootstrap.py:65-66).
 */
int plspm_bootstrap(plspm_model_t* m, int64_t B, uint64_t seed, int64_t rep_offset, const int32_t* idx, double* out,
                    int32_t* status, int32_t* iters);

/* Same, leaving the results in device memory owned by the handle (valid until the next call on it):
 * *d_out -> [B * plspm_row_stride()] fp64, *d_status / *d_iters -> [B] int32.  Work is enqueued on the handle's stream;
 * plspm_sync() waits for it.  Lets a caller hand the buffers to RCCL without a host round trip. */
int plspm_bootstrap_device(plspm_model_t* m, int64_t B, uint64_t seed, int64_t rep_offset, const int32_t* d_idx, void** d_out,
                           void** d_status, void** d_iters);
int plspm_sync(plspm_model_t* m);
/* Enqueue now what the first bootstrap call on the uploaded data would have to build before its first replicate (the int8 digit planes
 * of the pair products, ~0.1 ms at 10k x 60): a host that knows a bootstrap follows the fit (Plspm(bootstrap=True): plspm.py:78-82 calls
 * Bootstrap right behind the estimate) calls this after plspm_upload.  Enqueue only -- the call never waits for the device: with the
 * automatic plane count it starts the column statistics and their copy to pinned memory, the plspm_fit that follows finds them on the host
 * when its own synchronisation returns and cuts the planes in its tail, beside the caller's unpacking of the fit.  Optional.  Anything that
 * rewrites the resident rows afterwards (plspm_upload, plspm_model_set_incomplete_rows) discards what was prepared. */
int plspm_bootstrap_prepare(plspm_model_t* m);
/* Host copy of replicates [first, first + count) of the LAST plspm_bootstrap(_device) call on this handle, whose records are still
 * in HBM: out [count*R], status / iters [count] (each may be NULL).  Lets a caller keep the rows on the device (summaries:
 * plspm_bootstrap_summary) and pay for the PCIe transfer only when individual replicates are asked for.  PLSPM_E_STATE when the
 * handle holds no records (no bootstrap yet, or a later upload replaced the data). */
int plspm_bootstrap_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status, int32_t* iters);
/* The handle's HIP stream (a hipStream_t), so that a caller can order its own work -- e.g. an RCCL collective -- behind the
 * enqueued kernels with stream/event semantics instead of a host synchronisation. */
void* plspm_stream(plspm_model_t* m);

/* Replace the handle's records by B host records [B * plspm_row_stride()] in the device layout [row | status | iterations] -- for a
 * caller that merged the shards of several processes with a transport of its own (MPI, gloo, files) and wants the device summary
 * (plspm_bootstrap_summary with d_rows = NULL) of the merged set. */
int plspm_bootstrap_store(plspm_model_t* m, const double* records, int64_t B);

/*
 * Summary statistics of a bootstrap on the device (reference _create_summary, plspm/bootstrap.py:24-32): for every result
 * column c: summary[c*6 + 0..5] = original, mean, std.error (ddof 1), perc.025, perc.975 (linear interpolation), t stat. --
 * over the replicates whose status is PLSPM_OK.
 *   d_rows   NULL: the rows of the last plspm_bootstrap(_device) call on this handle (stride = plspm_row_stride(); B must be
 *            that call's B, else PLSPM_E_ARG; PLSPM_E_STATE when the handle holds no records);
 *            else a device buffer [B * stride] in the same record layout (e.g. the all-gathered records of all GPUs);
 *            records whose status column is not exactly 0 (failed replicates, NaN-marked padding of ragged shards) are skipped
 *   B        1 <= B <= 2^30
 *   original [R] host: the full-sample estimates;  summary [R*6] host;  n_used: number of OK replicates (may be NULL)
 */
int plspm_bootstrap_summary(plspm_model_t* m, const void* d_rows, int64_t B, int32_t stride, const double* original, double* summary,
                            int64_t* n_used);

/*
 * ---- Two-group permutation test (multi-group analysis) -------------------------------------------------------------------------
 * Is an estimate different between two groups of the rows?  Permutation r (global id) splits the N uploaded rows into group a of n1 rows
 * and group b of N - n1: row i carries the key  word (i & 3) of Philox4x32-10(counter = (i >> 2, 1, lo32(r), hi32(r)), key = (lo32(seed),
 * hi32(seed)))  (the bootstrap's stream with counter word 1 = 1 instead of 0), and group a holds the n1 rows with the smallest (key, row)
 * pairs in lexicographic order -- exactly n1 rows, a function of (seed, r, N, n1) only.  Both groups are estimated like bootstrap
 * replicates (same record layout; each group's own n, treatment and `scaled` scalar from its moments), on the int8 Gram route with at
 * least seven digit planes (correctly rounded moment sums whatever the group size), whatever "gram_path" / "i8_min_batch" say.
 * Plain metric handles only (no non-metric scales, no missing values, not part of a two-stage pair): PLSPM_E_ARG otherwise; PLSPM_E_LIMIT where the int8
 * route is closed (N >= 2^24, digit planes above their budget).
 *
 * plspm_permutation_device: permutations [rep_offset, rep_offset + B), 1 <= B <= 2^29, 1 <= n1 < N.  Enqueues 2B problems: record 2p =
 *   group a of permutation rep_offset + p, record 2p + 1 = its group b; they stay on the handle as its last records (plspm_bootstrap_fetch
 *   reads them; 2B of them).  *d_out / *d_status / *d_iters as plspm_bootstrap_device.
 *   member  NULL: the splits above, drawn on the device;  else [B*N] host bytes 0/1, row p = the membership of permutation p (group a = 1),
 *           each with exactly n1 ones (test seam, like `idx` of plspm_bootstrap).
 * plspm_permutation_counts: on the handle's last 2B records (B of the last plspm_permutation_device call), per result column j
 *   exceed[j] = #{valid p : |d_pj| >= |observed_diff[j]|},  d_pj = record[2p][j] - record[2p + 1][j];  a NaN on either side counts as
 *   "not >=".  Valid: both records of the permutation have status PLSPM_OK; *n_used = their number (may be NULL).
 *   observed_diff [R] host (est_a - est_b on the observed split), exceed [R] host.
 *   p-value of this project: p_j = (1 + exceed[j]) / (1 + n_used), NaN where observed_diff[j] is NaN.
 */
int plspm_permutation_device(plspm_model_t* m, int64_t B, uint64_t seed, int64_t rep_offset, int64_t n1, const uint8_t* member, void** d_out,
                             void** d_status, void** d_iters);
int plspm_permutation_counts(plspm_model_t* m, int64_t B, const double* observed_diff, int64_t* exceed, int64_t* n_used);

/*
 * ---- Two-group bootstrap (multi-group analysis) ---------------------------------------------------------------------------------
 * Each group is bootstrapped on its own.  member [N] host bytes 0/1 (1 = group a) define the row lists rows_a, rows_b (ascending row order)
 * of n_a, n_b >= 2 rows.  Resample r (global id) makes problem s = 2r: n_a draws, draw j = rows_a[to_index(word (j & 3) of
 * Philox4x32-10(counter = (j >> 2, 2, lo32(s), hi32(s)), key = (lo32(seed), hi32(seed))), n_a)] (to_index(u, n) = (u * n) >> 32; counter word 1
 * is 2 where the bootstrap's is 0 and the permutation's 1), and problem s = 2r + 1: n_b draws from rows_b, likewise.  Both problems are
 * estimated like bootstrap replicates (each group's own n, treatment and `scaled` scalar from its moments) on the int8 Gram route with at least
 * seven digit planes, whatever "gram_path" / "i8_min_batch" say; the floor belongs to this call (a later bootstrap keeps its own planes).
 * Plain metric handles only: PLSPM_E_ARG otherwise; PLSPM_E_LIMIT where the int8 route is closed or a multiplicity exceeds 127.
 *
 * plspm_stratified_bootstrap_device: resamples [rep_offset, rep_offset + B), 1 <= B <= 2^29.  Enqueues 2B problems and waits for them: record 2p
 *   = group a of resample rep_offset + p, 2p + 1 = its group b; they stay on the handle as its last records (plspm_bootstrap_fetch reads
 *   them; plspm_bootstrap_summary on *d_out with stride 2 * row_stride summarises group a, on *d_out + row_stride group b).
 *   draws  NULL: the Philox draws above;  else [B*N] host rows (test seam): row p holds resample p's draws, entries [0, n_a) rows of group a,
 *          [n_a, N) rows of group b -- PLSPM_E_ARG when an entry is not a row of its group.
 * plspm_stratified_pair_counts: on the handle's last 2B records (B of the last stratified call), per result column j
 *   above[j] = #{(i, k) : u_a,i > u_b,k},  u_a = 2 center_a[j] - x over group a's records of status PLSPM_OK, u_b = 2 center_b[j] - x over
 *   group b's (that fp64 expression; a NaN on either side never counts).  *used_a / *used_b: the OK records of each group (may be NULL).
 *   center_a, center_b [R] host (the groups' bootstrap means for Henseler's PLS-MGA test), above [R] host.
 */
int plspm_stratified_bootstrap_device(plspm_model_t* m, int64_t B, uint64_t seed, int64_t rep_offset, const uint8_t* member, const int32_t* draws,
                                      void** d_out, void** d_status, void** d_iters);
int plspm_stratified_pair_counts(plspm_model_t* m, int64_t B, const double* center_a, const double* center_b, int64_t* above, int64_t* used_a,
                                 int64_t* used_b);

/*
 * ---- Out-of-sample prediction: repeated k-fold cross-validation (PLSpredict) ------------------------------------------------------
 * How well does the model predict rows it was not fitted on?  Repetition r (global id) cuts the N uploaded rows into k folds: row i carries the
 * key  word (i & 3) of Philox4x32-10(counter = (i >> 2, 3, lo32(r), hi32(r)), key = (lo32(seed), hi32(seed)))  (counter word 1 is 3 where the
 * bootstrap's is 0, the permutation's 1, the stratified draws' 2); the rows ordered by (key, row), the one at position j belongs to fold
 * (j * k) / N (integer division) -- a function of (seed, r, N, k) only; fold sizes differ by at most one and every row is held out exactly once per
 * repetition.  Problem q = r * k + f is the model estimated on the rows outside fold f of repetition r, like a bootstrap replicate (same record
 * layout; its own n, treatment and `scaled` scalar from its moments), on the int8 Gram route with at least seven digit planes whatever
 * "gram_path" / "i8_min_batch" say; the floor belongs to this call (a later bootstrap keeps its own planes).
 * Plain metric handles only (no non-metric scales, no missing values, not part of a two-stage pair): PLSPM_E_ARG otherwise; PLSPM_E_LIMIT where the int8 route
 * is closed (N >= 2^24, digit planes above their budget).  2 <= k <= 256, every training set of at least four rows, 1 <= reps, reps * k <= 2^29.
 *
 * plspm_cv_device: repetitions [rep_offset, rep_offset + reps).  Enqueues reps * k problems; their records stay on the handle as its last records
 *   (plspm_bootstrap_fetch reads them), beside the fold ids, the rows in fold order and the training moments of every problem, until the next
 *   bootstrap-like call or upload.  *d_out / *d_status / *d_iters as plspm_bootstrap_device.
 *   fold   NULL: the folds above, drawn on the device;  else [reps*N] host bytes (test seam): row r holds the fold id of every row in repetition r,
 *          every id below k and every fold non-empty, else PLSPM_E_ARG.
 * plspm_cv_moments: the training moments of the last plspm_cv_device call's problems (reps, k: that call's, else PLSPM_E_ARG; PLSPM_E_STATE when a later
 *   call replaced them), accumulated in fp64 on the resident rows (full sample minus fold).  Any output may be NULL.
 *   n_train [reps*k];  mean [reps*k*P] the training mean of every raw column (device column order);  cross [reps*k*P(P+1)/2] the cross-products
 *   sum (x_p - mean_p)(x_p' - mean_p') of the training rows, upper triangle by rows: (p, p'), p <= p', at p P - p (p - 1) / 2 + p' - p.
 * plspm_cv_targets: the T target indicators -- the device columns of every latent variable that has a predecessor, ascending -- into cols
 *   (may be NULL); returns T.
 * plspm_cv_predict: the errors of an affine prediction x_hat = C_q [1; x_raw] (C_q [T][P + 1], x_raw in device column order) of every problem
 *   on its held-out rows, e = x_t - x_hat_t in fp64:  sse / sae / sst [reps*k*T] = sum e^2, sum |e|, sum (x_t - training mean_t)^2;
 *   rows [reps*k] = the held-out rows the problem covered.  A problem whose matrix holds a NaN covers nothing: its sums and rows are 0.
 *   coef   NULL: the PLS prediction of each problem's own fit.  The score of latent variable l for an unseen row is the one plspm_fit's `scores`
 *          would give it under the training fit (training means, the training `scaled` scalar, the normalised weights, the fit's sign); the
 *          predicted score of an endogenous j is sum_i beta_ji y_i over its predecessors -- technique 0 ("direct antecedents"): y_i the row's own
 *          score; technique 1 ("earliest antecedents"): the predicted score where i has predecessors itself --; indicator p of j is predicted as
 *          training mean_p + loading_p sd_p * predicted score (sd_p the training rows' population standard deviation; the scores' is 1).
 *          A problem whose status is not PLSPM_OK gets a NaN matrix.
 *          else [reps*k*T*(P+1)] host: explicit matrices (the linear-model benchmark; tests); technique is ignored.
 *   pred_sum [N*T], pred_cnt [N] (both or neither): per row the sum of its predictions over the problems that covered it, and their number
 *          (added up by atomics: the order of the repetitions' terms is not fixed).
 *   PLSPM_E_LIMIT when the model has more than 256 targets, or its matrix -- (P + 1) x T doubles beside a tile of 16 rows -- does not fit the
 *   160 KiB of LDS (128 targets among 128 columns fit).
 */
int plspm_cv_device(plspm_model_t* m, int64_t reps, int32_t k, uint64_t seed, int64_t rep_offset, const uint8_t* fold, void** d_out, void** d_status,
                    void** d_iters);
int plspm_cv_moments(plspm_model_t* m, int64_t reps, int32_t k, double* n_train, double* mean, double* cross);
int plspm_cv_targets(plspm_model_t* m, int32_t* cols);
int plspm_cv_predict(plspm_model_t* m, int64_t reps, int32_t k, int32_t technique, const double* coef, double* sse, double* sae, double* sst,
                     int64_t* rows, double* pred_sum, int32_t* pred_cnt);

/*
 * ---- Jackknife (delete-one / delete-a-group) ------------------------------------------------------------------------------------
 * Problem g of G (2 <= G <= N) is the model estimated on the rows i with i % G != g: G = N is the ordinary leave-one-out jackknife, G < N the
 * delete-a-group jackknife (group sizes differ by at most one; every problem keeps at least four rows, else PLSPM_E_ARG).  Problems are estimated
 * like bootstrap replicates (same record layout; each problem's own n, treatment and `scaled` scalar from its moments) on the int8 Gram route with
 * at least seven digit planes whatever "gram_path" / "i8_min_batch" say; the floor belongs to this call (a later bootstrap keeps its own planes).
 * Plain metric handles only (no non-metric scales, no missing values, not part of a two-stage pair): PLSPM_E_ARG otherwise; PLSPM_E_LIMIT where
 * the int8 route is closed (N >= 2^24, digit planes above their budget).
 *
 * plspm_jackknife_device: enqueues the G problems.  Their records, status and iteration counts live in buffers of their own: the records of the
 *   handle's last bootstrap-like call (plspm_bootstrap_fetch / _summary / _intervals), its status and its iteration counts are untouched, bit
 *   for bit.  *d_out [G * plspm_row_stride()] / *d_status / *d_iters [G]: device pointers owned by the handle, valid until the next
 *   plspm_jackknife_device or upload (any may be NULL).
 * plspm_jackknife_fetch: host copy of problems [first, first + count) of the last plspm_jackknife_device call: out [count*R], status, iters
 *   [count] (any may be NULL).  PLSPM_E_STATE without a jackknife on the handle.
 * plspm_jackknife_stats: per record column over the n problems of status PLSPM_OK (G: the last plspm_jackknife_device call's, else PLSPM_E_ARG;
 *   PLSPM_E_STATE without one), every sum in one fixed order (bit-reproducible), with d_g = mean - theta_(g):
 *     mean = sum theta_(g) / n,   std_error = sqrt((n - 1) / n  sum d_g^2),   accel = sum d_g^3 / (6 (sum d_g^2)^1.5)  (NaN where sum d_g^2 = 0)
 *   mean, std_error, accel [R] host (any may be NULL); *n_used = n (may be NULL); n = 0: every output NaN.
 */
int plspm_jackknife_device(plspm_model_t* m, int64_t G, void** d_out, void** d_status, void** d_iters);
int plspm_jackknife_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status, int32_t* iters);
int plspm_jackknife_stats(plspm_model_t* m, int64_t G, double* mean, double* std_error, double* accel, int64_t* n_used);

/*
 * ---- FIMIX-PLS (latent-class segmentation of the inner model) --------------------------------------------------------------------
 * A finite mixture of inner-model regressions on the latent variable scores the last plspm_fit left on the handle (Y [N x L]).  With E the
 * LVs that have predecessors (n_endo), pred(j) the predecessors of j and n_dir the number of direct paths, segment k of a problem of K segments models
 *     y_ij = sum_{p in pred(j)} beta_kjp y_ip + e,   e ~ N(0, psi_kj)                       (no intercept; recursive model: Jacobian 1)
 * and one problem is (K, an initial hard assignment of the rows to the K segments).  Iteration t = 1, 2, ...:
 *   M-step on P^(t-1) (P^0: one-hot of the assignment): n_k = sum_i P_ik, rho_k = n_k / N, m_k[a,b] = sum_i P_ik y_ia y_ib; beta_kj solves
 *     m_k[pred,pred] beta = m_k[pred,j] by the library's regression (pivot rule, minimum-norm answer for collinear predecessors);
 *     psi_kj = (m_k[j,j] - beta_kj . m_k[pred,j]) / n_k.  The problem ends with PLSPM_SINGULAR at that t when an n_k < 1, a psi_kj <= 1e-10 m_k[j,j] / n_k
 *     or a regression without an answer: its record is NaN.
 *   E-step: a_ik = ln rho_k + sum_j [-1/2 ln(2 pi psi_kj) - r_ikj^2 / (2 psi_kj)], lse_i the log-sum-exp over k (row maximum subtracted),
 *     lnL = sum_i lse_i, P_ik = exp(a_ik - lse_i), H = -sum_ik P_ik ln P_ik (0 ln 0 = 0).  PLSPM_NONFINITE (NaN record) when lnL is not finite.
 *   Stop: PLSPM_OK when t >= 2 and |lnL^t - lnL^(t-1)| <= tol; PLSPM_NOT_CONVERGED at t = max_iter with the complete record of that t (tol = 0 runs
 *     exactly max_iter iterations).
 * Record, plspm_fimix_width() = 2 + kmax (1 + n_dir + n_endo) doubles:  lnL | H | rho[kmax] | beta[kmax][n_dir] | psi[kmax][n_endo]  -- beta in the
 * direct-path order of plspm_structural_paths (from-major), psi in LV order, segments in the order the EM left them, NaN in the slots k >= K.
 * Every sum runs in one fixed order: a call repeated on the same inputs gives the same bits.  Plain metric handles only (no non-metric scales, no
 * missing values, not part of a two-stage pair): PLSPM_E_ARG otherwise.
 *
 * plspm_fimix_device: enqueues nprob problems, one workgroup each; k_of [nprob] host, 1..16; kmax >= every K (and <= 16); init [nprob*N] host, the segment
 *   of every row (below its problem's K, else PLSPM_E_ARG), or NULL: row i of problem s goes to segment floor(u K) of the Philox draw keyed by
 *   (seed, start_offset + s, i) (plspm_fimix_starts).  max_iter >= 1, tol >= 0.  PLSPM_E_STATE when the handle holds no scores of a fit on the rows now
 *   resident (plspm_fit with `scores`; an upload voids them); PLSPM_E_LIMIT when one problem's state exceeds a workgroup's 160 KiB of LDS.
 *   *d_out [nprob * (width + 2)] (values | status | iterations) / *d_status / *d_iters [nprob]: device pointers owned by the handle, valid until the
 *   next plspm_fimix_device or upload (any may be NULL).
 * plspm_fimix_fetch: host copy of problems [first, first + count) of the last call: out [count*width], status, iters [count] (any may be NULL).
 * plspm_fimix_posteriors: the posteriors P [N x K] of one stored problem's parameters (row-major), out [N*K] host.
 * PLSPM_E_STATE from the last two without a call on the handle (none yet; an upload voids it).
 */
int plspm_fimix_device(plspm_model_t* m, int64_t nprob, const int32_t* k_of, int32_t kmax, uint64_t seed, int64_t start_offset, const uint8_t* init, int32_t max_iter,
                       double tol, void** d_out, void** d_status, void** d_iters);
int32_t plspm_fimix_width(const plspm_model_t* m, int32_t kmax);
int plspm_fimix_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status, int32_t* iters);
int plspm_fimix_posteriors(plspm_model_t* m, int64_t problem, double* out);

/*
 * ---- REBUS-PLS (response-based unit segmentation) -------------------------------------------------------------------------------
 * Classes of rows that differ in their outer AND inner model (Esposito Vinzi, Trinchera, Squillacciotti and Tenenhaus 2008).  This library's
 * definitions; equality with R's rebus.pls is not claimed.  Inputs: the N uploaded rows, K classes (1..16), labels c^0 [N] below K.  Iteration t = 1, 2, ...:
 *   local models   problem k = the model on the rows with c^(t-1) = k, estimated like a bootstrap replicate (same record layout; its own n_k, treatment and `scaled`
 *                  scalar) on the int8 route with at least seven digit planes; mean_pk, sd_pk the population mean and sd of column p over the class's rows
 *   residuals      of every row i under every class k: y_ilk the score plspm_fit's `scores` would give row i under class k's fit (plspm_cv_predict's rule: class
 *                  means, the class's `scaled` scalar, the record's weights, the fit's sign); z_ipk = (x_ip - mean_pk) / sd_pk; e_ipk = z_ipk - lambda_pk y_i,lv(p),k
 *                  (lambda: the record's loading); f_ijk = y_ijk - sum_{q in pred(j)} beta_kjq y_iqk for every LV j with predecessors;
 *                  A_ik = sum_p e_ipk^2 / lambda_pk^2, B_ik = sum_j f_ijk^2 / R^2_jk
 *   closeness      CM_ik = sqrt( A_ik / (sum_i A_ik / (N - 2)) * B_ik / (sum_i B_ik / (N - 2)) ), both sums over all N rows
 *   assignment     c^t_i = argmin_k CM_ik (ties: the lowest k; a NaN never wins; a row whose every CM is NaN keeps its class); changed_t = #{i : c^t_i != c^(t-1)_i}
 *   stop           PLSPM_OK when changed_t / N < stop_crit; PLSPM_NOT_CONVERGED at t = max_iter (max_iter = 0: no iteration, the final pass on c^0);
 *                  PLSPM_SINGULAR at iteration t when a class has fewer than min_size rows, a local fit is not PLSPM_OK, an sd_pk is 0, or a lambda_pk^2 or an
 *                  R^2_jk is not above 1e-10: the labels stay c^(t-1)
 *   final pass     local models, residuals and closeness once more on c^t, without reassigning: the reported records and CM, and per class the within-class sums
 *                  sum_{i in k} e_ipk^2 [P] and sum_{i in k} f_ijk^2 [n_endo].  The same checks; PLSPM_SINGULAR there as well.  Skipped after PLSPM_SINGULAR:
 *                  labels and history stay, every other output is NaN (status and iteration counts of the local records: -1).
 * Every floating-point sum runs in one fixed order: a repeated call gives the same bits.  Plain metric handles whose every block is Mode A and whose model has a
 * path: PLSPM_E_ARG otherwise, as for K outside 1..16 or a start label that is not below K; PLSPM_E_STATE without data; PLSPM_E_LIMIT where the int8 route is
 * closed or one class's parameters exceed a workgroup's 160 KiB of LDS.  The handle's bootstrap records survive the call bit for bit.
 *
 * plspm_rebus_device: runs the iteration (host-driven, one host wait per iteration: changed_t, the sizes and the validity flags; the labels stay on the device).
 *   start [N] host.  *d_labels [N] int32 / *d_cm [N * K] (NULL after PLSPM_SINGULAR): device pointers owned by the handle, valid until the next plspm_rebus_*
 *   call or upload (either may be NULL).  Returns 0 whatever the run's status.
 * plspm_rebus_fetch: of the last run -- labels [N]; cm [N * K] row-major; records [K * plspm_row_width()], rec_status, rec_iters [K]; sizes [K] of the labels;
 *   within_e [K * P] (device column order), within_f [K * n_endo] (LV order); run [3] = status, iterations, h = iterations whose counters are history (h =
 *   iterations, or iterations - 1 where the iteration itself ended PLSPM_SINGULAR); hist_changed [h], hist_sizes [h * K].  Any may be NULL; the caller sizes the
 *   last two by max_iter.  PLSPM_E_STATE without a run (none yet; an upload or plspm_rebus_residuals voids it).
 * plspm_rebus_residuals: e and f of every row under the one-class model (K = 1, every row in class 0): out [N * (P + n_endo)] host, row-major, e in device column
 *   order then f in LV order; NaN where that model is not valid.  Needs no prior run.
 */
int plspm_rebus_device(plspm_model_t* m, int32_t K, const int32_t* start, int32_t max_iter, double stop_crit, int64_t min_size, void** d_labels, void** d_cm);
int plspm_rebus_fetch(plspm_model_t* m, int32_t* labels, double* cm, double* records, int32_t* rec_status, int32_t* rec_iters, int64_t* sizes, double* within_e, double* within_f,
                      int32_t* run, int32_t* hist_changed, int32_t* hist_sizes);
int plspm_rebus_residuals(plspm_model_t* m, double* out);

/*
 * ---- Bootstrap confidence intervals ---------------------------------------------------------------------------------------------
 * Two-sided intervals at a chosen level on bootstrap records in HBM, every handle kind; d_rows / B / stride as plspm_bootstrap_summary (NULL: the
 * handle's last records; else a device buffer in the record layout, e.g. the gathered records of all GPUs).  Per result column c over the m
 * replicates of status PLSPM_OK:  out[c*6 + 0..5] = lower, upper, z0, accel, level.lower, level.upper.
 * With alpha = (1 - level) / 2 and 1 - alpha = (1 + level) / 2, both rounded to twelve decimals (level 0.95 gives exactly 0.025 and 0.975), q(p) the
 * quantile by numpy's linear interpolation at position p (m - 1) -- plspm_bootstrap_summary's rule --, theta the column's `original`:
 *   method 0 percentile  lower = q(alpha), upper = q(1 - alpha)          (level 0.95: perc.025 / perc.975 of the summary, bit for bit)
 *          1 basic       lower = 2 theta - q(1 - alpha), upper = 2 theta - q(alpha)
 *          2 bc          as bca with a = 0
 *          3 bca         z0 = Phi^-1(#{theta* < theta} / m) (strict inequality); lower = q(p_lo), upper = q(p_hi),
 *                        p = Phi(z0 + (z0 + z) / (1 - a (z0 + z))) for z = Phi^-1(alpha), Phi^-1(1 - alpha); a = accel[c] (plspm_jackknife_stats)
 * level.lower / level.upper: the two levels the quantiles were taken at.  z0 is reported by every method; accel is NaN for methods 0 and 1, 0 for 2.
 * NaN: all six where m = 0 or original[c] is NaN; lower, upper and both levels of bc / bca where the proportion is 0 or 1 (z0 is -inf / +inf there:
 * constant columns such as absent paths); lower, upper, accel and both levels of bca where accel[c] is NaN.
 *   original [R] host;  accel [R] host, NULL unless method 3 (then PLSPM_E_ARG);  0 < level < 1;  out [R*6] host;  n_used: m (may be NULL)
 */
int plspm_bootstrap_intervals(plspm_model_t* m, const void* d_rows, int64_t B, int32_t stride, const double* original, const double* accel,
                              int32_t method, double level, double* out, int64_t* n_used);

/*
 * ---- Measurement-model assessment of the bootstrap ------------------------------------------------------------------------------
 * Reliability and discriminant validity of every replicate, computed on the device from the replicate's moment matrix -- which exists only between the
 * Gram and the next pass -- and the weights w and loadings lambda of its record (one more kernel behind the solver).  With n, the column
 * sums and the cross products M of a replicate:  c_pq = M_pq / n - mu_p mu_q,  s_p = sqrt(c_pp),  r_pq = c_pq / (s_p s_q);  v_p = w_p s_p, normalised per
 * block so that v_b' R_bb v_b = 1 (the `scaled` scalar cancels);  u_p = sum_{q in block(p)} r_pq v_q;  sigma_l = sign(sum_{p in l} u_p lambda_p), +1 for 0.
 *   per LV l of k items (k = 1: all four are 1)
 *     alpha   max(0, k / (k - 1) * 2 sum_{i>j} r_ij / sum_ij r_ij)
 *     rho_a   Mode A: (v'v)^2 v'(R_bb - I)v / ((v'v)^2 - sum v_p^4)  (Dijkstra-Henseler);  Mode B: 1
 *     rho_c   (sum lambda)^2 / ((sum lambda)^2 + sum (1 - lambda^2))
 *     ave     sum lambda^2 / k
 *   per LV pair (i, j), i < j, i-major; npairs = L (L - 1) / 2
 *     htmt    mean_{p in i, q in j} |r_pq| / sqrt(m_i m_j),  m_l = mean of |r_pq| over p < q in block l (1 for a single item)
 *     htmt2   the same with geometric means (exp of the mean log; a zero correlation gives 0)
 *     lv_cor  sigma_i sigma_j v_i' R_ij v_j
 * Assessment record, width A = 4 L + 3 npairs:  alpha[L] | rho_a[L] | rho_c[L] | ave[L] | htmt[npairs] | htmt2[npairs] | lv_cor[npairs];  device records
 * carry the replicate's status and iteration count behind it as doubles (pitch A + 2).  A replicate whose status is not PLSPM_OK has NaN in all A values;
 * IEEE results stand where a formula divides by zero.  Plain metric handles only (no non-metric scales, no missing values, not part of a two-stage pair):
 * PLSPM_E_ARG otherwise.
 *
 * plspm_assess_enable: on != 0: every later plspm_bootstrap / plspm_bootstrap_device call on this handle also writes the assessment records of its
 *   replicates into a buffer of their own, indexed like the bootstrap's records; the bootstrap's records, status and iteration counts are bit for bit
 *   what they are without it.  Off (the default): no launch, no allocation.  Permutation, stratified, cross-validation, jackknife and group calls write
 *   none.
 * plspm_assess_width: A.
 * plspm_assess_fit: the full-sample values, out [A]: the same kernel on the moments of all uploaded rows and one solver problem (plspm_fit's); *status (may
 *   be NULL): that problem's status.  Needs no plspm_assess_enable.
 * plspm_assess_fetch: host copy of the assessment records [first, first + count) of the last assessed bootstrap: out [count*A], status [count] (may be NULL).
 * plspm_assess_summary / plspm_assess_intervals: plspm_bootstrap_summary / plspm_bootstrap_intervals on the assessment records (B: the last assessed
 *   bootstrap's, else PLSPM_E_ARG): original [A] host, summary / out [A*6] host, *n_used (may be NULL).  Methods 0 (percentile), 1 (basic), 2 (bc); 3 (bca)
 *   is PLSPM_E_ARG: the jackknife writes no assessment records.
 * PLSPM_E_STATE from the last three without assessment records on the handle (none written yet; an upload, or a later call that replaced the bootstrap's
 * records, voids them).
 */
int plspm_assess_enable(plspm_model_t* m, int32_t on);
int32_t plspm_assess_width(const plspm_model_t* m);
int plspm_assess_fit(plspm_model_t* m, double* out, int32_t* status);
int plspm_assess_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status);
int plspm_assess_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used);
int plspm_assess_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used);

/*
 * ---- Consistent PLS (PLSc) of the bootstrap -------------------------------------------------------------------------------------
 * Dijkstra and Henseler's (2015) correction for attenuation, for every replicate: one more kernel behind the assessment kernel.  From the
 * assessment's quantities of a data set -- the normalised standardised weights v (v_l' R_ll v_l = 1), the fit's sign sigma_l, rho_a[l] and the signed construct
 * correlations lv_cor_ij -- and a factor mask (which LVs are common factors; default: every Mode-A block of two items or more):
 *     Q_l       rho_a[l] for a factor, 1 otherwise
 *     rc_ij     lv_cor_ij / sqrt(Q_i Q_j) for i != j, rc_ii = 1                      the corrected construct correlations
 *     inner model: the solver's own, on rc in place of the score covariance -- per endogenous LV the normal equations on its predecessors (the same pivot
 *               rule, the same minimum-norm fallback), R2_j = beta' rc_pj, indirect effects by forward substitution, total = direct + indirect on the
 *               pairs of plspm_effect_pairs.  With an all-zero mask this is the bootstrap record up to rounding.
 *     loadings  factor l: sigma_l v_p sqrt(Q_l) / (v_l' v_l); any other LV: the record's.  Weights: the record's.
 * PLSc record, width W = R + npairs (R = plspm_row_width, npairs = L (L - 1) / 2):  weights[P] | r2[L] | total[n_eff] | direct[n_eff] | loadings[P] |
 * lv_cor_c[npairs] (i < j, i-major);  device records carry a status and the replicate's iteration count behind it as doubles (pitch W + 2).  A replicate whose
 * bootstrap status is not PLSPM_OK keeps that status and has NaN in all W values.  PLSPM_INADMISSIBLE (NaN in all W values, not counted in n_used): a factor's
 * rho_a is not finite or <= 0, or some |rc_ij| is not below 1 (a NaN included).  PLSPM_SINGULAR: a regression the shared routine reports as failed (the
 * values stand, as in the solver).  Plain metric handles only (no non-metric scales, no missing values, not part of a two-stage pair): PLSPM_E_ARG otherwise.
 *
 * plspm_plsc_enable: on != 0: every later plspm_bootstrap / plspm_bootstrap_device call on this handle also writes the PLSc records of its replicates into a
 *   buffer of their own, indexed like the bootstrap's records -- and the assessment records as well (the PLSc kernel reads them), whether or not
 *   plspm_assess_enable was called; the bootstrap's records, status and iteration counts, and the assessment records, are bit for bit what they are without
 *   it.  factor [L] of 0 / 1, or NULL for the default mask; naming a Mode-B or single-item LV as a factor is PLSPM_E_ARG.  Off (the default): no launch, no
 *   allocation.  Permutation, stratified, cross-validation, jackknife and group calls write none.
 * plspm_plsc_width: W.
 * plspm_plsc_fit: the full-sample record, out [W]: the same two kernels on the moments of all uploaded rows and one solver problem (plspm_fit's), with the mask
 *   of the last plspm_plsc_enable (the default mask if there was none); *status (may be NULL): the record's status.
 * plspm_plsc_fetch: host copy of the PLSc records [first, first + count) of the last PLSc bootstrap: out [count*W], status [count] (may be NULL).
 * plspm_plsc_summary / plspm_plsc_intervals: plspm_bootstrap_summary / plspm_bootstrap_intervals on the PLSc records (B: that bootstrap's, else PLSPM_E_ARG):
 *   original [W] host, summary / out [W*6] host, *n_used (may be NULL).  Methods 0 (percentile), 1 (basic), 2 (bc); 3 (bca) is PLSPM_E_ARG: the jackknife
 *   writes no PLSc records.
 * PLSPM_E_STATE from the last three without PLSc records on the handle (none written yet; an upload, or a later call that replaced the bootstrap's records,
 * voids them; a jackknife leaves them alone).
 */
int plspm_plsc_enable(plspm_model_t* m, int32_t on, const uint8_t* factor /*[L] or NULL = default mask*/);
int32_t plspm_plsc_width(const plspm_model_t* m);
int plspm_plsc_fit(plspm_model_t* m, double* out, int32_t* status);
int plspm_plsc_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status);
int plspm_plsc_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used);
int plspm_plsc_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used);

/*
 * ---- Model fit of the bootstrap: SRMR and d_ULS ----------------------------------------------------------------------------------
 * The discrepancy between a data set's indicator correlations r_pq and the correlations its own model implies, for every replicate: one more kernel behind
 * the PLSc kernel.  From the replicate's PLSc record -- lambda*_p its loadings (a factor's corrected, any other LV's the fit's), rc_ij its
 * construct correlations, beta_jm its direct effects -- and the handle's factor mask (the one plspm_plsc_enable sets):
 *     Phi       saturated model: rc.  Estimated model, LVs in path order:  Phi_jj = 1;  j, k both without predecessors: rc_jk;  j with predecessors, every
 *               k < j: sum_{m in pred(j)} beta_jm Phi_mk in ascending j (the structural residual of j is uncorrelated with everything before it);  j without,
 *               an earlier k with predecessors: sum_{m in pred(k)} beta_km Phi_jm in ascending k
 *     sigma_pq  p, q in blocks i != j: lambda*_p Phi_ij lambda*_q;  p != q in one block: lambda*_p lambda*_q for a factor, r_pq itself for a composite (Mode A
 *               outside the mask, every Mode-B block: a composite reproduces its own block);  sigma_pp = 1
 *     d_uls     sum_{p<q} (r_pq - sigma_pq)^2 = 1/2 ||R - Sigma||_F^2            srmr   sqrt(2 d_uls / (P (P + 1)))
 * Model-fit record, width 4:  srmr_sat | d_uls_sat | srmr_est | d_uls_est;  device records carry a status and the replicate's iteration count behind it as
 * doubles (pitch 6).  A replicate whose bootstrap status is not PLSPM_OK keeps that status and has NaN in all four.  Otherwise the status is the PLSc
 * record's; PLSPM_INADMISSIBLE (NaN in all four, not counted in n_used) where that record is inadmissible, where a column is constant in the replicate, and
 * where a value is not finite.  Plain metric handles only: PLSPM_E_ARG otherwise.
 *
 * plspm_modelfit_enable: on != 0: every later plspm_bootstrap / plspm_bootstrap_device call on this handle also writes the model-fit records of its replicates
 *   into a buffer of their own, indexed like the bootstrap's records -- and the assessment and PLSc records as well, whether or not their own switches are on;
 *   all of those, and the bootstrap's records, status and iteration counts, are bit for bit what they are without it.  factor [L] of 0 / 1 sets the handle's
 *   factor mask as plspm_plsc_enable does (the same argument errors); NULL keeps the mask the handle has (the default mask if none was ever set); an all-zero
 *   mask is the plain composite model.  Off (the default): no launch, no allocation.  Permutation, stratified, cross-validation, jackknife and group calls
 *   write none.
 * plspm_modelfit_width: 4.
 * plspm_modelfit_fit: the full-sample record, out [4]: the same three kernels on the moments of all uploaded rows and one solver problem (plspm_fit's);
 *   *status (may be NULL): the record's status.
 * plspm_modelfit_fetch: host copy of the records [first, first + count) of the last model-fit bootstrap: out [count*4], status [count] (may be NULL).
 * plspm_modelfit_summary / plspm_modelfit_intervals: plspm_bootstrap_summary / plspm_bootstrap_intervals on the model-fit records (B: that bootstrap's, else
 *   PLSPM_E_ARG): original [4] host, summary / out [4*6] host, *n_used (may be NULL).  Methods 0 (percentile), 1 (basic), 2 (bc); 3 (bca) is PLSPM_E_ARG.
 * PLSPM_E_STATE from the last three without model-fit records on the handle (none written yet; whatever voids the PLSc records voids these; a jackknife leaves
 * them alone).
 */
int plspm_modelfit_enable(plspm_model_t* m, int32_t on, const uint8_t* factor /*[L] or NULL = keep the handle's mask*/);
int32_t plspm_modelfit_width(const plspm_model_t* m);
int plspm_modelfit_fit(plspm_model_t* m, double* out, int32_t* status);
int plspm_modelfit_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status);
int plspm_modelfit_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used);
int plspm_modelfit_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used);

/*
 * ---- model fit: the geodesic discrepancy d_G ------------------------------------------------------------------------------------
 * The third discrepancy of the family, for every replicate of a plain bootstrap: one more kernel behind the model-fit kernel, which needs the replicate's
 * indicator correlations while they are on the device.  This library's definition, with the quantities of the model-fit records above:
 *     d_G(Sigma) = 1/2 sum_{k=1..P} (ln phi_k)^2,  phi_k the eigenvalues of R^-1 Sigma -- those of the symmetric G^-1 Sigma G^-T with R = G G' (Cholesky)
 * Geodesic record, width 2:  d_g_sat | d_g_est;  device records carry a status and the replicate's iteration count behind it as doubles (pitch 4).  A
 * replicate whose bootstrap status is not PLSPM_OK keeps that status and has NaN in both.  Otherwise the status is the model-fit record's; PLSPM_INADMISSIBLE
 * (NaN in both, not counted in n_used) where that record is inadmissible, and in this record only where a Cholesky pivot of R is not above 1e-12, where an
 * eigenvalue phi_k of either model is not positive (Sigma is not positive definite), and where a value is not finite.  Plain metric handles only:
 * PLSPM_E_ARG otherwise; PLSPM_E_LIMIT from the call that launches the kernel where one replicate's two P x P triangles exceed a workgroup's 160 KiB of LDS.
 *
 * plspm_geodesic_enable: on != 0: every later plspm_bootstrap / plspm_bootstrap_device call on this handle also writes the geodesic records of its replicates
 *   into a buffer of their own, indexed like the bootstrap's records -- and the assessment, PLSc and model-fit records as well, whether or not their own
 *   switches are on; all of those, and the bootstrap's records, status and iteration counts, are bit for bit what they are without it.  factor: exactly
 *   plspm_modelfit_enable's (the handle has one factor mask).  Off (the default): no launch, no allocation.  Permutation, stratified, cross-validation,
 *   jackknife and group calls write none.
 * plspm_geodesic_width: 2.
 * plspm_geodesic_fit: the full-sample record, out [2]: the same four kernels on the moments of all uploaded rows and one solver problem (plspm_fit's);
 *   *status (may be NULL): the record's status.
 * plspm_geodesic_fetch: host copy of the records [first, first + count) of the last geodesic bootstrap: out [count*2], status [count] (may be NULL).
 * plspm_geodesic_summary / plspm_geodesic_intervals: plspm_bootstrap_summary / plspm_bootstrap_intervals on the geodesic records (B: that bootstrap's, else
 *   PLSPM_E_ARG): original [2] host, summary / out [2*6] host, *n_used (may be NULL).  Methods 0 (percentile), 1 (basic), 2 (bc); 3 (bca) is PLSPM_E_ARG.
 * PLSPM_E_STATE from the last three without geodesic records on the handle (none written yet; whatever voids the PLSc records voids these; a jackknife leaves
 * them alone).
 */
int plspm_geodesic_enable(plspm_model_t* m, int32_t on, const uint8_t* factor /*[L] or NULL = keep the handle's mask*/);
int32_t plspm_geodesic_width(const plspm_model_t* m);
int plspm_geodesic_fit(plspm_model_t* m, double* out, int32_t* status);
int plspm_geodesic_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status);
int plspm_geodesic_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used);
int plspm_geodesic_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used);

/*
 * ---- Structural-model assessment of the bootstrap -------------------------------------------------------------------------------
 * The f2 effect size and the inner VIF of every direct path, and every specific indirect effect, for every replicate: one more kernel behind the assessment
 * kernel, beside PLSc and what follows it.  This library's definitions, for one data set: rc [L x L] its construct correlation matrix -- the
 * assessment record's signed lv_cor, diagonal 1 --, pred(j) the predecessors of LV j, and R2(j | S) the R squared of regressing j on the LVs in S on rc with the
 * solver's own regression (Cholesky pivots above 1e-13 of the diagonal, else the minimum-norm solution; R2 = beta' rc_Sj; exactly 0 for an empty S).
 *   per direct path i -> j, in the order of plspm_effect_pairs restricted to the pairs with a path of their own, with S = pred(j) without i
 *     f2        (R2(j | pred(j)) - R2(j | S)) / (1 - R2(j | pred(j)))
 *     vif       1 / (1 - R2(i | S))                                         (exactly 1 for an empty S)
 *   per specific indirect effect -- a directed chain i -> m_1 -> ... -> j with at least one mediator --, ordered by effect pair, then lexicographically by
 *   node sequence
 *     specific  the product of the replicate's own `direct` entries along the chain, multiplied left to right
 * Structural record, width S = 2 n_dir + n_spec:  f2[n_dir] | vif[n_dir] | specific[n_spec];  device records carry a status and the replicate's iteration count
 * behind it as doubles (pitch S + 2).  A replicate whose bootstrap status is not PLSPM_OK keeps that status and has NaN in all S values.  Otherwise
 * PLSPM_SINGULAR where a regression reports failure and PLSPM_NONFINITE where an f2 or vif is not finite (an R squared of 1); the values stand.  Plain metric
 * handles only (no non-metric scales, no missing values, not part of a two-stage pair): PLSPM_E_ARG otherwise.  A path model with more than 4,096 specific
 * indirect effects is PLSPM_E_LIMIT from the first of these calls that lists them (the chains are counted before they are enumerated; the message names the
 * count), and so is a model whose rc and one regression's scratch exceed a workgroup's 160 KiB of LDS.
 *
 * plspm_structural_enable: on != 0: every later plspm_bootstrap / plspm_bootstrap_device call on this handle also writes the structural records of its
 *   replicates into a buffer of their own, indexed like the bootstrap's records -- and the assessment records, which the kernel reads, whether or not
 *   plspm_assess_enable was called.  The stage is a branch behind the assessment: it runs whether or not PLSc, model fit and the geodesic discrepancy do, and
 *   the records of all of those, the assessment records and the bootstrap's records, status and iteration counts are bit for bit what they are without it.
 *   Off (the default): no launch, no allocation.  Permutation, stratified, cross-validation, jackknife and group calls write none.
 * plspm_structural_width: S (0 before the paths were listed: plspm_structural_enable, plspm_structural_paths or plspm_structural_fit).
 * plspm_structural_paths: the direct paths and the chains in record order: *n_dir, dir_from [n_dir], dir_to [n_dir], *n_spec, chain_off [n_spec + 1] (offsets
 *   into chain_nodes), chain_nodes [chain_off[n_spec]] (every chain's LVs from its first to its last).  Any pointer may be NULL: ask for the sizes first
 *   (chain_off alone gives the length of chain_nodes).
 * plspm_structural_fit: the full-sample record, out [S]: the same two kernels on the moments of all uploaded rows and one solver problem (plspm_fit's); *status
 *   (may be NULL): the record's status.  Needs no plspm_structural_enable.
 * plspm_structural_fetch: host copy of the records [first, first + count) of the last structural bootstrap: out [count*S], status [count] (may be NULL).
 * plspm_structural_summary / plspm_structural_intervals: plspm_bootstrap_summary / plspm_bootstrap_intervals on the structural records (B: that bootstrap's,
 *   else PLSPM_E_ARG): original [S] host, summary / out [S*6] host, *n_used (may be NULL).  Methods 0 (percentile), 1 (basic), 2 (bc); 3 (bca) is PLSPM_E_ARG:
 *   the jackknife writes no structural records.
 * PLSPM_E_STATE from the last three without structural records on the handle (none written yet; whatever voids the assessment records voids these; a jackknife
 * leaves them alone).
 */
int plspm_structural_enable(plspm_model_t* m, int32_t on);
int32_t plspm_structural_width(const plspm_model_t* m);
int plspm_structural_paths(plspm_model_t* m, int32_t* n_dir, int32_t* dir_from, int32_t* dir_to, int32_t* n_spec, int32_t* chain_off, int32_t* chain_nodes);
int plspm_structural_fit(plspm_model_t* m, double* out, int32_t* status);
int plspm_structural_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status);
int plspm_structural_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used);
int plspm_structural_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used);

/* Moderation analysis by the two-stage approach (this project's definitions, csrc/moderation_core.h): does the effect of a predictor LV a on a
 * target LV j depend on a moderator LV b?  A term is (a, b, j), three different LVs with the paths a -> j and b -> j in the model.  Stage 1 is the model as it
 * stands.  Per data set (the full sample, or one replicate with its row multiplicities) the stage-1 scores y_l are those of the record's weights by the
 * assessment's conventions (v normalised per block, the sign rule; mean 0, variance 1), the product z_t = y_a y_b is neither centred nor rescaled, and every
 * target that has terms is regressed on its predecessors (LV order) and then its terms (term order) on the correlation matrix of those scores and products, by
 * the library's own regression.  The products of a replicate need a pass over the rows: four kernels behind the metric solver of every pass.
 * Record, width W = n_dir + 4 T + L:  direct2 [n_dir] (the order of plspm_structural_paths) | interaction [T] | f2 [T] (dropping the term alone) |
 * slope_low [T] | slope_high [T] (direct2[a -> j] -/+ interaction: the simple slope one SD below / above the moderator's mean) | r2 [L]; status and iterations
 * behind it as doubles (pitch W + 2).  A target without terms keeps the bootstrap record's direct and r2 entries bit for bit.  A replicate whose bootstrap status
 * is not PLSPM_OK keeps that status and has NaN in all W values; otherwise PLSPM_SINGULAR where a regression reports failure and PLSPM_NONFINITE where a value
 * is not finite (a product without variance, an R squared of 1); the values stand.  Plain metric handles only: PLSPM_E_ARG otherwise.
 *
 * plspm_moderation_enable: n_terms > 0: the terms (LV indices; at most 8, no two with the same pair and target) -- every later plspm_bootstrap /
 *   plspm_bootstrap_device call on this handle also writes the moderation records of its replicates into a buffer of their own, indexed like the bootstrap's
 *   records; the bootstrap's records, status and iteration counts and every derived record are bit for bit what they are without it.  n_terms = 0: off (the
 *   default): no launch, no allocation.  PLSPM_E_ARG for a term outside the definitions (the message names it); PLSPM_E_LIMIT for more than 65,535 uploaded rows
 *   (the row multiplicities are one LDS histogram of 16-bit counters; also raised at the start of a call, before anything of it runs), for more than 128 row
 *   sums per replicate, and for a model whose workspaces exceed a workgroup's 160 KiB of LDS.  Permutation, stratified, cross-validation, jackknife and group
 *   calls write none.
 * plspm_moderation_width: W (0 before the first plspm_moderation_enable with terms).
 * plspm_moderation_fit: the full-sample record, out [W]: the same kernels on one problem with every multiplicity 1; *status (may be NULL): the record's status.
 * plspm_moderation_fetch / _summary / _intervals: as plspm_structural_fetch / _summary / _intervals, on the moderation records.
 * PLSPM_E_STATE from the last three without moderation records on the handle (whatever voids the assessment records voids these; a jackknife leaves them alone).
 */
int plspm_moderation_enable(plspm_model_t* m, int32_t n_terms, const int32_t* predictor, const int32_t* moderator, const int32_t* target);
int32_t plspm_moderation_width(const plspm_model_t* m);
int plspm_moderation_fit(plspm_model_t* m, double* out, int32_t* status);
int plspm_moderation_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status);
int plspm_moderation_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used);
int plspm_moderation_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used);

/* Confirmatory tetrad analysis (CTA-PLS; this project's definitions, csrc/tetrad_core.h): is a block reflective at all?  Under a one-factor
 * reflective model every tetrad tau(a, b, c, d) = x_ab x_cd - x_ac x_bd of four items of the block vanishes, x the items' correlations (matrix 0, the
 * assessment's r_pq) or covariances c_pq = M_pq / n - mu_p mu_q (matrix 1) of the data set: two rounded products and one subtraction, no fma.  A block is
 * testable with at least four items, numbered 1 .. k in device order.  Set 0 (basis), k (k - 3) / 2 per block: for i = 4 .. k tau(1,3,i,2), tau(1,2,i,3), then
 * for 4 <= i < j <= k, i-major, tau(1,2,i,j) -- a non-redundant set of the model-implied vanishing tetrads.  Set 1 (all), 2 C(k, 4) per block: per quadruple
 * a < b < c < d in lexicographic order tau(a,b,c,d), tau(a,c,d,b) (the third is minus their sum).
 * Record, width n_tet: the tetrads by block and then as above; status and iterations behind it as doubles (pitch n_tet + 2).  A replicate whose bootstrap status
 * is not PLSPM_OK keeps that status and has NaN in all values; otherwise PLSPM_NONFINITE where a tetrad is not finite (a column that is constant in the
 * resample, under the correlations); the values stand.  Plain metric handles only: PLSPM_E_ARG otherwise.
 *
 * plspm_tetrad_enable: on != 0: mask [L] names the tested blocks (NULL: every testable block) -- every later plspm_bootstrap / plspm_bootstrap_device call on
 *   this handle also writes the tetrad records of its replicates into a buffer of their own, indexed like the bootstrap's records; every other record is bit for
 *   bit what it is without it.  on = 0: off (the default): no launch, no allocation.  PLSPM_E_ARG for a mask entry on a block of fewer than four items (the message
 *   names the LV), for no testable block and for a set or matrix outside 0 / 1; PLSPM_E_LIMIT for more than 4,096 tetrads (the message has the count) and for lists
 *   whose staged correlations exceed a workgroup's 160 KiB of LDS.  Permutation, stratified, cross-validation, jackknife and group calls write none.
 * plspm_tetrad_width: n_tet (0 before the first plspm_tetrad_enable that switched it on).
 * plspm_tetrad_list: *n_tet and per tetrad its block (LV index) and its items a, b, c, d as device-order MV indices; any pointer may be NULL.
 * plspm_tetrad_fit: the full-sample record, out [n_tet]: the same kernel on the moments of all uploaded rows; *status (may be NULL): the record's status.
 * plspm_tetrad_fetch / _summary / _intervals: as plspm_structural_fetch / _summary / _intervals, on the tetrad records (methods 0 .. 2, any level in (0, 1)).
 * PLSPM_E_STATE from the last three without tetrad records on the handle (whatever voids the assessment records voids these; a jackknife leaves them alone).
 */
int plspm_tetrad_enable(plspm_model_t* m, int32_t on, const uint8_t* mask, int32_t set, int32_t matrix);
int32_t plspm_tetrad_width(const plspm_model_t* m);
int plspm_tetrad_list(plspm_model_t* m, int32_t* n_tet, int32_t* block, int32_t* a, int32_t* b, int32_t* c, int32_t* d);
int plspm_tetrad_fit(plspm_model_t* m, double* out, int32_t* status);
int plspm_tetrad_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status);
int plspm_tetrad_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used);
int plspm_tetrad_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used);

/* Importance-performance map analysis (IPMA; this project's definitions after Ringle & Sarstedt 2016, csrc/ipma_core.h): for a target construct,
 * which antecedent constructs and indicators matter most (their unstandardised total effects) and how well do they perform on a 0-100 scale?  With fixed bounds
 * lo_p < hi_p per MV (range_p = hi_p - lo_p), the rescaled indicator x~_p = 100 (x_p - lo_p) / range_p, and per data set mu_p, s_p, r_pq as the assessment has
 * them, the raw mean m_p = shift_p + mu_p, v = w s normalised per block to v' R v = 1 and the fit's sign sigma_l:  a_p = sigma_l v_p range_p / (100 s_p) is the
 * coefficient of x~_p in the standardised score, A_l = sum_{p in l} a_p.
 * Record, width W = 2 L + 2 n_eff + 2 P + n_t P:
 *     perf [L] | sd [L] | total_u [n_eff] | direct_u [n_eff] | weight_r [P] | mvperf [P] | mvimp [n_t x P]
 * weight_r_p = a_p / A_l (1 in sum per block), mvperf_p = 100 (m_p - lo_p) / range_p, perf_l = sum weight_r_p mvperf_p (the mean of Y_l = sum weight_r_p x~_p),
 * sd_l = 1 / A_l (its standard deviation), total_u[e] = total[e] A_i / A_j and direct_u[e] likewise for the effect pair e = (i -> j) of plspm_effect_pairs,
 * mvimp[t][p] = weight_r_p total_u(l -> target t) for the MV p of LV l (0 without an effect pair l -> t and for the target's own block).  MVs in device order,
 * targets in ascending LV order; status and iterations behind the values as doubles (pitch W + 2).  A replicate whose bootstrap status is not PLSPM_OK keeps that
 * status and has NaN in all values; otherwise PLSPM_NONFINITE where a value is not finite (a column that is constant in the resample), otherwise 4
 * (inadmissible, as the PLSc records) where a rescaled weight is negative -- the values stand under both, and neither enters a summary or an interval.
 * Plain metric handles only: PLSPM_E_ARG otherwise.
 *
 * plspm_ipma_enable: on != 0: targets [L] names the target LVs (NULL: every LV with a predecessor), lo / hi [P] the bounds in device order -- every later
 *   plspm_bootstrap / plspm_bootstrap_device call on this handle also writes the IPMA records of its replicates into a buffer of their own, indexed like the
 *   bootstrap's records; every other record is bit for bit what it is without it.  on = 0: off (the default): no launch, no allocation.  PLSPM_E_ARG for a bound
 *   that is not finite or lo_p >= hi_p (the message names the MV), for a mask that names no LV or an LV without a predecessor; PLSPM_E_LIMIT where one replicate's
 *   statistics exceed a workgroup's 160 KiB of LDS.  Permutation, stratified, cross-validation, jackknife and group calls write none.
 * plspm_ipma_width: W (0 before the first plspm_ipma_enable that switched it on).
 * plspm_ipma_targets: *n_t and the targets' LV indices, ascending; either pointer may be NULL.
 * plspm_ipma_fit: the full-sample record, out [W]: the same kernel on the moments of all uploaded rows; *status (may be NULL): the record's status.
 * plspm_ipma_fetch / _summary / _intervals: as plspm_tetrad_fetch / _summary / _intervals, on the IPMA records (methods 0 .. 2, any level in (0, 1)).
 * PLSPM_E_STATE from the last three without IPMA records on the handle (whatever voids the assessment records voids these; a jackknife leaves them alone).
 */
int plspm_ipma_enable(plspm_model_t* m, int32_t on, const uint8_t* targets, const double* lo, const double* hi);
int32_t plspm_ipma_width(const plspm_model_t* m);
int plspm_ipma_targets(plspm_model_t* m, int32_t* n_t, int32_t* lv);
int plspm_ipma_fit(plspm_model_t* m, double* out, int32_t* status);
int plspm_ipma_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status);
int plspm_ipma_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used);
int plspm_ipma_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used);

/*
 * ---- MICOM: permutation test of measurement invariance --------------------------------------------------------------------------
 * Measurement invariance of composite models (Henseler, Ringle and Sarstedt 2016), steps 2 and 3, for every permutation of plspm_permutation_device: one more
 * kernel behind the solver reads both halves' moment matrices and records.  Per group g of a permutation (problem 2r: a, 2r + 1: b), from its
 * moments M_g:  mu_g,p = M_p1 / n_g,  c_g,pq = M_pq / n_g - mu_g,p mu_g,q,  s_g,p = sqrt(c_g,pp) (zero below the solver's 1e-9 threshold),  v_g,p = w_g,p s_g,p
 * with the record's weights w_g.  From ALL uploaded rows, once per upload: the sds s_0, the diagonal blocks R_0,ll of the correlation matrix, the weights w_0
 * of the full-sample fit (plspm_fit's problem), v_0,p = w_0,p s_0,p normalised per block so that v_0' R_0,ll v_0 = 1, and u_p = v_0,p / s_0,p.  Per LV l:
 *     c        v_a' R_0,ll v_b / sqrt((v_a' R_0,ll v_a) (v_b' R_0,ll v_b))      compositional invariance (step 2): the correlation over all rows of the two
 *                                                                             composites of pooled-standardised indicators; it carries a genuine sign
 *     dmean    sum_{p in l} u_p (mu_a,p - mu_b,p)                                step 3: mean of the pooled composite, a - b
 *     dlogvar  log(n_a / (n_a - 1) u' C_a,ll u) - log(n_b / (n_b - 1) u' C_b,ll u)   step 3: log ratio of its (ddof = 1) variances
 * MICOM record, width 3 L:  c[L] | dmean[L] | dlogvar[L];  device records carry a status (0 iff both problems are PLSPM_OK, else the first problem's status
 * when that is not OK, else the second's) and the larger of the two iteration counts behind it as doubles (pitch 3 L + 2).  A permutation whose status is not 0
 * has NaN in all 3 L values; IEEE results stand where a formula divides by zero.  Plain metric handles only: PLSPM_E_ARG otherwise.
 *
 * plspm_micom_enable: on != 0: every later plspm_permutation_device call on this handle also writes the MICOM records of its B permutations into a buffer of
 *   their own (record p of the call at position p); the 2B permutation records, status and iteration counts are bit for bit what they are without it.  Off (the
 *   default): no launch, no allocation.  The observed split's record is a B = 1 call with explicit `member`.
 * plspm_micom_width: 3 L.
 * plspm_micom_fetch: host copy of the MICOM records [first, first + count) of the last MICOM permutation call: out [count*3L], status [count] (may be NULL).
 * plspm_micom_summary / plspm_micom_intervals: plspm_bootstrap_summary / plspm_bootstrap_intervals on the MICOM records (B: that call's, else PLSPM_E_ARG):
 *   original [3L] host, summary / out [3L*6] host, *n_used (may be NULL).  Methods 0 (percentile), 1 (basic), 2 (bc).
 * plspm_micom_counts: per record column j over the valid records (status 0) of that call, on the records in HBM: below[j] = #{r : x_rj <= observed[j]},
 *   exceed[j] = #{r : |x_rj| >= |observed[j]|} (a NaN on either side compares false); *n_used: the valid records.  observed [3L], below / exceed [3L] host.
 * PLSPM_E_STATE from the last four without MICOM records on the handle (none written yet; an upload, or a later call that replaced the handle's records,
 * voids them).
 */
int plspm_micom_enable(plspm_model_t* m, int32_t on);
int32_t plspm_micom_width(const plspm_model_t* m);
int plspm_micom_fetch(plspm_model_t* m, int64_t first, int64_t count, double* out, int32_t* status);
int plspm_micom_summary(plspm_model_t* m, int64_t B, const double* original, double* summary, int64_t* n_used);
int plspm_micom_intervals(plspm_model_t* m, int64_t B, const double* original, int32_t method, double level, double* out, int64_t* n_used);
int plspm_micom_counts(plspm_model_t* m, int64_t B, const double* observed, int64_t* below, int64_t* exceed, int64_t* n_used);

/*
 * ---- Multi-GPU: replicate shards + ONE RCCL all-gather --------------------------------------------------------------------------
 * Reference: Bootstrap.__init__ forks `processes` workers, each running iterations / processes replicates, and merges their
 * frames through a Queue (plspm/bootstrap.py:89-111; `processes` kwarg plspm/plspm.py:35-37,60-61).  Here a GROUP of handles --
 * the same compiled model with the same data uploaded, one handle per MI355X -- runs the replicate ids
 * [rep_offset, rep_offset + B) of one logical stream: rank r of nranks takes the contiguous shard plspm_group_shard(B, r), every
 * rank's [row | status | iterations] records are written into its send buffer by the solver kernel, and ONE ncclAllGather over
 * xGMI (librccl.so.1, loaded on first use) leaves all records on every rank.  Results are bit-identical for every nranks
 * (Philox stream keyed by (seed, replicate id)).  Nothing here needs PyTorch.
 *
 * Two objects: a COMMUNICATOR (plspm_comm_t: the RCCL communicators of this process's ranks -- expensive, of the order of a
 * second, create once per process) and a GROUP (plspm_group_t: binds one uploaded handle per local rank to the communicator --
 * cheap: a gather stream, four events and the record buffers per handle).  Two ways to form a communicator:
 *   single process   n_local == nranks ranks on DISTINCT devices (ncclCommInitAll); unique_id = NULL, first_rank = 0.
 *                    Ranks that share a device (testing on a 1-GPU box; RCCL refuses duplicate devices) exchange their records
 *                    with device-to-device copies (one copy launch when every handle shares a device) instead of RCCL -- same buffers, same ordering, same results.
 *   one process per GPU (torchrun / mpirun)   n_local == 1, first_rank = this process's rank, unique_id = the 128 bytes that
 *                    rank 0 obtained from plspm_rccl_unique_id() and handed to every rank (ncclCommInitRank: collective call).
 * A communicator serves one group at a time; a handle belongs to at most one group at a time and must outlive it.  Group calls
 * are not re-entrant.
 *
 * Stream semantics: plspm_group_bootstrap only ENQUEUES (shard kernels on each handle's stream, the all-gather on a second
 * stream per handle behind an event); records are double-buffered so that the collective of call k overlaps the kernels of call
 * k+1.  plspm_group_summary / _rows / _sync wait for the last call's collective.
 */
typedef struct plspm_comm plspm_comm_t;
typedef struct plspm_group plspm_group_t;
#define PLSPM_UNIQUE_ID_BYTES 128
int plspm_rccl_unique_id(uint8_t* id /* [PLSPM_UNIQUE_ID_BYTES] */);
/* device_ids [n_local]: HIP device of every local rank; local rank i is global rank first_rank + i.  NULL on failure. */
plspm_comm_t* plspm_comm_create(const int32_t* device_ids, int32_t n_local, int32_t nranks, int32_t first_rank, const uint8_t* unique_id);
void plspm_comm_destroy(plspm_comm_t* c);                  /* a group still bound to it is released (streams, buffers, its hold on the handles): later
                                                              calls on that group return PLSPM_E_STATE; its owner still calls plspm_group_destroy */
/* The same with the transport and RCCL's footprint chosen (round 5):
 *   transport     PLSPM_TRANSPORT_AUTO   RCCL between distinct devices, one copy launch among ranks that share a device (plspm_comm_create)
 *                 PLSPM_TRANSPORT_RCCL   RCCL or failure
 *                 PLSPM_TRANSPORT_COPY   single-process jobs only (n_local == nranks): no RCCL -- every rank pulls its peers' shards with
 *                                        device-to-device copies on peer-mapped buffers (hipDeviceEnablePeerAccess): the SDMA engines move the
 *                                        records over xGMI and no kernel of the exchange takes a CU from the next step's Gram
 *   max_channels  0: RCCL's default; n > 0: the communicator's collectives run at most n workgroups (ncclConfig_t.maxCTAs) -- a Gram workgroup
 *                 needs a whole CU, so every CU an RCCL channel occupies is missing from a launch cut for all of them; the one all-gather of
 *                 44 MB per 0.48 ms step (eight ranks) does not need RCCL's default channel count.  The NCCL_* environment variables of the
 *                 caller are not touched.
 * plspm_comm_split: a second communicator over the same ranks with its own max_channels, split off an RCCL communicator (ncclCommSplit --
 * collective over the parent, every rank calls it; no new unique id): lets a job time RCCL's default against a capped one (bench.py). */
enum { PLSPM_TRANSPORT_AUTO = 0, PLSPM_TRANSPORT_RCCL = 1, PLSPM_TRANSPORT_COPY = 2 };
plspm_comm_t* plspm_comm_create_ex(const int32_t* device_ids, int32_t n_local, int32_t nranks, int32_t first_rank, const uint8_t* unique_id, int32_t transport,
                                   int32_t max_channels);
plspm_comm_t* plspm_comm_split(plspm_comm_t* parent, int32_t max_channels);
int32_t plspm_comm_size(const plspm_comm_t* c);            /* nranks */
int32_t plspm_comm_uses_rccl(const plspm_comm_t* c);       /* 1: records travel through RCCL; 0: device-to-device copies */
int32_t plspm_comm_transport(const plspm_comm_t* c);       /* PLSPM_TRANSPORT_RCCL / PLSPM_TRANSPORT_COPY / 3: ranks share a device (one copy launch) */
int32_t plspm_comm_max_channels(const plspm_comm_t* c);    /* the cap the communicator was created with (0: RCCL's default) */
/* models [n_local of the communicator]: handle i lives on the communicator's device i, data uploaded.  NULL on failure. */
plspm_group_t* plspm_group_create(plspm_comm_t* c, plspm_model_t* const* models);
void plspm_group_destroy(plspm_group_t* g);
/* Text of the last error on this group (or of the last failed plspm_comm_create / plspm_group_create / plspm_rccl_unique_id
 * when NULL). */
const char* plspm_group_last_error(const plspm_group_t* g);
int32_t plspm_group_size(const plspm_group_t* g);          /* nranks */
/* Shard of rank `rank`: balanced contiguous ranges, the first B % nranks ranks hold one replicate more. */
int plspm_group_shard(const plspm_group_t* g, int64_t B, int32_t rank, int64_t* first, int64_t* count);
/* Enqueue B replicates split over the group + the all-gather.  Returns without host synchronisation for metric models.
 * ONE call hides its merge (round 5): the call runs as up to three SUB-BATCHES -- consecutive ranges of the replicate ids, each sharded over the
 * ranks like a call of its own (plspm_group_plan) -- and the all-gather of sub-batch k runs on the gather streams beside the shard kernels of
 * sub-batch k + 1; only the last, smallest gather is exposed.  Results do not depend on the cut (Philox stream keyed by (seed, replicate id)).
 * Options (plspm_group_set_option): "chunks" 0 (default: automatic -- one sub-batch below 2 MiB of records per rank, on a one-rank group and among
 * ranks that share a device, else up to three, sizes falling by "chunk_ratio" percent) | 1 .. 8 sub-batches -- a caller that issues calls back to back (bench.py's
 * step loop) sets 1: the gather of call k then overlaps the kernels of call k + 1 anyway; "chunk_ratio" 10 .. 100 (default 50); "chunk_align"
 * 0 (default: every sub-batch but the last fills whole ROUNDS of the device per rank -- a part that ends inside a round of Gram tiles pays for
 * the whole round; models whose round holds more replicates than the call has stay in one piece) | n: multiples of n replicates per rank;
 * "gather_root" 0 (default: every rank receives every shard -- ncclAllGather) | 1: only rank 0 -- the rank whose handle summarises, as only the
 * reference's parent process merges (bootstrap.py:96-111) -- receives them: grouped ncclSend / ncclRecv to rank 0 (or its copy engines alone pulling, in a
 * one-process job on the copy transport): 1 / nranks of the bytes on the links, nothing arriving at the other ranks.  plspm_group_summary then computes the
 * table on rank 0 and hands it to every rank in one small ncclBroadcast (every rank calls it, as before); plspm_group_records / _rows / _adopt report
 * PLSPM_E_STATE on the ranks that hold no records.  The automatic sub-batch alignment is agreed across the ranks (max) in the first call that needs it. */
int plspm_group_bootstrap(plspm_group_t* g, int64_t B, uint64_t seed, int64_t rep_offset);
int plspm_group_set_option(plspm_group_t* g, const char* key, int32_t value);
/* The sub-batches a call of B replicates is cut into: *n_sub (<= 8) ranges [sub_first[k], sub_first[k] + sub_count[k]) (arrays of 8), in
 * replicate-id order; rank r computes plspm_group_shard(sub_count[k], r) of each, offset by sub_first[k]. */
int plspm_group_plan(const plspm_group_t* g, int64_t B, int32_t* n_sub, int64_t* sub_first, int64_t* sub_count);
/* Wait for everything enqueued on the group's streams (every local handle). */
int plspm_group_sync(plspm_group_t* g);
/* Gathered records of the last plspm_group_bootstrap on local handle `local`: *d_records -> [*n_records * *stride] fp64 in HBM.  One sub-batch
 * (plspm_group_plan): n_records = nranks * ceil(B / nranks); rank r's shard starts at record r * ceil(B / nranks); the unused tail records of
 * a ragged split carry NaN in the status column.  Several sub-batches: one such block per sub-batch, one after the other (the replicates stay
 * in id order; n_records = nranks * sum_k ceil(sub_count[k] / nranks)).  Valid until the next-but-one plspm_group_bootstrap. */
int plspm_group_records(plspm_group_t* g, int32_t local, void** d_records, int64_t* n_records, int32_t* stride);
/* _create_summary (bootstrap.py:24-32) of the last plspm_group_bootstrap, on local handle 0's copy of the gathered records:
 * same outputs as plspm_bootstrap_summary. */
int plspm_group_summary(plspm_group_t* g, const double* original, double* summary, int64_t* n_used);
/* Host copy of the last plspm_group_bootstrap's replicates in replicate-id order: out [B*R], status / iters [B] (may be NULL). */
int plspm_group_rows(plspm_group_t* g, double* out, int32_t* status, int32_t* iters);
/* Hand the last plspm_group_bootstrap's records to local handle 0 (device-to-device, replicate-id order): the handle then answers
 * plspm_bootstrap_fetch / plspm_bootstrap_summary(d_rows = NULL) for them like for its own plspm_bootstrap_device, and the group --
 * and with it the communicator's one group slot -- can be destroyed (the merge of Bootstrap.__init__, bootstrap.py:96-111, keeps
 * nothing of the workers alive either). */
int plspm_group_adopt(plspm_group_t* g);
/* Collective helpers for a caller's timing protocol (bench.py): barrier = all-reduce of one word on the gather stream + host
 * wait; max = all-reduce(max) of one double over the ranks. */
int plspm_group_barrier(plspm_group_t* g);
int plspm_group_max(plspm_group_t* g, double* value);
/* Host time of the last plspm_group_bootstrap call on this process, in milliseconds: enqueue of the shard kernels of all local handles
 * (resident threads, one per handle) and enqueue of the exchange (event waits + ONE ncclAllGather per handle inside a group call, or the
 * device copies of ranks that share a GPU).  Diagnostics for tools/group_enqueue.py. */
int plspm_group_enqueue_times(const plspm_group_t* g, double* shards_ms, double* exchange_ms);

/*
 * ---- Operator seam ------------------------------------------------------------------------------------------------------------
 * The reference's strategy objects, callable on their own; each call uploads its operands, forms their moment
 * matrix with the MFMA Gram kernel and finishes in one small kernel (csrc/solver_ops.h).  Errors: plspm_last_error(NULL).
 *   plspm_op_inner_weights  Scheme.X.value.calculate(path, y)            plspm/scheme.py:27-28, 36-37, 45-54
 *       scheme PLSPM_SCHEME_*; path [L*L] row-major 0/1 strictly lower triangular; y [N*L] row-major LV scores; E [L*L] row-major:
 *       centroid sign(corrcoef(y) * (path + path')), factorial cov1(y) * (path + path'), path: OLS coefficients (no intercept,
 *       minimum norm) of every LV on its predecessors / correlations with its successors, column i = LV i
 *   plspm_op_outer_weights  Mode.X.value.outer_weights_metric(data, Z, lv, mvs)   plspm/mode.py:28-29, 50-52
 *       Xk [N*k] row-major: the block's (treated) MVs; z [N]: the LV's inner estimate; w [k]:
 *       Mode A  X_k' z / N;  Mode B  least squares of z on X_k (minimum norm when X_k is rank deficient, as scipy.linalg.lstsq)
 *   plspm_op_outer_weights_nonmetric  Mode.X.value.outer_weights_nonmetric(mv_grouped_by_lv, mv_grouped_by_lv_missing, Z, lv, correction)
 *       plspm/mode.py:31-42, 54-61.  Xk [N*k] row-major: the block's quantified MVs (NaN where missing); present [N*k] 0/1 or NULL when
 *       the block has no missing cell (the reference's mv_grouped_by_lv_missing[lv]); z [N]; returns w [k] and the LV's new scores Y [N]:
 *       Mode A  w = X'z / sum z^2 (NaN-aware ratios with a mask), Mode B least squares of z on X (no mask allowed); Y = X w (row-wise
 *       normalised with a mask), then (Y - mean) / std1 * correction (util.py:43-53)
 */
int plspm_op_inner_weights(int32_t device_id, int32_t scheme, int32_t L, const uint8_t* path, const double* y, int64_t N, double* E);
int plspm_op_outer_weights(int32_t device_id, int32_t mode, const double* Xk, const double* z, int64_t N, int32_t k, double* w);
int plspm_op_outer_weights_nonmetric(int32_t device_id, int32_t mode, const double* Xk, const uint8_t* present, const double* z, int64_t N, int32_t k,
                                     double correction, double* w, double* Y);

/* Kernel timing with HIP events on the handle's own stream (for the roofline figures in bench.py).
 * kernel ids: 0 resample/compact, 1 gram (MFMA), 2 solver, 3 scores, 4 upload/pack, 5 gram reduce (and the counts on records), 6 assessment (and the MICOM, PLSc, model-fit, tetrad and IPMA kernels),
 * 7 .. 10 the moderation kernels: counts, prepare, row pass, finish. */
enum { PLSPM_K_RESAMPLE = 0, PLSPM_K_GRAM = 1, PLSPM_K_SOLVER = 2, PLSPM_K_SCORES = 3, PLSPM_K_PACK = 4, PLSPM_K_REDUCE = 5, PLSPM_K_ASSESS = 6, PLSPM_K_MOD_COUNTS = 7, PLSPM_K_MOD_PREPARE = 8, PLSPM_K_MOD_ROWS = 9,
       PLSPM_K_MOD_FINISH = 10, PLSPM_K_COUNT = 11 };
/* on: 0 off, 1 every kernel, 2 + id only kernel `id` (an event pair costs dispatch latency on both sides: bracketing one kernel of a
 * step perturbs the step less than bracketing all of them). */
int plspm_profile_enable(plspm_model_t* m, int32_t on);
int plspm_profile_read(plspm_model_t* m, int32_t kernel_id, double* total_ms, int64_t* launches);
int plspm_profile_reset(plspm_model_t* m);

#ifdef __cplusplus
}
#endif
#endif /* PLSPM_HIP_H */
