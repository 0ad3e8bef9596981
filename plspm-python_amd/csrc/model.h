// Host-side state of one libplspm_hip handle (include/plspm_hip.h), shared by the translation units of the library:
// the .hip translation units (kernels + single-device entry points; host_internal.h lists them) and plspm_group.cpp (multi-GPU groups over RCCL).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/plspm_hip_test.h"
#include "gram_route.h"
#include "derived_route.h"
#include "moderation_core.h"
#include "group_route.h"
#include "options.h"

inline thread_local std::string g_create_error;

// Caching allocator of the library (defined in plspm_hip.hip).  A Plspm() call creates a handle, uploads, fits and destroys it:
// without a cache every call pays ~40 hipMalloc / hipHostMalloc / hipFree round trips (measured 12 of the 17 ms of a 10k x 60
// Plspm() fit).  Freed blocks are kept per device (and for pinned host memory) and handed out again best-fit; a block is only
// ever returned by an owner whose stream has been synchronised, so a cached block has no work in flight.
// plspm_release_cached_memory() (C-ABI) gives everything back to the runtime.
hipError_t plspm_dmalloc(void** p, size_t bytes);       // device memory on the CURRENT device
void plspm_dfree(void* p);
hipError_t plspm_hmalloc(void** p, size_t bytes);       // pinned host memory
void plspm_hfree(void* p);
// Streams are cached the same way (hipStreamCreate / hipStreamDestroy set up and tear down a hardware queue: ~1-2 ms each):
// a stream goes back only after it has been synchronised.  Non-blocking streams of the CURRENT device.
hipError_t plspm_stream_acquire(hipStream_t* s);
void plspm_stream_release(hipStream_t s);

// The specs of the batch kinds that bring their own counts (host_internal.h): a BatchCall below points at its kind's.
struct PermSpec;      // two-group permutation: the splits (plspm_permute.hip)
struct StratSpec;     // stratified bootstrap of the two-group test: the draws inside each group (plspm_permute.hip)
struct CvSpec;        // cross-validation: the folds (plspm_cv.hip)
struct JackSpec;      // jackknife: the number of groups (plspm_jackknife.hip)
struct RebusSpec;     // REBUS-PLS: the rows' class labels (plspm_rebus.hip)

// Kernel timing (plspm_profile_*): event pairs are recycled through `pool`, so a profiled launch costs two hipEventRecord only.
struct ProfSlot { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev, pool; double total_ms = 0.0; int64_t launches = 0; };

struct plspm_model {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = true;      // an attached second stage runs on its first stage's stream
    int P = 0, L = 0, PA = 0, T = 0, scheme = 0, scaled = 1, max_iter = 100, kmax = 0, n_eff = 0, n_chol = 0;
    double tol = 1e-6;
    std::vector<int> boff, lvof, mode, chol_off, eff_from, eff_to, pred_off, pred_idx, succ_off, succ_idx;
    std::vector<uint8_t> C;
    int *d_boff = nullptr, *d_lvof = nullptr, *d_mode = nullptr, *d_chol_off = nullptr, *d_eff_from = nullptr, *d_eff_to = nullptr;
    int *d_pred_off = nullptr, *d_pred_idx = nullptr, *d_succ_off = nullptr, *d_succ_idx = nullptr;
    uint8_t* d_C = nullptr;
    int64_t N = 0;
    double* d_Xa = nullptr;
    // A block of the caching allocator and its owner: the block goes back to the allocator with the owner, i.e. with `delete m` for a member of the handle -- behind
    // the synchronisation of the handle's streams in plspm_model_destroy, as the allocator asks.  Buf: device memory, grow-only through ensure() below; Pin: pinned
    // host memory.
    template <hipError_t (*ALLOC)(void**, size_t), void (*FREE)(void*)>
    struct Block {
        void* p = nullptr;
        size_t cap = 0;
        Block() = default;
        Block(const Block&) = delete;
        Block& operator=(const Block&) = delete;
        Block(Block&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
        Block& operator=(Block&& o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
        ~Block() { reset(); }
        void reset() { if (p) FREE(p); p = nullptr; cap = 0; }
        // at least `bytes` (device memory: on the CURRENT device); a block that is too small is given back first, so the caller has made sure that nothing in flight uses it
        hipError_t reserve(size_t bytes) {
            if (bytes <= cap) return hipSuccess;
            reset();
            const hipError_t e = ALLOC(&p, bytes);
            if (e == hipSuccess) cap = bytes;
            return e;
        }
    };
    using Buf = Block<plspm_dmalloc, plspm_dfree>;
    using Pin = Block<plspm_hmalloc, plspm_hfree>;
    // (a member x_buf owns the block that the typed pointer d_x points at: the other units, and the kernels' descriptors, read the pointer)
    Buf shift_buf;
    double* d_shift = nullptr;
    Buf ent, nent, gram, gram_partial, rows, status, iters, gS, gsmall, fitout, idx, err, ghist, nmstate, nmpartial, nmactive, nmlist, gK16, sum_buf, cols;
    int nonmetric = 0;           // Scale.NUM / Scale.RAW data: population-standardised MVs, score-based stop rule
    bool codes_valid = false;    // m->codes holds the category codes of the uploaded rows (nm_conv_codes_kernel)
    bool ind8_valid = false;     // m->ind8 holds their indicator bytes in MFMA fragment order (kernels_nmp.h)
    long last_nm_problems = 0;   // problems of the last run_nonmetric (plspm_nonmetric_criteria)
    int last_strat_rows = 0;     // 1 / 2: the last stratified counts read the group's rows through L2 / from LDS (plspm_permute.hip)
    int last_i8_nibbles = 0;     // 1: the last int8 resample drew into 4-bit counters (data sets beyond one 16-bit window)
    int last_nm_direct16 = 0;    // 1: the last categorical bootstrap's count matrices were written by the int8 product itself (uint16, no scatter pass)
    int last_nm_mfma = 0;        // 1: the last non-metric bootstrap's stop-rule passes ran as int8 matrix products (kernels_nmp.h)
    int last_nm_wave = 0;        // 1: the last categorical iteration ran one wave per problem (kernels_nmw.h)
    int last_nm_wave16 = 0;      // 1: the last Scale.NUM / RAW bootstrap batch ran as one solver launch + verification (plspm_nonmetric.hip run_nonmetric_wave)
    int last_nm_one = 0;         // 1: the last categorical bootstrap batch ran as one solver launch + verification (plspm_nonmetric.hip, round 6)
    int last_nm_exact = 0;       // categorical wave step (round 6): (problem, step) pairs of the last bootstrap whose lower bound decided nothing and that took the pass over all rows
    int last_nm_flagged = 0, last_nm_replayed = 0;      // ... (replicate, step) pairs its lower-bound pass left to the exact pass / replicates whose stop moved
    Buf nmw_maps, nmw_ints, nmw_vsum;
    int last_nm_codes = 0;       // 1: the last non-metric bootstrap's stop-rule passes ran on category codes
    bool cat_pure = false;       // every logical MV is ORD / NOM: all device columns are 0/1 indicators
    int categorical = 0;         // Scale.ORD / NOM present: device columns are aug columns (solver_nmg.h); Pm logical MVs
    int Pm = 0, cmax = 1, kmv = 1;
    std::vector<int> mv_off, mv_kind, lmv_off, mv_lv, no_chol, mv_base, mv_base2, lmv2_off;
    int *d_mv_off = nullptr, *d_mv_kind = nullptr, *d_lmv_off = nullptr, *d_mv_lv = nullptr, *d_no_chol = nullptr, *d_mv_base = nullptr, *d_mv_base2 = nullptr, *d_lmv2_off = nullptr;
    Buf gSm, mv_base2_buf, lmv2_off_buf;      // (the last two: d_mv_base2, d_lmv2_off of an attached second stage)
    // metric data with missing values: Pg = P + n_ind device columns (data | missing indicators); PA / T describe the Gram of
    // those, PAs / Ts the P-column moment matrix the solver reads (impute_collapse maps one to the other).  Pg == P otherwise.
    int Pg = 0, PAs = 0, Ts = 0, n_ind = 0;
    std::vector<int> ind_of;
    int* d_ind_of = nullptr;
    Buf gram2, ind_of_buf;
    // two-stage higher order constructs (solver_hoc.h): `stage2` of a data-holding handle / `stage1` of its attached second stage
    plspm_model* stage2 = nullptr;
    plspm_model* stage1 = nullptr;
    std::vector<int> lv_first, col2_lv1, col2_p1, hcol, hidx;
    std::vector<int> lv_cols;
    int* d_lv_cols = nullptr;
    int *d_lv_first = nullptr, *d_col2_lv1 = nullptr, *d_col2_p1 = nullptr, *d_hcol = nullptr, *d_hidx = nullptr;
    Buf pseudo;
    // non-metric data with missing values (solver_nmx.h): K incomplete rows live in side tables, their rows of Xa are zero
    Buf dcnt, ctable, Xt;        // dense stop-rule pass of the non-metric bootstrap: uint16 histograms, coefficient table, tiled copy of Xa
    long dcnt_stride = 0;
    bool Xt_valid = false;
    int nmx_K = 0, nmx_raw = 0;
    double *d_Xk = nullptr, *d_Mk = nullptr;
    int* d_rowid = nullptr;
    Buf Xk_buf, Mk_buf, rowid_buf;      // (plspm_hip.hip drop_incomplete_rows)
    Pin flag_pin;
    int* h_flag = nullptr;        // pinned (a view of flag_pin): active-problem counter of the non-metric iteration
    hipEvent_t ev_flag = nullptr;
    Pin h_stage;                  // pinned host staging for plspm_fit results (fit_route.h stage_need)
    // result bookkeeping: `rows` holds the records of the last plspm_bootstrap(_device) only (the fit's scores have their own buffer)
    Buf scores;
    Buf xa, up_raw, up_ci, up_partial;   // resident matrix (d_Xa points into `xa` while data are uploaded) and the upload staging
    int64_t rows_B = 0;           // number of valid records in `rows` (0: none)
    bool err_clean = false;       // the device error word is zero and no call since could have raised it (plspm_detail_bootstrap; batch_route.h batch_may_raise)
    // launch-geometry options (plspm_model_set_option): defaults, accepted values and what a change voids in options.h
    using Tune = plspm::Tune;
    Tune tune;
    // int8 digit-plane Gram of bootstrap batches (kernels_gram_i8.h): per data set the digit planes `zs` of all pair products and the
    // pair tables (p, q, k, slot in the packed matrix | 2^-k); per call the dense int8 multiplicities `cd`
    Buf zs, cd, cd1, err2, pair_tab, pair_scale, zs_stat, codes, ind8, tab8, scl8, pp_ctl;      // pp_ctl: tile counters of the persistent Gram (kernels_gram_i8p.h GramI8PPCtl)
    // set_option("resample_aux", 1..3): the int8 counts are drawn on a second stream (1 lowest / 2 default / 3 highest priority) into
    // alternating buffers, so that the draws of call k+1 -- enqueued while the Gram / solver of call k still run -- take the CUs those
    // leave idle (the Gram's last, partial round of workgroups first of all); the Gram waits for its counts by event.  Measured
    // (tools/aux_ab.py, 5,000 replicates per step): 0.647 ms off, 0.635 lowest, 0.654 default, 0.634 highest priority.  OFF by default:
    // 2 % is inside the box-to-box spread, and with it every Gram launch shares the chip with another kernel (0.455 -> 0.49 ms per
    // launch), so per-kernel timings would no longer describe the kernel alone.
    // persistent ("stream-K") int8 Gram, set_option("i8_sched", 1): one accumulator slot + one flag per wave of every workgroup, launch serial
    Buf sk_partial, sk_flags;
    unsigned sk_epoch = 0;
    int cu_count = 0;
    hipStream_t aux = nullptr;
    hipEvent_t ev_counts[2] = {nullptr, nullptr}, ev_cdfree[2] = {nullptr, nullptr};
    bool cdfree_set[2] = {false, false};
    int cd_slot = 0;
    bool zs_valid = false;
    bool zs_stats_ready = false;  // phase 1 of the digit planes is enqueued (pair tables, column statistics on their way to h_zstat): plspm_gram_i8.hip prepare_zs_stats
    int zs_stats_S = 0;           // ... for this value of the "i8_slices" option
    Pin h_zstat;                  // pinned copy of the column statistics (automatic plane count)
    hipEvent_t ev_zstat = nullptr;
    int zs_S = 0, zs_KB = 0, zs_NT = 0, zs_npair = 0, zs_npg = 0;
    int zs_floor = 0;           // the plane floor the current planes were cut under (prepare_zs: 0 = the handle's own choice, 7 = a permutation call)
    bool zs_ind = false;        // one plane per pair group, launched through the seven-plane main loop (gram_i8_kernel<.., IND>)
    double zs_ratio = 0.0;      // smallest sum|z| / max|z| over the pair columns (automatic plane count; 0: not evaluated)
    Buf perm_thr, perm_member, perm_io;      // plspm_permutation_device: the splits' thresholds, explicit memberships, the exceedance counts' in / out block
    Buf strat_rows, strat_draws, strat_io, strat_u;      // plspm_stratified_bootstrap_device: both groups' row lists, explicit draws, the pair counts' in / out block and u values
    std::vector<uint8_t> strat_member;       // ... the memberships strat_rows was built from (uploaded again only when they change)
    Buf cv_fold, cv_thr, cv_idx, cv_off, cv_mom, cv_coef, cv_io, cv_pred, cv_tab;      // plspm_cv_device: fold ids, thresholds, rows in fold order + offsets, training moments, coefficient matrices, error sums, predictions, small tables
    int64_t cv_reps = 0; int cv_k = 0;       // ... the last plspm_cv_device call whose folds, moments and records are on the handle (0: none)
    Buf jack_rows, jack_status, jack_iters, jack_io;      // plspm_jackknife_device: its records, status and iteration counts (buffers of their own: the bootstrap's survive the call), the statistics' out block
    int64_t jack_G = 0;                      // ... the last plspm_jackknife_device call whose records are on the handle (0: none)
    // FIMIX-PLS (plspm_fimix.hip): the fit's scores describe the rows that are resident now (plspm_fit with scores sets it, an upload clears it); the last
    // plspm_fimix_device call's records [nprob x (width + 2)], status and iteration counts in buffers of their own, its descriptor tables, segment counts and explicit starts
    bool scores_valid = false;
    Buf fimix_rows, fimix_status, fimix_iters, fimix_desc, fimix_k, fimix_init, fimix_post;
    int64_t fimix_nprob = 0;                 // ... problems of that call (0: none)
    // REBUS-PLS (plspm_rebus.hip): the labels, the K local records with status and iteration counts in buffers of their own (the bootstrap's survive
    // the call), the class moments' slices, the classes' parameters and validity flags, A | B [2][K][N], the tiles' partial sums, CM [N][K], the members-only sums
    // (per tile, then [K][P + n_endo]), the per-iteration counters [max_iter + 1][1 + K] (changed | sizes: the history), the small tables, the one-class residuals
    Buf rebus_label, rebus_rows, rebus_status, rebus_iters, rebus_mom, rebus_par, rebus_flags, rebus_ab, rebus_part, rebus_cm, rebus_within_part, rebus_within, rebus_ctr, rebus_tab, rebus_resid;
    Pin rebus_pin;                           // ... what the driver reads back after a round: changed | sizes [K] | flags [K]
    int rebus_K = 0;                         // ... classes of the last plspm_rebus_device call whose results are on the handle (0: none)
    int rebus_status_run = 0, rebus_iters_run = 0, rebus_hist = 0;      // ... its run status, its iterations and the iterations whose counters are history
    std::vector<int> rebus_sizes;            // ... the class sizes of its labels
    int last_rebus_loads = 0;                // LDS loads per row tile of the last REBUS row pass (read-only option "last_rebus_loads")
    int fimix_kmax = 0;                      // ... and its kmax
    std::vector<int> fimix_k_of;             // ... and every problem's K
    // The records derived from a plain bootstrap's replicates (plspm_derived.hip; the stages, what each reads and its record: derived_route.h kDerivedStage): per stage
    // its switch (plspm_<stage>_enable), the replicates' records [B x (width + 2)] in a buffer of their own, indexed by the replicate's position in the whole call, and
    // the last plain bootstrap whose records of the stage are on the handle (0: none).  A stage's records are written whenever those of a stage that reads them are.
    struct DerivedRecords { bool on = false; Buf rows; int64_t B = 0; };
    DerivedRecords derived[plspm::kDerivedStages];
    Buf derived_fit;                         // the full-sample problem and its records of the stages one plspm_<stage>_fit takes (derived_route.h derived_fit_layout)
    // consistent PLS, and the model fit and geodesic discrepancy behind it: one factor mask for the three
    std::vector<uint8_t> plsc_factor;        // ... the factor mask [L] it was enabled with (the default mask until then)
    Buf plsc_side, plsc_mask;                // ... a pass's side output of assess_kernel [nb x 3 L]; the mask on the device
    // structural-model assessment: the direct paths and the chains are enumerated once, at plspm_structural_enable
    bool structural_listed = false;          // ... the lists below describe this handle's path matrix
    std::vector<int> struct_dir_from, struct_dir_to, struct_chain_off, struct_chain_nodes;      // [n_dir] x 2, [n_spec + 1], [chain_off[n_spec]]
    Buf structural_desc;                     // ... dir_from | dir_to | chain_off | chain_eff on the device (structural_core.h StructDesc)
    // moderation analysis (plspm_moderation.hip): the switch and the terms' lists (moderation_core.h) from plspm_moderation_enable; the replicates' records
    // [mod_B x (width + 2)] in a buffer of their own, indexed by the replicate's position in the whole call; a pass's counts, tables, correlations and partial sums
    bool mod_on = false;
    plspm::ModLayout mod_lay{};
    int mod_e_total = 0;
    std::vector<int> mod_terms;              // ... predictor | moderator | target, [3 T]
    Buf mod_desc, mod_rows, mod_cnt, mod_table, mod_rc, mod_partial, mod_fit;
    int64_t mod_B = 0;                       // ... the last plain bootstrap whose moderation records are on the handle (0: none)
    // confirmatory tetrad analysis (plspm_tetrad.hip): the switch, the set, the matrix, the tested blocks and the tetrads' lists (tetrad_core.h) from
    // plspm_tetrad_enable; the replicates' records [tet_B x (tet_n + 2)] in a buffer of their own, indexed by the replicate's position in the whole call
    bool tet_on = false;
    int tet_set = 0, tet_matrix = 0;
    std::vector<uint8_t> tet_mask;           // ... [L]: the blocks whose triangles are staged
    std::vector<int> tet_block, tet_items;   // ... per tetrad its block [tet_n] and its items a, b, c, d as device-order MV indices [4 tet_n]
    int tet_n = 0; long tet_tri = 0;         // ... tetrads; doubles of the staged triangles
    Buf tet_desc, tet_rows, tet_fit;         // ... descriptors | triangle offsets on the device; the records; the full-sample problem and its record
    int64_t tet_B = 0;                       // ... the last plain bootstrap whose tetrad records are on the handle (0: none)
    // importance-performance map analysis (plspm_ipma.hip): the switch and the targets (ascending LV indices) from plspm_ipma_enable; the
    // lists on the device (ipma_core.h IpmaBuild: lvof | targets | eff_of) and the bounds it was given (lo | hi, [P] each, device order); the replicates' records [ipma_B x (W + 2)] in a buffer of
    // their own, indexed by the replicate's position in the whole call
    bool ipma_on = false;
    int ipma_nt = 0;                         // ... targets (0: never enabled)
    std::vector<int> ipma_targets;
    Buf ipma_ints, ipma_bounds, ipma_rows, ipma_fit;      // ... the lists; the bounds; the records; the full-sample problem and its record
    int64_t ipma_B = 0;                      // ... the last plain bootstrap whose IPMA records are on the handle (0: none)
    // MICOM records of a permutation call's splits (kernels_micom.h; plspm_micom_*): records [micom_B x (3 L + 2)] in a buffer of their own, indexed by the
    // permutation's position in the call; the pooled inputs (u, the diagonal blocks of R_0; plspm_micom.hip micom_prepare) once per upload
    bool micom_on = false;                   // plspm_micom_enable
    Buf micom_rows, micom_pool, micom_io;    // ... the permutations' records; the pooled inputs + the full-sample solver problem behind them; the counts' in / out block
    int64_t micom_B = 0;                     // ... the last permutation call whose MICOM records are on the handle (0: none)
    bool micom_pool_valid = false;           // ... micom_pool describes the rows that are resident now
    int last_micom_layout = 0;               // 1 dense / 2 tile-packed: the moment layout the last MICOM launch read (read-only option "last_micom_layout"; 0: none yet)
    int last_gram_path = 0;       // 1 fp64 MFMA, 2 int8 digit planes: what the last bootstrap call used (plspm_model_get_info)
    int last_boot_passes = 0;     // passes the last plspm_detail_bootstrap batch was cut into (read-only option "last_boot_passes")
    int last_i8_dma = 0;          // 1 global_load_lds, 2 buffer_load ... lds: the LDS-DMA form of the last int8 Gram launch
    int last_i8_persist = 0;      // 1: ... as one persistent workgroup per CU (gram_i8pp_kernel)
    int last_i8_priv = 0;         // 1: the last int8 Gram launch was gram_i8p_kernel (private count fragments)
    int last_i8_rt = 0;           // count tiles (16 replicates each) per workgroup of the last int8 Gram launch: 16, 20 or 8
    plspm::GramI8Cut mix_cut{};      // gram_route.h gram_i8_plan: the last tile-row cut and its key
    int last_i8_mt = 0;           // count tiles (padded) of the last int8 Gram launch: 16 x this many replicate slots went through the matrix pipe
    int last_i8_short = 0;        // ... and, with 20, how many of its tile rows were short ones (16 count tiles: gram_route.h i8_mix_plan)
    int last_solver = 0;          // the SolverRoute (solver_route.h) of the last metric or Scale.NUM / RAW bootstrap batch
    // grow-only pinned host staging for uploads / row downloads (two halves: copy-in of chunk k+1 overlaps the DMA of chunk k)
    Pin h_pin;
    hipEvent_t ev_pin[2] = {nullptr, nullptr};
    hipEvent_t ev_pin_async = nullptr;   // behind copies that left the staging area without a host wait (plspm_hip.hip pin_leave_async)
    bool pin_pending = false;
    enum { BLOB_MODEL = 0, BLOB_CATEGORICAL = 1, BLOB_HOC = 2, BLOB_COUNT = 3 };
    void* blobs[BLOB_COUNT] = {nullptr, nullptr, nullptr};     // descriptor blocks, one per call site (several small arrays uploaded as one: plspm_hip.hip upload_blob)
    void* group = nullptr;        // the plspm_group this handle currently belongs to (plspm_group.cpp)
    // plspm_bootstrap as sub-batches (plspm_bootstrap.hip): the copy stream the records of sub-batch k leave on while sub-batch k + 1 computes,
    // one event per sub-batch
    hipStream_t dl = nullptr;
    hipEvent_t ev_part[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool profiling = false;
    int prof_only = -1;          // >= 0: only this kernel id is bracketed by events (plspm_profile_enable(m, 2 + id))
    ProfSlot prof[PLSPM_K_COUNT];
    std::string error;
};

// One call of the batch driver, described in full: nothing about a call lives on the handle while it runs.  The entry points of every kind fill one in
// and hand it to plspm_detail_bootstrap; the properties of a kind that the driver, the int8 Gram and plspm_bootstrap() act on are the predicates below.
struct BatchCall {
    // where the problems' counts come from: PLAIN draws B resamples (Philox keys of `seed`, replicates rep_offset .., or the explicit rows at d_idx [B][N]);
    // the other kinds bring a spec (host_internal.h) their own count kernel reads, and leave seed / rep_offset / d_idx at zero
    enum Kind { PLAIN, PERMUTATION, STRATIFIED, CROSS_VALIDATION, JACKKNIFE, REBUS } kind = PLAIN;
    union { const PermSpec* perm = nullptr; const StratSpec* strat; const CvSpec* cv; const JackSpec* jack; const RebusSpec* rebus; };
    int64_t B = 0, rep_offset = 0;       // B problems
    uint64_t seed = 0;
    const int32_t* d_idx = nullptr;
    // where the results go: null = the handle's own buffer, which the driver sizes (records: `rows`, valid afterwards as rows_B; `status`; `iters`).  A caller's
    // record buffer (pitch plspm_row_stride: a group's send buffer, a sub-batch's place in `rows`, the jackknife's jack_rows) is the caller's to size; caller's
    // status / iteration buffers (the jackknife's) are grown by the driver
    double* rows_out = nullptr;
    plspm_model::Buf *status_out = nullptr, *iters_out = nullptr;
    double* moments_out = nullptr;       // test seam (plspm_bootstrap_moments): the problems' dense moment matrices go here and the solver is skipped
    int64_t chain_off = -1;              // >= 0: the call is a sub-batch of plspm_bootstrap() whose derived records (plspm_derived.hip) start here in the caller's buffers
    // in: the LAST kernel of the batch may signal this event on completion instead of a hipEventRecord behind it (plspm_group.cpp: ~5 us of every step);
    // out: a launch took it (the dense metric solvers do, plspm_fit.hip launch_signalling; every other route leaves the event to the caller)
    hipEvent_t stop_event = nullptr;
    bool stop_taken = false;
};
// The kind brings its own counts: the int8 route whatever "gram_path" / "i8_min_batch" say (its caller asked gram_counts_route_open), seven digit planes at
// least (their counts add up to less than N: plspm_gram_i8.hip prepare_zs), and no draws on the aux stream.
inline bool brings_counts(const BatchCall& c) { return c.kind != BatchCall::PLAIN; }
// The call leaves the handle's records alone (the jackknife: buffers of its own, so that the bootstrap whose BCa intervals ask for it keeps its records; REBUS-PLS:
// the local models of a round, in buffers of their own as well).
inline bool keeps_records(const BatchCall& c) { return c.kind == BatchCall::JACKKNIFE || c.kind == BatchCall::REBUS; }
// Problems 2p / 2p + 1 are the two sides of split p of the resident rows: what a MICOM record compares.
inline bool pairs_problems(const BatchCall& c) { return c.kind == BatchCall::PERMUTATION; }
// The handle kinds the two-group tests, the cross-validation, the jackknife, the assessment and MICOM cover.
inline bool plain_metric(const plspm_model* m) { return !m->nonmetric && !m->categorical && !m->n_ind && !m->nmx_K && !m->stage1 && !m->stage2; }
// (which plain bootstrap gets derived records: plspm_derived.hip derived_begin)

// The records on a handle, and the one place that voids them.  A batch call voids whatever went with the bootstrap records it replaces (REC_ROWS itself only
// when it writes the handle's own `rows`); plspm_bootstrap_store replaces the bootstrap records from the host; an upload voids everything.
enum : unsigned { REC_ROWS = 1, REC_CV = 2, REC_ASSESS = 4, REC_MICOM = 8, REC_JACK = 16, REC_PLSC = 32, REC_ALL = 63 };
inline void void_records(plspm_model* m, unsigned which) {
    if (which & REC_ROWS) m->rows_B = 0;
    if (which & REC_CV) m->cv_reps = 0;
    if (which & REC_MICOM) m->micom_B = 0;
    if (which & REC_JACK) m->jack_G = 0;
    // REC_ASSESS / REC_PLSC: that stage's records, and with them those of every stage that was computed from them (derived_route.h kDerivedStage: a stage's
    // records go when a stage it reads goes, and a row reads rows before it).  PLSc reads the assessment, so REC_ASSESS takes every derived record with it and
    // REC_PLSC those from PLSc on; every caller names the two together.
    static_assert(plspm::kDerivedStage[plspm::STAGE_PLSC].reads & plspm::stage_bit(plspm::STAGE_ASSESS), "REC_ASSESS voids the PLSc records and what follows them");
    if (which & REC_ASSESS) m->mod_B = m->tet_B = m->ipma_B = 0;      // (the moderation, the tetrad and the IPMA records go exactly when the derived records do)
    int gone = (which & REC_ASSESS ? plspm::stage_bit(plspm::STAGE_ASSESS) : 0) | (which & REC_PLSC ? plspm::stage_bit(plspm::STAGE_PLSC) : 0);
    for (int s = 0; s < plspm::kDerivedStages; ++s)
        if (gone & (plspm::stage_bit(s) | plspm::kDerivedStage[s].reads)) { gone |= plspm::stage_bit(s); m->derived[s].B = 0; }
}
// (an entry point voids its own kind's records before it prepares the call -- plspm_cv_device REC_CV, plspm_jackknife_device REC_JACK -- and sets the count
//  again behind the driver; so does plspm_bootstrap() with REC_ASSESS, which every one of its sub-batches voids here once more)
inline void void_records(plspm_model* m, const BatchCall& c) {
    if (!keeps_records(c)) void_records(m, REC_CV | REC_ASSESS | REC_PLSC | REC_MICOM | (c.rows_out ? 0u : REC_ROWS));
}

// What is derived from the resident rows, and the one place that voids it: the tiled copy, the category codes and indicator bytes, the digit planes and their
// statistics.  replaced: plspm_upload brought new rows -- the records, the MICOM pool and an attached second stage's codes describe the old ones and go as well.
// plspm_model_set_incomplete_rows rewrote some rows in place and voids none of those: it takes Scale.NUM handles outside a two-stage pair only, which have no
// second stage and, not being plain metric, no MICOM pool and no records but the bootstrap's own.  That those (REC_ROWS) survive the call is inherited behaviour.
inline void void_resident(plspm_model* m, bool replaced) {
    m->Xt_valid = false; m->codes_valid = false; m->ind8_valid = false; m->zs_valid = false; m->zs_stats_ready = false;
    if (!replaced) return;
    if (m->stage2) { m->stage2->codes_valid = false; m->stage2->ind8_valid = false; }
    void_records(m, REC_ALL);
    m->micom_pool_valid = false;
    m->scores_valid = false; m->fimix_nprob = 0;      // (plspm_fimix.hip: the scores and the mixture records describe the old rows)
    m->rebus_K = 0;                                   // (plspm_rebus.hip: so do the classes)
}

// The batch driver (plspm_bootstrap.hip): enqueue the call's problems on the handle's stream.  No host synchronisation for metric models.
int plspm_detail_bootstrap(plspm_model* m, BatchCall& call);
// plspm_group.cpp: a handle that is destroyed while bound to a group takes the group's hold on every handle with it.
void plspm_detail_group_orphan(void* group);
// Host -> device copy through the handle's pinned staging halves (chunked; returns when the source may be re-used).
int plspm_detail_h2d(plspm_model* m, void* dst, const void* src, size_t bytes);
// Summary statistics of device records (plspm_bootstrap_summary without the argument checks on `rows`): `ncols` value columns, the status in column `ncols`
// (bootstrap records: plspm_row_width; assessment records: plspm_assess_width).
int plspm_detail_summary(plspm_model* m, const double* rows, int64_t B, int32_t stride, int32_t ncols, const double* original, double* summary, int64_t* n_used);
// Confidence intervals of device records (plspm_bootstrap_intervals without the argument checks on `rows`).
int plspm_detail_intervals(plspm_model* m, const double* rows, int64_t B, int32_t stride, int32_t ncols, const double* original, const double* accel, int32_t method, double level, double* out,
                           int64_t* n_used);
// Host copy of device records [B x stride] -> rows [B x R], status, iters (any may be NULL), through the pinned staging buffer.
int plspm_detail_fetch_records(plspm_model* m, const double* d_records, int64_t B, int32_t stride, double* out, int32_t* status, int32_t* iters);

// Sub-batches of ONE call of B units (replicates) whose results leave the device behind the kernels -- over PCIe (plspm_bootstrap) or through the
// collective (plspm_group_bootstrap): sizes in a geometric progression (ratio_pct / 100: what moving a unit costs relative to computing it), so that
// the transfer of sub-batch k hides under the kernels of sub-batch k + 1 and only the last, smallest transfer is exposed; every part but the last
// a multiple of `align` units (64: whole count tiles of the int8 Gram; plspm_detail_round_units: whole rounds of the machine).  chunks_opt 0: automatic (one part below 2 MiB of results, else up to three),
// n >= 1: n parts.  Returns the number of parts (<= kBootChunksMax), sizes in parts[].  Host arithmetic only (group_route.h chunk_plan).
using plspm::kBootChunksMax;
int plspm_detail_chunk_plan(int64_t B, int64_t bytes_per_unit, int chunks_opt, int ratio_pct, int64_t* parts, int64_t align = 64);
// Replicates that fill ONE round of the device with tall tiles of the int8 Gram on this handle's model (whole tile rows: a row of tall tiles
// is 320 / 256 replicates x every pair tile) -- the alignment of the sub-batches of a call: a part that ends inside a round pays for the
// whole round (5,000 replicates of the headline model as 2,560 + 1,536 + 904: Gram 0.42 ms; as 2,560 + 1,280 + 1,160: 0.35; one batch 0.334).
// 64 when the handle's bootstrap does not take that Gram.  plspm_gram_i8.hip.
int64_t plspm_detail_round_units(plspm_model* m);
// The same figure from the handle's state AS IT IS -- no allocation, no launch, no host wait: 64 while the digit planes of the current upload
// have not been built (read-only queries: plspm_model_get_option "boot_round_units", plspm_group_plan).
int64_t plspm_detail_round_units_peek(const plspm_model* m);
// plspm_group.cpp: the sub-batch alignment a group's ranks agreed on is void after an upload / option change on one of its handles (calls
// every rank of a job makes alike); the next plspm_group_bootstrap agrees again.
void plspm_detail_group_plan_changed(void* group);
struct FetchSeg { int64_t b0, nb; hipEvent_t ready; };

// Same-device record exchange of a group (plspm_bootstrap.hip): send[i] -> recv[d] + i * doubles for all i, d < n, one launch on `stream`.
#define PLSPM_GATHER_LOCAL_MAX 16
// ndst: the first `ndst` receive buffers are filled (n: all-gather; 1: the gather to rank 0 of group option "gather_root").
int plspm_detail_gather_local(hipStream_t stream, int n, const double* const* send, double* const* recv, size_t doubles, int ndst);

inline int fail(plspm_model* m, int code, const std::string& msg) {
    if (m) m->error = msg; else g_create_error = msg;
    return code;
}
#define HIPCHK(m, call)                                                                                         \
    do {                                                                                                        \
        hipError_t e__ = (call);                                                                                \
        if (e__ != hipSuccess) { (void)hipGetLastError(); /* (the runtime's last-error word is per thread and sticky: a later hipGetLastError() check of ANOTHER handle must not inherit it) */ \
            return fail((m), -(int)e__, std::string(#call) + ": " + hipGetErrorString(e__)); }                  \
    } while (0)

inline int ensure(plspm_model* m, plspm_model::Buf& b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    if (b.p) HIPCHK(m, hipStreamSynchronize(m->stream));     // nothing of this handle may still be using the old block
    HIPCHK(m, b.reserve(bytes));      // (plspm_group.cpp calls reserve itself: it has synchronised every stream of the group, and its errors are the group's)
    return 0;
}

struct ProfScope {
    plspm_model* m; int id; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
    bool on;
    ProfScope(plspm_model* m_, int id_, hipStream_t stream = nullptr) : m(m_), id(id_), s(stream ? stream : m_->stream), on(m_->profiling && (m_->prof_only < 0 || m_->prof_only == id_)) {
        if (on) {
            auto& pool = m->prof[id].pool;
            if (pool.empty()) { hipEventCreate(&a); hipEventCreate(&b); }
            else { a = pool.back().first; b = pool.back().second; pool.pop_back(); }
            hipEventRecord(a, s);
        }
    }
    ~ProfScope() {
        if (on) { hipEventRecord(b, s); m->prof[id].ev.emplace_back(a, b); }
    }
};
inline void prof_collect(plspm_model* m) {
    for (int k = 0; k < PLSPM_K_COUNT; ++k) {
        for (auto& pr : m->prof[k].ev) {
            float ms = 0.f;
            hipEventSynchronize(pr.second);
            hipEventElapsedTime(&ms, pr.first, pr.second);
            m->prof[k].total_ms += ms; m->prof[k].launches += 1;
            m->prof[k].pool.push_back(pr);
        }
        m->prof[k].ev.clear();
    }
}
