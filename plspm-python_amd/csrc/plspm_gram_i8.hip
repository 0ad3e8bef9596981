// plspm_gram_i8.hip -- host side, part 3: the digit planes of the resident data and the int8 MFMA Gram of bootstrap batches (resample counts
// + one exact integer product; kernels_gram_i8.h, kernels_gram_i8p.h), the cut of a batch into tile rows, plspm_bootstrap_prepare.
#include "host_internal.h"

#include <optional>
#include "philox.h"
#include "wave_ops.h"
#include "kernels_gram_i8.h"
#include "kernels_gram_i8p.h"

// ------------------------------------------------------------------------------------------------ int8 digit-plane Gram (kernels_gram_i8.h)
// (whether the route is open for a data set and which calls take it: batch_route.h gram_i8_closed / choose_gram_path)
static int cu_count_of(plspm_model* m) {
    if (!m->cu_count && hipDeviceGetAttribute(&m->cu_count, hipDeviceAttributeMultiprocessorCount, m->device) != hipSuccess) m->cu_count = 0;
    return m->cu_count;
}

// Digit planes + pair tables of the resident data (once per upload / digit count).
// How many digit planes ("i8_slices" 0 = automatic).  S planes represent every product with an absolute error of at most
// 2^-(8S-1) max|z| of its column (zs_scale_kernel), so a replicate's sum is off by at most N 2^-(8S-1) max|z| (the multiplicities add up
// to N) -- the integer sum itself is exact.  A sequential fp64 accumulation of the same N terms carries the a-priori bound gamma_N sum|z|
// ~ N 2^-53 sum|z|.  S planes are therefore within the error bound of fp64 arithmetic on the same data whenever
//       sum_i |z_i|  >=  2^(54 - 8S) max_i |z_i|        in every pair column:      S = 7: always,   S = 6: sum >= 64 max.
// Automatic = 6 planes if every column clears that bar with a factor 4 to spare (sum >= 256 max; a resample re-weights the terms:
// sum_i c_i |z_i| scatters by a few percent around sum_i |z_i|), else 7.  Data sets of a few hundred rows stay at 7; 10,000 rows of
// anything bell-shaped reach several hundred.  Measured against 80-bit sums on the 10k x 60 benchmark data (tests/test_gpu_gram_i8.py,
// error relative to sqrt(M_pp M_qq)): seven planes 1e-16 (correctly rounded), six planes 3e-15, the blocked fp64 MFMA accumulation
// 1.6e-15 -- all nine orders below the 1e-6 the records are held to.
static int choose_slices(plspm_model* m, const unsigned long long* h, long npair, int* S_out, int floor) {      // h: [max bits | fixed-point sums | OR of the scaled integers], on the host
    double worst = 1e300;
    unsigned long long any = 0ull;
    for (long j = 0; j < npair; ++j) any |= h[2 * npair + j];
    for (long j = 0; j < npair; ++j) {
        const unsigned long long mb = h[j];
        if (mb == 0) continue;                                            // an all-zero column has nothing to round
        const int ef = (int)((mb >> 52) & 0x7ffull);
        if (ef < 64 || ef >= 0x7ff) { worst = 0.0; break; }               // tiny or non-finite maximum: not evaluated, full plane count
        double zmax;
        memcpy(&zmax, &mb, sizeof(double));
        const double sum = std::ldexp((double)h[npair + j], (ef - 1022) - 40);
        worst = std::min(worst, sum / zmax);
    }
    m->zs_ratio = worst;
    // (round 5: EIGHT planes when some column's sum barely exceeds its largest product -- sum < 2 max: one gross outlier row carries the column.  A
    //  replicate that does not draw that row sums products that are tiny against the column maximum the planes are scaled to; seven planes then
    //  leave ~1e-14 of ITS moment (measured: tests/test_gpu_gram_i8.py, a 900-sigma cell), eight stay below fp64's own rounding.  Same a-priori
    //  argument as for six / seven with the dominant row taken out of the sum: sum - max >= 2^(56 - 8S) max.)
    int S = worst >= 257.0 ? 6 : (worst >= 2.0 ? 7 : 8);
    if (m->tune.i8_min_slices > S) S = m->tune.i8_min_slices;              // "i8_min_slices": the automatic choice, but never fewer (Plspm(precision="strict"): 7)
    if (floor > S) S = floor;                                               // (prepare_zs's floor: the same rule for one kind of call)
    // planes that would be identically zero in the seven-plane decomposition carry nothing: dropping them changes no sum
    int zero_planes = 0;
    if (worst > 0.0) {
        zero_planes = 6;
        if (any) { int tz = 0; while (!((any >> tz) & 1ull)) ++tz; zero_planes = std::min(6, tz / 8); }
    }
    if (zero_planes > 0) S = std::min(S, 7 - zero_planes);                   // (data on a coarse binary grid are EXACT on fewer planes, whatever the rule above asked for)
    if (m->tune.i8_shape == 32) S = std::max(S, 5);                            // (the 32x32x32 layout is instantiated for 5 .. 8 planes)
    *S_out = S;
    return 0;
}

// Phase 1 of the digit planes (enqueue only -- plspm_bootstrap_prepare): pair tables, column maxima of the pair products and, for the
// automatic plane count, the two column statistics, copied to a pinned block behind an event.  Nothing here waits for the device: the
// plane count is read in phase 2 (prepare_zs), by which time the fit that was enqueued behind this has long synchronised the stream.
int prepare_zs_stats(plspm_model* m) {
    if (m->zs_valid || m->zs_stats_ready) return 0;
    const int C = m->Pg + 1;
    const long npair = i8_pairs(m);
    std::vector<int> tab(7 * (size_t)npair);
    int* hp = tab.data(); int* hq = hp + npair; int* hd = hq + 2 * npair;       // [p | q | k (device) | packed slot | dense slot | mirrored dense slot | uint16 count-matrix slot]
    int* hd1 = hd + npair; int* hd2 = hd1 + npair; int* hd16 = hd2 + npair;
    const int PSd = cov_ld(m->Pg), ld16 = (C + 7) & ~7;                          // (ld16: the pitch of run_nonmetric's uint16 count matrices)
    long j = 0;
    for (int p = 0; p < C; ++p)
        for (int q = p; q < C; ++q, ++j) {
            hp[j] = p; hq[j] = q; hd[j] = (int)packed_index(m->T, p, q);
            hd1[j] = p * PSd + q; hd2[j] = (p == q) ? -1 : q * PSd + p;
            hd16[j] = p * ld16 + q;
        }
    int rc;
    if ((rc = ensure(m, m->pair_tab, tab.size() * sizeof(int)))) return rc;
    if ((rc = ensure(m, m->pair_scale, (size_t)npair * sizeof(double)))) return rc;
    if ((rc = ensure(m, m->zs_stat, 3 * (size_t)npair * sizeof(unsigned long long)))) return rc;
    if ((rc = plspm_detail_h2d(m, m->pair_tab.p, tab.data(), tab.size() * sizeof(int)))) return rc;
    int* d_p = (int*)m->pair_tab.p; int* d_q = d_p + npair;
    ProfScope ps(m, PLSPM_K_PACK);
    unsigned long long* d_max = (unsigned long long*)m->zs_stat.p;
    HIPCHK(m, hipMemsetAsync(d_max, 0, 3 * (size_t)npair * sizeof(unsigned long long), m->stream));
    const int RB = (int)std::max<size_t>(1, std::min<size_t>(64, (kMaxLds - 1024) / ((size_t)(C | 1) * sizeof(double))));
    const size_t lds = (size_t)RB * (C | 1) * sizeof(double);
    if ((rc = allow_lds(m, (const void*)zs_max_kernel, lds))) return rc;
    hipLaunchKernelGGL(zs_max_kernel, dim3((unsigned)((m->N + RB - 1) / RB)), dim3(256), lds, m->stream, (const double*)m->d_Xa, (long)m->N, m->PA, C, d_p, d_q, (int)npair, RB, d_max);
    if (m->tune.i8_slices == 0) {
        if ((rc = allow_lds(m, (const void*)zs_abssum_kernel, lds))) return rc;
        hipLaunchKernelGGL(zs_abssum_kernel, dim3((unsigned)((m->N + RB - 1) / RB)), dim3(256), lds, m->stream, (const double*)m->d_Xa, (long)m->N, m->PA, C, d_p, d_q, (int)npair, RB,
                           (const unsigned long long*)d_max, d_max + npair, d_max + 2 * npair);
        HIPCHK(m, hipGetLastError());
        const size_t bytes = 3 * (size_t)npair * sizeof(unsigned long long);
        HIPCHK(m, m->h_zstat.reserve(bytes));
        if (!m->ev_zstat) HIPCHK(m, hipEventCreateWithFlags(&m->ev_zstat, hipEventDisableTiming));
        HIPCHK(m, hipMemcpyAsync(m->h_zstat.p, d_max, bytes, hipMemcpyDeviceToHost, m->stream));
        HIPCHK(m, hipEventRecord(m->ev_zstat, m->stream));
    }
    HIPCHK(m, hipGetLastError());
    m->zs_stats_ready = true; m->zs_stats_S = m->tune.i8_slices;
    return 0;
}

// floor > 0: never fewer than `floor` planes, for the calls that ask for it (the two-group permutation test: 7, plspm_permute.hip) -- the automatic
// rule above assumes multiplicities that add up to N, a group of n1 << N rows does not.  Planes of the current upload built under another floor
// are cut again from the column statistics already at hand (no second pass over the data, no host wait): such calls and the bootstrap's own
// automatic choice can alternate on one handle.
int prepare_zs(plspm_model* m, int floor) {
    if (m->zs_valid && m->zs_floor == floor) return 0;
    if (m->zs_valid) {
        if (m->zs_stats_S == m->tune.i8_slices) m->zs_stats_ready = true;      // (pair tables, column maxima and the pinned statistics of this upload are still in place)
        m->zs_valid = false;
    }
    int rc;
    if (m->zs_stats_ready && m->zs_stats_S != m->tune.i8_slices) m->zs_stats_ready = false;      // the option changed in between
    if ((rc = prepare_zs_stats(m))) return rc;
    int S = m->tune.i8_slices ? std::max(m->tune.i8_slices, floor) : 0;
    const long npair = i8_pairs(m);
    const int npg = (int)((npair + 31) / 32) * 2;             // pair groups of 16, padded to whole workgroup tiles (two groups)
    const int KB = i8_kblocks(m->N);
    int* d_p = (int*)m->pair_tab.p; int* d_q = d_p + npair; int* d_k = d_q + npair;
    unsigned long long* d_max = (unsigned long long*)m->zs_stat.p;
    ProfScope ps(m, PLSPM_K_PACK);
    if (S == 0) {
        HIPCHK(m, hipEventSynchronize(m->ev_zstat));          // (long done when a fit ran behind plspm_bootstrap_prepare)
        if ((rc = choose_slices(m, (const unsigned long long*)m->h_zstat.p, npair, &S, floor))) return rc;
    }
    hipLaunchKernelGGL(zs_scale_kernel, dim3((unsigned)((npair + 255) / 256)), dim3(256), 0, m->stream, d_max, (int)npair, S, d_k, (double*)m->pair_scale.p);
    // one plane (0/1 data): the product runs through the seven-plane main loop with the planes of a wave standing for seven consecutive
    // pair groups (gram_i8_kernel<.., IND>): the buffer is padded to whole tiles of 2 x 7 groups
    const bool ind = S == 1 && m->tune.i8_shape == 16 && m->tune.i8_ind != 0;
    const int npg_built = ind ? ((npg + 13) / 14) * 14 : npg;
    const int NT = npg_built * S;
    if ((rc = ensure(m, m->zs, (size_t)(KB + I8_SLACK_KB) * (size_t)NT * 1024))) return rc;      // (sized once the plane count is known: 0/1 data take one plane)
    const dim3 grid((unsigned)KB, (unsigned)((npg_built + 3) / 4));
#define ZSB(SS) hipLaunchKernelGGL((zs_build_kernel<SS>), grid, dim3(256), 0, m->stream, (const double*)m->d_Xa, (long)m->N, m->PA, d_p, d_q, d_k, (int)npair, npg_built, NT, m->tune.i8_shape, (uint4*)m->zs.p)
    switch (S) { case 1: ZSB(1); break; case 2: ZSB(2); break; case 3: ZSB(3); break; case 4: ZSB(4); break; case 5: ZSB(5); break; case 6: ZSB(6); break; case 7: ZSB(7); break; default: ZSB(8); break; }
#undef ZSB
    HIPCHK(m, hipGetLastError());
    m->zs_S = S; m->zs_KB = KB; m->zs_NT = NT; m->zs_npair = (int)npair; m->zs_npg = npg_built; m->zs_ind = ind;
    m->zs_valid = true; m->zs_stats_ready = false; m->zs_floor = floor;
    return 0;
}

// ------------------------------------------------------------------------------------------------ one chunk through the int8 Gram, phase by phase
// gram_route.h decides the form of the launch (gram_i8_plan); the launchers below only carry it out.
static GramI8Data gram_data_of(const plspm_model* m) { return GramI8Data{m->zs_S, m->zs_KB, m->zs_NT, m->zs_npg, m->zs_ind}; }
static GramI8Options gram_options_of(const plspm_model* m) {
    return GramI8Options{m->tune.i8_priv, m->tune.i8_persist, m->tune.i8_rt, m->tune.i8_short, m->tune.i8_cus, m->tune.i8_dma, m->tune.i8_nibbles, m->tune.i8_waves, m->tune.i8_shape, m->tune.i8_sched, m->tune.i8_variant};
}

// the one launch of a kernel with dynamic LDS
template <class K, class... A>
static int launch_lds(plspm_model* m, hipStream_t stream, K kfn, size_t lds_bytes, dim3 grid, dim3 block, A... args) {
    if (const int rc = allow_lds(m, (const void*)kfn, lds_bytes)) return rc;
    hipLaunchKernelGGL(kfn, grid, block, lds_bytes, stream, args...);
    return 0;
}

// What the product's launch reads beside the plan: the counts, the destination table and stride of the moment matrices, the replicates whose results are stored
struct GramLaunch { plspm_model* m; const GramI8Plan& p; const void* cd; const int* d_dst; double* out; long out_stride; long nrep; };
// ... and the launch: every Gram kernel starts with the same eight arguments
template <class K, class... A>
static int launch_gram(const GramLaunch& g, K kfn, size_t lds_bytes, A... tail) {
    return launch_lds(g.m, g.m->stream, kfn, lds_bytes, dim3((unsigned)g.p.grid), dim3((unsigned)g.p.block), (const uint4*)g.cd, (const uint4*)g.m->zs.p, g.m->zs_KB, g.p.MT, g.m->zs_NT,
                      g.p.ntx, g.p.nty, g.d_dst, tail...);
}
// the round-3 kernel (kernels_gram_i8.h gram_i8_kernel).  No second destination table: a mirrored second store per element cost 0.08 ms per 5,000 replicates of the
// metric benchmark -- the rows solver reads the triangle instead.  Categorical problems, whose solver wants the full square: Gram 1.40 -> 2.07 ms per 1,000 problems with
// the mirrored stores against 0.4 ms saved in nmg_prepare's scatter -- not taken either.
template <int S, int WM, int VAR, int SH = 16, int RT = 16, bool IND = false>
static int launch_r3(const GramLaunch& g) {
    using G = GramI8<S, WM, VAR, SH, RT>;
    if (g.p.nty_short && !G::MIX) return fail(g.m, PLSPM_E_STATE, "int8 Gram: short tile rows planned for a kernel form without them");
    return launch_gram(g, gram_i8_kernel<S, WM, VAR, SH, RT, IND>, G::LDS_BYTES, (const int*)nullptr, (const double*)g.m->pair_scale.p, g.m->zs_npair, (long)g.p.call.nb, g.out, g.out_stride,
                       IND ? (g.p.to16 ? -1 : 0) : g.p.nty_short);
}
// the private-count kernel (kernels_gram_i8p.h gram_i8p_kernel): MTW count tiles per wave of a tall row
template <int S, int VAR>
static int launch_priv(const GramLaunch& g) {
    constexpr int MTW = gram_i8p_tall(S) / 4;
    const auto kfn = g.p.nty_short ? gram_i8p_kernel<S, MTW, VAR, true> : gram_i8p_kernel<S, MTW, VAR, false>;
    return launch_gram(g, kfn, GramI8P<S, MTW, VAR>::LDS_BYTES, (const double*)g.m->pair_scale.p, g.m->zs_npair, g.nrep, g.out, g.out_stride, g.p.nty_short);
}
// ... and the same tiles on ONE persistent workgroup per CU (gram_i8pp_kernel: tiles from a per-XCD counter, the next tile's prologue in front of this tile's
// epilogue; "i8_persist" 0: the tiled launch, kept as the A/B reference)
template <int S>
static int launch_persist(const GramLaunch& g) {
    constexpr int MTW = gram_i8p_tall(S) / 4;
    const auto kfn = g.p.nty_short ? gram_i8pp_kernel<S, MTW, 64, true> : gram_i8pp_kernel<S, MTW, 64, false>;
    return launch_gram(g, kfn, GramI8P<S, MTW, 64>::LDS_BYTES + 64, (const double*)g.m->pair_scale.p, g.m->zs_npair, g.nrep, g.out, g.out_stride, g.p.nty_short, (GramI8PPCtl*)g.m->pp_ctl.p);
}
// the plane count as a template argument
template <int WM, int VAR>
static int launch_planes(const GramLaunch& g) {
    switch (g.m->zs_S) {
        case 1: return launch_r3<1, WM, VAR>(g); case 2: return launch_r3<2, WM, VAR>(g); case 3: return launch_r3<3, WM, VAR>(g); case 4: return launch_r3<4, WM, VAR>(g);
        case 5: return launch_r3<5, WM, VAR>(g); case 6: return launch_r3<6, WM, VAR>(g); case 7: return launch_r3<7, WM, VAR>(g); default: return launch_r3<8, WM, VAR>(g);
    }
}
template <int VAR>
static int launch_priv_planes(const GramLaunch& g) { return g.m->zs_S == 6 ? launch_priv<6, VAR>(g) : launch_priv<7, VAR>(g); }

// the forms of the round-3 kernel that exist with eight waves (WM 4) and with four (WM 2): one plane per pair group, the 320-replicate tile (its buffer form deals
// 20 count blocks to four waves only), any plane count on the 256-replicate tile; VB: LDS-DMA as buffer_load ... lds, 32-bit offsets from per-workgroup descriptors
template <int WM>
static int launch_round3(const GramLaunch& g) {
    constexpr int V0 = I8_DEFAULT_VAR, VB = I8_DEFAULT_VAR + 800;
    switch (g.p.form) {
        case GRAM_I8_IND: return g.p.dma_buffer ? launch_r3<7, WM, VB, 16, 16, true>(g) : launch_r3<7, WM, V0, 16, 16, true>(g);
        case GRAM_I8_WIDE20: if constexpr (WM == 2) { if (g.p.dma_buffer) return launch_r3<6, WM, VB, 16, 20>(g); } return launch_r3<6, WM, V0, 16, 20>(g);
        default: return g.p.dma_buffer ? launch_planes<WM, VB>(g) : launch_planes<WM, V0>(g);
    }
}

// Release library: the eight-wave forms of the round-3 kernel and the private-count kernel only -- four waves measured equal, the 32x32x32 layout 16 % slower, the narrow
// 128-replicate tile 2.6 % slower, the persistent stream-K launch neutral with a starvation hazard: DESIGN.md 7b.  `make experiments` builds them, the schedule variants
// and the timing probe: launch_gram_experiment takes the launches that exist only there (its value: how the launch went) and declines the others (no value).
#ifdef PLSPM_I8_EXPERIMENTS
static constexpr bool kI8Experiments = true;
template <int... VV, class F>
static bool for_variant(int v, std::integer_sequence<int, VV...>, F&& f) { return ((v == VV && (f(std::integral_constant<int, VV>{}), true)) || ...); }
template <int S, int WM>
static int launch_sk(const GramLaunch& g) {       // persistent stream-K schedule (kernels_gram_i8.h gram_i8_sk_kernel)
    return launch_gram(g, gram_i8_sk_kernel<S, WM>, GramI8<S, WM, I8_DEFAULT_VAR, 16>::LDS_BYTES, (const double*)g.m->pair_scale.p, g.m->zs_npair, (long)g.p.call.nb, g.out, g.out_stride,
                       (i32x4*)g.m->sk_partial.p, (unsigned*)g.m->sk_flags.p, ++g.m->sk_epoch, (int*)g.m->err.p);
}
static std::optional<int> launch_gram_experiment(GramLaunch& g) {
    plspm_model* m = g.m;
    const GramI8Plan& p = g.p;
    constexpr int V0 = I8_DEFAULT_VAR;
    const bool four = p.waves == 4;
    const int S = m->zs_S;
    std::optional<int> rc;
    // timing probe (results are garbage): "i8_nostore" 1 launches both forms of the private-count kernel with nrep = 0 -- every epilogue store (and the fp64
    // recombination in front of it) is skipped; tools/persist_ab.py prices the epilogue of the tiled and of the persistent form with it
    if (m->tune.i8_nostore && (p.form == GRAM_I8_PRIV || p.form == GRAM_I8_PERSIST)) g.nrep = 0;
    switch (p.form) {
        case GRAM_I8_PRIV:
            // "i8_variant" v >= 0: the template's VAR itself -- bits 0-3 ablations, bit 4 digit blocks through staging registers, bits 5-6 the filler schedule
            // (0 strides / 1 one per gap, DMAs last / 2 VMEM evenly spaced = the release kernel), bit 7 one barrier per two k-steps
            for_variant(p.variant, std::integer_sequence<int, 0, 1, 2, 4, 8, 15, 16, 32, 128, 192, 64, 65, 66, 68, 72, 69, 77, 79>{}, [&](auto v) { rc = launch_priv_planes<decltype(v)::value>(g); });
            return rc ? rc : fail(m, PLSPM_E_ARG, "i8_variant: not a built variant of the private-count kernel");
        case GRAM_I8_SK:
            return four ? (S == 5 ? launch_sk<5, 2>(g) : S == 6 ? launch_sk<6, 2>(g) : launch_sk<7, 2>(g)) : (S == 5 ? launch_sk<5, 4>(g) : S == 6 ? launch_sk<6, 4>(g) : launch_sk<7, 4>(g));
        case GRAM_I8_PLAIN:
            if (p.variant >= 0) {      // every schedule variant of the 7-plane kernel (tools/i8_bench.py --variants); a number that is not built: 33
                auto go = [&](auto v) { constexpr int V = decltype(v)::value; rc = four ? launch_r3<7, 2, V>(g) : launch_r3<7, 4, V>(g); };
                if (!for_variant(p.variant, std::integer_sequence<int, 0, 3, 6, 4, 803, 103, 203, 303, 403, 503, 703, 12, 18, 21, 24, 30>{}, go)) go(std::integral_constant<int, 33>{});
                return rc;
            }
            return four ? launch_round3<2>(g) : rc;
        case GRAM_I8_IND: return four ? launch_round3<2>(g) : rc;
        case GRAM_I8_WIDE20:
            if (p.variant < 0) return four ? launch_round3<2>(g) : rc;
            for_variant(p.variant, std::integer_sequence<int, 0, 1, 3, 4, 5, 6, 7, 12, 13, 18, 21, 103, 203, 403, 703>{}, [&](auto v) { rc = launch_r3<6, 4, decltype(v)::value, 16, 20>(g); });
            return rc ? rc : fail(m, PLSPM_E_ARG, "i8_variant: not built for the 320-replicate tile");
        case GRAM_I8_NARROW: return launch_r3<7, 2, V0, 16, 8>(g);
        case GRAM_I8_SHAPE32:          // v_mfma_i32_32x32x32_i8: four waves (64 replicates x 32 pairs x S planes each)
            return S == 5 ? launch_r3<5, 2, V0, 32>(g) : S == 6 ? launch_r3<6, 2, V0, 32>(g) : S == 7 ? launch_r3<7, 2, V0, 32>(g) : launch_r3<8, 2, V0, 32>(g);
        default: return rc;
    }
}
#else
static constexpr bool kI8Experiments = false;
static std::optional<int> launch_gram_experiment(GramLaunch&) { return std::nullopt; }
#endif

// plan: the three inputs of gram_i8_plan from the handle and the call; the handle keeps the last tile-row cut
static int gram_i8_plan_chunk(plspm_model* m, const BatchCall& call, int64_t nb, bool want16, GramI8Plan& p) {
    if (!cu_count_of(m)) return fail(m, PLSPM_E_STATE, "hipDeviceGetAttribute(multiprocessor count) failed");
    p = gram_i8_plan(gram_data_of(m), gram_options_of(m), GramI8Call{nb, call.d_idx != nullptr, brings_counts(call), want16, m->cu_count, kI8Experiments}, &m->mix_cut);
    return 0;
}

static int launch_resample(plspm_model* m, const GramI8Plan& p, hipStream_t stream, const int32_t* d_idx, uint64_t seed, int64_t rep0, void* cd, void* err) {
    const dim3 grid((unsigned)p.call.nb, p.hist_windows), block(p.hist_threads);
    // (4-bit counters: option "i8_nibbles" 2 sends every replicate through the 8-bit second try -- tests)
    if (p.hist == GRAM_I8_HIST4)
        return launch_lds(m, stream, resample_i8_nib_kernel, p.hist_bytes, grid, block, (int)m->N, m->zs_KB, p.MT, seed, rep0, (uint4*)cd, (int*)err, m->tune.i8_nibbles == 2 ? 1 : 0);
    const auto kfn = p.hist == GRAM_I8_HIST8 ? resample_i8_kernel<true> : resample_i8_kernel<false>;
    return launch_lds(m, stream, kfn, p.hist_bytes, grid, block, (int)m->N, m->zs_KB, p.MT, m->tune.i8_shape, d_idx, seed, rep0, (uint4*)cd, (int*)err);
}

// counts: the chunk's dense int8 multiplicities into *cd_out (buffer `*slot_out` of the two that alternate under "resample_aux")
static int gram_i8_counts(plspm_model* m, const BatchCall& call, const GramI8Plan& p, int64_t b0, int* slot_out, plspm_model::Buf** cd_out) {
    const int64_t nb = p.call.nb, rep0 = call.rep_offset + b0;
    const int32_t* const d_idx = call.d_idx ? call.d_idx + b0 * m->N : nullptr;
    int rc = 0;
    if (m->tune.resample_aux && !m->aux) {
        int lo = 0, hi = 0;
        HIPCHK(m, hipDeviceGetStreamPriorityRange(&lo, &hi));                // (numerically: lowest priority first)
        HIPCHK(m, hipStreamCreateWithPriority(&m->aux, hipStreamNonBlocking, m->tune.resample_aux == 2 ? 0 : (m->tune.resample_aux == 3 ? hi : lo)));
        for (int k = 0; k < 2; ++k) {
            HIPCHK(m, hipEventCreateWithFlags(&m->ev_counts[k], hipEventDisableTiming));
            HIPCHK(m, hipEventCreateWithFlags(&m->ev_cdfree[k], hipEventDisableTiming));
        }
        if ((rc = ensure(m, m->err2, sizeof(int)))) return rc;
        HIPCHK(m, hipMemsetAsync(m->err2.p, 0, sizeof(int), m->aux));
    }
    // counts of this chunk: the buffer the Gram before last read; grown only with both streams idle
    const int slot = m->aux ? (m->cd_slot ^= 1) : 0;
    plspm_model::Buf& cd = slot ? m->cd1 : m->cd;
    if (p.cd_bytes > cd.cap) { if (m->aux) HIPCHK(m, hipStreamSynchronize(m->aux)); if ((rc = ensure(m, cd, p.cd_bytes))) return rc; m->cdfree_set[slot] = false; }
    *slot_out = slot; *cd_out = &cd;
    // Philox draws: on the low-priority stream, as soon as the Gram that last read this buffer is done -- i.e. beside the Gram and the solver of the PREVIOUS call when
    // the host runs ahead; this call's Gram waits for the counts by event.  Explicit index lists (test / parity seam) and the kinds that bring their own counts
    // (rep_offset is 0, so rep0 is the chunk's first problem) arrive on the main stream: drawn there, and the host looks at the flag
    const bool on_aux = !d_idx && !p.call.own_counts && m->aux;
    const hipStream_t stream = on_aux ? m->aux : m->stream;
    if (m->aux && m->cdfree_set[slot]) HIPCHK(m, hipStreamWaitEvent(stream, m->ev_cdfree[slot], 0));
    {
        ProfScope ps(m, PLSPM_K_RESAMPLE, stream);
        switch (call.kind) {
            case BatchCall::PERMUTATION: rc = launch_perm_counts(m, *call.perm, nb, rep0, p.MT, m->zs_KB, cd.p); break;           // 0/1 counts of random splits, plspm_permute.hip
            case BatchCall::STRATIFIED: rc = launch_strat_counts(m, *call.strat, nb, rep0, p.MT, m->zs_KB, cd.p); break;          // ... its stratified bootstrap: draws inside each group
            case BatchCall::CROSS_VALIDATION: rc = launch_cv_counts(m, *call.cv, nb, rep0, p.MT, m->zs_KB, cd.p); break;         // 0/1 counts of the training folds, plspm_cv.hip
            case BatchCall::JACKKNIFE: rc = launch_jack_counts(m, *call.jack, nb, rep0, p.MT, m->zs_KB, cd.p); break;            // 0/1 counts of the rows a problem keeps, plspm_jackknife.hip
            case BatchCall::REBUS: rc = launch_rebus_counts(m, *call.rebus, nb, rep0, p.MT, m->zs_KB, cd.p); break;            // 0/1 counts of a class's rows, plspm_rebus.hip
            case BatchCall::PLAIN: rc = launch_resample(m, p, stream, d_idx, call.seed, rep0, cd.p, on_aux ? m->err2.p : m->err.p); break;
        }
    }
    if (rc) return rc;
    if (on_aux) {
        HIPCHK(m, hipEventRecord(m->ev_counts[slot], m->aux));
        HIPCHK(m, hipStreamWaitEvent(m->stream, m->ev_counts[slot], 0));
    }
    return 0;
}

// overflow check: explicit indices can carry a multiplicity above 127 (Philox draws of N >= 128 rows cannot, P < 1e-200): the host looks at the flag before the
// product and reports *fallback so that the caller takes the fp64 Gram for this chunk
static int gram_i8_overflow(plspm_model* m, bool* fallback) {
    int* h_err = (int*)m->h_flag + 9;
    HIPCHK(m, hipMemcpyAsync(h_err, m->err.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (*h_err & 2) {
        const int keep = *h_err & 1;
        HIPCHK(m, hipMemcpyAsync(m->err.p, &keep, sizeof(int), hipMemcpyHostToDevice, m->stream));
        HIPCHK(m, hipStreamSynchronize(m->stream));
        *fallback = true;
    }
    return 0;
}

// note: what get_option("last_i8_*") reports of the launch
static void gram_i8_note(plspm_model* m, const GramI8Plan& p) {
    m->last_i8_nibbles = p.hist == GRAM_I8_HIST4 ? 1 : 0; m->last_i8_dma = p.dma_buffer ? 2 : 1;
    m->last_i8_rt = p.rt_tall; m->last_i8_short = p.nty_short; m->last_i8_mt = p.MT;
    m->last_i8_priv = (p.form == GRAM_I8_PRIV || p.form == GRAM_I8_PERSIST) ? 1 : 0; m->last_i8_persist = p.form == GRAM_I8_PERSIST ? 1 : 0;
}

// gram: the product of the counts at `cd` with the digit planes.  packed: the tile-packed slots the LDS solver / impute kernel read; dense: [(Pg+1) x cov_ld(Pg)]
// row-major, upper triangle (rows solver); to16: uint16 [nb][C][ld16], upper triangle, at out16
static int gram_i8_product(plspm_model* m, const GramI8Plan& p, const void* cd, double* out, bool dense, unsigned short* out16, bool* wrote16) {
    const int* d_dst = (const int*)m->pair_tab.p + (p.to16 ? 6 : (dense ? 4 : 3)) * (size_t)m->zs_npair;
    const long out_stride = p.to16 ? (long)(m->Pg + 1) * ((m->Pg + 1 + 7) & ~7) : (dense ? cov_doubles(m->Pg) : packed_size(m->T));
    if (p.to16) { out = reinterpret_cast<double*>(out16); *wrote16 = true; }
    int rc;
    if (p.form == GRAM_I8_SK) {
        const size_t bytes = (size_t)p.sk_grid * 32 * m->zs_S * 1024;      // per workgroup: 16 count tiles x 2 pair groups x S planes x 1 KB of int32
        if (bytes > m->sk_partial.cap && (rc = ensure(m, m->sk_partial, bytes))) return rc;
        if (!m->sk_flags.p) {
            if ((rc = ensure(m, m->sk_flags, (size_t)2048 * 8 * sizeof(unsigned)))) return rc;
            HIPCHK(m, hipMemsetAsync(m->sk_flags.p, 0, (size_t)2048 * 8 * sizeof(unsigned), m->stream));
            m->sk_epoch = 0;
        }
    }
    if (p.form == GRAM_I8_PERSIST && !m->pp_ctl.p) {
        if ((rc = ensure(m, m->pp_ctl, sizeof(GramI8PPCtl)))) return rc;
        HIPCHK(m, hipMemsetAsync(m->pp_ctl.p, 0, sizeof(GramI8PPCtl), m->stream));      // (once: the kernel leaves the counters at zero)
    }
    ProfScope ps(m, PLSPM_K_GRAM);
    GramLaunch g{m, p, cd, d_dst, out, out_stride, (long)p.call.nb};
    if (const std::optional<int> took = launch_gram_experiment(g)) rc = *took;
    else if (p.form == GRAM_I8_PERSIST) rc = m->zs_S == 6 ? launch_persist<6>(g) : launch_persist<7>(g);
    else rc = p.form == GRAM_I8_PRIV ? launch_priv_planes<64>(g) : launch_round3<4>(g);
    if (!rc) HIPCHK(m, hipGetLastError());
    return rc;
}

// Resample nb replicates into dense int8 counts and multiply with the digit planes: the nb moment matrices land at `out` -- or, res->wrote16, as uint16 at out16
// (the one-plane launch on 0/1 data; any other launch writes `out` as ever).
int run_gram_i8(plspm_model* m, const BatchCall& call, int64_t nb, int64_t b0, double* out, bool dense, unsigned short* out16, GramI8Result* res) {
    *res = GramI8Result{};
    GramI8Plan p;
    plspm_model::Buf* cd = nullptr;
    int rc, slot = 0;
    if ((rc = gram_i8_plan_chunk(m, call, nb, out16 != nullptr, p))) return rc;
    if ((rc = gram_i8_counts(m, call, p, b0, &slot, &cd))) return rc;
    if (call.d_idx && ((rc = gram_i8_overflow(m, &res->fallback)) || res->fallback)) return rc;
    if (m->tune.i8_shape == 16) { res->counts = cd->p; res->counts_MT = p.MT; }       // (16-row pieces: what nm_conv_dense_kernel<.., CNT8> reads)
    gram_i8_note(m, p);
    if ((rc = gram_i8_product(m, p, cd->p, out, dense, out16, &res->wrote16))) return rc;
    if (m->aux) { HIPCHK(m, hipEventRecord(m->ev_cdfree[slot], m->stream)); m->cdfree_set[slot] = true; }     // the counts buffer is free once this Gram has run
    return 0;
}

int64_t plspm_detail_round_units_peek(const plspm_model* m) {
    if (!m || !m->d_Xa || m->nonmetric || m->n_ind || !m->zs_valid || !m->cu_count || choose_gram_path(m, (int64_t)1 << 20) != 2) return 64;
    return gram_i8_round_units(gram_data_of(m), gram_options_of(m), m->cu_count, kI8Experiments);
}

int64_t plspm_detail_round_units(plspm_model* m) {
    if (!m || !m->d_Xa || m->nonmetric || m->n_ind || choose_gram_path(m, (int64_t)1 << 20) != 2) return 64;
    if (hipSetDevice(m->device) != hipSuccess || prepare_zs(m) || !cu_count_of(m)) return 64;            // (the plane count decides the tile height; built once per upload anyway)
    return plspm_detail_round_units_peek(m);
}

extern "C" {

int plspm_bootstrap_prepare(plspm_model_t* m) {
    if (!m) return PLSPM_E_ARG;
    if (!m->d_Xa || m->N < 2) return fail(m, PLSPM_E_STATE, "plspm_bootstrap_prepare: no data uploaded");
    HIPCHK(m, hipSetDevice(m->device));
    // what the first bootstrap call on this data would build before its first replicate: the digit planes of the pair products
    // (enqueue only; a model that takes the fp64 Gram has nothing to prepare)
    // (automatic plane count: the column statistics are enqueued and copied to pinned memory behind an event -- no host wait here; the
    //  planes are cut by the first bootstrap call, which finds the statistics on the host.  A fixed plane count has nothing to read back:
    //  everything is enqueued now)
    if (choose_gram_path(m, (int64_t)1 << 20) == 2) return m->tune.i8_slices == 0 ? prepare_zs_stats(m) : prepare_zs(m);
    return 0;
}

int plspm_gram_tile_plan(int64_t count_tiles, int64_t pair_tiles, int32_t cus, int32_t mix, int32_t* tall, int32_t* shrt) {
    if (!tall || !shrt || count_tiles < 1 || pair_tiles < 1 || cus < 1 || count_tiles > ((int64_t)1 << 26) || pair_tiles > ((int64_t)1 << 20)) return PLSPM_E_ARG;
    return i8_mix_plan((long)count_tiles, (long)pair_tiles, std::max(8, (int)cus), mix != 0, tall, shrt) ? 1 : 0;
}

}  // extern "C"
