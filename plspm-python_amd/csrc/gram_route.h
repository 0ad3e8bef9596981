// gram_route.h -- which form of the int8 digit-plane Gram a bootstrap chunk takes (kernel, tile rows, grid, resample histogram, buffer sizes): a pure function of
// what the data set fixed, the i8_* options and the call, read by the launcher and by the round units of the sub-batch plan (plspm_gram_i8.hip).
// Free of the HIP runtime: the CPU tests compile it (tests/hostemu).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

// layout constants shared with the kernels (kernels_gram_i8.h)
#define I8_SLACK_KB 6             // k-blocks of readable slack behind the counts and the digit planes (the DMA ring runs up to 5 k-steps ahead)
#define I8_HIST_KB 1024           // k-blocks (64 rows each) per resample window of 16-bit counters: 65,536 rows ...
#define I8_HIST_KB_BYTES 2048     // ... of 8-bit counters ...
#define I8_HIST_KB_NIB 4096       // ... and of 4-bit counters

namespace plspm {

// Tile rows of the six-plane int8 Gram for `ct` count tiles (16 replicates each) x `ntx` pair tiles on `cus` CUs in 8 XCDs: `tall` rows of
// 20 count tiles and -- `mix` -- `shrt` rows of 16 in one launch of gram_i8_kernel<6, 4, ., 16, 20>, or (return false) the 256-replicate
// kernel.  Cost model = what the device does: an XCD's workgroups go in order to the CU that is free first (one workgroup per CU), so the
// makespan of a cut is that of list scheduling its tall tiles first, then its short ones, per XCD.  Costs in count-tile rows: 20 per
// tall tile, 16.6 per short one (the same DMA ring for 4/5 of the MFMAs), 16.35 per tile of the 256-replicate kernel (measured on 960 tiles
// of each kind, tools/i8_mix_calib.py: 0.391 / 0.3245 / 0.3195 ms).  Deterministic in (ct, ntx, cus): every rank of a job cuts alike -- and the sums are exact
// integers, so the cut never shows in a result.
// (profiles/r04_i8_mix_calib.jsonl: 960 tiles of each height, 0.3628 / 0.2990 ms with six planes, 0.3435 / 0.2700 with seven)
static constexpr double kI8pTall6 = 20.0, kI8pShort6 = 16.5, kI8pTall7 = 16.0, kI8pShort7 = 12.6;
// Tile heights and their costs: `rt_tall` / `rt_short` count tiles per row, `ca` / `cb` what a tile of each costs (any common unit).  The
// round-3 kernel: 20 / 16 at 20 / 16.6; gram_i8p_kernel: the four constants above.
inline bool i8_mix_plan(long ct, long ntx, int cus, bool mix, int* tall, int* shrt, int rt_tall = 20, int rt_short = 16, double ca = 20.0, double cb = 16.6, bool vs_rt16 = true) {
    const int per_xcd = std::max(1, cus / 8);
    // (tiles of one kind are interchangeable: after the tall ones the CUs of an XCD sit on at most two load levels, and the short ones raise
    //  the lowest level a whole group of CUs at a time -- a handful of steps per XCD instead of one per tile)
    auto xcd_span = [&](long na, long nb2, double ca, double cb) {
        const long c = per_xcd, q = na / c, r = na % c;
        double lv[3] = {q * ca, (q + 1) * ca, 0.0};
        long cnt[3] = {c - r, r, 0};
        int n = r ? 2 : 1;
        long left = nb2;
        while (left > 0) {
            int lo = 0;
            for (int k = 1; k < n; ++k) if (lv[k] < lv[lo]) lo = k;
            if (left >= cnt[lo]) { left -= cnt[lo]; lv[lo] += cb; }
            else { lv[n] = lv[lo] + cb; cnt[n] = left; cnt[lo] -= left; left = 0; ++n; }
            for (int k = 0; k < n; ++k)                      // merge equal levels (keeps n <= 2 before the last step)
                for (int k2 = k + 1; k2 < n; ++k2)
                    if (lv[k2] == lv[k]) { cnt[k] += cnt[k2]; lv[k2] = lv[n - 1]; cnt[k2] = cnt[n - 1]; --n; --k2; }
        }
        double worst = 0.0;
        for (int k = 0; k < n; ++k) if (cnt[k] > 0) worst = std::max(worst, lv[k]);
        return worst;
    };
    auto makespan = [&](long a, long b, double ca, double cb) {
        double worst = 0.0;
        const long ta = a * ntx, tb = b * ntx, pa = (ta + 7) / 8, pb = (tb + 7) / 8;
        long seen_a = -1, seen_b = -1;
        for (int x = 0; x < 8; ++x) {
            const long na = std::max(0L, std::min(pa, ta - x * pa)), nb2 = std::max(0L, std::min(pb, tb - x * pb));
            if (na == seen_a && nb2 == seen_b) continue;
            seen_a = na; seen_b = nb2;
            worst = std::max(worst, xcd_span(na, nb2, ca, cb));
        }
        return worst;
    };
    const long rows16 = (ct + 15) / 16, rows_s = (ct + rt_short - 1) / rt_short;
    const double ref16 = vs_rt16 ? makespan(rows16, 0, 16.35, 0.0) : 1e300;
    double best = 1e300;
    long ba = 0, bb = 0;
    for (long b = 0; b <= (mix ? std::min(rows_s, 48L) : 0L); ++b) {
        const long a = std::max(0L, (ct - (long)rt_short * b + rt_tall - 1) / rt_tall);
        if (a == 0 && b * rt_short < ct) continue;
        const double t = makespan(a, b, ca, cb);
        if (t < best - 1e-9) { best = t; ba = a; bb = b; }
        if (a == 0) break;
    }
    *tall = (int)ba; *shrt = (int)bb;
    return best <= ref16;
}

// What the data set fixed (prepare_zs): digit planes, k-blocks of 64 rows, 1 KB digit blocks per k-block, pair groups of 16; zs_ind: one plane per pair group (0/1 data)
struct GramI8Data { int S, KB, NT, npg; bool zs_ind; };
// The i8_* options (plspm_model_set_option; short_rows is "i8_short_rows")
struct GramI8Options { int priv, persist, rt, short_rows, cus, dma, nibbles, waves, shape, sched, variant; };
// One chunk: explicit_idx = index lists come with it (they can carry any multiplicity), own_counts = the call's kind launches its own count kernel, want16 = the caller
// takes uint16 co-occurrence counts where the launch can write them, experiments = the build with the measured-neutral / slower forms (make experiments)
struct GramI8Call { int64_t nb; bool explicit_idx, own_counts, want16; int cu_count; bool experiments; };
// The tile-row cut of i8_mix_plan and the key it is a function of: count tiles, pair tiles, CUs, 2 + S for the private-count kernel else whether short rows may mix in.
// The launcher keeps the last one (a bootstrap calls with the same B again and again, and the search costs of the order of a millisecond).
struct GramI8Cut { bool valid, wide; long key[4]; int tall, shrt; };

// PLAIN: gram_i8_kernel on 256-replicate tiles (any plane count); IND: the same on one plane per pair group, seven groups per wave; WIDE20: on 320-replicate tiles with six
// planes (rows of 256 mixed in where the kernel form has them); PRIV: gram_i8p_kernel (private count fragments); PERSIST: gram_i8pp_kernel, one workgroup per CU.
// Experiments build only: SK (gram_i8_sk_kernel), NARROW (128-replicate tiles), SHAPE32 (v_mfma_i32_32x32x32_i8).
enum GramI8Form { GRAM_I8_PLAIN = 0, GRAM_I8_IND = 1, GRAM_I8_WIDE20 = 2, GRAM_I8_PRIV = 3, GRAM_I8_PERSIST = 4, GRAM_I8_SK = 5, GRAM_I8_NARROW = 6, GRAM_I8_SHAPE32 = 7 };
enum GramI8Hist { GRAM_I8_HIST16 = 0, GRAM_I8_HIST8 = 1, GRAM_I8_HIST4 = 2 };

struct GramI8Plan {
    GramI8Call call;
    // form: GramI8Form; waves per workgroup; variant: the kernel template's VAR where the options name one (PRIV / PERSIST: 64 is the release kernel), -1: the round-3
    // kernel's default schedule; dma_buffer: LDS-DMA as buffer_load ... lds (VAR + 800) instead of global_load_lds
    int form, waves, variant;
    // count tiles (16 replicates) per tile row (rt_short 0: rows of one height only) and the rows; pair tiles; count tiles of the padded batch; workgroups per XCD of the
    // tiled launch and the launch itself; PERSIST: workgroups per XCD, SK: workgroups
    int rt_tall, rt_short, nty_tall, nty_short, nty, ntx, MT, per_xcd, grid, block, pp_wgs, sk_grid;
    // the resample histogram (GramI8Hist): per (replicate, window of rows) one workgroup of hist_threads threads on hist_bytes of LDS
    int hist;
    unsigned hist_windows, hist_threads;
    size_t hist_bytes, cd_bytes;      // ... and the dense int8 counts
    bool dma_buffer, to16;            // to16: the launch writes uint16 co-occurrence counts
};

// count tiles of a tall tile row of gram_i8p_kernel / gram_i8pp_kernel at S planes: 320 replicates with six planes, 256 with seven (MTW = a quarter of it per wave)
constexpr int gram_i8p_tall(int S) { return S == 6 ? 20 : 16; }
// The private-count kernel takes this data set under these options (an explicit other tile height, the 32x32x32 layout, the stream-K schedule and -- release build --
// a schedule variant name a round-3 kernel)
inline bool gram_i8_priv_takes(const GramI8Data& d, const GramI8Options& o, bool experiments) {
    return o.priv != 0 && o.shape == 16 && o.sched == 0 && (experiments || o.variant < 0) && (d.S == 6 || d.S == 7) && !d.zs_ind && (o.rt == 0 || o.rt == gram_i8p_tall(d.S));
}
// The CU count a cut is made for ("i8_cus": fewer CUs than the device has -- a launch that shares the chip with a collective's kernels)
inline int gram_i8_cut_cus(int i8_cus, int cu_count) { return std::max(8, i8_cus > 0 ? std::min(i8_cus, cu_count) : cu_count); }
// Replicates of one round of the device: what the sub-batch plan aligns to (plspm_detail_round_units).  Results never depend on the cut -- the sums are exact integers.
inline int64_t gram_i8_round_units(const GramI8Data& d, const GramI8Options& o, int cu_count, bool experiments) {
    return gram_i8_priv_takes(d, o, experiments) ? (int64_t)std::max(1, gram_i8_cut_cus(o.cus, cu_count) / std::max(1, d.npg / 2)) * gram_i8p_tall(d.S) * 16 : 64;
}

// A cut not yet searched, under the key that decides it (priv_S: the plane count where the private-count kernel takes the launch, else 0)
inline GramI8Cut gram_i8_cut_key(long ct, long ntx, int cus, int priv_S, bool mix_ok) { return GramI8Cut{true, false, {ct, ntx, (long)cus, priv_S ? 2L + priv_S : (long)mix_ok}, 0, 0}; }

// `last`: the launcher's cut cache -- read when its key is this launch's, written when a cut was searched (null: searched here, kept nowhere)
inline GramI8Plan gram_i8_plan(const GramI8Data& d, const GramI8Options& o, const GramI8Call& c, GramI8Cut* last = nullptr) {
    GramI8Plan p{};
    p.call = c;
    const int S = d.S, KB = d.KB;
    // workgroup tile of the product: 16 RT replicates x 32 pairs.  Six planes leave registers for a taller tile: 320 replicates x 32 pairs (`RT` 20: 30 accumulator tiles
    // per wave with eight waves) moves 9 % fewer LDS-DMA bytes and reads 12 % fewer fragments per MFMA than 256 x 32 -- 2.2 % on the step when the tile grid fills the
    // machine equally well (5,000 replicates: 960 tiles = 3.75 rounds against 1,200 = 4.69, both five tile-units per CU).  "i8_rt" 0 (default) takes it when its rounds
    // cost no more than those of the 256-replicate tile.  Private count fragments ("i8_priv"): tile rows of 320 / 256 replicates with six planes, 256 / 192 with seven.
    const bool var20 = o.variant < 0 || (c.experiments && o.rt == 20);      // experiments build: the schedule variants exist for the 320-replicate tile too
    const bool priv = gram_i8_priv_takes(d, o, c.experiments);
    bool wide20 = !priv && o.shape == 16 && o.sched == 0 && var20 && S == 6 && !d.zs_ind && (o.rt == 20 || o.rt == 0);
    const bool mix_ok = priv || (o.waves == 8 && var20 && o.dma != 2);     // short rows: every private-count launch, the eight-wave FLAT-global form of the round-3 kernel
    const int rt_tall = priv ? gram_i8p_tall(S) : 20, rt_short = rt_tall - 4, cus = gram_i8_cut_cus(o.cus, c.cu_count);
    const long ct = (long)((c.nb + 15) / 16);
    if ((wide20 || priv) && o.rt == 0 && o.short_rows < 0) {
        // the cut is planned: rows of both heights in ONE launch, so that the last round of the machine is as full as the others (5,000 replicates x 60 pair tiles: 11 + 6
        // rows = 1,020 tiles, every CU three tall + one short = 76 count-tile rows, against 16 rows of 320 = 960 tiles, 80 on three CUs of four)
        GramI8Cut cut = gram_i8_cut_key(ct, d.npg / 2, cus, priv ? S : 0, mix_ok);
        if (last && last->valid && std::equal(cut.key, cut.key + 4, last->key)) cut = *last;
        // (tile costs of gram_i8p_kernel, tools/i8_mix_calib.py on 960 tiles of each height: six planes 320 / 256 replicates, seven planes 256 / 192)
        else if (priv) cut.wide = i8_mix_plan(ct, cut.key[1], cus, true, &cut.tall, &cut.shrt, rt_tall, rt_short, S == 6 ? kI8pTall6 : kI8pTall7, S == 6 ? kI8pShort6 : kI8pShort7, false);
        else cut.wide = i8_mix_plan(ct, cut.key[1], cus, mix_ok, &cut.tall, &cut.shrt);
        if (last) *last = cut;
        if (!priv) wide20 = cut.wide;
        p.nty_tall = cut.tall; p.nty_short = cut.shrt;
    } else if (wide20 || priv) {
        // tall rows only, or -- "i8_short_rows" n >= 0 (test seam) -- n short rows behind as many tall ones as it takes
        if (o.short_rows > 0 && mix_ok) p.nty_short = (int)std::min<long>(o.short_rows, (ct + rt_short - 1) / rt_short);
        p.nty_tall = (int)std::max(0L, (ct - (long)rt_short * p.nty_short + rt_tall - 1) / rt_tall);
    }
    // narrow tiles (RT 8) only in the plain four-wave 16x16x64 launch
    const bool rows2 = wide20 || priv, narrow8 = !rows2 && o.rt == 8 && o.shape == 16 && o.waves == 4 && o.sched == 0 && o.variant < 0 && S == 7;
    const bool ind = d.zs_ind && o.sched == 0 && o.variant < 0;
    // persistent stream-K schedule: one workgroup per CU, whole CUs per XCD (S = 8 spills in the persistent kernel)
    const bool sk = o.sched == 1 && o.shape == 16 && o.variant < 0 && S >= 5 && S <= 7;
    const bool persist = priv && o.persist != 0 && (o.variant < 0 || o.variant == 64);
    const bool variants7 = S == 7 && o.variant >= 0;                      // experiments build: every schedule variant of the seven-plane kernel
    p.form = persist ? GRAM_I8_PERSIST : priv ? GRAM_I8_PRIV : sk ? GRAM_I8_SK : variants7 ? GRAM_I8_PLAIN : ind ? GRAM_I8_IND : wide20 ? GRAM_I8_WIDE20
           : narrow8 ? GRAM_I8_NARROW : (o.shape == 32 && S >= 5) ? GRAM_I8_SHAPE32 : GRAM_I8_PLAIN;
    p.waves = (priv || p.form == GRAM_I8_NARROW || p.form == GRAM_I8_SHAPE32) ? 4 : o.waves;
    p.variant = priv ? (persist || o.variant < 0 ? 64 : o.variant) : (variants7 || (p.form == GRAM_I8_WIDE20 && o.waves == 8)) ? o.variant : -1;
    p.rt_tall = rows2 ? rt_tall : narrow8 ? 8 : 16; p.rt_short = rows2 ? rt_short : 0;
    if (!rows2) { p.nty_tall = (int)((c.nb + 16 * p.rt_tall - 1) / (16 * p.rt_tall)); p.nty_short = 0; }
    p.nty = p.nty_tall + p.nty_short; p.MT = p.nty_tall * p.rt_tall + p.nty_short * p.rt_short; p.ntx = ind ? d.npg / 14 : d.npg / 2;
    p.per_xcd = (p.ntx * p.nty_tall + 7) / 8 + (p.ntx * p.nty_short + 7) / 8;      // an XCD walks its share of the tall rows, then of the short ones
    p.sk_grid = sk ? std::max(8, (c.cu_count / 8) * 8) : 0;
    p.pp_wgs = persist ? std::max(1, std::min(cus / 8, p.per_xcd)) : 0;           // one workgroup per CU of an XCD, never more than the XCD has tiles
    p.grid = persist ? 8 * p.pp_wgs : p.form == GRAM_I8_SK ? p.sk_grid : 8 * p.per_xcd; p.block = 64 * p.waves;
    // the buffer form of the LDS-DMA needs every byte offset of a workgroup's walk (incl. the slack k-blocks) below 4 GiB
    const bool dma_fits = (uint64_t)(KB + I8_SLACK_KB) * (uint64_t)std::max(p.MT, d.NT) * 1024ull < (1ull << 32);
    p.dma_buffer = !priv && o.dma != 1 && dma_fits && o.shape == 16 && !sk && !narrow8 && (!wide20 || o.waves == 4) && o.variant < 0;
    // resample counts from an LDS histogram per (replicate, window of rows): 65,536 rows of 16-bit counters, or -- Philox draws of a data set that would need more than
    // one such window -- 131,072 rows of 8-bit counters, or 262,144 rows of 4-bit counters with an exact overflow test and an 8-bit second try ("i8_nibbles" 0: the
    // 8-bit histogram).  Explicit index lists can carry any multiplicity: they keep the 16-bit counters, where the overflow bit is reliable.
    const bool hist_byte = KB > I8_HIST_KB && !c.explicit_idx, hist_nib = hist_byte && o.nibbles != 0 && o.shape == 16;
    const int hist_kb = hist_nib ? I8_HIST_KB_NIB : (hist_byte ? I8_HIST_KB_BYTES : I8_HIST_KB);
    p.hist = hist_nib ? GRAM_I8_HIST4 : hist_byte ? GRAM_I8_HIST8 : GRAM_I8_HIST16; p.hist_windows = (unsigned)((KB + hist_kb - 1) / hist_kb);
    p.hist_bytes = (size_t)std::min(KB, hist_kb) * (hist_nib ? 8 : (hist_byte ? 16 : 32)) * sizeof(unsigned);
    // threads per workgroup: the histogram decides how many workgroups share a CU (160 KB of LDS); the VALU-bound Philox loop wants the CU's wave slots filled either
    // way (N = 100,000: one 128 KB histogram per CU -- 256 threads left three quarters of the SIMD time idle)
    p.hist_threads = (unsigned)std::min(1024, std::max(256, 256 * (int)(8 / std::max<size_t>(1, (160 * 1024) / std::max<size_t>(1, p.hist_bytes)))));
    p.cd_bytes = (size_t)p.MT * 16 * ((size_t)KB + I8_SLACK_KB) * 64; p.to16 = c.want16 && ind && o.shape == 16;
    return p;
}

}  // namespace plspm
