// tetrad_core.h -- confirmatory tetrad analysis (CTA-PLS): the tetrad lists of a handle, the plan of a launch and the tetrads of one data set as ONE
// portable function the device kernel (kernels_tetrad.h, one wave per problem) and a stand-alone host program (tests/tetrad_host) both run.  Free of the HIP runtime.
//
// One data set: its moment matrix M of the P mean-shifted columns, row / column P the column sums, (P, P) the row count n.
//     mu_p = M_pP / n,  c_pq = M_pq / n - mu_p mu_q (one fma),  s_p = sqrt(c_pp) -- exactly 0 for a column that is constant in the data set, by the threshold of
//     kernels_moments.h mv_stats, whose arithmetic tetrad_mv_stats repeats --,  r_pq = c_pq (1/s_p 1/s_q), as kernels_assess.h has it
//     x_pq = r_pq (matrix = correlation) or c_pq (matrix = covariance)
//     tau(a, b, c, d) = x_ab x_cd - x_ac x_bd of four items of one block: two rounded products and one subtraction.  The products do NOT contract to an fma
//     (tetrad_value switches contraction off for its statement), so that a tetrad of bitwise equal products is exactly zero, the third tetrad of a quadruple is minus
//     the sum of the other two up to one rounding, and the NumPy mirror (plspm.tetrad._tetrads) computes the very same three operations.
// A block is testable with at least four items, numbered 1 .. k in device order.  Sets (tetrad_list):
//     basis  k (k - 3) / 2 per block:  for i = 4 .. k: tau(1,3,i,2), tau(1,2,i,3);  then for 4 <= i < j <= k, i-major: tau(1,2,i,j)
//     all    2 C(k, 4) per block:  per quadruple a < b < c < d in lexicographic order: tau(a,b,c,d), tau(a,c,d,b)
// Record, width n_tet:  tetrads[n_tet] | status | iterations, by block and then as above.  Status: ST_NONFINITE when a tetrad is not finite (a constant column under
// `correlation`) -- the values stand.  At most kTetradMax tetrads: a stated condition, as the chains of structural_core.h.
//
// One wave's LDS slice:  1/s [P] | mu [P] | the strict upper triangles x_pq, p < q, of the tested blocks, row-major, block behind block [T_tri] | tail [kTetradTail]
// (the flag of a non-finite tetrad).  A descriptor is four 16-bit offsets into the staged triangles: (ab), (cd), (ac), (bd).
//
// Execution model: `ex.lanes(f)` runs f(lane) for the 64 lanes of a group and ends with the group's hand-over; between two hand-overs the lanes touch disjoint
// entries of the slice (the flag apart, which every writer sets to the same value).  Mom: `double operator()(int p, int q) const`, the entry (p, q) of M.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <math.h>
#include <string>
#include <vector>
#include "solver_core.h"
#include "solver_route.h"         // kMaxLds

namespace plspm {

constexpr int kTetradMax = 4096;
constexpr int kTetradTail = 1;     // the flag of a non-finite tetrad
constexpr int kTetradRows = 8;     // rows of a block whose loads are in flight together while it is staged (kernels_assess.h ASSESS_ROWS is the precedent)
constexpr int kTetradBatch = 4;    // tetrads of one lane whose descriptor loads are in flight together
enum { TETRAD_BASIS = 0, TETRAD_ALL = 1 };
enum { TETRAD_CORRELATION = 0, TETRAD_COVARIANCE = 1 };

struct alignas(8) TetradDesc { uint16_t ab, cd, ac, bd; };
static_assert(sizeof(TetradDesc) == 8, "one 8-byte load per descriptor");
// a slice that fits the LDS has fewer than 65,536 doubles: every offset into it is a 16-bit number
static_assert(kMaxLds / sizeof(double) <= 65536, "the descriptors hold 16-bit offsets");

// ---- the lists
// tetrads of a block of k items under `set`; 64-bit: C(k, 4) of a wide block
inline long long tetrad_count(int k, int set) {
    if (k < 4) return 0;
    if (set == TETRAD_BASIS) return (long long)k * (k - 3) / 2;
    return 2 * ((long long)k * (k - 1) / 2 * (k - 2) / 3 * (k - 3) / 4);      // (each quotient is exact: a product of r consecutive numbers divides by r!)
}

// the quadruples of a block of k items, 0-based, appended to q as (a, b, c, d)
inline void tetrad_list(int k, int set, std::vector<int>& q) {
    auto put = [&](int a, int b, int c, int d) { q.push_back(a); q.push_back(b); q.push_back(c); q.push_back(d); };
    if (k < 4) return;
    if (set == TETRAD_BASIS) {
        for (int i = 3; i < k; ++i) { put(0, 2, i, 1); put(0, 1, i, 2); }
        for (int i = 3; i < k; ++i) for (int j = i + 1; j < k; ++j) put(0, 1, i, j);
        return;
    }
    for (int a = 0; a < k; ++a) for (int b = a + 1; b < k; ++b) for (int c = b + 1; c < k; ++c) for (int d = c + 1; d < k; ++d) { put(a, b, c, d); put(a, c, d, b); }
}

// the strict upper triangle of a block of k items, row-major: the entry of the unordered pair (i, j), i != j
PLSPM_HD long tetrad_tri(int k, int i, int j) {
    const int a = i < j ? i : j, b = i < j ? j : i;
    return (long)a * k - (long)a * (a + 1) / 2 + (b - a - 1);
}

// What plspm_tetrad_enable builds once (and tests/tetrad_host): per tested block its triangle's offset, the tetrads' blocks and items (device-order MV indices)
// and their descriptors.  tri_off [L + 1]: block l's triangle at tri_off[l], tri_off[l + 1] - tri_off[l] entries, none for a block that is not tested.
struct TetradBuild {
    std::vector<int> tri_off, block, items;       // items: [4 n_tet] a, b, c, d
    std::vector<TetradDesc> desc;
    long T_tri = 0;
    int n_tet = 0;
};

// mask [L] or null (every testable block).  0, or an error: *limit says whether it is the cap (the count is in `why`) or an argument.
inline int tetrad_build(int L, const int* boff, const unsigned char* mask, int set, TetradBuild& tb, std::string& why, bool* limit) {
    *limit = false;
    long long total = 0;
    bool any = false;
    tb.tri_off.assign((size_t)L + 1, 0);
    for (int l = 0; l < L; ++l) {
        const int k = boff[l + 1] - boff[l];
        if (mask && mask[l] && k < 4) { why = "LV " + std::to_string(l) + " has " + std::to_string(k) + " items: a block is testable with at least four"; return 1; }
        const bool on = k >= 4 && (!mask || mask[l]);
        any = any || on;
        total += on ? tetrad_count(k, set) : 0;
        tb.tri_off[l + 1] = tb.tri_off[l] + (on ? k * (k - 1) / 2 : 0);
    }
    if (!any) { why = mask ? "the mask names no block" : "no block has four items: nothing to test"; return 1; }
    if (total > kTetradMax) {
        why = std::to_string(total) + " tetrads, more than the " + std::to_string(kTetradMax) + " a tetrad record holds";
        *limit = true;
        return 1;
    }
    tb.T_tri = tb.tri_off[L];
    tb.n_tet = (int)total;
    tb.block.clear(); tb.items.clear(); tb.desc.clear();
    if (tb.T_tri >= 65536) return 0;      // (no launch takes it: tetrad_plan refuses; the lists below would not fit their 16 bits)
    std::vector<int> q;
    for (int l = 0; l < L; ++l) {
        const int k = boff[l + 1] - boff[l], t0 = tb.tri_off[l];
        if (tb.tri_off[l + 1] == t0) continue;
        q.clear();
        tetrad_list(k, set, q);
        for (size_t e = 0; e < q.size(); e += 4) {
            const int a = q[e], b = q[e + 1], c = q[e + 2], d = q[e + 3];
            tb.block.push_back(l);
            for (int u = 0; u < 4; ++u) tb.items.push_back(boff[l] + q[e + u]);
            tb.desc.push_back(TetradDesc{(uint16_t)(t0 + tetrad_tri(k, a, b)), (uint16_t)(t0 + tetrad_tri(k, c, d)), (uint16_t)(t0 + tetrad_tri(k, a, c)),
                                         (uint16_t)(t0 + tetrad_tri(k, b, d))});
        }
    }
    return 0;
}

// ---- the plan
struct TetradShape { int P; long T_tri; int n_tet; };
PLSPM_HD long tetrad_wave_doubles(int P, long T_tri) { return 2L * P + T_tri + kTetradTail; }
// waves: 4, 2 or 1 per workgroup, the largest count whose slices fit kMaxLds (as derived_route.h derived_plan decides for the geodesic stage); one wave per problem;
// stride: the record pitch.  refused: one wave's slice does not fit.
struct TetradPlan { int waves; long wave_doubles; size_t lds; long grid; int stride; bool refused; };
inline TetradPlan tetrad_plan(const TetradShape& s, long nb) {
    TetradPlan p{};
    const long cap = (long)(kMaxLds / sizeof(double));
    p.wave_doubles = tetrad_wave_doubles(s.P, s.T_tri);
    int waves = 4;
    while (waves >= 1 && waves * p.wave_doubles > cap) waves >>= 1;
    p.refused = waves == 0;
    p.waves = waves < 1 ? 1 : waves;
    p.lds = (size_t)p.waves * p.wave_doubles * sizeof(double);
    p.grid = (nb + p.waves - 1) / p.waves;
    p.stride = s.n_tet + 2;
    return p;
}
inline const char* tetrad_refusal() { return "the statistics and the staged triangles of one replicate need more than 160 KiB of LDS"; }

// ---- the arithmetic
// kernels_moments.h mv_stats, operation for operation
struct TetradMv { double mean, sd; };
template <class Mom> PLSPM_HD TetradMv tetrad_mv_stats(const Mom& mom, int p, int P, double inv_n) {
    const double m = mom(p, P) * inv_n, m2 = mom(p, p) * inv_n, var = fma(-m, m, m2);
    const bool varies = var > 1e-9 * m2;
    return {m, varies ? sqrt(var) : ((var == var) ? 0.0 : var)};
}

PLSPM_HD double tetrad_value(double xab, double xcd, double xac, double xbd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double first = xab * xcd, second = xac * xbd;
    return first - second;
}

struct TetradDescs { int L, n_tet, matrix; const int* boff; const int* tri_off; const TetradDesc* desc; };

// slice: tetrad_wave_doubles(P, T_tri) doubles;  out: the record, pitch n_tet + 2;  iterations: the bootstrap record's, passed through
template <class Ex, class Mom>
PLSPM_HD void tetrad_record(Ex& ex, const TetradDescs& td, const Mom& mom, int P, double* slice, double iterations, double* out) {
    double* const isd = slice;
    double* const mu = slice + P;
    double* const tri = mu + P;
    double* const flag = tri + td.tri_off[td.L];
    const double inv_n = 1.0 / mom(P, P);
    const bool cor = td.matrix == TETRAD_CORRELATION;
    // phase 1: per-MV statistics
    ex.lanes([&](int lane) {
        for (int p = lane; p < P; p += 64) {
            const TetradMv mv = tetrad_mv_stats(mom, p, P, inv_n);
            isd[p] = 1.0 / mv.sd; mu[p] = mv.mean;
        }
        if (lane == 0) flag[0] = 0.0;
    });
    ex.mark(1);
    // phase 2: the diagonal blocks of the tested LVs as x_pq, p < q.  Lane q serves column q of a window of 64; row p is read along the lanes
    ex.lanes([&](int lane) {
        for (int l = 0; l < td.L; ++l) {
            const int t0 = td.tri_off[l];
            if (td.tri_off[l + 1] == t0) continue;
            const int b0 = td.boff[l], b1 = td.boff[l + 1], k = b1 - b0;
            for (int c0 = b0 + 1; c0 < b1; c0 += 64) {                          // (column b0 has no row above it: a block of k items has k - 1 staged columns, a second window from k = 66)
                const bool on = c0 + lane < b1;
                const int q = on ? c0 + lane : b1 - 1;
                const double muq = mu[q], isq = isd[q];
                const int pend = (c0 + 63 < b1 - 1) ? c0 + 63 : b1 - 1;         // rows p < the window's last column
                for (int p0 = b0; p0 < pend; p0 += kTetradRows) {
                    double mm[kTetradRows];
#pragma unroll
                    for (int u = 0; u < kTetradRows; ++u) mm[u] = (on && p0 + u < q) ? mom(p0 + u, q) : 0.0;
#pragma unroll
                    for (int u = 0; u < kTetradRows; ++u) {
                        const int p = p0 + u;
                        if (on && p < q) {
                            const double c = fma(-mu[p], muq, mm[u] * inv_n);
                            tri[t0 + tetrad_tri(k, p - b0, q - b0)] = cor ? c * (isd[p] * isq) : c;
                        }
                    }
                }
            }
        }
    });
    ex.mark(2);
    // phase 3: lane t takes tetrads t, t + 64, ...
    ex.lanes([&](int lane) {
        bool bad = false;
        for (int t0 = lane; t0 < td.n_tet; t0 += 64 * kTetradBatch) {
            TetradDesc d[kTetradBatch];
#pragma unroll
            for (int u = 0; u < kTetradBatch; ++u) { const int t = t0 + 64 * u; d[u] = td.desc[t < td.n_tet ? t : t0]; }
#pragma unroll
            for (int u = 0; u < kTetradBatch; ++u) {
                const int t = t0 + 64 * u;
                if (t < td.n_tet) {
                    const double v = tetrad_value(tri[d[u].ab], tri[d[u].cd], tri[d[u].ac], tri[d[u].bd]);
                    bad = bad || !isfinite(v);
                    out[t] = v;
                }
            }
        }
        if (bad) flag[0] = 1.0;
    });
    ex.mark(3);
    ex.lanes([&](int lane) {
        if (lane == 0) { out[td.n_tet] = (double)(flag[0] != 0.0 ? ST_NONFINITE : ST_OK); out[td.n_tet + 1] = iterations; }
    });
}

// the executor of one host thread (tests/tetrad_host): the lanes one behind the other
struct TetradSerialExec {
    void mark(int) {}
    template <class F> void lanes(F f) { for (int lane = 0; lane < 64; ++lane) f(lane); }
};

}  // namespace plspm
