// fit_route.h -- the plan of one single fit (plspm_fit.hip plspm_fit): where every result lies in the device block and in its pinned copy, how many row chunks the
// dense Gram is cut into, which scores kernel runs on which grid, whether the scores ride the pinned block, and where the solver keeps its workspace.  Pure functions
// of what the handle fixes (FitShape), the call (FitCall) and the options (FitOptions).  Free of the HIP runtime: the CPU tests compile it (tests/hostemu).
#pragma once
#include <stddef.h>
#include <algorithm>
#include "solver_route.h"

namespace plspm {

// What the handle fixes.  Po: the MVs a result is reported for (categorical handles report per logical MV, Pm, not per aug column); PA / T: padded columns and
// 16-column tiles of the resident matrix; kmax, n_chol, nedge as RouteShape has them.
struct FitShape {
    long N;
    int P, Po, L, n_eff, PA, T, kmax, n_chol, nedge;
    bool categorical;
};
struct FitCall { bool want_scores, want_cov; };
struct FitOptions { int fit_chunks, scores_tile; };

// Row chunks (workgroups) of the dense Gram of all N rows: enough k-groups per wave to amortise the pipeline prologue; at most two workgroups per CU for the rows
// kernel (every wave holds all tiles), ONE for the tile-split kernels (a wave per SIMD already fills the register file; measured on 1M x 200: 256 chunks 0.941 +
// reduce 0.027 ms, 512: 0.939 + 0.063, 1024: 0.954 + 0.132).  Option "fit_chunks" overrides.
inline int fit_gram_chunks(long N, int T, int fit_chunks) {
    if (fit_chunks > 0) return fit_chunks;
    const long ng = (N + 3) / 4, per_wg = (T <= 4 ? 4 : 1) * 16L, cap = T <= 4 ? 512 : 256;
    return (int)std::max<long>(1, std::min<long>(cap, (ng + per_wg - 1) / per_wg));
}

// The scores launch.  tile_rows: 32 while two workgroups of them fit one CU's LDS, else 16 (wide models; option "scores_tile" overrides); cls: chunks per thread of
// the prefetching instantiation, 2 / 4 / 6 / 8 (PA <= 256), or 0: the plain kernel; grid: resident workgroups only, each walks its tiles with the prefetch running.
struct ScoresLaunch { int tile_rows, cls; size_t lds; long ntl; int per_cu, grid; };
inline size_t scores_lds_bytes(const FitShape& s, int tr) { return ((size_t)tr * (s.PA + 1) + s.P + s.L + (size_t)tr * s.L) * sizeof(double) + (size_t)(s.L + 2) * sizeof(int); }
inline ScoresLaunch fit_scores_launch(const FitShape& s, int scores_tile) {
    ScoresLaunch k{};
    const bool tr32 = scores_tile ? scores_tile == 32 : scores_lds_bytes(s, 32) <= 72 * 1024;
    k.tile_rows = tr32 ? 32 : 16;
    k.lds = scores_lds_bytes(s, k.tile_rows);
    const int nch = (s.PA / 2 + 15) / 16;
    k.cls = nch <= 2 ? 2 : nch <= 4 ? 4 : nch <= 6 ? 6 : nch <= 8 ? 8 : 0;
    k.ntl = (s.N + k.tile_rows - 1) / k.tile_rows;
    k.per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, kMaxLds / k.lds));
    k.grid = (int)std::min<long>(256L * k.per_cu, k.ntl);
    return k;
}

// The integer tail of the result block, behind o_end: ints 0 and 1, then L sign bytes from int 4.
enum { FIT_INT_ITERS = 0, FIT_INT_STATUS = 1, FIT_INT_SIGN = 4 };

struct FitPlan {
    FitCall call;
    // the device result block, offsets in doubles; o_row: the solver's record as a bootstrap replicate has it, of which the host reads the total and direct
    // effects at h_total / h_direct (n_eff doubles each, behind Po + L others)
    long o_w, o_ld, o_cl, o_pc, o_r2, o_lc, o_row, o_ind, o_sw, o_sc, o_mean, o_cov, o_end;
    int Po;                      // MVs the per-MV results are reported for
    long h_total, h_direct;
    size_t tail_bytes;           // the integer tail
    size_t fit_bytes;            // the whole block, tail included
    size_t block_bytes;          // what the download takes of the doubles: up to the covariance matrix unless the call wants it
    int nchunks;                 // fit_gram_chunks
    ScoresLaunch scores;
    size_t score_bytes;          // 0 unless the call wants scores
    bool stage_scores;           // small score matrices ride the pinned block too, behind fit_bytes
    size_t stage_need;           // bytes of the pinned block
    SolverLds solver;            // the metric solver's workspace placement for this one problem
};

inline FitPlan fit_plan(const FitShape& s, const FitCall& c, const FitOptions& o) {
    FitPlan p{};
    const long P = s.P, L = s.L, ne = s.n_eff;
    p.call = c; p.Po = s.Po;
    p.o_w = 0; p.o_ld = p.o_w + P; p.o_cl = p.o_ld + P; p.o_pc = p.o_cl + P * L; p.o_r2 = p.o_pc + L * L; p.o_lc = p.o_r2 + L;
    p.o_row = p.o_lc + L * L; p.o_ind = p.o_row + (2 * P + L + 2 * ne + 2); p.o_sw = p.o_ind + std::max(ne, 1L); p.o_sc = p.o_sw + P; p.o_mean = p.o_sc + L;
    p.o_cov = p.o_mean + P; p.o_end = p.o_cov + P * P;
    p.h_total = p.o_row + s.Po + L; p.h_direct = p.h_total + ne;
    p.tail_bytes = 64 + (size_t)L + 16;
    p.fit_bytes = (size_t)p.o_end * sizeof(double) + p.tail_bytes;
    p.block_bytes = (size_t)(c.want_cov ? p.o_end : p.o_cov) * sizeof(double);
    p.nchunks = fit_gram_chunks(s.N, s.T, o.fit_chunks);
    p.scores = fit_scores_launch(s, o.scores_tile);
    p.score_bytes = c.want_scores ? sizeof(double) * (size_t)s.N * L : 0;
    p.stage_scores = p.score_bytes > 0 && p.score_bytes <= ((size_t)8 << 20);
    p.stage_need = p.fit_bytes + (p.stage_scores ? p.score_bytes : 0);
    p.solver = solver_lds(RouteShape{s.P, s.L, s.kmax, s.n_chol, s.n_eff, s.nedge, nullptr}, 1);
    return p;
}

}  // namespace plspm
