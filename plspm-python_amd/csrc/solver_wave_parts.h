// solver_wave_parts.h -- what the one-wave-per-problem solvers share (solver_wave.h, solver_wave16.h incl. its NM form, solver_quad.h): the fast reciprocals,
// the in-register LDL', the regressions of the LV role and the inner-model block built on them, the Mode-B inverses and the outer-step product, the status
// word.  ONE copy of each: a finding on this arithmetic is applied here.
// These kernels sit at the register limit (256 VGPRs, 0 .. 42 of them spilled), so every helper takes the caller's locals as plain scalars and pointers and
// reports through `bool&` -- nothing bundled into a struct that would live across the iteration loop -- and is inlined: the allocator sees the code the
// solvers spelled out themselves before.  Even the ORDER of two scalar arguments moves the allocation of the kernels that spill (wave_regress: nk in front
// of fpack, the order the solvers declare them in): check the resource table of every kernel after a change here.
// Executor: solver_wave.h.
#pragma once
#include "solver_core.h"
#include <type_traits>

namespace plspm {

// 1 / sqrt(x) and 1 / x to the last bit or two (not correctly rounded): v_rsq_f64 / v_rcp_f64 seeds + Newton steps on the device -- a
// fraction of the dependent instructions of the IEEE sqrt + divide sequences, which sit on the critical path of every small phase.
// The CPU emulation runs the SAME refinement on a seed of the hardware's accuracy (the exact value rounded to fp32's 24 bits, exponent kept
// apart so that any double is in range): what the emulation tests then hold against the oracle is this arithmetic, not the IEEE divide.
PLSPM_HD double wave_rsqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r = __builtin_amdgcn_rsq(x);                           // ~2^-26 relative
#else
    double r;
    if (!(x > 0.0) || x > 1.7976931348623157e308) r = 1.0 / sqrt(x);      // 0, negative, inf, NaN: what the instruction returns
    else {
        int e;
        double m = frexp(x, &e);                                  // x = m 2^e, m in [1/2, 1)
        if (e & 1) { m *= 2.0; --e; }                             // even exponent: sqrt(2^e) is a power of two
        r = ldexp((double)(float)(1.0 / sqrt(m)), -e / 2);
    }
#endif
    const double hx = 0.5 * x;
    r = fma(r, fma(-hx * r, r, 0.5), r);                          // r (1 + (1/2 - x r^2 / 2))
    r = fma(r, fma(-hx * r, r, 0.5), r);
    return r;
}
PLSPM_HD double wave_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r = __builtin_amdgcn_rcp(x);
#else
    double r;
    if (!(fabs(x) > 0.0) || fabs(x) > 1.7976931348623157e308) r = 1.0 / x;
    else {
        int e;
        const double m = frexp(x, &e);
        r = ldexp((double)(float)(1.0 / m), -e);
    }
#endif
    r = fma(r, fma(-x, r, 1.0), r);
    r = fma(r, fma(-x, r, 1.0), r);
    return r;
}
// Normal equations M[f, f] x = M[f, col], f = the k <= 4 indices packed one per byte in `fpack`, M an L x L matrix with pitch ld in the
// workspace: square-root-free factorisation A = U' D U in registers (as solver_core.h spd_solve_fixed; identity padding beyond k),
// reciprocals by wave_rcp.  Returns false at a pivot that is not safely positive (the caller takes the minimum-norm route).
PLSPM_HD bool wave_ldl4(const double* M, int ld, unsigned fpack, int k, int col, double* x) {
    constexpr int K = 4;
    double A[K][K], b[K];
    int f[K];
#pragma unroll
    for (int r = 0; r < K; ++r) f[r] = (r < k) ? (int)((fpack >> (8 * r)) & 255u) : 0;
#pragma unroll
    for (int r = 0; r < K; ++r) {
#pragma unroll
        for (int c = r; c < K; ++c) A[r][c] = (r < k && c < k) ? M[f[r] * ld + f[c]] : ((r == c) ? 1.0 : 0.0);
        b[r] = (r < k) ? M[f[r] * ld + col] : 0.0;
    }
    bool ok = true;
    double T[K][K], invd[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double ajj = A[j][j];
        double d = ajj;
#pragma unroll
        for (int r = 0; r < j; ++r) d -= A[r][j] * T[r][j];
        ok = ok && (d > PLSPM_PIVOT_RTOL * ajj);
        invd[j] = wave_rcp(d);
#pragma unroll
        for (int c = j + 1; c < K; ++c) {
            double t = A[j][c];
#pragma unroll
            for (int r = 0; r < j; ++r) t -= A[r][j] * T[r][c];
            T[j][c] = t;
            A[j][c] = t * invd[j];
        }
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double t = b[i];
#pragma unroll
        for (int r = 0; r < i; ++r) t -= A[r][i] * b[r];
        b[i] = t;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) b[i] *= invd[i];
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
        double t = b[i];
#pragma unroll
        for (int c = i + 1; c < K; ++c) t -= A[i][c] * b[c];
        b[i] = t;
    }
#pragma unroll
    for (int r = 0; r < K; ++r) if (r < k) x[r] = b[r];
    return ok;
}

// LV role: predecessor r of an LV -- the first four packed one byte each in `fpack`, the rest in md.pred_idx (`fglob`: the LV's slice)
PLSPM_HD int wave_pred(unsigned fpack, const int* fglob, int r) { return r < 4 ? (int)((fpack >> (8 * r)) & 255u) : fglob[r]; }

// LV role: normal equations M[f, f] x = M[f, t] over the nk predecessors f of LV t, M with pitch ld -- up to four in registers (wave_ldl4: every
// LV lane runs the same straight-line code, identity-padded), five and more by Cholesky in `scratch` (LDS; x behind it); a rank-deficient system
// takes the minimum-norm answer of the reference's pinv / gelsd (solver_core.h pinv_solve), and sets `singular` where that fails too.
template <class Ex>
PLSPM_HD void wave_regress(Ex& ex, const double* M, int ld, int nk, unsigned fpack, const int* fglob, int t, double* scratch, double* x, bool& singular) {
    bool ok;
    if (nk <= 4) {
        unsigned fp = fpack;
        ex.opaque(fp);            // the 14 gather addresses are recomputed here (a few integer operations) instead of living -- spilled -- across the loop
        ok = wave_ldl4(M, ld, fp, nk, t, x);
    } else {
        for (int r = 0; r < nk; ++r) {
            for (int c = 0; c < nk; ++c) scratch[r * nk + c] = M[fglob[r] * ld + fglob[c]];
            x[r] = M[fglob[r] * ld + t];
        }
        ok = chol_factor(scratch, nk);
        if (ok) chol_solve(scratch, nk, x);
    }
    if (!ok && !(nk > 1 && pinv_solve(M, ld, fglob, nk, t, x, scratch))) singular = true;
}

// Inner model of LV t (inner_model.py:58-75): OLS with intercept == centred normal equations on the score covariance Cs; x = regress(Cs) are the
// coefficients on its nk > 0 predecessors: row t of the path matrix Bm; returns R^2.
PLSPM_HD double wave_inner_model(const double* x, const double* Cs, double* Bm, int ld, int t, int nk, unsigned fpack, const int* fglob) {
    double expl = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (r < nk) { const int fr = wave_pred(fpack, fglob, r); Bm[t * ld + fr] = x[r]; expl += x[r] * Cs[fr * ld + t]; }
    for (int r = 4; r < nk; ++r) { const int fr = wave_pred(fpack, fglob, r); Bm[t * ld + fr] = x[r]; expl += x[r] * Cs[fr * ld + t]; }
    return expl / Cs[t * ld + t];
}

// Mode-B blocks (mode.py:50-52: w_b = argmin |X_b w - z| = S_bb^-1 (X_b' z / N)): S_bb does not change over the iterations, so its
// inverse is formed once, into ws.inv (block lp at boffB = chol_off[lp] / 2, full k x k).  Gauss-Jordan sweep without pivoting (S_bb is positive
// definite; pivot j is the same Schur complement the Cholesky factorisation of solver_core.h tests, so a rank-deficient block is recognised by the
// same rule), every MV lane of a Mode-B block (`modeb`; block columns [bb0, bb0 + bk), the lane's row bi) owning ROW bi of its k x k matrix, all
// blocks at once, out of place: step j reads A, writes A' -- no lane reads what another rewrites in the same step, ONE exchange per step --
// ping-ponging between ws.inv and the staging area ws.stage (free until the first S W).
//     i == j:  A'[j][c] = A[j][c] / piv  (c != j),  A'[j][j] = 1 / piv
//     i != j:  A'[i][c] = A[i][c] - A[i][j] A[j][c] / piv  (c != j),  A'[i][j] = -A[i][j] / piv
// A block whose sweep meets a pivot that is not safely positive takes the minimum-norm route of the reference's gelsd (jacobi_pinv, on
// its LV lane, one such block at a time in the staging area; `singular` where that fails) -- the outer step multiplies with the full symmetric
// matrix either way.  s: column p of the treated covariance; sdp: its standard deviation; kbB: the widest Mode-B block.  Overwrites ws.mu.
template <int LMAX, class Ex, class Ws, int PMAX>
PLSPM_HD void wave_modeb_inverses(Ex& ex, const ModelDesc& md, const Ws& ws, const double (&s)[PMAX], int p, int lp, int L, double sdp, int kbB, bool modeb,
                                  int bb0, int bk, int bi, long boffB, bool& singular) {
    ex.sync();                                              // (every lane is done with the column sums ws.mu held)
    ws.mu[p] = (sdp > 0.0) ? sdp * sdp : 1e300;             // the treated diagonal S_pp: the scale a pivot is measured against (a zero-variance column: no pivot passes -- the block takes the minimum-norm route, weight 0 for it)
    double* A = (kbB & 1) ? ws.stage : ws.inv;              // an odd number of steps ends in ws.inv
    double* An = (kbB & 1) ? ws.inv : ws.stage;
    auto fill_block = [&](double* dst) {                    // row bi of S_bb out of the column registers (S is symmetric)
#pragma unroll
        for (int q = 0; q < PMAX; ++q)
            if (modeb && q >= bb0 && q < bb0 + bk) dst[boffB + bi * bk + (q - bb0)] = s[q];
    };
    // the same with every lane storing every column -- the ones outside its block into a slot of its own behind the pivot rows of the
    // sweep below (an address select instead of an exec-masked branch per column: 7 k -> 2 k clocks)
    auto fill_block_all = [&](double* dst) {
        double* mine_row = dst + boffB + bi * bk - bb0;      // column q of my block lands at mine_row[q]
        double* junk = ws.stage + 2 * LMAX * 16 + p;
        const unsigned bkm = modeb ? (unsigned)bk : 0u;
#pragma unroll
        for (int q = 0; q < PMAX; ++q) {
            double* d = ((unsigned)(q - bb0) < bkm) ? mine_row + q : junk;
            *d = s[q];
        }
    };
    bool okrow = true;
    ex.mark(20);
    // blocks of at most 16 MVs: every lane keeps ITS row of the block in registers; step j = the pivot lane publishes its row
    // (double-buffered at the head of the staging area), one exchange, every lane updates its row with straight-line code (compile-time
    // column index, `c == j` a scalar test) -- where the loop over LDS-resident matrices below pays two dependent LDS round trips per
    // column and step (5 k clocks per step at k = 10 against ~1 k).  Same formulas, same pivot test.  KR = registers of a row: 8 / 12 / 16.
    auto sweep_rows = [&](auto krc) {
        constexpr int KR = decltype(krc)::value;
        fill_block_all(ws.inv);
        ex.sync();
        ex.mark(21);
        double row[KR];
        {
            const double* Ib0 = ws.inv + boffB + bi * bk;
#pragma unroll
            for (int c = 0; c < KR; ++c) row[c] = (modeb && c < bk) ? Ib0[c] : 0.0;
        }
        ex.mark(22);
        for (int j = 0; j < kbB; ++j) {
            double* Pj = ws.stage + ((j & 1) * LMAX + lp) * 16;
            if (modeb && bi == j) {
#pragma unroll
                for (int c = 0; c < KR; ++c) Pj[c] = row[c];
            }
            ex.sync();
            if (modeb && j < bk) {
                double f = 0.0;
#pragma unroll
                for (int c = 0; c < KR; ++c) f = (c == j) ? row[c] : f;
                const double piv = Pj[j];
                okrow = okrow && (piv > PLSPM_PIVOT_RTOL * ws.mu[bb0 + j]);
                const double ip = wave_rcp(piv);
                const bool pivlane = bi == j;
                const double fip = f * ip;
#pragma unroll
                for (int c = 0; c < KR; ++c) {
                    const double rjc = Pj[c] * ip;
                    const double off = pivlane ? rjc : row[c] - f * rjc;
                    const double dia = pivlane ? ip : -fip;
                    row[c] = (c == j) ? dia : off;
                }
            }
        }
        ex.mark(23);
#pragma unroll
        for (int c = 0; c < KR; ++c) if (modeb && c < bk) ws.inv[boffB + bi * bk + c] = row[c];
        ex.sync();
        ex.mark(24);
    };
    if (kbB <= 8) sweep_rows(std::integral_constant<int, 8>{});
    else if (kbB <= 12) sweep_rows(std::integral_constant<int, 12>{});
    else if (kbB <= 16) sweep_rows(std::integral_constant<int, 16>{});
    else {
        fill_block(A);
        ex.sync();
        for (int j = 0; j < kbB; ++j) {
            if (modeb) {
                const double* Ab = A + boffB;
                double* Ob = An + boffB;
                if (j < bk) {
                    const double piv = Ab[j * bk + j];
                    okrow = okrow && (piv > PLSPM_PIVOT_RTOL * ws.mu[bb0 + j]);
                    const double ip = 1.0 / piv;
                    const double f = Ab[bi * bk + j];
                    for (int c = 0; c < bk; ++c) {
                        const double rjc = Ab[j * bk + c] * ip;
                        double v;
                        if (bi == j) v = (c == j) ? ip : rjc;
                        else v = (c == j) ? -f * ip : Ab[bi * bk + c] - f * rjc;
                        Ob[bi * bk + c] = v;
                    }
                } else {
                    for (int c = 0; c < bk; ++c) Ob[bi * bk + c] = Ab[bi * bk + c];      // a smaller block waits out the larger ones' steps
                }
            }
            ex.sync();
            double* t = A; A = An; An = t;
        }
    }
    // rank-deficient blocks, one at a time: S_bb once more from the registers, pseudo-inverse on the block's LV lane (scratch: the staging area)
    const bool any_bad = ex.vote_any(modeb && !okrow);      // (one ballot instead of a descriptor walk when every sweep went through)
    for (int l = 0; any_bad && l < L; ++l) {
        if (md.mode[l] != MODE_B) continue;
        const int k = md.boff[l + 1] - md.boff[l];
        const bool bad_here = ex.vote_any(modeb && lp == l && !okrow);
        if (!bad_here) continue;
        if (lp == l) fill_block(ws.inv);
        ex.sync();
        if (p == l) {
            double* F = ws.inv + md.chol_off[l] / 2;
            bool ok = k > 1 && jacobi_pinv(F, k, ws.stage);
            if (!ok) singular = true;
            for (int r = 0; r < k; ++r) for (int c = 0; c < r; ++c) F[r * k + c] = F[c * k + r];      // jacobi_pinv leaves the upper triangle
        }
        ex.sync();
    }
    ex.mark(25);
}

// Mode-B outer step (mode.py:51), entry bi of w_b = S_bb^-1 c_b: Ib = row bi of the block's inverse (above), cb = the block's slice of the Mode-A answers
// every lane published; even and odd terms in chains of their own
PLSPM_HD double wave_modeb_dot(const double* Ib, const double* cb, int bk) {
    double a0 = 0.0, a1 = 0.0;
    int q = 0;
    for (; q + 1 < bk; q += 2) { a0 += Ib[q] * cb[q]; a1 += Ib[q + 1] * cb[q + 1]; }
    if (q < bk) a0 += Ib[q] * cb[q];
    return a0 + a1;
}

// Status word from the (already voted) flags: singular before not converged, non-finite only over an otherwise clean problem.
PLSPM_HD int wave_status(bool sing, bool not_converged, bool bad) {
    int st = sing ? ST_SINGULAR : (not_converged ? ST_NOT_CONVERGED : ST_OK);
    if (st == ST_OK && bad) st = ST_NONFINITE;
    return st;
}

}  // namespace plspm
