// TEST INFRASTRUCTURE ONLY.  CPU emulation build of the device-side solver (csrc/solver_core.h):
// the same source the HIP kernel compiles, executed by NT std::threads with a std::barrier playing
// __syncthreads().  Lets the CPU test-suite (and ThreadSanitizer) check the solver's algebra and its
// barrier discipline against the oracle without a GPU.  Never loaded by the product package.
#include <algorithm>
#include <barrier>
#include <cstring>
#include <thread>
#include <vector>

#include "../../plspm-python_amd/csrc/solver_core.h"
#include "../../plspm-python_amd/csrc/solver_nmg.h"
#include "../../plspm-python_amd/csrc/solver_hoc.h"
#include "../../plspm-python_amd/csrc/solver_nmx.h"
#include "../../plspm-python_amd/csrc/solver_ops.h"
#include "../../plspm-python_amd/csrc/solver_wave.h"
#include "../../plspm-python_amd/csrc/solver_quad.h"
#include "../../plspm-python_amd/csrc/solver_wave16.h"
#include "../../plspm-python_amd/csrc/solver_route.h"
#include "../../plspm-python_amd/csrc/nm_route.h"
#include "../../plspm-python_amd/csrc/gram_route.h"
#include "../../plspm-python_amd/csrc/batch_route.h"
#include "../../plspm-python_amd/csrc/fit_route.h"
#include "../../plspm-python_amd/csrc/derived_route.h"
#include "../../plspm-python_amd/csrc/group_route.h"
#include "../../plspm-python_amd/csrc/options.h"

using namespace plspm;

struct HostExec {
    static constexpr int kcap = 8;
    int tid, nt;
    std::barrier<>* bar;
    template <class F> void par(int n, F f) { for (int i = tid; i < n; i += nt) f(i); bar->arrive_and_wait(); }
    template <class F> void one(F f) { if (tid == 0) f(); bar->arrive_and_wait(); }
    void mark(int) {}
    void sync() { bar->arrive_and_wait(); }
    unsigned long long uniform(unsigned long long v) { return v; }
    double* sink(double*) { static thread_local double mine[64]; return mine; }       // (no shared writes: ThreadSanitizer runs this code)
    // (device: w as a DPP broadcast operand of the multiply-adds, block ends by scalar bit tests; same order of additions)
    template <int PMAX> void seg_products(const double (&s)[PMAX], const double* w, int P, unsigned long long ends, double* vrow) {
        double r0 = 0.0, r1 = 0.0;
        for (int q = 0; q < PMAX && q < P; ++q) {
            if (q & 1) r1 += s[q] * w[q]; else r0 += s[q] * w[q];
            if ((ends >> q) & 1ull) { *vrow++ = r0 + r1; r0 = 0.0; r1 = 0.0; }
        }
    }
    // (device_exec.h seg_products2: a second store per block, the sum times `scale`, OFF2 bytes behind the first)
    template <int PMAX, int OFF2> void seg_products2(const double (&s)[PMAX], const double* w, int P, unsigned long long ends, double* vrow, double scale) {
        double r0 = 0.0, r1 = 0.0;
        for (int q = 0; q < PMAX && q < P; ++q) {
            if (q & 1) r1 += s[q] * w[q]; else r0 += s[q] * w[q];
            if ((ends >> q) & 1ull) { const double v = r0 + r1; *vrow = v; vrow[OFF2 / 8] = v * scale; ++vrow; r0 = 0.0; r1 = 0.0; }
        }
    }
    // (device: rows read along the lanes + LDS transposition, device_exec.h; here the plain symmetric lookup)
    template <int PMAX> void load_cov_block(const double* Md, int PS, int, int pc, int q0, int nq, double (&s)[PMAX]) {
        for (int q = 0; q < PMAX; ++q) {
            const int qc = q0 + ((q < nq) ? q : nq - 1);
            s[q] = Md[(qc <= pc) ? qc * PS + pc : pc * PS + qc];
        }
    }
    template <class F> void par2(int n0, int n1, F f) {
        for (int e = tid; e < n0 * n1; e += nt) f(e % n0, e / n0);
        bar->arrive_and_wait();
    }
    template <class F> void par_chunks64(int nchunks, const double* src, F f) {
        for (int c = tid; c < nchunks; c += nt) for (int lane = 0; lane < 64; ++lane) f(c, lane, src[c * 64 + lane]);
        bar->arrive_and_wait();
    }
    double* red;
    template <class F> double sum(int n, F f) {
        double s = 0.0;
        for (int i = tid; i < n; i += nt) s += f(i);
        red[tid] = s;
        bar->arrive_and_wait();
        double t = 0.0;
        for (int k = 0; k < nt; ++k) t += red[k];
        bar->arrive_and_wait();
        return t;
    }
    // ---- wave executor of solver_wave.h (nt == 64: one emulated thread per lane) ----
    // butterfly sum in the device's order (v += value of lane ^ 1, 2, ... 32: wave_ops.h): bitwise the same value on every lane
    double allsum(double v) {
        for (int off = 1; off < 64; off <<= 1) {
            red[tid] = v;
            bar->arrive_and_wait();
            const double t = red[tid ^ off];
            bar->arrive_and_wait();
            v += t;
        }
        return v;
    }
    int vote_count(bool b) {
        red[tid] = b ? 1.0 : 0.0;
        bar->arrive_and_wait();
        int c = 0;
        for (int k = 0; k < nt; ++k) c += red[k] != 0.0 ? 1 : 0;
        bar->arrive_and_wait();
        return c;
    }
    bool vote_any(bool b) { return vote_count(b) > 0; }
    // ballot over the caller's 64-lane wave (solver_quad.h: nt == 256, four emulated waves)
    int wave_vote_count(bool b) {
        red[tid] = b ? 1.0 : 0.0;
        bar->arrive_and_wait();
        int c = 0;
        for (int k = tid & ~63; k < (tid & ~63) + 64 && k < nt; ++k) c += red[k] != 0.0 ? 1 : 0;
        bar->arrive_and_wait();
        return c;
    }
    void fence() {}
    double uniform_d(double v) { return v; }
    int uniform_i(int v) { return v; }
    double bcast(double, int q, const double* published) { return published[q]; }
    void opaque(unsigned&) {}
    void opaque(int&) {}
    void pin8(double&, double&, double&, double&, double&, double&, double&, double&) {}
    // column `tid` of the symmetric moment matrix out of its upper triangle (device: coalesced rows + an LDS transpose)
    template <int PMAX> void load_cov(const double* Md, int PS, int P, double (&s)[PMAX], double*, double& mu, double& diag) {
        for (int q = 0; q < PMAX; ++q) s[q] = (q < P && tid < P) ? Md[(long)(q < tid ? q : tid) * PS + (q < tid ? tid : q)] : 0.0;
        mu = tid < P ? Md[(long)tid * PS + P] : 0.0;
        diag = tid < P ? Md[(long)tid * PS + tid] : 0.0;
    }
    template <class F> bool any(int n, F f) {
        double s = 0.0;
        for (int i = tid; i < n; i += nt) if (f(i)) s = 1.0;
        red[tid] = s;
        bar->arrive_and_wait();
        bool t = false;
        for (int k = 0; k < nt; ++k) t = t || (red[k] != 0.0);
        bar->arrive_and_wait();
        return t;
    }
};

// Host-side model descriptors shared by the entry points below.
struct EmuModel {
    std::vector<int> lvof, chol_off, pred_off, pred_idx, succ_off, succ_idx;
    ModelDesc md{};
    EmuModel(int P, int L, int PA, int scheme, int scaled, int max_iter, double tol, const int* boff, const unsigned char* C, const int* mode,
             const double* shift, int n_eff, const int* eff_from, const int* eff_to)
        : lvof(P), chol_off(L, -1), pred_off(L + 1, 0), succ_off(L + 1, 0) {
        int kmax = 0, n_chol = 0;
        for (int l = 0; l < L; ++l) {
            for (int p = boff[l]; p < boff[l + 1]; ++p) lvof[p] = l;
            int k = 0;
            for (int j = 0; j < L; ++j) k += C[l * L + j] ? 1 : 0;
            kmax = k > kmax ? k : kmax;
            if (mode[l] == MODE_B) { int kb = boff[l + 1] - boff[l]; chol_off[l] = n_chol; n_chol += (int)chol_block_doubles(kb); }
        }
        for (int i = 0; i < L; ++i) {
            for (int j = 0; j < L; ++j) if (C[i * L + j]) pred_idx.push_back(j);
            pred_off[i + 1] = (int)pred_idx.size();
            for (int s2 = 0; s2 < L; ++s2) if (C[s2 * L + i]) succ_idx.push_back(s2);
            succ_off[i + 1] = (int)succ_idx.size();
        }
        md.n_edges = pred_off[L];
        pred_idx.push_back(0); succ_idx.push_back(0);
        md.P = P; md.L = L; md.PA = PA; md.T = PA / 16; md.scheme = scheme; md.scaled = scaled; md.max_iter = max_iter;
        md.kmax = kmax; md.n_eff = n_eff; md.n_chol = n_chol; md.tol = tol; md.boff = boff; md.lvof = lvof.data(); md.C = C;
        md.mode = mode; md.chol_off = chol_off.data(); md.eff_from = eff_from; md.eff_to = eff_to; md.shift = shift;
        md.pred_off = pred_off.data(); md.pred_idx = pred_idx.data(); md.succ_off = succ_off.data(); md.succ_idx = succ_idx.data();
        md.tile_tu = nullptr;
    }
};

template <class Body>
static void run_group(int nthreads_in, int P, int L, const ModelDesc& md, double* S, Body body) {
    const int nthreads = nthreads_in > 16 ? 16 : nthreads_in;
    std::vector<double> small(workspace_small_doubles(P, L, md.kmax, md.n_chol));
    std::barrier<> bar(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t]() {
            Workspace ws{};
            ws.S = S; ws.PS = cov_ld(P);
            carve_small(ws, small.data(), P, L, md.kmax, md.n_chol);
            HostExec ex{t, nthreads, &bar, ws.red};
            body(ex, ws);
        });
    for (auto& x : th) x.join();
}

template <class Body>
static void run_plain(int nthreads_in, Body body) {
    const int nthreads = nthreads_in > 16 ? 16 : nthreads_in;
    std::vector<double> red(nthreads);
    std::barrier<> bar(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t) th.emplace_back([&, t]() { HostExec ex{t, nthreads, &bar, red.data()}; body(ex); });
    for (auto& x : th) x.join();
}

// flat arrays -> the inputs of nm_plan (the order hostemu_nm_plan documents) and of batch_plan (hostemu_batch_plan)
static NmShape nm_shape_of(const long* sh) {
    NmShape s{};
    s.P = (int)sh[0]; s.P1 = (int)sh[1]; s.Pm = (int)sh[2]; s.L = (int)sh[3]; s.kmax = (int)sh[4]; s.n_chol = (int)sh[5]; s.n_eff = (int)sh[6]; s.nedge = (int)sh[7]; s.cmax = (int)sh[8];
    s.kmv = (int)sh[9]; s.kb = (int)sh[10]; s.max_iter = (int)sh[11]; s.N = sh[12]; s.nmx_K = (int)sh[13];
    s.nonmetric = sh[14]; s.categorical = sh[15]; s.cat_pure = sh[16]; s.src_cat_pure = sh[17]; s.all_mode_a = sh[18]; s.attached = sh[19]; s.has_stage2 = sh[20]; s.has_ind = sh[21];
    s.codes_tables = sh[22];
    return s;
}
static NmOptions nm_options_of(const int* o) { return NmOptions{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10], o[11], o[12]}; }
struct BatchIn { BatchShape s; BatchOptions o; BatchKind c; };
static BatchIn batch_in_of(const long* sh, const int* boff, const long* nm1, const long* nm2, const int* o, const int* onm1, const int* onm2, const long* call) {
    BatchIn in{};
    in.s.N = sh[0]; in.s.P = (int)sh[1]; in.s.Pg = (int)sh[2]; in.s.T = (int)sh[3]; in.s.L = (int)sh[4]; in.s.R = (int)sh[5]; in.s.n_ind = (int)sh[6];
    in.s.nonmetric = sh[7]; in.s.has_stage1 = sh[8]; in.s.has_stage2 = sh[9]; in.s.micom_on = sh[10]; in.s.plain_metric = sh[11];
    in.s.route = RouteShape{in.s.P, in.s.L, (int)sh[12], (int)sh[13], (int)sh[14], (int)sh[15], boff};
    in.s.nm = nm_shape_of(nm1); in.s.nm2 = nm_shape_of(nm2);
    in.o = BatchOptions{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10], nm_options_of(onm1), nm_options_of(onm2), o[11] != 0};
    in.c = BatchKind{call[0], call[1] != 0, call[2] != 0, call[3] != 0, call[4] != 0, call[5] != 0, call[6] != 0};
    return in;
}

extern "C" {

// ---- operator seam (csrc/solver_ops.h): Mp = tile-packed moment matrix of the SHIFTED columns + ones, shift = the column means
void hostemu_op_inner_weights(int L, int PA, int scheme, const unsigned char* C, const double* shift, const double* Mp, int nthreads, double* E) {
    std::vector<int> boff(L + 1), mode(L, MODE_A);
    for (int l = 0; l <= L; ++l) boff[l] = l;
    EmuModel em(L, L, PA, scheme, 0, 1, 1.0, boff.data(), C, mode.data(), shift, 0, nullptr, nullptr);
    run_group(nthreads, L, L, em.md, nullptr, [&](HostExec& ex, Workspace& ws) { op_inner_weights(ex, em.md, ws, Mp, E); });
}
int hostemu_op_outer_weights(int mode, int k, int PA, const double* shift, const double* Mp, int nthreads, double* w) {
    std::vector<double> scratch(3 * (size_t)k * k + 1);
    run_plain(nthreads, [&](HostExec& ex) {
        op_outer_weights(ex, mode, k, PA / 16, Mp, shift, scratch.data(), scratch.data() + (size_t)k * k, scratch.data() + 2 * (size_t)k * k, w, scratch.data() + 3 * (size_t)k * k);
    });
    return scratch[3 * (size_t)k * k] != 0.0 ? 0 : 2;
}

// ---- non-metric (NUM / RAW) entry points: S (R matrix, cov_doubles(P)) and state (nm_state_doubles) persist in caller memory
long hostemu_cov_doubles(int P) { return cov_doubles(P); }
long hostemu_nm_state_doubles(int P, int L, int n_chol) { return nm_state_doubles(P, L, n_chol); }

int hostemu_nm_prepare(int P, int L, int PA, int scheme, int max_iter, double tol, const int* boff, const unsigned char* C, const int* mode,
                       const double* shift, const double* Mp, int nthreads, double* S, double* state) {
    EmuModel em(P, L, PA, scheme, 1, max_iter, tol, boff, C, mode, shift, 0, nullptr, nullptr);
    run_group(nthreads, P, L, em.md, S, [&](HostExec& ex, Workspace& ws) {
        NmState st; nm_carve(st, state, P, L);
        nm_prepare(ex, em.md, ws, st, Mp);
    });
    return em.md.n_chol;
}
// returns 1 when the problem is still active after the call
int hostemu_nm_step(int P, int L, int PA, int scheme, int max_iter, double tol, const int* boff, const unsigned char* C, const int* mode,
                    const double* shift, int nthreads, double* S, double* state, const double* partial, int nparts) {
    EmuModel em(P, L, PA, scheme, 1, max_iter, tol, boff, C, mode, shift, 0, nullptr, nullptr);
    int active = 0;
    run_group(nthreads, P, L, em.md, S, [&](HostExec& ex, Workspace& ws) {
        NmState st; nm_carve(st, state, P, L);
        const bool a = nm_step(ex, em.md, ws, st, partial, nparts);
        if (ex.tid == 0) active = a ? 1 : 0;
    });
    return active;
}
int hostemu_nm_finish(int P, int L, int PA, int scheme, int max_iter, double tol, const int* boff, const unsigned char* C, const int* mode,
                      const double* shift, int n_eff, const int* eff_from, const int* eff_to, int nthreads, double* S, double* state, double* row,
                      double* crossloadings, double* path_coef, double* lv_cov, double* indirect, double* score_w, double* score_c, double* cov,
                      double* mean, int* iters, int* status) {
    EmuModel em(P, L, PA, scheme, 1, max_iter, tol, boff, C, mode, shift, n_eff, eff_from, eff_to);
    FitOutputs out{};
    out.row = row; out.crossloadings = crossloadings; out.path_coef = path_coef; out.lv_cov = lv_cov; out.indirect = indirect;
    out.score_w = score_w; out.score_c = score_c; out.cov = cov; out.mean = mean; out.iters = iters; out.status = status;
    run_group(nthreads, P, L, em.md, S, [&](HostExec& ex, Workspace& ws) {
        NmState st; nm_carve(st, state, P, L);
        nm_finish(ex, em.md, ws, st, out);
    });
    return 0;
}

// ---- categorical (ORD / NOM) non-metric entry points.  boff: aug-column block offsets per LV; mv_off / mv_kind / lmv_off: CatDesc.
struct EmuCat {
    CatDesc cd{};
    std::vector<int> mv_lv;
    EmuCat(int Pm, int L, const int* mv_off, const int* mv_kind, const int* lmv_off) : mv_lv(Pm) {
        cd.Pm = Pm; cd.mv_off = mv_off; cd.mv_kind = mv_kind; cd.lmv_off = lmv_off; cd.cmax = 1; cd.kmv = 1;
        for (int p = 0; p < Pm; ++p) cd.cmax = std::max(cd.cmax, mv_off[p + 1] - mv_off[p]);
        for (int l = 0; l < L; ++l) { cd.kmv = std::max(cd.kmv, lmv_off[l + 1] - lmv_off[l]); for (int p = lmv_off[l]; p < lmv_off[l + 1]; ++p) mv_lv[p] = l; }
    }
};
long hostemu_nmg_state_doubles(int Q, int Pm, int L, const int* mv_off, const int* mv_kind, const int* lmv_off) {
    EmuCat ec(Pm, L, mv_off, mv_kind, lmv_off);
    return nmg_state_doubles(Q, Pm, L, ec.cd.cmax, ec.cd.kmv);
}
// mode: 0 prepare, 1 step (returns active), 2 finish
int hostemu_nmg(int mode_op, int Q, int Pm, int L, int PA, int scheme, int max_iter, double tol, const int* boff, const unsigned char* C, const int* mode,
                const int* mv_off, const int* mv_kind, const int* lmv_off, const double* Mp, int nthreads, double* S, double* state,
                const double* partial, int nparts, int n_eff, const int* eff_from, const int* eff_to, double* row, double* crossloadings,
                double* path_coef, double* score_w, double* score_c, double* cov, int* iters, int* status) {
    std::vector<double> shift(Q, 0.0);
    EmuModel em(Q, L, PA, scheme, 1, max_iter, tol, boff, C, mode, shift.data(), n_eff, eff_from, eff_to);
    EmuCat ec(Pm, L, mv_off, mv_kind, lmv_off);
    std::vector<double> shift_m(Pm, 0.0);
    EmuModel emm(Pm, L, PA, scheme, 1, max_iter, tol, lmv_off, C, mode, shift_m.data(), n_eff, eff_from, eff_to);
    emm.md.n_chol = 0;
    std::vector<double> Sm((size_t)cov_doubles(Pm)), small_m(workspace_small_doubles(Pm, L, emm.md.kmax, 0));
    int active = 0;
    FitOutputs out{};
    out.row = row; out.crossloadings = crossloadings; out.path_coef = path_coef; out.score_w = score_w; out.score_c = score_c; out.cov = cov;
    out.iters = iters; out.status = status;
    em.md.n_chol = 0;
    run_group(nthreads, Q, L, em.md, S, [&](HostExec& ex, Workspace& ws) {
        NmState st; nm_carve(st, state, Q, L);
        NmgExtra x; nmg_carve(x, state + nm_state_doubles(Q, L, 0), Q, Pm, L, ec.cd.cmax, ec.cd.kmv);
        if (mode_op == 0) nmg_prepare(ex, em.md, ec.cd, ws, st, x, Mp);
        else if (mode_op == 1) { const bool a = nmg_step(ex, em.md, ec.cd, ws, st, x, partial, nparts); if (ex.tid == 0) active = a ? 1 : 0; }
        else {
            Workspace wsm{};
            wsm.S = Sm.data(); wsm.PS = cov_ld(Pm);
            carve_small(wsm, small_m.data(), Pm, L, emm.md.kmax, 0);
            nmg_finish(ex, em.md, ec.cd, emm.md, ws, wsm, st, x, out);
        }
    });
    return active;
}

// Mp: packed scatter (see packed_index); everything else mirrors ModelDesc / FitOutputs.
int hostemu_solve(int P, int L, int PA, int scheme, int scaled, int max_iter, double tol, const int* boff, const unsigned char* C,
                  const int* mode, const double* shift, int n_eff, const int* eff_from, const int* eff_to, const double* Mp,
                  int nthreads_in, double* row, double* crossloadings, double* path_coef, double* lv_cov, double* indirect,
                  double* score_w, double* score_c, double* cov, double* mean, int8_t* sign, int* iters, int* status) {
    const int nthreads = nthreads_in > 16 ? 16 : nthreads_in;
    std::vector<int> lvof(P), chol_off(L, -1);
    int kmax = 0, n_chol = 0;
    for (int l = 0; l < L; ++l) {
        for (int p = boff[l]; p < boff[l + 1]; ++p) lvof[p] = l;
        int k = 0;
        for (int j = 0; j < L; ++j) k += C[l * L + j] ? 1 : 0;
        kmax = k > kmax ? k : kmax;
        if (mode[l] == MODE_B) { int kb = boff[l + 1] - boff[l]; chol_off[l] = n_chol; n_chol += (int)chol_block_doubles(kb); }
    }
    std::vector<int> pred_off(L + 1, 0), pred_idx, succ_off(L + 1, 0), succ_idx;
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < L; ++j) if (C[i * L + j]) pred_idx.push_back(j);
        pred_off[i + 1] = (int)pred_idx.size();
        for (int s2 = 0; s2 < L; ++s2) if (C[s2 * L + i]) succ_idx.push_back(s2);
        succ_off[i + 1] = (int)succ_idx.size();
    }
    pred_idx.push_back(0); succ_idx.push_back(0);
    ModelDesc md{};
    md.pred_off = pred_off.data(); md.pred_idx = pred_idx.data(); md.succ_off = succ_off.data(); md.succ_idx = succ_idx.data();
    md.n_edges = pred_off[L];
    md.P = P; md.L = L; md.PA = PA; md.T = PA / 16; md.scheme = scheme; md.scaled = scaled; md.max_iter = max_iter;
    md.kmax = kmax; md.n_eff = n_eff; md.n_chol = n_chol; md.tol = tol; md.boff = boff; md.lvof = lvof.data(); md.C = C;
    md.mode = mode; md.chol_off = chol_off.data(); md.eff_from = eff_from; md.eff_to = eff_to; md.shift = shift;
    const int PS = cov_ld(P);
    std::vector<double> S((size_t)cov_doubles(P)), small(workspace_small_doubles(P, L, kmax, n_chol));
    FitOutputs out{};
    out.row = row; out.crossloadings = crossloadings; out.path_coef = path_coef; out.lv_cov = lv_cov; out.indirect = indirect;
    out.score_w = score_w; out.score_c = score_c; out.cov = cov; out.mean = mean; out.sign = sign; out.iters = iters; out.status = status;
    std::barrier<> bar(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t]() {
            Workspace ws{};
            ws.S = S.data(); ws.PS = PS;
            carve_small(ws, small.data(), P, L, kmax, n_chol);
            HostExec ex{t, nthreads, &bar, ws.red};
            solve_problem(ex, md, ws, Mp, out);
        });
    for (auto& x : th) x.join();
    return 0;
}

// Rows variant (solve_problem_rows<64>): Md = dense symmetric moment matrix [(P+1) x cov_ld(P)] of the shifted columns + ones; one
// emulated thread per lane of the device wave (at least P).
int hostemu_solve_rows(int P, int L, int PA, int scheme, int scaled, int max_iter, double tol, const int* boff, const unsigned char* C,
                       const int* mode, const double* shift, int n_eff, const int* eff_from, const int* eff_to, const double* Md,
                       int nthreads, double* row, double* crossloadings, double* path_coef, double* lv_cov, double* indirect,
                       double* score_w, double* score_c, double* cov, double* mean, int8_t* sign, int* iters, int* status) {
    // nthreads 256: the split form (solve_problem_rows<64, true>: 64 < P <= 128, two emulated threads per MV, no covariance output)
    const bool split = nthreads == 256;
    if (split ? (P <= 64 || P > 128 || rows_split_block(boff, L, 64) == 0) : (P > 64 || nthreads < P || nthreads > 64)) return 1;
    if (split) cov = nullptr;
    EmuModel em(P, L, PA, scheme, scaled, max_iter, tol, boff, C, mode, shift, n_eff, eff_from, eff_to);
    std::vector<double> small(workspace_small_doubles(P, L, em.md.kmax, em.md.n_chol)), red(nthreads);
    FitOutputs out{};
    out.row = row; out.crossloadings = crossloadings; out.path_coef = path_coef; out.lv_cov = lv_cov; out.indirect = indirect;
    out.score_w = score_w; out.score_c = score_c; out.cov = cov; out.mean = mean; out.sign = sign; out.iters = iters; out.status = status;
    std::barrier<> bar(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t]() {
            Workspace ws{};
            ws.S = nullptr; ws.PS = cov_ld(P);
            carve_small(ws, small.data(), P, L, em.md.kmax, em.md.n_chol);
            HostExec ex{t, nthreads, &bar, red.data()};
            if (split) solve_problem_rows<64, true>(ex, em.md, ws, Md, out);
            else solve_problem_rows<64>(ex, em.md, ws, Md, out);
        });
    for (auto& x : th) x.join();
    return 0;
}

// The wave solver's reciprocal forms (seed of the hardware's accuracy + two Newton steps): the emulation executes the same refinement.
double hostemu_wave_rsqrt(double x) { return wave_rsqrt(x); }
double hostemu_wave_rcp(double x) { return wave_rcp(x); }

// Wave solver (solver_wave.h solve_problem_wave<8>): same inputs as the rows variant, 64 emulated lanes; returns 1 for a model it does not cover.
int hostemu_solve_wave(int P, int L, int PA, int scheme, int scaled, int max_iter, double tol, const int* boff, const unsigned char* C,
                       const int* mode, const double* shift, int n_eff, const int* eff_from, const int* eff_to, const double* Md,
                       double* row, int* iters, int* status) {
    EmuModel em(P, L, PA, scheme, scaled, max_iter, tol, boff, C, mode, shift, n_eff, eff_from, eff_to);
    if (!wave_solver_covers<8>(P, L, em.md.n_chol)) return 1;
    const int nthreads = 64;
    std::vector<double> lds(wave_ws_doubles<8>(em.md.n_chol), 0.0), red(nthreads);
    FitOutputs out{};
    out.row = row; out.iters = iters; out.status = status;
    std::barrier<> bar(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t]() {
            WaveWs<8> ws{};
            wave_carve(ws, lds.data());
            HostExec ex{t, nthreads, &bar, red.data()};
            if (em.md.n_chol > 0) solve_problem_wave<8, true>(ex, em.md, ws, Md, out);
            else solve_problem_wave<8, false>(ex, em.md, ws, Md, out);
        });
    for (auto& x : th) x.join();
    return 0;
}

// Wave solver for 9 .. 16 LVs (solver_wave16.h solve_problem_wave16<16>): 64 emulated lanes; returns 1 for a model it does not cover.
int hostemu_solve_wave16(int P, int L, int PA, int scheme, int scaled, int max_iter, double tol, const int* boff, const unsigned char* C,
                         const int* mode, const double* shift, int n_eff, const int* eff_from, const int* eff_to, const double* Md,
                         double* row, int* iters, int* status) {
    EmuModel em(P, L, PA, scheme, scaled, max_iter, tol, boff, C, mode, shift, n_eff, eff_from, eff_to);
    if (!wave16_solver_covers<16>(P, L, em.md.n_chol, em.md.kmax)) return 1;
    const int nthreads = 64;
    std::vector<double> lds(wave16_ws_doubles<16>(L, em.md.kmax, em.md.n_chol), 0.0), red(nthreads);
    FitOutputs out{};
    out.row = row; out.iters = iters; out.status = status;
    std::barrier<> bar(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t]() {
            Wave16Ws<16> ws{};
            wave16_carve(ws, lds.data(), L, em.md.kmax);
            HostExec ex{t, nthreads, &bar, red.data()};
            if (em.md.n_chol > 0) solve_problem_wave16<16, true>(ex, em.md, ws, Md, out);
            else solve_problem_wave16<16, false>(ex, em.md, ws, Md, out);
        });
    for (auto& x : th) x.join();
    return 0;
}

// The same source at LMAX = 8 (one matrix entry per pair lane, the product stream's second copy w V: the A/B form of the wave solver's own class,
// set_option("solver_wave", 2)); returns 1 for a model it does not cover.
int hostemu_solve_wave16_l8(int P, int L, int PA, int scheme, int scaled, int max_iter, double tol, const int* boff, const unsigned char* C,
                            const int* mode, const double* shift, int n_eff, const int* eff_from, const int* eff_to, const double* Md,
                            double* row, int* iters, int* status) {
    EmuModel em(P, L, PA, scheme, scaled, max_iter, tol, boff, C, mode, shift, n_eff, eff_from, eff_to);
    if (!wave_solver_covers<8>(P, L, em.md.n_chol)) return 1;
    const int nthreads = 64;
    std::vector<double> lds(wave16_ws_doubles<8>(L, em.md.kmax, em.md.n_chol), 0.0), red(nthreads);
    FitOutputs out{};
    out.row = row; out.iters = iters; out.status = status;
    std::barrier<> bar(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t]() {
            Wave16Ws<8> ws{};
            wave16_carve(ws, lds.data(), L, em.md.kmax);
            HostExec ex{t, nthreads, &bar, red.data()};
            if (em.md.n_chol > 0) solve_problem_wave16<8, true>(ex, em.md, ws, Md, out);
            else solve_problem_wave16<8, false>(ex, em.md, ws, Md, out);
        });
    for (auto& x : th) x.join();
    return 0;
}

// The non-metric (Scale.NUM / RAW) instantiation of the same source (solver_wave16.h NM; round 6): LMAX = 8 for at most 8 LVs, else 16.  maps: [(max_iter + 2) x (P + L)]
// score maps of the steps the problem continued behind (or null), force_T > 0: stop behind exactly that many steps.  Returns 1 for a model it does not cover.
int hostemu_solve_nmwave16(int P, int L, int PA, int scheme, int scaled, int max_iter, double tol, const int* boff, const unsigned char* C,
                           const int* mode, const double* shift, int n_eff, const int* eff_from, const int* eff_to, const double* Md,
                           double* row, int* iters, int* status, double* maps, int force_T, int* steps) {
    EmuModel em(P, L, PA, scheme, scaled, max_iter, tol, boff, C, mode, shift, n_eff, eff_from, eff_to);
    const bool small = L <= 8, big = L > 16;
    if (small ? !(P <= 64 && em.md.n_chol / 2 <= 16 * 66) : (big ? !(em.md.n_chol == 0 && wave16_solver_covers<32>(P, L, 0, em.md.kmax)) : !wave16_solver_covers<16>(P, L, em.md.n_chol, em.md.kmax))) return 1;
    const int nthreads = 64;
    const long wsd = small ? wave16_ws_doubles<8>(L, em.md.kmax, em.md.n_chol) : (big ? wave16_ws_doubles<32>(L, em.md.kmax, 0) : wave16_ws_doubles<16>(L, em.md.kmax, em.md.n_chol));
    std::vector<double> lds(wsd + 64, 0.0), red(nthreads);
    FitOutputs out{};
    out.row = row; out.iters = iters; out.status = status;
    NmWaveIo io{maps, force_T, steps, 1.0};
    std::barrier<> bar(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t]() {
            HostExec ex{t, nthreads, &bar, red.data()};
            if (small) {
                Wave16Ws<8> ws{};
                wave16_carve(ws, lds.data(), L, em.md.kmax);
                if (em.md.n_chol > 0) solve_problem_wave16<8, true, true>(ex, em.md, ws, Md, out, &io, lds.data() + wsd);
                else solve_problem_wave16<8, false, true>(ex, em.md, ws, Md, out, &io, lds.data() + wsd);
            } else if (big) {
                Wave16Ws<32> ws{};
                wave16_carve(ws, lds.data(), L, em.md.kmax);
                solve_problem_wave16<32, false, true>(ex, em.md, ws, Md, out, &io, lds.data() + wsd);
            } else {
                Wave16Ws<16> ws{};
                wave16_carve(ws, lds.data(), L, em.md.kmax);
                if (em.md.n_chol > 0) solve_problem_wave16<16, true, true>(ex, em.md, ws, Md, out, &io, lds.data() + wsd);
                else solve_problem_wave16<16, false, true>(ex, em.md, ws, Md, out, &io, lds.data() + wsd);
            }
        });
    for (auto& x : th) x.join();
    return 0;
}

// ... and at LMAX = 32 (sixteen matrix entries per pair lane: all-Mode-A models of 17 ... 32 LVs); returns 1 for a model it does not cover.
int hostemu_solve_wave16_l32(int P, int L, int PA, int scheme, int scaled, int max_iter, double tol, const int* boff, const unsigned char* C,
                             const int* mode, const double* shift, int n_eff, const int* eff_from, const int* eff_to, const double* Md,
                             double* row, int* iters, int* status) {
    EmuModel em(P, L, PA, scheme, scaled, max_iter, tol, boff, C, mode, shift, n_eff, eff_from, eff_to);
    if (em.md.n_chol != 0 || !wave16_solver_covers<32>(P, L, 0, em.md.kmax)) return 1;
    const int nthreads = 64;
    std::vector<double> lds(wave16_ws_doubles<32>(L, em.md.kmax, 0), 0.0), red(nthreads);
    FitOutputs out{};
    out.row = row; out.iters = iters; out.status = status;
    std::barrier<> bar(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t]() {
            Wave16Ws<32> ws{};
            wave16_carve(ws, lds.data(), L, em.md.kmax);
            HostExec ex{t, nthreads, &bar, red.data()};
            solve_problem_wave16<32, false>(ex, em.md, ws, Md, out);
        });
    for (auto& x : th) x.join();
    return 0;
}

// Quad solver (solver_quad.h solve_problem_quad<16>): 256 emulated threads = four waves; returns 1 for a model it does not cover.
int hostemu_solve_quad(int P, int L, int PA, int scheme, int scaled, int max_iter, double tol, const int* boff, const unsigned char* C,
                       const int* mode, const double* shift, int n_eff, const int* eff_from, const int* eff_to, const double* Md,
                       double* row, int* iters, int* status) {
    EmuModel em(P, L, PA, scheme, scaled, max_iter, tol, boff, C, mode, shift, n_eff, eff_from, eff_to);
    if (!quad_solver_covers<16>(P, L, em.md.n_chol, em.md.kmax, boff)) return 1;
    const int nthreads = 256;
    std::vector<double> lds(quad_ws_doubles<16>(L, em.md.kmax), 0.0), red(nthreads);
    FitOutputs out{};
    out.row = row; out.iters = iters; out.status = status;
    std::barrier<> bar(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t]() {
            QuadWs<16> ws{};
            quad_carve(ws, lds.data());
            HostExec ex{t, nthreads, &bar, red.data()};
            solve_problem_quad<16>(ex, em.md, ws, Md, out);
        });
    for (auto& x : th) x.join();
    return 0;
}

// Mean imputation on the moments (solver_core.h impute_collapse): aug packed Gram (Ta tiles) -> P-column packed moments (Ts tiles).
void hostemu_impute_collapse(int P, int Qa, int Ta, int Ts, const int* ind_of, const double* Min, double* Mout, int nthreads_in) {
    const int nthreads = nthreads_in > 16 ? 16 : nthreads_in;
    std::vector<double> gam(P), red(nthreads);
    std::barrier<> bar(nthreads);
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; ++t)
        th.emplace_back([&, t]() {
            HostExec ex{t, nthreads, &bar, red.data()};
            impute_collapse(ex, P, Qa, Ta, Ts, ind_of, Min, Mout, gam.data());
        });
    for (auto& x : th) x.join();
}

// ---- two-stage higher order constructs (solver_hoc.h)
static HocDesc emu_hoc_desc(int P1, int L1, int P2, int L2, int T1, int T2, const int* boff1, const int* boff2, const int* lv_first, const int* col2_lv1,
                            const int* col2_p1, int nh, const int* hcol, const int* hidx) {
    HocDesc hd{};
    hd.P1 = P1; hd.L1 = L1; hd.P2 = P2; hd.L2 = L2; hd.T1 = T1; hd.T2 = T2; hd.boff1 = boff1; hd.boff2 = boff2; hd.lv_first = lv_first;
    hd.col2_lv1 = col2_lv1; hd.col2_p1 = col2_p1; hd.nh = nh; hd.hcol = hcol; hd.hidx = hidx;
    return hd;
}
void hostemu_hoc_moments(int P1, int L1, int P2, int L2, int T1, int T2, const int* boff1, const int* boff2, const int* lv_first, const int* col2_lv1,
                         const int* col2_p1, int nh, const int* hcol, const int* hidx, const double* M1, const double* c1, const double* k1, int ok,
                         double* M2, int nthreads) {
    const HocDesc hd = emu_hoc_desc(P1, L1, P2, L2, T1, T2, boff1, boff2, lv_first, col2_lv1, col2_p1, nh, hcol, hidx);
    std::vector<double> V((size_t)(nh > 0 ? nh : 1) * (P1 + 1));
    run_plain(nthreads, [&](HostExec& ex) { hoc_second_stage_moments(ex, hd, M1, c1, k1, ok != 0, M2, V.data()); });
}
void hostemu_hoc_compose(int P1, int L1, int P2, int L2, const int* boff1, const int* boff2, const int* lv_first, const int* col2_lv1, const double* c1,
                         const double* k1, double* state2, double* pseudo, int nthreads) {
    const HocDesc hd = emu_hoc_desc(P1, L1, P2, L2, 0, 0, boff1, boff2, lv_first, col2_lv1, nullptr, 0, nullptr, nullptr);
    run_plain(nthreads, [&](HostExec& ex) { NmState st2; nm_carve(st2, state2, P2, L2); hoc_compose_score_maps(ex, hd, c1, k1, st2, pseudo); });
}

// ---- non-metric data with missing values (solver_nmx.h).  mode_op: 0 prepare, 1 step (returns active), 2 finish.  The caller
// writes the incomplete rows' weights ck[K] at state[nm_state_doubles(P, L, n_chol)] before the prepare call.
long hostemu_nmx_state_doubles(int P, int L, int n_chol, int K) { return nmx_state_doubles(P, L, n_chol, K); }
int hostemu_nmx(int mode_op, int raw, int P, int L, int PA, int scheme, int max_iter, double tol, const int* boff, const unsigned char* C, const int* mode, int K,
                const double* Xk, const double* Mk, const double* Mp, int nthreads, double* S, double* state, const double* partial, int nparts, int n_eff,
                const int* eff_from, const int* eff_to, double* row, double* crossloadings, double* path_coef, double* score_w, double* score_c, double* cov,
                int* iters, int* status) {
    std::vector<double> shift(P, 0.0);
    EmuModel em(P, L, PA, scheme, 1, max_iter, tol, boff, C, mode, shift.data(), n_eff, eff_from, eff_to);
    MissDesc xd{raw, K, Xk, Mk};
    int active = 0;
    FitOutputs out{};
    out.row = row; out.crossloadings = crossloadings; out.path_coef = path_coef; out.score_w = score_w; out.score_c = score_c; out.cov = cov;
    out.iters = iters; out.status = status;
    run_group(nthreads, P, L, em.md, S, [&](HostExec& ex, Workspace& ws) {
        NmState st; nm_carve(st, state, P, L);
        NmxExtra x; nmx_carve(x, state + nm_state_doubles(P, L, em.md.n_chol), P, L, K);
        if (mode_op == 0) nmx_prepare(ex, em.md, xd, ws, st, x, Mp);
        else if (mode_op == 1) { const bool a = nmx_step(ex, em.md, xd, ws, st, x, partial, nparts); if (ex.tid == 0) active = a ? 1 : 0; }
        else nmx_finish(ex, em.md, xd, ws, st, x, out);
    });
    return active;
}

// The solver route of a model shape (csrc/solver_route.h): nm_wave_route when nm != 0, else metric_batch_route under the three solver options.
int hostemu_solver_route(int P, int L, int kmax, int n_chol, int n_eff, int nedge, const int* boff, int solver_wave, int solver_quad, int solver_rows, int nm) {
    const RouteShape s{P, L, kmax, n_chol, n_eff, nedge, boff};
    return nm ? nm_wave_route(s) : metric_batch_route(s, solver_wave, solver_quad, solver_rows);
}

// The route of a non-metric call (csrc/nm_route.h nm_plan).  shape: P, P1, Pm, L, kmax, n_chol, n_eff, nedge, cmax, kmv, kb, max_iter, N, nmx_K, then the flags nonmetric,
// categorical, cat_pure, src_cat_pure, all_mode_a, attached, has_stage2, has_ind, codes_tables; call: nproblems, counts8, lists_dcnt, counts16_ready, finish; opts in the
// order of NmOptions.  out: error, dense, dense_whole, use_codes, use_mfma, flag_from_list, k16, wave_step, bound_ok, sub_pass, one_launch, step LMAX, CMAX, CPL, num_one,
// direct16, KS, tpc, nparts, nsub, cat_fast
void hostemu_nm_plan(const long* sh, const long* call, const int* o, long* out) {
    const NmPlan p = nm_plan(nm_shape_of(sh), NmCall{call[0], call[1] != 0, call[2] != 0, call[3] != 0, call[4] != 0}, nm_options_of(o));
    const long v[] = {p.error, p.dense, p.dense_whole, p.use_codes, p.use_mfma, p.flag_from_list, p.k16, p.wave_step, p.bound_ok, p.sub_pass, p.one_launch, p.step_lmax, p.step_cmax, p.step_cpl,
                      p.num_one, p.direct16, p.KS, p.tpc, p.nparts, p.nsub, p.cat_fast};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}

// The launch form of one chunk of the int8 Gram (csrc/gram_route.h gram_i8_plan).  data: S, KB, NT, npg, zs_ind; opts in the order of GramI8Options; call: nb, explicit_idx,
// own_counts, want16, cu_count, experiments.  out: form, waves, variant, dma_buffer, rt_tall, rt_short, nty_tall, nty_short, nty, ntx, MT, per_xcd, grid, block, pp_wgs, sk_grid,
// hist, hist_bytes, hist_windows, hist_threads, cd_bytes, to16, then whether the private-count kernel takes the data set and the round units of the sub-batch plan
void hostemu_gram_i8_plan(const int* data, const int* o, const long* call, long* out) {
    const GramI8Data d{data[0], data[1], data[2], data[3], data[4] != 0};
    const GramI8Options opt{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10]};
    const GramI8Call c{call[0], call[1] != 0, call[2] != 0, call[3] != 0, (int)call[4], call[5] != 0};
    const GramI8Plan p = gram_i8_plan(d, opt, c);
    const long v[] = {p.form, p.waves, p.variant, p.dma_buffer, p.rt_tall, p.rt_short, p.nty_tall, p.nty_short, p.nty, p.ntx, p.MT, p.per_xcd, p.grid, p.block, p.pp_wgs, p.sk_grid,
                      p.hist, (long)p.hist_bytes, (long)p.hist_windows, (long)p.hist_threads, (long)p.cd_bytes, p.to16,
                      gram_i8_priv_takes(d, opt, c.experiments), (long)gram_i8_round_units(d, opt, c.cu_count, c.experiments)};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}

// The plan of one call of the batch driver (csrc/batch_route.h batch_plan).  sh: N, P, Pg, T, L, R, n_ind, then the flags nonmetric, has_stage1, has_stage2, micom_on,
// plain_metric, then kmax, n_chol, n_eff, nedge of the RouteShape (boff beside it); nm1 / nm2: the NmShape of the handle and of its second stage as hostemu_nm_plan takes
// them; o: gram_path, i8_min_batch, i8_slices, nm_counts8, resample_aux, i8_shape, i8_sched, solver_wave, solver_quad, solver_rows, boot_pass, aux_stream; onm1 / onm2 in the
// order of NmOptions; call: B, own_counts, pairs, stratified, explicit_idx, moments, rows_out.  out: gpath, plane_floor, lds_hist, counts8_plan, want_dcnt, route, rows_solver,
// nm_wave, dense, need_lists, need_ghist, cat_one, want16, micom, raises, ent_stride, dcnt_stride, psize, gk16_stride, micom_stride, kpad, then the bytes per problem ent, gram_budget,
// gram, ghist, dcnt, counts, verify, nent, gk16, then per_rep, budget, chunk, passes, then the int8 route's predicates: closed at the handle's plane count, open for a call
// that brings its counts, nm_counts8_possible, sub-batches allowed
void hostemu_batch_plan(const long* sh, const int* boff, const long* nm1, const long* nm2, const int* o, const int* onm1, const int* onm2, const long* call, long* out) {
    const BatchIn in = batch_in_of(sh, boff, nm1, nm2, o, onm1, onm2, call);
    const BatchPlan p = batch_plan(in.s, in.o, in.c);
    const long v[] = {p.gpath, p.plane_floor, p.lds_hist, p.counts8_plan, p.want_dcnt, p.route, p.rows_solver, p.nm_wave, p.dense, p.need_lists, p.need_ghist, p.cat_one, p.want16, p.micom, p.raises,
                      p.ent_stride, p.dcnt_stride, p.psize, p.gk16_stride, p.micom_stride, (long)p.kpad, (long)p.ent_bytes, (long)p.gram_budget_bytes, (long)p.gram_bytes, (long)p.ghist_bytes,
                      (long)p.dcnt_bytes, (long)p.counts_bytes, (long)p.verify_bytes, (long)p.nent_bytes, (long)p.gk16_bytes, (long)p.per_rep, (long)p.budget, (long)p.chunk, (long)p.passes,
                      gram_i8_closed(in.s, in.o, in.o.i8_slices), gram_counts_route_open(in.s, in.o), nm_counts8_possible(in.s, in.o), batch_sub_batches_ok(in.s.nonmetric, p.raises)};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}

// What a pass of `nb` problems revises of that plan (batch_chunk): the same inputs, then nb, fell_back, wrote16.  out: f64_gram, counts8, build_lists, lists, dense_solver,
// route, solve, then the NmCall of the pass and of a HOC pair's second stage (nproblems, counts8, lists_dcnt, counts16_ready, finish each)
void hostemu_batch_chunk(const long* sh, const int* boff, const long* nm1, const long* nm2, const int* o, const int* onm1, const int* onm2, const long* call, const long* pass, long* out) {
    const BatchIn in = batch_in_of(sh, boff, nm1, nm2, o, onm1, onm2, call);
    const BatchChunk k = batch_chunk(batch_plan(in.s, in.o, in.c), pass[0], pass[1] != 0, pass[2] != 0);
    const long v[] = {k.f64_gram, k.counts8, k.build_lists, k.lists, k.dense_solver, k.route, k.solve, k.call.nproblems, k.call.counts8, k.call.lists_dcnt, k.call.counts16_ready, k.call.finish,
                      k.call2.nproblems, k.call2.counts8, k.call2.lists_dcnt, k.call2.counts16_ready, k.call2.finish};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}

// The plan of one call of the group driver (csrc/group_route.h group_plan).  in: B, nranks, RS, then the options chunks, ratio, align, then units (the alignment the ranks
// agreed on) and nothing_to_hide.  out: K, cap, send_bytes, recv_bytes, group_consults_units, kBootChunksMax, then first, B, cap, off of each of the K sub-batches, then for every
// (k, rank), k-major: group_segment's rec0, first, count, group_shard's first and whether the shard is full -- 6 + 4 K + 5 K nranks values (at most 6 + 32 + 40 nranks)
void hostemu_group_plan(const long* in, long* out) {
    const GroupOptions o{(int)in[3], (int)in[4], (int)in[5]};
    const GroupPlan p = group_plan(in[0], (int)in[1], (int)in[2], o, in[6], in[7] != 0);
    long* v = out;
    *v++ = p.K; *v++ = p.cap; *v++ = (long)p.send_bytes; *v++ = (long)p.recv_bytes; *v++ = group_consults_units(o, in[7] != 0); *v++ = kBootChunksMax;
    for (int k = 0; k < p.K; ++k) { *v++ = p.sub[k].first; *v++ = p.sub[k].B; *v++ = p.sub[k].cap; *v++ = p.sub[k].off; }
    for (int k = 0; k < p.K; ++k)
        for (int r = 0; r < p.nranks; ++r) {
            const GroupSegment sg = group_segment(p, k, r);
            const GroupShard sh = group_shard(p, k, r);
            *v++ = sg.rec0; *v++ = sg.first; *v++ = sg.count; *v++ = sh.first; *v++ = group_shard_full(p, k, sh.count);
        }
}

// The plan of one single fit (csrc/fit_route.h fit_plan).  sh: N, P, Po, L, n_eff, PA, T, kmax, n_chol, nedge, categorical; call: want_scores, want_cov, then the options
// fit_chunks, scores_tile.  out: the offsets o_w, o_ld, o_cl, o_pc, o_r2, o_lc, o_row, o_ind, o_sw, o_sc, o_mean, o_cov, o_end, then h_total, h_direct, tail_bytes, fit_bytes,
// block_bytes, nchunks, the scores launch tile_rows, cls, lds, ntl, per_cu, grid, then score_bytes, stage_scores, stage_need, then the solver's placement (solver_route.h
// solver_lds) s_in_lds, small_in_lds, lds as the plan has it for one problem and the same three for a batch, then the tail's named ints: iterations, status, signs
void hostemu_fit_plan(const long* sh, const long* call, long* out) {
    const FitShape s{sh[0], (int)sh[1], (int)sh[2], (int)sh[3], (int)sh[4], (int)sh[5], (int)sh[6], (int)sh[7], (int)sh[8], (int)sh[9], sh[10] != 0};
    const FitPlan p = fit_plan(s, FitCall{call[0] != 0, call[1] != 0}, FitOptions{(int)call[2], (int)call[3]});
    const SolverLds b = solver_lds(RouteShape{s.P, s.L, s.kmax, s.n_chol, s.n_eff, s.nedge, nullptr}, 2);
    const long v[] = {p.o_w, p.o_ld, p.o_cl, p.o_pc, p.o_r2, p.o_lc, p.o_row, p.o_ind, p.o_sw, p.o_sc, p.o_mean, p.o_cov, p.o_end, p.h_total, p.h_direct, (long)p.tail_bytes, (long)p.fit_bytes,
                      (long)p.block_bytes, p.nchunks, p.scores.tile_rows, p.scores.cls, (long)p.scores.lds, p.scores.ntl, p.scores.per_cu, p.scores.grid, (long)p.score_bytes, p.stage_scores,
                      (long)p.stage_need, p.solver.s_in_lds, p.solver.small_in_lds, (long)p.solver.lds, b.s_in_lds, b.small_in_lds, (long)b.lds, FIT_INT_ITERS, FIT_INT_STATUS, FIT_INT_SIGN};
    for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) out[i] = v[i];
}

// The plan of the derived records (csrc/derived_route.h derived_plan).  sh: P, L, kmax, R, n_dir, n_spec; enabled: the switches, bit s = stage s in launch order
// (assessment, structural, PLSc, model fit, geodesic); nb problems.  out: runs, nslots, side_bytes, refused, then per stage stride, waves, wave_doubles, lds, grid
// (zeros for a stage that does not run).  target >= 0: behind them derived_fit_layout of that stage -- runs, o_stage per stage, o_side, o_ints, bytes.
void hostemu_derived_plan(const long* sh, long enabled, long nb, long target, long* out) {
    const DerivedShape s{(int)sh[0], (int)sh[1], (int)sh[2], (int)sh[3], (int)sh[4], (int)sh[5]};
    const DerivedPlan p = derived_plan(s, (int)enabled, nb);
    long* v = out;
    *v++ = p.runs; *v++ = p.nslots; *v++ = (long)p.side_bytes; *v++ = p.refused;
    for (const DerivedLaunch& k : p.stage) { *v++ = k.stride; *v++ = k.waves; *v++ = k.wave_doubles; *v++ = (long)k.lds; *v++ = k.grid; }
    if (target < 0) return;
    const DerivedFitLayout f = derived_fit_layout(s, (int)target);
    *v++ = f.plan.runs;
    for (long o : f.o_stage) *v++ = o;
    *v++ = f.o_side; *v++ = f.o_ints; *v++ = (long)f.bytes;
}
// a row of the stage table: what it reads (bits), waves, min_waves, plain_only; word 0 .. 4: api, noun, last, title, lds_need ("" for none)
void hostemu_derived_stage(int s, long* out) {
    const DerivedStageRow& r = kDerivedStage[s];
    out[0] = r.reads; out[1] = r.waves; out[2] = r.min_waves; out[3] = r.plain_only;
}
const char* hostemu_derived_word(int s, int which) { const DerivedStageRow& r = kDerivedStage[s]; const char* w[] = {r.api, r.noun, r.last, r.title, r.lds_need}; return w[which] ? w[which] : ""; }

// The option table (csrc/options.h) over a bare Tune of default options.  set: `name` = `value` on a Tune that holds `start` in that option (-1 << 31: its default) and
// defaults elsewhere; out: option_set's result (0 ok, 1 out of range, 2 experiments only, 3 unknown name), the effect bits it reported (1 planes, 2 statistics), how many
// fields of the Tune differ from before the call, what option_get reads afterwards.  get: 1 and the default of `name`, or 0 for a name the table does not have.
void hostemu_option_set(const char* name, int start, int value, int experiments, int* out) {
    Tune t;
    if (start != INT32_MIN && option_set(t, name, start, true, nullptr) != OPTION_OK) { out[0] = -1; return; }
    const Tune before = t;
    OptionEffect effect = OPTION_VOIDS_PLANES_AND_STATS;
    out[0] = option_set(t, name, value, experiments != 0, &effect);
    out[1] = (int)effect;
    out[2] = 0;
    static_assert(sizeof(Tune) % sizeof(int) == 0, "Tune holds ints only");
    for (size_t i = 0; i < sizeof(Tune) / sizeof(int); ++i) out[2] += ((const int*)&t)[i] != ((const int*)&before)[i];
    out[3] = INT32_MIN;
    option_get(t, name, &out[3]);
}
int hostemu_option_get(const char* name, int* value) { const Tune t; return option_get(t, name, value); }
int hostemu_option_count() { return (int)(sizeof(kOptions) / sizeof(kOptions[0])); }
const char* hostemu_option_name(int i) { return kOptions[i].name; }

long hostemu_packed_index(int T, int p, int q) { return packed_index(T, p, q); }
long hostemu_packed_size(int T) { return packed_size(T); }
}
