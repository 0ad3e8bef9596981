// fimix_route.h -- the plan of one plspm_fimix_device call (plspm_fimix.hip): the record width, the threads of a workgroup, a thread's accumulators and the
// sweeps per iteration they make of a model's moment entries, the regression slots, the LDS of one problem and the refusal when it does not fit.  Pure functions
// of the model's shape, N and the call's kmax.  Free of the HIP runtime: tests/fimix_host compiles it.
#pragma once
#include "fimix_core.h"

namespace plspm {

constexpr long kFimixMaxLds = 160 * 1024;      // a workgroup's LDS (solver_route.h kMaxLds)
// A thread's moment accumulators: KP segments x 32 / KP entries.  With its posteriors, residuals and n_k (4 KP doubles at KP = 16) that is 96 doubles, 192 registers
// and what the E-step's exp / log keep in flight: inside the 512 registers of a thread of a 256-thread workgroup.  A 512-thread workgroup (256 registers a thread)
// holds 16 without scratch and sweeps twice as often: measured slower at N = 1,000 and at N = 10,000, so every N gets 256 threads; 1,024 threads
// would leave 128 registers, less than KP = 8 needs.
constexpr int kFimixThreads = 256;
constexpr int kFimixAcc = 32;
constexpr int kFimixSlotsMax = 64;             // regressions in flight: one wave's lanes

// n_dir direct paths, n_endo LVs with predecessors, at most kmax_pred of them for one LV, E moment entries (fimix_core.h fimix_entries)
struct FimixShape { long N; int L, n_dir, n_endo, kmax_pred, E; };
struct FimixPlan {
    int width;          // of a record; status and iterations behind it
    int threads, waves;
    int acc;            // a thread's accumulators
    int nslots;         // regressions in flight
    long lds_bytes;
    bool fits;          // one problem's state fits the LDS (with one slot at least)
};

inline int fimix_threads(long) { return kFimixThreads; }      // (from N: the measurement found no N at which another size wins)
// entries per sweep and sweeps per iteration of a problem of K segments
inline int fimix_chunk_entries(int K) { return kFimixAcc / fimix_kpad(K); }
inline int fimix_chunks(int K, int E) { const int ce = fimix_chunk_entries(K); return (E + ce - 1) / ce; }
inline long fimix_lds_bytes(const FimixShape& s, int kmax, int waves, int nslots) {
    return (long)sizeof(double) * fimix_ws_doubles(s.L, s.n_dir, s.n_endo, s.kmax_pred, kmax, waves, kFimixAcc, nslots);
}

inline FimixPlan fimix_plan(const FimixShape& s, int kmax) {
    FimixPlan p{};
    p.width = fimix_record_width(kmax, s.n_dir, s.n_endo);
    p.threads = fimix_threads(s.N); p.waves = p.threads / 64;
    p.acc = kFimixAcc;
    const int ntask = kmax * s.n_endo;
    p.nslots = ntask < kFimixSlotsMax ? (ntask < 1 ? 1 : ntask) : kFimixSlotsMax;
    while (p.nslots > 1 && fimix_lds_bytes(s, kmax, p.waves, p.nslots) > kFimixMaxLds) p.nslots = (p.nslots + 1) / 2;
    p.lds_bytes = fimix_lds_bytes(s, kmax, p.waves, p.nslots);
    p.fits = p.lds_bytes <= kFimixMaxLds;
    return p;
}

}  // namespace plspm
