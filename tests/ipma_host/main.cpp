// TEST INFRASTRUCTURE: csrc/ipma_core.h on the host.  Built with -fsanitize=address,undefined (Makefile); every array is a heap block of exactly its size, so
// that an index past an end is reported.  Two commands:
//
//   ipma_host record [INPUT]        ipma_check_bounds + ipma_build + ipma_record on one data set read from a text file (or from standard input), on the serial
//                                   executor.  Input, whitespace separated:  L  n_eff  |  boff [L + 1]  |  eff_from [n_eff]  eff_to [n_eff]  |  has_mask  mask [L]
//                                   (if has_mask)  |  lo [P]  hi [P]  |  the bootstrap record [2 P + L + 2 n_eff]  |  n  |  X [n x P], row-major, device column
//                                   order.  The moment matrix is built here as the device holds it: of the columns shifted by their means, row / column P the
//                                   column sums, (P, P) = n.  Prints n_t and the targets, W, the W values one per line, then status and iterations.
//   ipma_host plan L N_EFF N_T P... ipma_plan of (P, L, n_eff, n_t) on 1,000 problems for every P: "P waves wave_doubles lds grid refused stride" per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ipma_core.h"

using namespace plspm;

struct HostMoments {
    const double* M; int ld;
    double operator()(int p, int q) const { return M[(size_t)p * ld + q]; }
};

static int run_plan(int argc, char** argv) {
    const int L = atoi(argv[2]), ne = atoi(argv[3]), nt = atoi(argv[4]);
    for (int i = 5; i < argc; ++i) {
        const int P = atoi(argv[i]);
        const IpmaShape s{P, L, ne, nt};
        const IpmaPlan pl = ipma_plan(s, 1000);
        printf("%d %d %ld %zu %ld %d %ld\n", P, pl.waves, pl.wave_doubles, pl.lds, pl.grid, pl.refused ? 1 : 0, pl.stride);
    }
    return 0;
}

template <class T> static bool read_all(FILE* f, std::vector<T>& v, const char* fmt) {
    for (auto& x : v) if (fscanf(f, fmt, &x) != 1) { fprintf(stderr, "short input\n"); return false; }
    return true;
}

static int run_record(FILE* f) {
    int L, ne;
    if (fscanf(f, "%d %d", &L, &ne) != 2 || L < 1 || L > 4096 || ne < 0 || ne > L * L) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int> boff((size_t)L + 1), eff_from((size_t)ne), eff_to((size_t)ne);
    if (!read_all(f, boff, "%d") || !read_all(f, eff_from, "%d") || !read_all(f, eff_to, "%d")) return 2;
    int has_mask;
    if (fscanf(f, "%d", &has_mask) != 1) { fprintf(stderr, "short input\n"); return 2; }
    std::vector<unsigned char> mask;
    if (has_mask) {
        mask.resize((size_t)L);
        for (auto& v : mask) { int x; if (fscanf(f, "%d", &x) != 1) { fprintf(stderr, "short input\n"); return 2; } v = (unsigned char)x; }
    }
    const int P = boff[L];
    if (P < 1) { fprintf(stderr, "bad shape\n"); return 2; }
    std::vector<double> lo((size_t)P), hi((size_t)P), rec((size_t)2 * P + L + 2 * ne);
    if (!read_all(f, lo, "%lf") || !read_all(f, hi, "%lf") || !read_all(f, rec, "%lf")) return 2;
    long n;
    if (fscanf(f, "%ld", &n) != 1 || n < 2) { fprintf(stderr, "bad shape\n"); return 2; }
    std::vector<double> X((size_t)n * P);
    if (!read_all(f, X, "%lf")) return 2;

    std::string why;
    if (ipma_check_bounds(P, lo.data(), hi.data(), why)) { printf("refused arg %s\n", why.c_str()); return 3; }
    IpmaBuild ib;
    if (ipma_build(L, boff.data(), ne, eff_from.data(), eff_to.data(), has_mask ? mask.data() : nullptr, ib, why)) { printf("refused arg %s\n", why.c_str()); return 3; }
    const IpmaShape shape{P, L, ne, ib.n_t};
    const IpmaPlan pl = ipma_plan(shape, 1);
    if (pl.refused) { printf("refused limit %s\n", ipma_refusal()); return 3; }

    // the moments of the mean-shifted columns, full symmetric [(P + 1) x (P + 1)]
    const int ld = P + 1;
    std::vector<double> shift((size_t)P, 0.0), M((size_t)ld * ld, 0.0);
    for (int p = 0; p < P; ++p) { double s = 0.0; for (long i = 0; i < n; ++i) s += X[(size_t)i * P + p]; shift[p] = s / (double)n; }
    for (long i = 0; i < n; ++i)
        for (int p = 0; p <= P; ++p) {
            const double xp = p < P ? X[(size_t)i * P + p] - shift[p] : 1.0;
            for (int q = 0; q <= P; ++q) M[(size_t)p * ld + q] += xp * (q < P ? X[(size_t)i * P + q] - shift[q] : 1.0);
        }

    const long W = ipma_width(shape);
    std::vector<double> slice((size_t)pl.wave_doubles), out((size_t)W + 2, -777.0);
    IpmaDescs d{P, L, ne, ib.n_t, boff.data(), ib.lvof.data(), ib.targets.data(), ib.eff_of.data(), eff_from.data(), eff_to.data(), shift.data(), lo.data(), hi.data()};
    IpmaSerialExec ex;
    ipma_record(ex, d, HostMoments{M.data(), ld}, rec.data(), slice.data(), 7.0, out.data());
    printf("%d", ib.n_t);
    for (int t : ib.targets) printf(" %d", t);
    printf("\n%ld\n", W);
    for (long k = 0; k < W + 2; ++k) printf("%.17g\n", out[(size_t)k]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 6 && !strcmp(argv[1], "plan")) return run_plan(argc, argv);
    if ((argc == 2 || argc == 3) && !strcmp(argv[1], "record")) {
        FILE* f = argc == 3 ? fopen(argv[2], "r") : stdin;
        if (!f) { perror(argv[2]); return 2; }
        const int rc = run_record(f);
        if (f != stdin) fclose(f);
        return rc;
    }
    fprintf(stderr, "usage: ipma_host record [INPUT] | ipma_host plan L N_EFF N_T P...\n");
    return 2;
}
