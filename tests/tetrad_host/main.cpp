// TEST INFRASTRUCTURE: csrc/tetrad_core.h on the host.  Built with -fsanitize=address,undefined (Makefile); every array is a heap block of exactly its size, so
// that an index past an end is reported.  Two commands:
//
//   tetrad_host record [INPUT]   tetrad_build + tetrad_record on one data set read from a text file (or from standard input), on the serial executor.  Input,
//                                whitespace separated:  L  set  matrix  |  boff [L + 1]  |  has_mask  mask [L] (if has_mask)  |  n  |  X [n x P], row-major, device
//                                column order.  The moment matrix is built here as the device holds it: of the columns shifted by their means, row / column P the
//                                column sums, (P, P) = n.  Prints n_tet, then per tetrad "block a b c d value", then status and iterations.
//   tetrad_host plan P T_TRI...  tetrad_plan of (P, T_tri, 0 tetrads) on 1,000 problems for every T_TRI: "T_tri waves wave_doubles lds grid refused" per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "tetrad_core.h"

using namespace plspm;

struct HostMoments {
    const double* M; int ld;
    double operator()(int p, int q) const { return M[(size_t)p * ld + q]; }
};

static int run_plan(int argc, char** argv) {
    const int P = atoi(argv[2]);
    for (int i = 3; i < argc; ++i) {
        const long T = atol(argv[i]);
        const TetradPlan pl = tetrad_plan(TetradShape{P, T, 0}, 1000);
        printf("%ld %d %ld %zu %ld %d\n", T, pl.waves, pl.wave_doubles, pl.lds, pl.grid, pl.refused ? 1 : 0);
    }
    return 0;
}

static int run_record(FILE* f) {
    int L, set, matrix;
    if (fscanf(f, "%d %d %d", &L, &set, &matrix) != 3 || L < 1 || L > 4096) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int> boff((size_t)L + 1);
    for (auto& v : boff) if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "short input\n"); return 2; }
    int has_mask;
    if (fscanf(f, "%d", &has_mask) != 1) { fprintf(stderr, "short input\n"); return 2; }
    std::vector<unsigned char> mask;
    if (has_mask) {
        mask.resize((size_t)L);
        for (auto& v : mask) { int x; if (fscanf(f, "%d", &x) != 1) { fprintf(stderr, "short input\n"); return 2; } v = (unsigned char)x; }
    }
    const int P = boff[L];
    long n;
    if (fscanf(f, "%ld", &n) != 1 || n < 2 || P < 1) { fprintf(stderr, "bad shape\n"); return 2; }
    std::vector<double> X((size_t)n * P);
    for (auto& v : X) if (fscanf(f, "%lf", &v) != 1) { fprintf(stderr, "short input\n"); return 2; }

    TetradBuild tb;
    std::string why;
    bool limit = false;
    if (tetrad_build(L, boff.data(), has_mask ? mask.data() : nullptr, set, tb, why, &limit)) { printf("refused %s %s\n", limit ? "limit" : "arg", why.c_str()); return 3; }
    const TetradPlan pl = tetrad_plan(TetradShape{P, tb.T_tri, tb.n_tet}, 1);
    if (pl.refused) { printf("refused limit %s\n", tetrad_refusal()); return 3; }

    // the moments of the mean-shifted columns, full symmetric [(P + 1) x (P + 1)]
    const int ld = P + 1;
    std::vector<double> shift((size_t)P, 0.0), M((size_t)ld * ld, 0.0);
    for (int p = 0; p < P; ++p) { double s = 0.0; for (long i = 0; i < n; ++i) s += X[(size_t)i * P + p]; shift[p] = s / (double)n; }
    for (long i = 0; i < n; ++i)
        for (int p = 0; p <= P; ++p) {
            const double xp = p < P ? X[(size_t)i * P + p] - shift[p] : 1.0;
            for (int q = 0; q <= P; ++q) M[(size_t)p * ld + q] += xp * (q < P ? X[(size_t)i * P + q] - shift[q] : 1.0);
        }

    std::vector<double> slice((size_t)pl.wave_doubles), out((size_t)tb.n_tet + 2, -777.0);
    TetradDescs td{L, tb.n_tet, matrix, boff.data(), tb.tri_off.data(), tb.desc.data()};
    TetradSerialExec ex;
    tetrad_record(ex, td, HostMoments{M.data(), ld}, P, slice.data(), 7.0, out.data());
    printf("%d\n", tb.n_tet);
    for (int t = 0; t < tb.n_tet; ++t)
        printf("%d %d %d %d %d %.17g\n", tb.block[t], tb.items[4 * (size_t)t], tb.items[4 * (size_t)t + 1], tb.items[4 * (size_t)t + 2], tb.items[4 * (size_t)t + 3], out[t]);
    printf("%.17g\n%.17g\n", out[tb.n_tet], out[tb.n_tet + 1]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !strcmp(argv[1], "plan")) return run_plan(argc, argv);
    if ((argc == 2 || argc == 3) && !strcmp(argv[1], "record")) {
        FILE* f = argc == 3 ? fopen(argv[2], "r") : stdin;
        if (!f) { perror(argv[2]); return 2; }
        const int rc = run_record(f);
        if (f != stdin) fclose(f);
        return rc;
    }
    fprintf(stderr, "usage: tetrad_host record [INPUT] | tetrad_host plan P T_TRI...\n");
    return 2;
}
