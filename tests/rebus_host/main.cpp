// TEST INFRASTRUCTURE: csrc/rebus_core.h and csrc/rebus_route.h on the host.  Built with -fsanitize=address,undefined (Makefile); every array is a heap block of
// exactly its size, so that an index past an end is reported.  Two commands:
//
//   rebus_host step [INPUT]         one pass of REBUS-PLS on given local records, read from a text file (or from standard input), on the serial executor:
//                                   rebus_compose per class, rebus_row per (row, class), rebus_cm, rebus_argmin.  Input, whitespace separated:
//                                   L  n_eff  scaled  K  N  |  boff [L + 1]  |  eff_from [n_eff]  eff_to [n_eff]  |  path [L x L] (row = target)  |
//                                   K x (status, record [2 P + L + 2 n_eff])  |  labels [N]  |  X [N x P], row-major, device column order.
//                                   The rows are shifted by their column means first, as the device holds them.  Prints the K flags on one line, then per row
//                                   "label cm_0 .. cm_{K-1}".
//   rebus_host plan P L N_ENDO K N CAP...   rebus_plan for every cap: "param_doubles xs classes_per_load loads rows tiles assign_grid slices slice_rows lds refused".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rebus_route.h"

using namespace plspm;

template <class T> static bool read_all(FILE* f, std::vector<T>& v, const char* fmt) {
    for (auto& x : v) if (fscanf(f, fmt, &x) != 1) { fprintf(stderr, "short input\n"); return false; }
    return true;
}

static int run_plan(int argc, char** argv) {
    const RebusShape s{atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atol(argv[6])};
    for (int i = 7; i < argc; ++i) {
        const RebusPlan p = rebus_plan(s, atoi(argv[i]));
        printf("%d %d %d %d %d %ld %ld %d %ld %ld %d\n", p.param_doubles, p.xs, p.classes_per_load, p.loads, p.rows, p.tiles, p.assign_grid, p.slices, p.slice_rows, p.lds_bytes,
               p.refused ? 1 : 0);
    }
    return 0;
}

static int run_step(FILE* f) {
    int L, ne_eff, scaled, K;
    long N;
    if (fscanf(f, "%d %d %d %d %ld", &L, &ne_eff, &scaled, &K, &N) != 5 || L < 1 || L > 4096 || ne_eff < 0 || K < 1 || K > kRebusMaxClasses || N < 1) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int> boff((size_t)L + 1), eff_from((size_t)ne_eff), eff_to((size_t)ne_eff), path((size_t)L * L);
    if (!read_all(f, boff, "%d") || !read_all(f, eff_from, "%d") || !read_all(f, eff_to, "%d") || !read_all(f, path, "%d")) return 2;
    const int P = boff[(size_t)L];
    if (P < 1) { fprintf(stderr, "bad shape\n"); return 2; }
    const int R = 2 * P + L + 2 * ne_eff;
    std::vector<int> status((size_t)K);
    std::vector<std::vector<double>> rec((size_t)K, std::vector<double>((size_t)R));
    for (int k = 0; k < K; ++k)
        if (fscanf(f, "%d", &status[(size_t)k]) != 1 || !read_all(f, rec[(size_t)k], "%lf")) return 2;
    std::vector<int> label((size_t)N);
    std::vector<double> X((size_t)N * P);
    if (!read_all(f, label, "%d") || !read_all(f, X, "%lf")) return 2;

    std::vector<int> lvof((size_t)P), endo;
    for (int l = 0; l < L; ++l) {
        for (int p = boff[(size_t)l]; p < boff[(size_t)l + 1]; ++p) lvof[(size_t)p] = l;
        bool has = false;
        for (int q = 0; q < L; ++q) has = has || path[(size_t)l * L + q] != 0;
        if (has) endo.push_back(l);
    }
    const int ne = (int)endo.size();
    std::vector<int> eff_of((size_t)ne * L, -1);
    for (int jj = 0; jj < ne; ++jj)
        for (int q = 0; q < L; ++q)
            if (path[(size_t)endo[(size_t)jj] * L + q])
                for (int x = 0; x < ne_eff; ++x) if (eff_from[(size_t)x] == q && eff_to[(size_t)x] == endo[(size_t)jj]) eff_of[(size_t)jj * L + q] = x;
    std::vector<double> shift((size_t)P, 0.0);
    for (int p = 0; p < P; ++p) { double s = 0.0; for (long i = 0; i < N; ++i) s += X[(size_t)i * P + p]; shift[(size_t)p] = s / (double)N; }
    for (long i = 0; i < N; ++i) for (int p = 0; p < P; ++p) X[(size_t)i * P + p] -= shift[(size_t)p];

    const RebusModel md{P, L, ne, ne_eff, scaled, boff.data(), lvof.data(), endo.data(), eff_of.data(), shift.data()};
    const int PD = rebus_param_doubles(P, L, ne);
    std::vector<std::vector<double>> par((size_t)K, std::vector<double>((size_t)PD));
    std::vector<int> flag((size_t)K);
    RebusSerialExec ex;
    for (int k = 0; k < K; ++k) {
        std::vector<double> S1((size_t)P, 0.0), S2((size_t)P, 0.0), work((size_t)2 * P + L);
        double n = 0.0;
        for (long i = 0; i < N; ++i)
            if (label[(size_t)i] == k) {
                n += 1.0;
                for (int p = 0; p < P; ++p) { const double x = X[(size_t)i * P + p]; S1[(size_t)p] += x; S2[(size_t)p] += x * x; }
            }
        flag[(size_t)k] = rebus_compose(ex, md, rec[(size_t)k].data(), status[(size_t)k], n, S1.data(), S2.data(), par[(size_t)k].data(), work.data());
    }
    std::vector<double> A((size_t)K * N), B((size_t)K * N), SA((size_t)K, 0.0), SB((size_t)K, 0.0), y((size_t)L), cm((size_t)K);
    for (int k = 0; k < K; ++k) {
        const RebusParamsT<const double> pr = rebus_params<const double>(par[(size_t)k].data(), P, L, ne);
        for (long i = 0; i < N; ++i) {
            const double* x = X.data() + (size_t)i * P;
            double a, b;
            rebus_row(P, L, ne, boff.data(), endo.data(), pr, [&](int p) { return x[p]; }, [&](int l) -> double& { return y[(size_t)l]; }, [](int, double) {}, a, b);
            A[(size_t)k * N + i] = a; B[(size_t)k * N + i] = b;
            SA[(size_t)k] += a; SB[(size_t)k] += b;
        }
    }
    for (int k = 0; k < K; ++k) printf("%d%c", flag[(size_t)k], k + 1 < K ? ' ' : '\n');
    for (long i = 0; i < N; ++i) {
        for (int k = 0; k < K; ++k) cm[(size_t)k] = rebus_cm(A[(size_t)k * N + i], B[(size_t)k * N + i], SA[(size_t)k], SB[(size_t)k], (double)N);
        printf("%d", rebus_argmin(cm.data(), 1, K, label[(size_t)i]));
        for (int k = 0; k < K; ++k) printf(" %.17g", cm[(size_t)k]);
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 8 && !strcmp(argv[1], "plan")) return run_plan(argc, argv);
    if ((argc == 2 || argc == 3) && !strcmp(argv[1], "step")) {
        FILE* f = argc == 3 ? fopen(argv[2], "r") : stdin;
        if (!f) { perror(argv[2]); return 2; }
        const int rc = run_step(f);
        if (f != stdin) fclose(f);
        return rc;
    }
    fprintf(stderr, "usage: rebus_host step [INPUT] | rebus_host plan P L N_ENDO K N CAP...\n");
    return 2;
}
