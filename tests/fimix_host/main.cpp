// TEST INFRASTRUCTURE: csrc/fimix_core.h fimix_problem on one problem read from a text file (or from standard input), on the serial host executor, and the plan of
// csrc/fimix_route.h for a table of shapes.  Built with -fsanitize=address,undefined (Makefile); every array is a heap block of exactly its size, so that an index
// past an end is reported.
//
//   fimix_host [INPUT]        input, whitespace separated:  N L K Kmax max_iter tol  |  C [L x L] (C[i][j] = 1 iff LV j -> LV i, strictly lower triangular)  |
//                             Y [N x L]  |  init [N] segments below K.
//                             Prints the record (values, status, iterations), one number per line.
//   fimix_host plan [INPUT]   lines of  N L n_dir n_endo kmax_pred E kmax ; prints per line  width threads acc nslots lds_bytes fits chunks , chunks being the sweeps
//                             per iteration of a problem of kmax segments.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fimix_route.h"

using namespace plspm;

template <class T> static bool read_all(FILE* f, std::vector<T>& v, const char* fmt) {
    for (auto& x : v) if (fscanf(f, fmt, &x) != 1) return false;
    return true;
}

static int plan_table(FILE* f) {
    long N;
    int L, n_dir, n_endo, kmax_pred, E, kmax;
    while (fscanf(f, "%ld %d %d %d %d %d %d", &N, &L, &n_dir, &n_endo, &kmax_pred, &E, &kmax) == 7) {
        if (N < 1 || L < 1 || kmax < 1 || kmax > kFimixMaxK) { fprintf(stderr, "bad shape\n"); return 2; }
        const FimixPlan p = fimix_plan(FimixShape{N, L, n_dir, n_endo, kmax_pred, E}, kmax);
        printf("%d %d %d %d %ld %d %d\n", p.width, p.threads, p.acc, p.nslots, p.lds_bytes, p.fits ? 1 : 0, fimix_chunks(kmax, E));
    }
    return 0;
}

int main(int argc, char** argv) {
    const bool plan = argc >= 2 && !strcmp(argv[1], "plan");
    const int file_arg = plan ? 2 : 1;
    if (argc > file_arg + 1) { fprintf(stderr, "usage: fimix_host [plan] [INPUT]\n"); return 2; }
    FILE* f = argc == file_arg + 1 ? fopen(argv[file_arg], "r") : stdin;
    if (!f) { perror(argv[file_arg]); return 2; }
    if (plan) return plan_table(f);
    long N;
    int L, K, Kmax, max_iter;
    double tol;
    if (fscanf(f, "%ld %d %d %d %d %lf", &N, &L, &K, &Kmax, &max_iter, &tol) != 6 || N < 1 || N > (1 << 24) || L < 2 || L > 1024 || K < 1 || K > Kmax || Kmax > kFimixMaxK ||
        max_iter < 1 || !(tol >= 0.0)) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<int> C((size_t)L * L), init_in((size_t)N);
    std::vector<double> Y((size_t)N * L);
    if (!read_all(f, C, "%d") || !read_all(f, Y, "%lf") || !read_all(f, init_in, "%d")) { fprintf(stderr, "short input\n"); return 2; }
    if (f != stdin) fclose(f);
    for (int i = 0; i < L; ++i) for (int j = i; j < L; ++j) if (C[i * L + j]) { fprintf(stderr, "the path matrix must be strictly lower triangular\n"); return 2; }
    std::vector<unsigned char> init((size_t)N);
    for (long i = 0; i < N; ++i) {
        if (init_in[i] < 0 || init_in[i] >= K) { fprintf(stderr, "bad initial segment\n"); return 2; }
        init[i] = (unsigned char)init_in[i];
    }
    // the tables as the library builds them (plspm_fimix.hip fimix_tables)
    std::vector<int> pred_off(L + 1, 0), pred_idx, endo;
    int kmax_pred = 0;
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < L; ++j) if (C[i * L + j]) pred_idx.push_back(j);
        pred_off[i + 1] = (int)pred_idx.size();
        if (pred_off[i + 1] > pred_off[i]) endo.push_back(i);
        kmax_pred = std::max(kmax_pred, pred_off[i + 1] - pred_off[i]);
    }
    const int n_dir = (int)pred_idx.size(), n_endo = (int)endo.size();
    if (!n_dir) { fprintf(stderr, "the model has no path\n"); return 2; }
    std::vector<int> dir_of(n_dir);
    int dpath = 0;
    for (int fr = 0; fr < L; ++fr)
        for (int to = 0; to < L; ++to)
            for (int e = pred_off[to]; e < pred_off[to + 1]; ++e) if (pred_idx[e] == fr) dir_of[e] = dpath++;
    const int E = fimix_entries(L, pred_off.data(), pred_idx.data(), nullptr);
    std::vector<int> ent(E);
    fimix_entries(L, pred_off.data(), pred_idx.data(), ent.data());
    const FimixDesc d{L, n_endo, n_dir, kmax_pred, E, pred_off.data(), pred_idx.data(), endo.data(), dir_of.data(), ent.data()};
    const int W = fimix_record_width(Kmax, n_dir, n_endo);
    std::vector<double> lds((size_t)fimix_ws_doubles(L, n_dir, n_endo, kmax_pred, Kmax, 1, kFimixAcc, 1)), rec((size_t)W + 2, -777.0);
    FimixWs w;
    fimix_carve(w, lds.data(), L, n_dir, n_endo, Kmax, 1, kFimixAcc, 1);
    FimixSerialExec ex;
    int status = -1, iters = -1;
    fimix_problem<kFimixAcc>(ex, d, w, Y.data(), N, K, Kmax, init.data(), 0, 0, max_iter, tol, rec.data(), &status, &iters);
    if ((double)status != rec[W] || (double)iters != rec[W + 1]) { fprintf(stderr, "status / iterations differ from the record's\n"); return 3; }
    for (double x : rec) printf("%.17g\n", x);
    return 0;
}
