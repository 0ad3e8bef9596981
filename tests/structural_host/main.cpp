// TEST INFRASTRUCTURE: csrc/structural_core.h structural_record on one problem read from a text file (or from standard input), on the serial host executor; prints
// the structural record (values, status, iterations), one number per line.  Built with -fsanitize=address,undefined (Makefile); every array is a heap block of
// exactly its size, so that an index past an end is reported.
//
// Input, whitespace separated:  L  |  C [L x L] (C[i][j] = 1 iff LV j -> LV i, strictly lower triangular)  |  lv_cor [npairs]  |  direct [n_eff] (the record's
// direct entries, in effect-pair order)  |  n_spec  |  per chain: its length and its LVs
// The chains come from the caller (the mirror's enumeration); the effect pairs and the direct paths are built here as the library builds them.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "structural_core.h"

using namespace plspm;

template <class T> static bool read_all(FILE* f, std::vector<T>& v, const char* fmt) {
    for (auto& x : v) if (fscanf(f, fmt, &x) != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc > 2) { fprintf(stderr, "usage: structural_host [INPUT]\n"); return 2; }
    FILE* f = argc == 2 ? fopen(argv[1], "r") : stdin;
    if (!f) { perror(argv[1]); return 2; }
    int L;
    if (fscanf(f, "%d", &L) != 1 || L < 2 || L > 1024) { fprintf(stderr, "bad header\n"); return 2; }
    const int npairs = L * (L - 1) / 2;
    std::vector<int> C((size_t)L * L);
    std::vector<double> lv_cor(npairs);
    if (!read_all(f, C, "%d") || !read_all(f, lv_cor, "%lf")) { fprintf(stderr, "short input\n"); return 2; }
    for (int i = 0; i < L; ++i) for (int j = i; j < L; ++j) if (C[i * L + j]) { fprintf(stderr, "the path matrix must be strictly lower triangular\n"); return 2; }
    // the descriptors as the library builds them (plspm_model_create): predecessors in CSR form, effect pairs from the transitive closure, from-major
    std::vector<int> pred_off(L + 1, 0), pred_idx, eff_from, eff_to;
    int kmax = 0;
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < L; ++j) if (C[i * L + j]) pred_idx.push_back(j);
        pred_off[i + 1] = (int)pred_idx.size();
        kmax = std::max(kmax, pred_off[i + 1] - pred_off[i]);
    }
    std::vector<int> reach(C), eff_of((size_t)L * L, -1);
    for (int k = 0; k < L; ++k) for (int i = 0; i < L; ++i) for (int j = 0; j < L; ++j) if (reach[i * L + k] && reach[k * L + j]) reach[i * L + j] = 1;
    for (int fr = 0; fr < L; ++fr) for (int t = 0; t < L; ++t) if (fr != t && reach[t * L + fr]) { eff_of[t * L + fr] = (int)eff_from.size(); eff_from.push_back(fr); eff_to.push_back(t); }
    const int n_eff = (int)eff_from.size();
    std::vector<int> dir_from, dir_to;
    for (int e = 0; e < n_eff; ++e) if (C[eff_to[e] * L + eff_from[e]]) { dir_from.push_back(eff_from[e]); dir_to.push_back(eff_to[e]); }
    std::vector<double> direct(n_eff);
    int n_spec;
    if (!read_all(f, direct, "%lf") || fscanf(f, "%d", &n_spec) != 1 || n_spec < 0) { fprintf(stderr, "short input\n"); return 2; }
    std::vector<int> chain_off(1, 0), chain_eff;
    for (int s = 0; s < n_spec; ++s) {
        int len;
        if (fscanf(f, "%d", &len) != 1 || len < 3 || len > L) { fprintf(stderr, "bad chain\n"); return 2; }
        std::vector<int> nodes(len);
        if (!read_all(f, nodes, "%d")) { fprintf(stderr, "short input\n"); return 2; }
        for (int r = 0; r < len; ++r) {
            if (nodes[r] < 0 || nodes[r] >= L || (r + 1 < len && (nodes[r + 1] < 0 || nodes[r + 1] >= L || !C[nodes[r + 1] * L + nodes[r]]))) { fprintf(stderr, "bad chain\n"); return 2; }
            chain_eff.push_back(r + 1 < len ? eff_of[nodes[r + 1] * L + nodes[r]] : 0);
        }
        chain_off.push_back((int)chain_eff.size());
    }
    if (f != stdin) fclose(f);
    // the bootstrap record of a model of L single-item blocks: weights [L] | r2 [L] | total [n_eff] | direct [n_eff] | loadings [L] | status | iterations; only the
    // direct entries, the status and the iterations are read
    const int P = L, R = 2 * P + L + 2 * n_eff;
    std::vector<double> rec((size_t)R + 2, -555.0);
    std::copy(direct.begin(), direct.end(), rec.begin() + P + L + n_eff);
    rec[R] = 0.0; rec[R + 1] = 7.0;
    ModelDesc md{};
    md.P = P; md.L = L; md.kmax = kmax; md.n_eff = n_eff;
    md.pred_off = pred_off.data(); md.pred_idx = pred_idx.data(); md.eff_from = eff_from.data(); md.eff_to = eff_to.data(); md.n_edges = (int)pred_idx.size();
    const int n_dir = (int)dir_from.size(), S = 2 * n_dir + n_spec;
    StructDesc sd{n_dir, n_spec, dir_from.data(), dir_to.data(), chain_off.data(), chain_eff.data()};
    std::vector<double> lds((size_t)structural_ws_doubles(L, kmax, 1)), out((size_t)S + 2, -777.0);
    StructWs w;
    structural_carve(w, lds.data(), L);
    StructSerialExec ex;
    structural_record(ex, md, sd, w, 1, lv_cor.data(), rec.data(), R, out.data());
    for (double x : out) printf("%.17g\n", x);
    return 0;
}
