// TEST INFRASTRUCTURE: csrc/geodesic_core.h (geodesic_record, behind modelfit_core.h modelfit_phi) on one problem read from a text file, on the serial host
// executor; prints the geodesic record (two values, status, iterations) and behind it the eigenvalues of R^-1 Sigma^ of the saturated and of the estimated
// model in ascending order [P each], one number per line (NaN where the record stopped before them).  Built with -fsanitize=address,undefined (Makefile);
// every array is a heap block of exactly its size, so that an index past an end is reported.
//
// Input, whitespace separated (tests/modelfit_host's):  P L  |  boff [L + 1]  |  C [L x L] (C[i][j] = 1 iff LV j -> LV i)  |  factor [L]  |  lambda* [P]  |
// lv_cor_c [npairs]  |  direct [n_eff] (the effect pairs from-major, as the library orders them)  |  R [P x P]  |  model-fit status, iterations
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "geodesic_core.h"

using namespace plspm;

template <class T> static bool read_all(FILE* f, std::vector<T>& v, const char* fmt) {
    for (auto& x : v) if (fscanf(f, fmt, &x) != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: geodesic_host INPUT\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int P, L;
    if (fscanf(f, "%d %d", &P, &L) != 2 || P < 1 || L < 1) { fprintf(stderr, "bad header\n"); return 2; }
    const int npairs = L * (L - 1) / 2;
    std::vector<int> boff(L + 1), C((size_t)L * L), factor_i(L);
    if (!read_all(f, boff, "%d") || !read_all(f, C, "%d") || !read_all(f, factor_i, "%d")) { fprintf(stderr, "short input\n"); return 2; }
    // the descriptors as the library builds them (plspm_model_create): predecessors in CSR form, effect pairs from the transitive closure, from-major
    std::vector<unsigned char> factor(L);
    for (int l = 0; l < L; ++l) factor[l] = (unsigned char)factor_i[l];
    std::vector<int> lvof(P), pred_off(L + 1, 0), pred_idx, eff_from, eff_to;
    for (int l = 0; l < L; ++l) for (int p = boff[l]; p < boff[l + 1]; ++p) lvof[p] = l;
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < L; ++j) if (C[i * L + j]) pred_idx.push_back(j);
        pred_off[i + 1] = (int)pred_idx.size();
    }
    std::vector<int> reach(C);
    for (int k = 0; k < L; ++k) for (int i = 0; i < L; ++i) for (int j = 0; j < L; ++j) if (reach[i * L + k] && reach[k * L + j]) reach[i * L + j] = 1;
    for (int fr = 0; fr < L; ++fr) for (int t = 0; t < L; ++t) if (fr != t && reach[t * L + fr]) { eff_from.push_back(fr); eff_to.push_back(t); }
    std::vector<double> lam(P), lv_cor_c(npairs), direct(eff_from.size()), R((size_t)P * P), tail(2);
    if (!read_all(f, lam, "%lf") || !read_all(f, lv_cor_c, "%lf") || !read_all(f, direct, "%lf") || !read_all(f, R, "%lf") || !read_all(f, tail, "%lf")) {
        fprintf(stderr, "short input\n"); return 2;
    }
    fclose(f);
    ModelDesc md{};
    md.P = P; md.L = L; md.n_eff = (int)eff_from.size();
    md.boff = boff.data(); md.lvof = lvof.data(); md.pred_off = pred_off.data(); md.pred_idx = pred_idx.data();
    md.eff_from = eff_from.data(); md.eff_to = eff_to.data(); md.n_edges = (int)pred_idx.size();
    std::vector<double> lds((size_t)geodesic_ws_doubles(P, L)), out(GEODESIC_WIDTH + 2, -777.0), eig((size_t)2 * P, sqrt(-1.0));
    GeodesicWs w;
    geodesic_carve(w, lds.data(), P, L);
    for (int p = 0; p < P; ++p) { w.mf.isd[p] = 1.0; w.mf.mu[p] = 0.0; w.mf.lam[p] = lam[p]; }
    GeodesicSerialExec ex;
    modelfit_phi(ex, md, w.mf, lv_cor_c.data(), direct.data());
    const auto corr = [&](int p, int q) { return R[(size_t)p * P + q]; };
    geodesic_record(ex, md, w, factor.data(), corr, tail[0], tail[1], out.data(), eig.data());
    for (double x : out) printf("%.17g\n", x);
    for (double x : eig) printf("%.17g\n", x);
    return 0;
}
