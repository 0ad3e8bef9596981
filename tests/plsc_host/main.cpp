// TEST INFRASTRUCTURE: csrc/plsc_core.h plsc_record on one problem read from a text file, on the serial host executor; prints the PLSc record (values, status,
// iterations), one number per line.  Built with -fsanitize=address,undefined (Makefile); every array is a heap block of exactly its size, so that an index
// past an end is reported.
//
// Input, whitespace separated:  P L R  |  boff [L + 1]  |  C [L x L] (C[i][j] = 1 iff LV j -> LV i)  |  factor [L]  |  rho_a [L]  |  lv_cor [npairs]  |
// side [3 L] (sigma | v'Rv | v'v)  |  v [P]  |  record [R + 2]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plsc_core.h"

using namespace plspm;

template <class T> static bool read_all(FILE* f, std::vector<T>& v, const char* fmt) {
    for (auto& x : v) if (fscanf(f, fmt, &x) != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: plsc_host INPUT\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int P, L, R;
    if (fscanf(f, "%d %d %d", &P, &L, &R) != 3 || P < 1 || L < 1 || R < 2 * P + L) { fprintf(stderr, "bad header\n"); return 2; }
    const int npairs = L * (L - 1) / 2, W = R + npairs;
    std::vector<int> boff(L + 1), C((size_t)L * L), factor_i(L);
    std::vector<double> rho_a(L), lv_cor(npairs), side(3 * (size_t)L), v(P), rec((size_t)R + 2);
    if (!read_all(f, boff, "%d") || !read_all(f, C, "%d") || !read_all(f, factor_i, "%d") || !read_all(f, rho_a, "%lf") || !read_all(f, lv_cor, "%lf") ||
        !read_all(f, side, "%lf") || !read_all(f, v, "%lf") || !read_all(f, rec, "%lf")) { fprintf(stderr, "short input\n"); return 2; }
    fclose(f);
    // the descriptors as the library builds them (plspm_model_create): predecessors in CSR form, effect pairs from the transitive closure, from-major
    std::vector<unsigned char> factor(L);
    for (int l = 0; l < L; ++l) factor[l] = (unsigned char)factor_i[l];
    std::vector<int> lvof(P), pred_off(L + 1, 0), pred_idx, eff_from, eff_to;
    for (int l = 0; l < L; ++l) for (int p = boff[l]; p < boff[l + 1]; ++p) lvof[p] = l;
    int kmax = 0;
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < L; ++j) if (C[i * L + j]) pred_idx.push_back(j);
        pred_off[i + 1] = (int)pred_idx.size();
        kmax = std::max(kmax, pred_off[i + 1] - pred_off[i]);
    }
    std::vector<int> reach(C);
    for (int k = 0; k < L; ++k) for (int i = 0; i < L; ++i) for (int j = 0; j < L; ++j) if (reach[i * L + k] && reach[k * L + j]) reach[i * L + j] = 1;
    for (int fr = 0; fr < L; ++fr) for (int t = 0; t < L; ++t) if (fr != t && reach[t * L + fr]) { eff_from.push_back(fr); eff_to.push_back(t); }
    if (R != 2 * P + L + 2 * (int)eff_from.size()) { fprintf(stderr, "R does not match the model\n"); return 2; }
    ModelDesc md{};
    md.P = P; md.L = L; md.kmax = kmax; md.n_eff = (int)eff_from.size();
    md.boff = boff.data(); md.lvof = lvof.data(); md.pred_off = pred_off.data(); md.pred_idx = pred_idx.data();
    md.eff_from = eff_from.data(); md.eff_to = eff_to.data(); md.n_edges = (int)pred_idx.size();
    std::vector<double> lds((size_t)plsc_ws_doubles(P, L, kmax)), out((size_t)W + 2, -777.0);
    PlscWs w;
    plsc_carve(w, lds.data(), P, L, kmax);
    for (int p = 0; p < P; ++p) w.v[p] = v[p];
    PlscSerialExec ex;
    plsc_record(ex, md, w, factor.data(), rho_a.data(), lv_cor.data(), side.data(), rec.data(), R, out.data());
    for (double x : out) printf("%.17g\n", x);
    return 0;
}
