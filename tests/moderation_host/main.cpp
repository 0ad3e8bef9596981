// TEST INFRASTRUCTURE: csrc/moderation_core.h on one problem read from a text file (or from standard input), on the serial host executor.  Built with
// -fsanitize=address,undefined (Makefile); every array is a heap block of exactly its size, so that an index past an end is reported.
//
// Input, whitespace separated:  the word "record" or "plan"  |  L  |  C [L x L] (C[i][j] = 1 iff LV j -> LV i, strictly lower triangular)  |  T  |  per term:
// predictor, moderator, target  |  the items of every LV [L]
//   record:  n  |  rc [nl x nl] of the needed LVs  |  the row sums [nsums]  |  direct [n_eff] and r2 [L] of the bootstrap record
//            -> the moderation record (values, status, iterations), one number per line
//   plan:    N  -> "key value" lines: the layout's sizes and the plan of a call on N rows
// A term the definitions refuse: exit code 3 and the reason on stderr.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "moderation_core.h"

using namespace plspm;

template <class T> static bool read_all(FILE* f, std::vector<T>& v, const char* fmt) {
    for (auto& x : v) if (fscanf(f, fmt, &x) != 1) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc > 2) { fprintf(stderr, "usage: moderation_host [INPUT]\n"); return 2; }
    FILE* f = argc == 2 ? fopen(argv[1], "r") : stdin;
    if (!f) { perror(argv[1]); return 2; }
    char mode[16];
    int L, T;
    if (fscanf(f, "%15s %d", mode, &L) != 2 || L < 2 || L > 1024) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int> Ci((size_t)L * L);
    if (!read_all(f, Ci, "%d") || fscanf(f, "%d", &T) != 1 || T < 0 || T > 64) { fprintf(stderr, "short input\n"); return 2; }
    for (int i = 0; i < L; ++i) for (int j = i; j < L; ++j) if (Ci[i * L + j]) { fprintf(stderr, "the path matrix must be strictly lower triangular\n"); return 2; }
    std::vector<int> ta(T), tb(T), tj(T), items(L);
    for (int t = 0; t < T; ++t) if (fscanf(f, "%d %d %d", &ta[t], &tb[t], &tj[t]) != 3) { fprintf(stderr, "short input\n"); return 2; }
    if (!read_all(f, items, "%d")) { fprintf(stderr, "short input\n"); return 2; }
    // the descriptors as the library builds them (plspm_model_create): block offsets, predecessors in CSR form, effect pairs from the transitive closure, from-major
    std::vector<unsigned char> C(Ci.begin(), Ci.end());
    std::vector<int> boff(L + 1, 0), pred_off(L + 1, 0), pred_idx, eff_from, eff_to;
    for (int l = 0; l < L; ++l) { if (items[l] < 1) { fprintf(stderr, "bad block\n"); return 2; } boff[l + 1] = boff[l] + items[l]; }
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < L; ++j) if (C[i * L + j]) pred_idx.push_back(j);
        pred_off[i + 1] = (int)pred_idx.size();
    }
    std::vector<int> reach(Ci);
    for (int k = 0; k < L; ++k) for (int i = 0; i < L; ++i) for (int j = 0; j < L; ++j) if (reach[i * L + k] && reach[k * L + j]) reach[i * L + j] = 1;
    for (int fr = 0; fr < L; ++fr) for (int t = 0; t < L; ++t) if (fr != t && reach[t * L + fr]) { eff_from.push_back(fr); eff_to.push_back(t); }
    const int n_eff = (int)eff_from.size(), P = boff[L];
    if (pred_idx.empty()) pred_idx.push_back(0);
    if (eff_from.empty()) { eff_from.push_back(0); eff_to.push_back(0); }
    ModBuild mb;
    std::string why;
    if (moderation_build(L, P, boff.data(), C.data(), pred_off.data(), pred_idx.data(), n_eff, eff_from.data(), eff_to.data(), T, ta.data(), tb.data(), tj.data(), mb, why)) {
        fprintf(stderr, "%s\n", why.c_str());
        return 3;
    }
    const ModLayout& y = mb.lay;
    if (!strcmp(mode, "plan")) {
        long N;
        if (fscanf(f, "%ld", &N) != 1 || N < 0) { fprintf(stderr, "short input\n"); return 2; }
        const ModPlan p = moderation_plan(y, mb.e_total, N);
        printf("width %d\nnsums %d\nnacc %d\nnl %d\nncoef %d\nntgt %d\nnjobs %d\nKM %d\nn_dir %d\nrow_block %d\nrow_blocks %d\ntable_in_lds %d\n", p.width, p.nsums, p.nacc, y.nl, y.ncoef,
               y.ntgt, y.njobs, y.KM, y.n_dir, p.row_block, p.row_blocks, (int)p.table_in_lds);
        printf("counts_lds %zu\nprepare_lds %zu\nrows_lds %zu\nfinish_lds %zu\nrefused %d\n", p.counts_lds, p.prepare_lds, p.rows_lds, p.finish_lds, p.refused);
        if (p.refused) printf("need %s\n", moderation_refusal(p.refused));
        return 0;
    }
    if (strcmp(mode, "record")) { fprintf(stderr, "bad mode\n"); return 2; }
    double n;
    std::vector<double> rcn((size_t)y.nl * y.nl), sums((size_t)y.nsums), direct((size_t)n_eff), r2((size_t)L);
    if (fscanf(f, "%lf", &n) != 1 || !read_all(f, rcn, "%lf") || !read_all(f, sums, "%lf") || !read_all(f, direct, "%lf") || !read_all(f, r2, "%lf")) {
        fprintf(stderr, "short input\n");
        return 2;
    }
    if (f != stdin) fclose(f);
    // the bootstrap record: weights [P] | r2 [L] | total [n_eff] | direct [n_eff] | loadings [P] | status | iterations; the r2 and direct entries, the status and the
    // iterations are read
    const int R = 2 * P + L + 2 * n_eff;
    std::vector<double> rec((size_t)R + 2, -555.0);
    std::copy(r2.begin(), r2.end(), rec.begin() + P);
    std::copy(direct.begin(), direct.end(), rec.begin() + P + L + n_eff);
    rec[R] = 0.0; rec[R + 1] = 7.0;
    const int W = moderation_width(y);
    std::vector<double> lds((size_t)moderation_finish_doubles(y, mb.e_total)), out((size_t)W + 2, -777.0);
    std::vector<int> blob(mb.blob);
    ModDesc d{y, blob.data()};
    ModWs w;
    moderation_carve(w, lds.data(), y, mb.e_total);
    std::copy(sums.begin(), sums.end(), w.tot);
    std::copy(rcn.begin(), rcn.end(), w.rcn);
    ModSerialExec ex;
    moderation_record(ex, d, w, n, rec.data(), R, out.data());
    for (double x : out) printf("%.17g\n", x);
    return 0;
}
