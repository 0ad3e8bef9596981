// plspm_permute.hip -- host side, part 5: the two-group permutation test (multi-group analysis).  B random splits of the resident rows into
// groups of n1 and N - n1 rows become 2B problems of the bootstrap's int8 route: 0/1 count rows instead of resample counts (kernels_permute.h),
// then the same Gram (run_gram_i8) and batch solver, which read each problem's n from the ones column of its moment matrix -- the moments of a
// count row that is 1 on a group's rows ARE that group's moments, treatment and the `scaled` scalar included.  The exceedance counts of the
// statistic |est_a - est_b| run on the 2B records left in HBM.
// The stratified bootstrap of the same test (plspm_stratified_bootstrap_device) takes the same road with int8 counts of draws made inside each
// group (kernels_strat.h); Henseler's all-pairs counts (plspm_stratified_pair_counts) run on its records in HBM as well.
#include "host_internal.h"

#include "philox.h"
#include "wave_ops.h"
#include "kernels_permute.h"
#include "kernels_strat.h"

int launch_perm_counts(plspm_model* m, const PermSpec& ps, int64_t nb, int64_t prob0, int MT, int KB, void* cd) {
    const int64_t np = nb / 2, p0 = prob0 / 2;               // (plspm_detail_bootstrap cuts a batch into whole 256-problem tiles: pairs stay together)
    const int N = (int)m->N;
    int rc;
    const uint2* thr = nullptr;
    if (!ps.d_member) {
        if ((rc = ensure(m, m->perm_thr, (size_t)np * sizeof(uint2)))) return rc;
        // the keys in LDS after the first radix pass while they fit 48 KB (three workgroups per CU); beyond that every pass draws them again
        const bool cache = N <= RANK_CACHE_ROWS;
        const size_t lds = cache ? (size_t)N * sizeof(unsigned) : 0;
        if ((rc = allow_lds(m, (const void*)perm_threshold_kernel, lds))) return rc;
        hipLaunchKernelGGL(perm_threshold_kernel, dim3((unsigned)np), dim3(RANK_NT), lds, m->stream, N, (int)ps.n1, ps.seed, ps.rep_offset + p0, cache ? 1 : 0,
                           (uint2*)m->perm_thr.p);
        thr = (const uint2*)m->perm_thr.p;
    }
    hipLaunchKernelGGL(perm_counts_kernel, count_rows_grid(np, KB), dim3(COUNT_NT), 0, m->stream, N, KB, MT, ps.seed, ps.rep_offset + p0, (int)np, thr,
                       ps.d_member ? ps.d_member + p0 * (int64_t)N : (const uint8_t*)nullptr, (uint4*)cd);
    HIPCHK(m, hipGetLastError());
    return 0;
}

int launch_strat_counts(plspm_model* m, const StratSpec& ss, int64_t nb, int64_t prob0, int MT, int KB, void* cd) {
    const int N = (int)m->N, n_a = (int)ss.n_a;
    const int ng_max = std::max(n_a, N - n_a);
    const size_t hist_bytes = (size_t)std::min(KB, STRAT_HIST_KB) * 32 * sizeof(unsigned);
    // the group's row list is read through L2: copying it into LDS first was slower on the 10k x 60 benchmark (tools/mga_boot_bench.py:
    // 0.106 against 0.098 ms per 10,000 problems at 5,000/5,000 rows, 0.150 against 0.118 at 2,000/8,000 -- the copy and the larger LDS
    // footprint cost more than the L2 hits they save).  "strat_rows" 2: from LDS wherever it fits the 160 KB (A/B and tests); 0, 1: L2
    const size_t rows_bytes = (size_t)ng_max * sizeof(int);
    const bool rows_lds = !ss.d_draws && m->tune.strat_rows == 2 && hist_bytes + rows_bytes <= (size_t)160 * 1024;
    const size_t lds = hist_bytes + (rows_lds ? rows_bytes : 0);
    const void* k = rows_lds ? (const void*)strat_counts_kernel<true> : (const void*)strat_counts_kernel<false>;
    int rc;
    if ((rc = allow_lds(m, k, lds))) return rc;
    // threads: as resample_i8_kernel -- the fewer workgroups the LDS lets share a CU, the more threads each
    const unsigned threads = (unsigned)std::min(1024, std::max(256, 256 * (int)(8 / std::max<size_t>(1, (160 * 1024) / std::max<size_t>(1, lds)))));
    const dim3 grid((unsigned)nb, (unsigned)((KB + STRAT_HIST_KB - 1) / STRAT_HIST_KB));
    if (rows_lds)
        hipLaunchKernelGGL(strat_counts_kernel<true>, grid, dim3(threads), lds, m->stream, N, KB, MT, n_a, ss.seed, ss.rep_offset, prob0, ss.d_rows, ss.d_draws, (uint4*)cd, (int*)m->err.p);
    else
        hipLaunchKernelGGL(strat_counts_kernel<false>, grid, dim3(threads), lds, m->stream, N, KB, MT, n_a, ss.seed, ss.rep_offset, prob0, ss.d_rows, ss.d_draws, (uint4*)cd, (int*)m->err.p);
    m->last_strat_rows = rows_lds ? 2 : 1;
    HIPCHK(m, hipGetLastError());
    return 0;
}

// rows of each group in ascending order: rows[0, n_a) = group a, rows[n_a, N) = group b; returns n_a, or -1 when a byte is not 0 / 1
static int64_t strat_split(const uint8_t* member, int64_t N, int32_t* rows) {
    int64_t n_a = 0;
    for (int64_t i = 0; i < N; ++i) { if (member[i] > 1) return -1; n_a += member[i]; }
    int64_t ia = 0, ib = n_a;
    for (int64_t i = 0; i < N; ++i) rows[member[i] ? ia++ : ib++] = (int32_t)i;
    return n_a;
}

extern "C" {

int plspm_stratified_draws(uint64_t seed, int64_t rep, int64_t N, const uint8_t* member, int32_t* rows) {
    if (!member || !rows || N < 4 || N > 0x7fffffffLL || rep < 0 || rep >= ((int64_t)1 << 62)) return PLSPM_E_ARG;
    std::vector<int32_t> grp((size_t)N);
    const int64_t n_a = strat_split(member, N, grp.data());
    if (n_a < 2 || N - n_a < 2) return PLSPM_E_ARG;
    for (int g = 0; g < 2; ++g) {
        const int64_t off = g ? n_a : 0, ng = g ? N - n_a : n_a;
        const uint64_t s = 2u * (uint64_t)rep + (uint64_t)g;
        for (int64_t q = 0; q < (ng + 3) / 4; ++q) {
            const u32x4 u = strat_quad(seed, s, (uint32_t)q);
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < ng) rows[off + 4 * q + j] = grp[(size_t)(off + to_index(u.v[j], (uint32_t)ng))];
        }
    }
    return 0;
}

int plspm_stratified_bootstrap_device(plspm_model_t* m, int64_t B, uint64_t seed, int64_t rep_offset, const uint8_t* member, const int32_t* draws, void** d_out,
                                      void** d_status, void** d_iters) {
    if (!m || B < 1 || B > ((int64_t)1 << 29) || rep_offset < 0 || rep_offset > ((int64_t)1 << 61) || !member)
        return fail(m, PLSPM_E_ARG, "plspm_stratified_bootstrap_device: bad arguments (1 <= B <= 2^29, rep_offset >= 0, member required)");
    int rc;
    if ((rc = counts_call_scope(m, "plspm_stratified_bootstrap_device", 4))) return rc;
    const int64_t N = m->N;
    std::vector<int32_t> grp((size_t)N);
    const int64_t n_a = strat_split(member, N, grp.data());
    if (n_a < 0) return fail(m, PLSPM_E_ARG, "plspm_stratified_bootstrap_device: memberships must be 0 or 1");
    if (n_a < 2 || N - n_a < 2) return fail(m, PLSPM_E_ARG, "plspm_stratified_bootstrap_device: each group needs at least two rows");
    if ((rc = counts_route_scope(m, "plspm_stratified_bootstrap_device"))) return rc;
    const size_t row_bytes = (size_t)N * sizeof(int32_t);
    if (!m->strat_rows.p || m->strat_member.size() != (size_t)N || !std::equal(member, member + N, m->strat_member.begin())) {
        if ((rc = ensure(m, m->strat_rows, row_bytes))) return rc;
        if ((rc = plspm_detail_h2d(m, m->strat_rows.p, grp.data(), row_bytes))) return rc;
        m->strat_member.assign(member, member + N);
    }
    const int32_t* d_draws = nullptr;
    if (draws) {
        // explicit draws (tests): entries [0, n_a) rows of group a, [n_a, N) rows of group b.  A multiplicity of 65,536 or more would wrap the
        // kernel's 16-bit counters unseen: refused here (128 .. 65,535 raise the device's flag)
        std::vector<uint32_t> seen((size_t)N);
        for (int64_t p = 0; p < B; ++p) {
            const int32_t* dp = draws + p * N;
            std::fill(seen.begin(), seen.end(), 0u);
            for (int64_t i = 0; i < N; ++i) {
                const int32_t r = dp[i];
                if (r < 0 || r >= N || (member[r] != 0) != (i < n_a))
                    return fail(m, PLSPM_E_ARG, "plspm_stratified_bootstrap_device: an explicit draw is not a row of its group");
                if (++seen[(size_t)r] > 0xffffu) return fail(m, PLSPM_E_LIMIT, "plspm_stratified_bootstrap_device: a multiplicity exceeded 127 on the int8 Gram path");
            }
        }
        if ((rc = ensure(m, m->strat_draws, (size_t)B * row_bytes))) return rc;
        if ((rc = plspm_detail_h2d(m, m->strat_draws.p, draws, (size_t)B * row_bytes))) return rc;
        d_draws = (const int32_t*)m->strat_draws.p;
    }
    const StratSpec spec{seed, rep_offset, n_a, (const int32_t*)m->strat_rows.p, d_draws};
    BatchCall call;
    call.kind = BatchCall::STRATIFIED; call.strat = &spec; call.B = 2 * B;       // problems 2p / 2p + 1 = the groups of resample rep_offset + p
    if ((rc = plspm_detail_bootstrap(m, call))) return rc;
    // the error word (cleared by the driver in front of the counts): a multiplicity above 127 never wraps silently
    int* h_err = (int*)m->h_flag + 9;
    HIPCHK(m, hipMemcpyAsync(h_err, m->err.p, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    if (*h_err & 2) { void_records(m, REC_ROWS); return fail(m, PLSPM_E_LIMIT, "plspm_stratified_bootstrap_device: a multiplicity exceeded 127 on the int8 Gram path"); }
    if (*h_err) { void_records(m, REC_ROWS); return fail(m, PLSPM_E_STATE, "plspm_stratified_bootstrap_device: the device reported error bits " + std::to_string(*h_err)); }
    hand_out(m->rows, m->status, m->iters, d_out, d_status, d_iters);
    return 0;
}

int plspm_stratified_pair_counts(plspm_model_t* m, int64_t B, const double* center_a, const double* center_b, int64_t* above, int64_t* used_a, int64_t* used_b) {
    if (!m || B < 1 || !center_a || !center_b || !above) return fail(m, PLSPM_E_ARG, "plspm_stratified_pair_counts: bad arguments");
    if (!m->rows_B || !m->rows.p) return fail(m, PLSPM_E_STATE, "plspm_stratified_pair_counts: no records on this handle");
    if (m->rows_B != 2 * B) return fail(m, PLSPM_E_ARG, "plspm_stratified_pair_counts: the handle's last records are not 2B (the last stratified call's B?)");
    HIPCHK(m, hipSetDevice(m->device));
    const int R = plspm_row_width(m), RS = plspm_row_stride(m);
    const long Bp = (long)((B + 1) & ~(int64_t)1);                      // (even: the pair kernel reads its LDS tile in pairs)
    int rc;
    // [centres 2R | above R | used 2] and the u values [2][R][Bp]
    if ((rc = ensure(m, m->strat_io, (size_t)(3 * R + 2) * sizeof(double)))) return rc;
    if ((rc = ensure(m, m->strat_u, (size_t)2 * R * Bp * sizeof(double)))) return rc;
    double* d_ctr = (double*)m->strat_io.p;
    unsigned long long* d_cnt = (unsigned long long*)(d_ctr + 2 * R);
    HIPCHK(m, hipMemcpyAsync(d_ctr, center_a, (size_t)R * sizeof(double), hipMemcpyHostToDevice, m->stream));
    HIPCHK(m, hipMemcpyAsync(d_ctr + R, center_b, (size_t)R * sizeof(double), hipMemcpyHostToDevice, m->stream));
    HIPCHK(m, hipMemsetAsync(d_cnt, 0, (size_t)(R + 2) * sizeof(unsigned long long), m->stream));
    {
        ProfScope ps(m, PLSPM_K_REDUCE);
        hipLaunchKernelGGL(strat_u_kernel, dim3((unsigned)((R + 31) / 32), (unsigned)((2 * B + 63) / 64)), dim3(STRAT_U_NT), 0, m->stream, (const double*)m->rows.p, (long)B, RS, R,
                           (const double*)d_ctr, (double*)m->strat_u.p, Bp, d_cnt + R);
        hipLaunchKernelGGL(strat_pair_kernel, dim3((unsigned)R, (unsigned)((B + STRAT_PAIR_NT * STRAT_PAIR_PER - 1) / (STRAT_PAIR_NT * STRAT_PAIR_PER))), dim3(STRAT_PAIR_NT), 0, m->stream,
                           (const double*)m->strat_u.p, (long)B, Bp, R, d_cnt);
    }
    HIPCHK(m, hipGetLastError());
    std::vector<unsigned long long> h((size_t)R + 2);
    HIPCHK(m, hipMemcpyAsync(h.data(), d_cnt, (size_t)(R + 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    for (int j = 0; j < R; ++j) above[j] = (int64_t)h[(size_t)j];
    if (used_a) *used_a = (int64_t)h[(size_t)R];
    if (used_b) *used_b = (int64_t)h[(size_t)R + 1];
    return 0;
}

int plspm_permutation_members(uint64_t seed, int64_t perm, int64_t N, int64_t n1, uint8_t* member) {
    if (!member || N < 2 || N > 0x7fffffffLL || perm < 0 || n1 < 1 || n1 >= N) return PLSPM_E_ARG;
    std::vector<std::pair<uint32_t, uint32_t>> key = row_keys(permute_quad, seed, perm, N);
    std::nth_element(key.begin(), key.begin() + (n1 - 1), key.end());
    const std::pair<uint32_t, uint32_t> last = key[(size_t)(n1 - 1)];       // the n1-th smallest (key, row) pair
    for (int64_t i = 0; i < N; ++i) member[i] = 0;
    for (const auto& k : key) if (k <= last) member[k.second] = 1;
    return 0;
}

int plspm_permutation_device(plspm_model_t* m, int64_t B, uint64_t seed, int64_t rep_offset, int64_t n1, const uint8_t* member, void** d_out, void** d_status,
                             void** d_iters) {
    if (!m || B < 1 || B > ((int64_t)1 << 29) || rep_offset < 0) return fail(m, PLSPM_E_ARG, "plspm_permutation_device: bad arguments (1 <= B <= 2^29, rep_offset >= 0)");
    int rc;
    if ((rc = counts_call_scope(m, "plspm_permutation_device"))) return rc;
    if (n1 < 1 || n1 >= m->N) return fail(m, PLSPM_E_ARG, "plspm_permutation_device: the group size must satisfy 1 <= n1 < N");
    if ((rc = counts_route_scope(m, "plspm_permutation_device"))) return rc;
    const uint8_t* d_member = nullptr;
    if (member) {
        // explicit memberships (tests): every row of bytes 0/1 with exactly n1 ones
        for (int64_t p = 0; p < B; ++p) {
            const uint8_t* mp = member + p * m->N;
            int64_t ones = 0;
            for (int64_t i = 0; i < m->N; ++i) { if (mp[i] > 1) return fail(m, PLSPM_E_ARG, "plspm_permutation_device: memberships must be 0 or 1"); ones += mp[i]; }
            if (ones != n1) return fail(m, PLSPM_E_ARG, "plspm_permutation_device: a membership row does not hold n1 ones");
        }
        const size_t bytes = (size_t)B * (size_t)m->N;
        if ((rc = ensure(m, m->perm_member, bytes))) return rc;
        if ((rc = plspm_detail_h2d(m, m->perm_member.p, member, bytes))) return rc;
        d_member = (const uint8_t*)m->perm_member.p;
    }
    if (m->micom_on && (rc = micom_prepare(m))) return rc;               // (the pooled inputs of the MICOM records: once per upload, in front of the batch that overwrites m->gram)
    const PermSpec spec{seed, rep_offset, n1, d_member};
    BatchCall call;
    call.kind = BatchCall::PERMUTATION; call.perm = &spec; call.B = 2 * B;       // problems 2p / 2p + 1 = the groups of permutation rep_offset + p
    if ((rc = plspm_detail_bootstrap(m, call))) return rc;
    hand_out(m->rows, m->status, m->iters, d_out, d_status, d_iters);
    return 0;
}

int plspm_permutation_counts(plspm_model_t* m, int64_t B, const double* observed_diff, int64_t* exceed, int64_t* n_used) {
    if (!m || B < 1 || !observed_diff || !exceed) return fail(m, PLSPM_E_ARG, "plspm_permutation_counts: bad arguments");
    if (!m->rows_B || !m->rows.p) return fail(m, PLSPM_E_STATE, "plspm_permutation_counts: no records on this handle");
    if (m->rows_B != 2 * B) return fail(m, PLSPM_E_ARG, "plspm_permutation_counts: the handle's last records are not 2B (the last permutation call's B?)");
    HIPCHK(m, hipSetDevice(m->device));
    const int R = plspm_row_width(m), RS = plspm_row_stride(m);
    int rc;
    // [observed differences R | exceedance counts R | valid permutations]
    if ((rc = ensure(m, m->perm_io, (size_t)(2 * R + 1) * sizeof(double)))) return rc;
    double* d_obs = (double*)m->perm_io.p;
    unsigned long long* d_exc = (unsigned long long*)(d_obs + R);
    HIPCHK(m, hipMemcpyAsync(d_obs, observed_diff, (size_t)R * sizeof(double), hipMemcpyHostToDevice, m->stream));
    {
        ProfScope ps(m, PLSPM_K_REDUCE);
        hipLaunchKernelGGL(perm_exceed_kernel, dim3((unsigned)R), dim3(PERM_NT), 0, m->stream, (const double*)m->rows.p, (long)B, RS, R, (const double*)d_obs, d_exc, d_exc + R);
    }
    HIPCHK(m, hipGetLastError());
    std::vector<unsigned long long> h((size_t)R + 1);
    HIPCHK(m, hipMemcpyAsync(h.data(), d_exc, (size_t)(R + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(m, hipStreamSynchronize(m->stream));
    for (int j = 0; j < R; ++j) exceed[j] = (int64_t)h[(size_t)j];
    if (n_used) *n_used = (int64_t)h[(size_t)R];
    return 0;
}

}  // extern "C"
