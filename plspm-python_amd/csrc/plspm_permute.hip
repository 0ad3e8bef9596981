// plspm_permute.hip -- host side, part 5: the two-group permutation test (multi-group analysis).  B random splits of the resident rows into
// groups of n1 and N - n1 rows become 2B problems of the bootstrap's int8 route: 0/1 count rows instead of resample counts (kernels_permute.h),
// then the same Gram (run_gram_i8) and batch solver, which read each problem's n from the ones column of its moment matrix -- the moments of a
// count row that is 1 on a group's rows ARE that group's moments, treatment and the `scaled` scalar included.  The exceedance counts of the
// statistic |est_a - est_b| run on the 2B records left in HBM.
#include "host_internal.h"

#include "philox.h"
#include "wave_ops.h"
#include "kernels_permute.h"

int launch_perm_counts(plspm_model* m, int64_t nb, int64_t prob0, int MT, int KB, void* cd) {
    const PermSpec& ps = *m->perm;
    const int64_t np = nb / 2, p0 = prob0 / 2;               // (plspm_detail_bootstrap cuts a batch into whole 256-problem tiles: pairs stay together)
    const int N = (int)m->N;
    int rc;
    const uint2* thr = nullptr;
    if (!ps.d_member) {
        if ((rc = ensure(m, m->perm_thr, (size_t)np * sizeof(uint2)))) return rc;
        // the keys in LDS after the first radix pass while they fit 48 KB (three workgroups per CU); beyond that every pass draws them again
        const bool cache = N <= PERM_CACHE_ROWS;
        const size_t lds = cache ? (size_t)N * sizeof(unsigned) : 0;
        if ((rc = allow_lds(m, (const void*)perm_threshold_kernel, lds))) return rc;
        hipLaunchKernelGGL(perm_threshold_kernel, dim3((unsigned)np), dim3(PERM_NT), lds, m->stream, N, (int)ps.n1, ps.seed, ps.rep_offset + p0, cache ? 1 : 0,
                           (uint2*)m->perm_thr.p);
        thr = (const uint2*)m->perm_thr.p;
    }
    const dim3 grid((unsigned)((np + 7) / 8), (unsigned)((KB * 4 + PERM_NT / 8 - 1) / (PERM_NT / 8)));
    hipLaunchKernelGGL(perm_counts_kernel, grid, dim3(PERM_NT), 0, m->stream, N, KB, MT, ps.seed, ps.rep_offset + p0, (int)np, thr,
                       ps.d_member ? ps.d_member + p0 * (int64_t)N : (const uint8_t*)nullptr, (uint4*)cd);
    HIPCHK(m, hipGetLastError());
    return 0;
}

extern "C" {

int plspm_permutation_members(uint64_t seed, int64_t perm, int64_t N, int64_t n1, uint8_t* member) {
    if (!member || N < 2 || N > 0x7fffffffLL || perm < 0 || n1 < 1 || n1 >= N) return PLSPM_E_ARG;
    std::vector<std::pair<uint32_t, uint32_t>> key((size_t)N);
    for (int64_t q = 0; q < (N + 3) / 4; ++q) {
        const u32x4 u = permute_quad(seed, (uint64_t)perm, (uint32_t)q);
        for (int j = 0; j < 4; ++j) if (4 * q + j < N) key[(size_t)(4 * q + j)] = {u.v[j], (uint32_t)(4 * q + j)};
    }
    std::nth_element(key.begin(), key.begin() + (n1 - 1), key.end());
    const std::pair<uint32_t, uint32_t> last = key[(size_t)(n1 - 1)];       // the n1-th smallest (key, row) pair
    for (int64_t i = 0; i < N; ++i) member[i] = 0;
    for (const auto& k : key) if (k <= last) member[k.second] = 1;
    return 0;
}

int plspm_permutation_device(plspm_model_t* m, int64_t B, uint64_t seed, int64_t rep_offset, int64_t n1, const uint8_t* member, void** d_out, void** d_status,
                             void** d_iters) {
    if (!m || B < 1 || B > ((int64_t)1 << 29) || rep_offset < 0) return fail(m, PLSPM_E_ARG, "plspm_permutation_device: bad arguments (1 <= B <= 2^29, rep_offset >= 0)");
    if (!m->d_Xa || m->N < 2) return fail(m, PLSPM_E_STATE, "plspm_permutation_device: no data uploaded");
    if (n1 < 1 || n1 >= m->N) return fail(m, PLSPM_E_ARG, "plspm_permutation_device: the group size must satisfy 1 <= n1 < N");
    if (m->nonmetric || m->categorical || m->n_ind || m->nmx_K || m->stage1 || m->stage2)
        return fail(m, PLSPM_E_ARG, "plspm_permutation_device: plain metric models only (no non-metric scales, no missing values, no two-stage pair)");
    if (m->tune.i8_shape != 16) return fail(m, PLSPM_E_ARG, "plspm_permutation_device: needs the 16x16x64 layout of the int8 Gram (i8_shape 16)");
    HIPCHK(m, hipSetDevice(m->device));
    // the int8 route whatever "gram_path" / "i8_min_batch" say (the dense 0/1 counts are what it reads), unless the route itself is closed
    const int keep_path = m->tune.gram_path, keep_slices = m->tune.i8_slices;
    m->tune.gram_path = 2;
    if (keep_slices && keep_slices < 7) m->tune.i8_slices = 7;           // (the budget of the seven planes this call cuts)
    const int route = choose_gram_path(m, 2 * B);
    m->tune.gram_path = keep_path; m->tune.i8_slices = keep_slices;
    if (route != 2) return fail(m, PLSPM_E_LIMIT, "plspm_permutation_device: the int8 Gram route is closed for this data set (N >= 2^24, or digit planes above their 24 GiB budget)");
    const uint8_t* d_member = nullptr;
    int rc;
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
    const PermSpec spec{seed, rep_offset, n1, d_member};
    m->perm = &spec;
    rc = plspm_detail_bootstrap(m, 2 * B, 0, 0, nullptr, nullptr);       // problems 2p / 2p + 1 = the groups of permutation rep_offset + p
    m->perm = nullptr;
    if (rc) return rc;
    if (d_out) *d_out = m->rows.p;
    if (d_status) *d_status = m->status.p;
    if (d_iters) *d_iters = m->iters.p;
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
