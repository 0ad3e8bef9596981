// wave_launch.h -- host side: the one launch form of the kernels that give every problem of a batch one wave and a slice of dynamic LDS (assess_kernel,
// plsc_kernel, modelfit_kernel, geodesic_kernel: plspm_derived.hip; micom_kernel: plspm_micom.hip).
#pragma once
#include "host_internal.h"
#include "kernels_moments.h"

// the moment matrices the chunk's solver read, still in place: dense where a dense solver read them, else tile-packed
inline MomentLayout moment_layout(const plspm_model* m, bool dense, const double* gram) {
    return {gram, dense ? cov_doubles(m->P) : packed_size(m->T), dense ? cov_ld(m->P) : m->T, m->P};
}

// `grid` workgroups of kernel `k` on `a`, `waves` waves and `lds` bytes of dynamic LDS each (the derived records: as derived_route.h plans them).  marks / nclocks /
// print: the phase clocks of problem 0 (`make marks`; never in the release library) -- the field of `a` that takes their device buffer, how many there are, and what
// writes them to stderr; null / 0: none.
template <class Args>
int launch_wave_per_problem(plspm_model* m, void (*k)(Args), Args& a, int waves, size_t lds, long grid, long long** marks = nullptr, int nclocks = 0,
                            void (*print)(const long long*) = nullptr) {
    if (int rc = allow_lds(m, (const void*)k, lds)) return rc;
#ifdef PLSPM_DEBUG_MARKS
    if (marks) HIPCHK(m, plspm_dmalloc((void**)marks, nclocks * sizeof(long long)));
#endif
    {
        ProfScope ps(m, PLSPM_K_ASSESS);
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(64 * waves), lds, m->stream, a);
    }
#ifdef PLSPM_DEBUG_MARKS
    if (marks) {
        std::vector<long long> h((size_t)nclocks);
        HIPCHK(m, hipStreamSynchronize(m->stream));
        HIPCHK(m, hipMemcpy(h.data(), *marks, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
        print(h.data());
        plspm_dfree(*marks);
    }
#endif
    return 0;
}
