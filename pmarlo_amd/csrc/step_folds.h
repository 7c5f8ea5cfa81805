// Device bodies that one kernel of their own and a neighbouring launch both run (one copy each): the neighbour takes
// the work over where the step would otherwise pay a launch for a handful of threads.
#pragma once
#include "wave.h"

// mean / divisor of reduction._preprocess for one column from its raw sums (standardise_params_kernel, moments.hip;
// the tail of the lagged moments, cov.hip):
//   mean  = shift + S1/cnt
//   sigma = sqrt((S2 - S1^2/cnt) / n_rows)      (NaNs were imputed with the mean: they add 0
//           to the centred square sum but count in the divisor), sigma < 10 eps -> 1
__device__ __forceinline__ void standardise_params_body(double cnt, double s1, double s2, double shift, double n_rows,
                                                        int with_std, double* __restrict__ mean,
                                                        double* __restrict__ scale, double* __restrict__ inv_scale) {
    double m = 0.0, sd = 1.0;
    if (cnt > 0.0) {
        m = shift + s1 / cnt;
        if (with_std) {
            const double var = (s2 - s1 * s1 / cnt) / n_rows;
            sd = var > 0.0 ? sqrt(var) : 0.0;
            if (sd < 10.0 * 2.220446049250313e-16) sd = 1.0;
        }
    }
    *mean = m;
    *scale = sd;
    *inv_scale = 1.0 / sd;
}

// trace(T) / k from the diagonal entries other workgroups left in `tdiag` with device-scope stores, by the ONE workgroup
// (MT threads, MT a multiple of 64 that divides 1024) that took the last arrival ticket: diag_mass_kernel's additions
// over its 1024 threads (msm.hip), MT at a time, so every way of closing gives the same bits.  red: 16 doubles of LDS.
template <int MT>
__device__ __forceinline__ void diag_mass_close(const double* tdiag, int k, double* red, double* __restrict__ diag_out) {
    for (int v0 = 0; v0 < 1024; v0 += MT) {
        const int v = v0 + threadIdx.x;
        double t = 0.0;
        for (int q = v; q < k; q += 1024) t += __hip_atomic_load(&tdiag[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = wave_sum_down(t);
        if ((v & 63) == 0) red[v >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < 16; ++w) s += red[w];
        *diag_out = k > 0 ? s / (double)k : __builtin_nan("");
    }
}
