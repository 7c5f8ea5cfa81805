// Posterior samples of the transition matrix for the implied-timescale confidence intervals.
//
// Reference: ITSMixin._its_compute_for_single_lag (S/markov_state_model/_its.py:272-357) draws
// n_samples matrices from deeptime's BayesianMSM and summarises their spectra
// (_summarize_its_stats :543-668).  deeptime's sampler is third-party C++ that is absent here and
// its random stream cannot be reproduced; this file samples the closed-form posterior of the
// estimator the engine uses (msm_transition_matrix mode 1: T = rownorm(C_active + alpha),
// reversible = False): row i ~ Dirichlet(C_active[i, :] + alpha), independent rows, so the
// posterior mean is exactly the point estimate.
//
// A Dirichlet row is a vector of gamma variates divided by its sum.  The variates (philox.h:
// Marsaglia & Tsang's squeeze method on Philox4x32-10) are carried as logarithms, so that the
// alpha-only cells (shape 1e-3: U^1000) cannot underflow a whole row to 0/0.  The generator is keyed
// by the seed with counter (column, row, sample, attempt): a cell's variate does not depend on the
// launch geometry, the batch it is drawn in, or any other cell.
#include "common.h"
#include "philox.h"

namespace {

constexpr int kPT = 256;

__device__ __forceinline__ double block_reduce(double v, double* sh, bool is_max) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int s = kPT / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] = is_max ? fmax(sh[tid], sh[tid + s]) : sh[tid] + sh[tid + s];
        __syncthreads();
    }
    const double out = sh[0];
    __syncthreads();
    return out;
}

// one workgroup per (packed row, sample)
template <typename CT>
__global__ __launch_bounds__(kPT) void sample_rows_kernel(const CT* __restrict__ counts, int k,
                                                          const int32_t* __restrict__ active,
                                                          const int32_t* __restrict__ n_active, double alpha,
                                                          Philox rng, uint32_t first_sample,
                                                          double* __restrict__ T, int64_t t_stride, int ld) {
    __shared__ double sh[kPT];
    const int n = *n_active;
    const int row = blockIdx.x;
    if (row >= n) return;
    const uint32_t sample = first_sample + blockIdx.y;
    double* out = T + (int64_t)blockIdx.y * t_stride + (int64_t)row * ld;
    const CT* crow = counts + (int64_t)active[row] * k;
    double mx = -INFINITY;
    for (int j = threadIdx.x; j < n; j += kPT) {
        const double shape = (double)crow[active[j]] + alpha;
        double lg = -INFINITY;
        if (shape > 0.0) lg = log_gamma_variate(rng, shape, (uint32_t)j, (uint32_t)row, sample);
        out[j] = lg;
        mx = fmax(mx, lg);
    }
    mx = block_reduce(mx, sh, true);
    double sum = 0.0;
    for (int j = threadIdx.x; j < n; j += kPT) {
        const double e = mx == -INFINITY ? 0.0 : exp(out[j] - mx);
        out[j] = e;
        sum += e;
    }
    sum = block_reduce(sum, sh, false);
    // a row without any positive shape (alpha = 0 and no counts) stays a self-loop, as rownorm leaves it
    for (int j = threadIdx.x; j < n; j += kPT) out[j] = sum > 0.0 ? out[j] / sum : (j == row ? 1.0 : 0.0);
}

__global__ void philox_kat_kernel(Philox rng, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t* out) {
    uint32_t c[4] = {c0, c1, c2, c3};
    rng(c);
    for (int i = 0; i < 4; ++i) out[i] = c[i];
}

}  // namespace

extern "C" {

msm_status msm_sample_transition_matrices(msm_ctx* ctx, const void* d_counts, int counts_are_f64, int k,
                                          const int32_t* d_active, const int32_t* d_n_active, double alpha,
                                          uint64_t seed, int first_sample, int n_samples, double* d_T,
                                          int64_t t_stride, int ld) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d_counts && d_active && d_n_active && d_T, "msm_sample_transition_matrices: null pointer");
    MSM_REQUIRE(ctx, k >= 1 && ld >= k && t_stride >= (int64_t)k * ld, "msm_sample_transition_matrices: bad shape");
    MSM_REQUIRE(ctx, n_samples >= 0 && n_samples <= 65535 && first_sample >= 0,
                "msm_sample_transition_matrices: 0 <= n_samples <= 65535 per call");
    MSM_REQUIRE(ctx, alpha >= 0.0, "msm_sample_transition_matrices: alpha must be >= 0");
    if (n_samples == 0) return MSM_OK;
    const Philox rng{(uint32_t)seed, (uint32_t)(seed >> 32)};
    const dim3 grid((unsigned)k, (unsigned)n_samples);
    if (counts_are_f64)
        sample_rows_kernel<double><<<grid, kPT, 0, ctx->stream>>>((const double*)d_counts, k, d_active, d_n_active, alpha,
                                                                   rng, (uint32_t)first_sample, d_T, t_stride, ld);
    else
        sample_rows_kernel<long long><<<grid, kPT, 0, ctx->stream>>>((const long long*)d_counts, k, d_active, d_n_active,
                                                                      alpha, rng, (uint32_t)first_sample, d_T, t_stride, ld);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_philox4x32(msm_ctx* ctx, uint64_t key, const uint32_t counter[4], uint32_t* d_out) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, counter && d_out, "msm_philox4x32: null pointer");
    philox_kat_kernel<<<1, 1, 0, ctx->stream>>>(Philox{(uint32_t)key, (uint32_t)(key >> 32)}, counter[0], counter[1],
                                                counter[2], counter[3], d_out);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
