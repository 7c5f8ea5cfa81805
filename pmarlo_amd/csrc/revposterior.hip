// Posterior samples of the REVERSIBLE transition matrix for the implied-timescale confidence intervals.
//
// Reference: ITSMixin._its_compute_for_single_lag (S/markov_state_model/_its.py:289-312) fits deeptime's
// BayesianMSM(lagtime, n_samples), whose default is the reversible sampler: every sample obeys detailed balance,
// and _summarize_its_stats (:543-668) takes medians and percentiles over them.  deeptime is absent here (parity
// unpinned); this file samples the published law of that sampler, Trendelkamp-Schroer, Wu, Paul and Noe,
// J. Chem. Phys. 143, 174101 (2015), with their improper "-1" prior.
//
// The distribution.  C is a non-negative f64 n x n count matrix (with whatever prior the caller has added),
// c_i = sum_j C_ij.  A reversible chain is a symmetric non-negative X with x_i = sum_k x_ik,
// T_ij = x_ij / x_i and pi_i = x_i / sum x.  The target, known up to the overall scale of X, is
//     p(X | C)  ~  prod_i x_ii^(C_ii - 1)  prod_{i<j} x_ij^(C_ij + C_ji - 1)  prod_i x_i^(-c_i).
// Cells:
//   * C_ij + C_ji == 0 exactly: x_ij is pinned at 0 and never updated.
//   * diagonal, exact Gibbs: given the rest s = x_i - x_ii of row i, x_ii / x_i ~ Beta(C_ii, c_i - C_ii), drawn as
//     log x_ii = log s + log G(C_ii) - log G(c_i - C_ii); skipped when either parameter is 0.
//   * off-diagonal: with v = x_ij, v1 = x_i - x_ij, v2 = x_j - x_ij, a = C_ij + C_ji the conditional density is
//     v^(a-1) (v + v1)^(-c_i) (v + v2)^(-c_j).  In w = log v that is exp h(w),
//         h(w) = a w - c_i log(e^w + v1) - c_j log(e^w + v2),
//     strictly concave, with its mode at the positive root of
//         (c_i + c_j - a) v^2 - [a (v1 + v2) - c_i v2 - c_j v1] v - a v1 v2 = 0
//     (written so that c_i + c_j - a -> 0, two states that all but only talk to each other, loses no digits; at
//     c_i + c_j == a there is no root: the conditional is improper and only the second step below runs).
//     Two Metropolis steps, both leaving exp h invariant:
//       1. an independence proposal v' ~ Gamma(k, theta) fitted to the mode and curvature of h:
//          k = -h''(w^) = c_i v^ v1 / (v^ + v1)^2 + c_j v^ v2 / (v^ + v2)^2, theta = k / v^ (for v^ << v1, v2 this is
//          Gamma(a, c_i / v1 + c_j / v2): the conditional itself to first order).  k and theta depend on v1, v2
//          and the counts only, never on v.  Accepted with min(1, [e^h / q](w') / [e^h / q](w)),
//          log q(w) = k w - theta e^w;
//       2. a log-normal random walk w' = w + sigma z, sigma = min(k^-1/2, 8) (1 without a mode), accepted with
//          min(1, e^(h(w') - h(w))): it reaches the polynomial tails the gamma proposal is too light for.
//     Proposal and acceptance arithmetic are carried in logarithms.
// Scale and floor.  sum x is renormalised to 1 once per sweep.  Cells that carry only the prior (shape 2e-3) draw
// values far below 1e-300, so every live cell is kept in [kFloor, kCap] = [1e-280, 1e100] relative to that unit
// sum: a draw below the floor is stored AS the floor, which then stands for the whole interval (0, floor] (step 1
// compares interval masses e^(a w) / a against e^(k w) / k there; step 2 leaves a cell at the floor alone and
// rejects proposals that leave the range), a draw above the cap is rejected or cut.  The law above 1e-280 is that of
// the target; no live cell can become 0, NaN or Inf (a NaN acceptance ratio compares false and rejects).
//
// One chain per sample, one workgroup per chain.  x_ij and x_kl are conditionally independent when {i,j} and {k,l}
// are disjoint, so a sweep is: all diagonals in parallel, then the n - 1 rounds of a round-robin tournament (circle
// method; n rounds with a bye for odd n), each round updating floor(n/2) disjoint pairs in parallel, one lane per
// pair, one barrier between rounds: a fixed systematic scan.  x_i lives in LDS and is written only by the lane that
// owns a pair containing i; X is the chain's own n x ldt slot of the output (full symmetric matrix), row-normalised
// in place into T at the end.  A single wave per chain where floor(n/2) <= 64, a workgroup of 256 striding over the
// round otherwise.  Every chain starts from X0 = diag(pi0) T0 of the reversible maximum-likelihood estimate and runs
// n_sweeps sweeps.
//
// Random numbers: philox.h, keyed by the seed, counter (j, i, sample number, sweep * 1024 + purpose * 128 + attempt)
// for the cell (i <= j): a chain's draws depend on neither the launch geometry, the batch, nor other chains.
#include "common.h"
#include "philox.h"
#include "wave.h"

namespace {

constexpr double kFloor = 1e-280;
constexpr double kCap = 1e100;
constexpr double kLogFloor = -644.7238260383328;   // log(1e-280)
constexpr double kLogCap = 230.25850929940458;     // log(1e100)
constexpr uint32_t kSweepStride = 1024;            // counter words per (cell, sample, sweep)
constexpr int kMaxSweeps = 1 << 22;                // sweep * kSweepStride stays below 2^32
constexpr int kRT = 256;

// c_i = sum_j C_ij, one wave per row
__global__ __launch_bounds__(kRT) void rev_rowsum_kernel(const double* __restrict__ C, int n, int ld, double* __restrict__ c) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (kRT / 64) + (threadIdx.x >> 6);
    if (i >= n) return;
    double a = 0.0;
    for (int j = lane; j < n; j += 64) a += C[(size_t)i * ld + j];
    a = wave_sum_xor(a);
    if (lane == 0) c[i] = a;
}

// out[a, b] = counts[active[a], active[b]] + alpha, packed n_active x n_active
template <typename CT>
__global__ __launch_bounds__(kRT) void active_counts_kernel(const CT* __restrict__ counts, int k,
                                                            const int32_t* __restrict__ active,
                                                            const int32_t* __restrict__ n_active, double alpha,
                                                            double* __restrict__ out) {
    const int n = *n_active;
    const int a = blockIdx.x;
    if (a >= n) return;
    const CT* crow = counts + (size_t)active[a] * k;
    for (int b = threadIdx.x; b < n; b += kRT) out[(size_t)a * n + b] = (double)crow[active[b]] + alpha;
}

struct PairCond {   // the conditional of one off-diagonal cell
    double a, ci, cj, v1, v2;
    __device__ __forceinline__ double h(double w, double v) const { return a * w - ci * log(v + v1) - cj * log(v + v2); }
};

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void rev_chain_kernel(const double* __restrict__ C, int n, int ld,
                                                          const double* __restrict__ c, const double* __restrict__ T0,
                                                          const double* __restrict__ pi0, Philox rng, uint32_t first_sample,
                                                          int n_sweeps, double* __restrict__ T, int64_t t_stride, int ldt,
                                                          double* __restrict__ pi) {
    extern __shared__ double xs[];   // x_i: the row sums of this chain's X
    __shared__ double red[BLOCK / 64];
    __shared__ double bc;
    constexpr int NW = BLOCK / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t sample = first_sample + blockIdx.x;
    double* X = T + (int64_t)blockIdx.x * t_stride;

    // start: X0 = diag(pi0) T0, symmetrised bit for bit; pinned cells exactly 0
    for (int i = wave; i < n; i += NW) {
        double acc = 0.0;
        for (int j = lane; j < n; j += 64) {
            double x = 0.0;
            if (C[(size_t)i * ld + j] + C[(size_t)j * ld + i] > 0.0)
                x = fmin(fmax(0.5 * (pi0[i] * T0[(size_t)i * ld + j] + pi0[j] * T0[(size_t)j * ld + i]), kFloor), kCap);
            X[(size_t)i * ldt + j] = x;
            acc += x;
        }
        acc = wave_sum_xor(acc);
        if (lane == 0) xs[i] = acc;
    }
    __syncthreads();

    const int m = n + (n & 1), half = m / 2;   // players of the tournament (player n is the bye of an odd n)
    for (int sweep = 0; sweep < n_sweeps; ++sweep) {
        const uint32_t base = (uint32_t)sweep * kSweepStride;
        // ---- all diagonals: x_ii / x_i ~ Beta(C_ii, c_i - C_ii)
        for (int i = tid; i < n; i += BLOCK) {
            const double cii = C[(size_t)i * ld + i], rest = c[i] - cii;
            if (!(cii > 0.0 && rest > 0.0)) continue;
            const double s = xs[i] - X[(size_t)i * ldt + i];
            if (!(s > 0.0)) continue;
            const double lg1 = log_gamma_variate(rng, cii, (uint32_t)i, (uint32_t)i, sample, base);
            const double lg2 = log_gamma_variate(rng, rest, (uint32_t)i, (uint32_t)i, sample, base + 128);
            const double w = fmin(fmax(log(s) + fmin(lg1 - lg2, kLogCap), kLogFloor), kLogCap);
            const double x = fmin(fmax(exp(w), kFloor), kCap);
            X[(size_t)i * ldt + i] = x;
            xs[i] = s + x;
        }
        __syncthreads();
        // ---- off-diagonals, one round of disjoint pairs at a time
        for (int r = 0; r < m - 1; ++r) {
            for (int p = tid; p < half; p += BLOCK) {
                const int pa = p == 0 ? m - 1 : (r + p) % (m - 1);
                const int pb = p == 0 ? r : (r - p + (m - 1)) % (m - 1);
                if (pa >= n || pb >= n) continue;                       // the bye
                const int i = min(pa, pb), j = max(pa, pb);
                PairCond q;
                q.a = C[(size_t)i * ld + j] + C[(size_t)j * ld + i];
                if (!(q.a > 0.0)) continue;                             // pinned
                q.ci = c[i];
                q.cj = c[j];
                double v = X[(size_t)i * ldt + j];
                q.v1 = fmax(xs[i] - v, 0.0);
                q.v2 = fmax(xs[j] - v, 0.0);
                double w = v <= kFloor ? kLogFloor : log(v);   // at the floor: the interval (0, floor]
                double hw = q.h(w, v);
                uint32_t ua[4] = {(uint32_t)j, (uint32_t)i, sample, base + 256};
                rng(ua);
                // mode of h: positive root of A v^2 - B v - Cq = 0
                const double A = q.ci + q.cj - q.a;
                const double B = q.a * (q.v1 + q.v2) - q.ci * q.v2 - q.cj * q.v1;
                const double Cq = q.a * q.v1 * q.v2;
                const double disc = sqrt(B * B + 4.0 * A * Cq);
                const double vhat = B > 0.0 ? (B + disc) / (2.0 * A) : 2.0 * Cq / (disc - B);
                double sigma = 1.0;
                if (vhat > 0.0 && vhat < INFINITY) {
                    const double d1 = vhat + q.v1, d2 = vhat + q.v2;
                    const double k = q.ci * (vhat / d1) * (q.v1 / d1) + q.cj * (vhat / d2) * (q.v2 / d2);
                    if (k > 0.0 && k < INFINITY) {
                        const double ltheta = log(k) - log(vhat);
                        const double lg = log_gamma_variate(rng, k, (uint32_t)j, (uint32_t)i, sample, base);
                        double wp = lg - ltheta;
                        if (wp <= kLogCap) {
                            double vp = exp(wp);
                            if (!(vp > kFloor)) { wp = kLogFloor; vp = kFloor; }
                            const double hp = q.h(wp, vp);
                            // log [e^h / q]; at the floor the masses of (0, floor]: e^(a w) / a against e^(k w) / k
                            const double at_floor = log(k) - log(q.a);
                            const double tp = hp - (k * wp - exp(ltheta + wp)) + (vp <= kFloor ? at_floor : 0.0);
                            const double tw = hw - (k * w - exp(ltheta + w)) + (v <= kFloor ? at_floor : 0.0);
                            if (log(unit_open(ua[0], ua[1])) < tp - tw) { w = wp; v = vp; hw = hp; }
                        }
                        sigma = fmin(1.0 / sqrt(k), 8.0);
                    }
                }
                if (v > kFloor) {
                    uint32_t ub[4] = {(uint32_t)j, (uint32_t)i, sample, base + 257};
                    rng(ub);
                    const double z = sqrt(-2.0 * log(unit_open(ub[0], ub[1]))) * cospi(2.0 * unit_open(ub[2], ub[3]));
                    const double wp = w + sigma * z;
                    const double vp = exp(wp);
                    if (vp > kFloor && wp <= kLogCap) {
                        const double hp = q.h(wp, vp);
                        if (log(unit_open(ua[2], ua[3])) < hp - hw) { w = wp; v = vp; }
                    }
                }
                v = fmin(fmax(v, kFloor), kCap);
                X[(size_t)i * ldt + j] = v;
                X[(size_t)j * ldt + i] = v;
                xs[i] = q.v1 + v;
                xs[j] = q.v2 + v;
            }
            __syncthreads();
        }
        // ---- sum x = 1.  Any common factor is a valid rescaling, so the tracked row sums give it; the row sums
        // themselves are then recomputed exactly from the rescaled cells.
        double part = 0.0;
        for (int i = tid; i < n; i += BLOCK) part += xs[i];
        const double tot = block_sum_bcast(part, red, &bc);
        const double scale = (tot > 0.0 && tot < INFINITY) ? 1.0 / tot : 1.0;
        for (int i = wave; i < n; i += NW) {
            double acc = 0.0;
            for (int j = lane; j < n; j += 64) {
                double x = X[(size_t)i * ldt + j];
                if (x > 0.0) {
                    x = fmin(fmax(x * scale, kFloor), kCap);
                    X[(size_t)i * ldt + j] = x;
                }
                acc += x;
            }
            acc = wave_sum_xor(acc);
            if (lane == 0) xs[i] = acc;
        }
        __syncthreads();
    }

    // T_ij = x_ij / x_i in place, pi_i = x_i / sum x
    double part = 0.0;
    for (int i = tid; i < n; i += BLOCK) part += xs[i];
    const double tot = block_sum_bcast(part, red, &bc);
    for (int i = wave; i < n; i += NW) {
        const double xi = xs[i];
        // a state without any flux keeps a self-loop (cannot happen on a connected count matrix)
        for (int j = lane; j < n; j += 64)
            X[(size_t)i * ldt + j] = xi > 0.0 ? X[(size_t)i * ldt + j] / xi : (j == i ? 1.0 : 0.0);
        if (lane == 0 && pi) pi[(size_t)blockIdx.x * n + i] = xi / tot;
    }
}

template <int BLOCK>
msm_status launch_chains(msm_ctx* ctx, const double* d_counts, int n, int ld, const double* c, const double* d_T0,
                         const double* d_pi0, Philox rng, int first_sample, int n_samples, int n_sweeps, double* d_T,
                         int64_t t_stride, int ldt, double* d_pi) {
    const size_t lds = (size_t)n * sizeof(double);
    if (lds > 48 * 1024)
        MSM_HIP(ctx, hipFuncSetAttribute((const void*)rev_chain_kernel<BLOCK>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds));
    rev_chain_kernel<BLOCK><<<(unsigned)n_samples, BLOCK, lds, ctx->stream>>>(d_counts, n, ld, c, d_T0, d_pi0, rng,
                                                                             (uint32_t)first_sample, n_sweeps, d_T,
                                                                             t_stride, ldt, d_pi);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // namespace

extern "C" {

msm_status msm_sample_reversible_transition_matrices(msm_ctx* ctx, const double* d_counts, int n, int ld,
                                                     const double* d_T0, const double* d_pi0, uint64_t seed,
                                                     int first_sample, int n_samples, int n_sweeps, double* d_T,
                                                     int64_t t_stride, int ldt, double* d_pi) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d_counts && d_T0 && d_pi0 && d_T, "msm_sample_reversible_transition_matrices: null pointer");
    MSM_REQUIRE(ctx, n >= 1 && ld >= n && ldt >= n && t_stride >= (int64_t)n * ldt,
                "msm_sample_reversible_transition_matrices: bad shape");
    MSM_REQUIRE(ctx, n_samples >= 0 && n_samples <= 65535 && first_sample >= 0,
                "msm_sample_reversible_transition_matrices: 0 <= n_samples <= 65535 per call");
    MSM_REQUIRE(ctx, n_sweeps >= 0 && n_sweeps < kMaxSweeps,
                "msm_sample_reversible_transition_matrices: 0 <= n_sweeps < %d", kMaxSweeps);
    if ((size_t)n * sizeof(double) > 96 * 1024)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_sample_reversible_transition_matrices: n = %d exceeds the LDS table", n);
    if (n_samples == 0) return MSM_OK;
    msm_status rs = msm_reserve_scratch(ctx, (size_t)n * sizeof(double));
    if (rs != MSM_OK) return rs;
    double* c = (double*)ctx->scratch;
    rev_rowsum_kernel<<<(unsigned)msm_ceil_div(n, kRT / 64), kRT, 0, ctx->stream>>>(d_counts, n, ld, c);
    MSM_CHECK_LAUNCH(ctx);
    const Philox rng{(uint32_t)seed, (uint32_t)(seed >> 32)};
    if (n / 2 <= 64)
        return launch_chains<64>(ctx, d_counts, n, ld, c, d_T0, d_pi0, rng, first_sample, n_samples, n_sweeps, d_T, t_stride,
                                 ldt, d_pi);
    return launch_chains<kRT>(ctx, d_counts, n, ld, c, d_T0, d_pi0, rng, first_sample, n_samples, n_sweeps, d_T, t_stride,
                              ldt, d_pi);
}

msm_status msm_active_counts(msm_ctx* ctx, const void* d_counts, int counts_are_f64, int k, const int32_t* d_active,
                             const int32_t* d_n_active, double alpha, double* d_out) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d_counts && d_active && d_n_active && d_out, "msm_active_counts: null pointer");
    MSM_REQUIRE(ctx, k >= 1 && alpha >= 0.0, "msm_active_counts: need k >= 1 and alpha >= 0");
    if (counts_are_f64)
        active_counts_kernel<double><<<(unsigned)k, kRT, 0, ctx->stream>>>((const double*)d_counts, k, d_active, d_n_active,
                                                                         alpha, d_out);
    else
        active_counts_kernel<long long><<<(unsigned)k, kRT, 0, ctx->stream>>>((const long long*)d_counts, k, d_active,
                                                                            d_n_active, alpha, d_out);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
