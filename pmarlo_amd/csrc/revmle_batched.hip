// Batched reversible maximum-likelihood estimate from raw resampled counts, and the kinetic importance scores of a
// batch of spectra.
//
// Reference: KineticImportanceScore.bootstrap_stability / _rebuild_msm (S/conformations/kinetic_importance.py:209-315)
// rebuilds one MSM per trajectory resample: ensure_connected_counts (active set, prior 1e-3 on every active cell),
// then deeptime's MaximumLikelihoodMSM(reversible=True), absent here (parity unpinned).  The estimator is the fixed
// point in the header comment of revmle.hip, iterated on the row sums alone.
//
// msm_reversible_mle (revmle.hip) spends one launch per iteration and polls the host; for a few hundred resamples of
// one or two thousand iterations each that is launch-bound.  Here a matrix belongs to ONE workgroup of 16 waves, which
// finds the active set, packs the symmetrised block C2 = (C + alpha) + (C + alpha)', and iterates to its own
// convergence inside one launch: two barriers per iteration, no host round trip, capturable.
//
//   row phase     wave w owns the rows w, w + 16, ..: xn_a = sum_b C2_ab / (v_a + v_b), lanes over b (stride 64,
//                 ascending), then the VALU butterfly (wave_sum_all)
//   barrier
//   normalise     every wave sums xn itself in the same fixed order (same bits in every wave, no barrier), thread t
//                 owns state t: x_t = xn_t / total, its term of the stopping measure, v_t = c_t / x_t; the wave
//                 maxima meet in LDS
//   barrier
//
// Nothing in the order of the sums depends on the workgroup's neighbours, on the path or on the number of waves: a
// matrix has the same bits whatever batch it is solved in.
//
// Where C2 lives: k <= kLdsMaxN keeps the packed block in LDS (k * k * 8 bytes next to five k-vectors and the index
// lists: 151 KiB of the 160 KiB a gfx950 workgroup may declare at k = 136); above, C2 is slab b of the context
// scratch and every iteration streams it (320 KB at k = 200: the slabs of a batch that fills the chip live in L2 and
// the Infinity Cache).  One workgroup per CU either way: a batch of resamples has about as many matrices as the chip
// has CUs, and 16 waves of fp64 divisions keep the four SIMDs of a CU busy (the division, ~12 VALU operations, is the
// arithmetic bound: n^2 of them per iteration).
#include "common.h"
#include "wave.h"

namespace {

constexpr int kBT = 1024;            // threads of a matrix's workgroup
constexpr int kBW = kBT / 64;
constexpr int kLdsMaxN = 136;        // largest k whose packed C2 stays in LDS
constexpr int kMaxK = 2048;          // the k-vectors and index lists of the streaming path: 97 KiB of LDS

__host__ __device__ constexpr size_t revmle_lds_bytes(int k, bool lds) {
    return ((size_t)5 * k + kBW + (lds ? (size_t)k * k : 0)) * sizeof(double) + ((size_t)2 * k + 2) * sizeof(int);
}
static_assert(revmle_lds_bytes(kLdsMaxN, true) <= 160 * 1024, "the LDS path must fit one workgroup's 160 KiB");
static_assert(revmle_lds_bytes(kMaxK, false) <= 160 * 1024, "the streaming path's vectors must fit LDS");

// sum of xn[0..n) by one wave, lanes over i (stride 64, ascending), then the VALU butterfly: the same bits in every
// lane of every wave
__device__ __forceinline__ double wave_total(const double* xn, int n, int lane) {
    double part = 0.0;
    for (int i = lane; i < n; i += 64) part += xn[i];
    return wave_sum_all(part);
}

template <bool kLds>
__global__ __launch_bounds__(kBT) void revmle_batched_kernel(const long long* __restrict__ counts, int k, double alpha,
                                                             double maxerr, int maxiter, double* __restrict__ scratch,
                                                             double* __restrict__ T_all, size_t t_stride, int ld,
                                                             double* __restrict__ pi_all, int* __restrict__ active_all,
                                                             int* __restrict__ n_active_all,
                                                             int* __restrict__ iterations_all,
                                                             double* __restrict__ err_all) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double* c = sm;                 // row sums of the regularised active block
    double* v = c + k;              // c_j / x_j of the current iterate
    double* xn = v + k;             // unnormalised new row sums
    double* xc = xn + k;            // current iterate (normalised)
    double* xo = xc + k;            // the other buffer of the pair
    double* red = xo + k;           // one slot per wave
    double* C2 = kLds ? red + kBW : scratch + (size_t)b * k * k;
    int* flag = (int*)(red + kBW + (kLds ? (size_t)k * k : 0));
    int* act = flag + k;            // packed index -> state
    int* meta = act + k;            // {n_active, a negative count was seen}
    const long long* C = counts + (size_t)b * k * k;
    double* T = T_all + (size_t)b * t_stride;

    // active set: rowsum_i + colsum_i > 1e-12 (integers: exact in any order)
    if (tid == 0) { meta[0] = 0; meta[1] = 0; }
    __syncthreads();
    for (int j = tid; j < k; j += kBT) {
        long long s = 0;
        bool neg = false;
        for (int i = 0; i < k; ++i) {
            const long long down = C[(size_t)i * k + j], along = C[(size_t)j * k + i];
            s += down + along;
            neg |= down < 0;        // thread j sees the whole column j
        }
        flag[j] = (double)s > 1e-12;
        if (neg) meta[1] = 1;
    }
    __syncthreads();
    if (wave == 0) {                // ascending compaction: ballot and prefix count, 64 states a step
        int base = 0;
        for (int j0 = 0; j0 < k; j0 += 64) {
            const int j = j0 + lane;
            const bool on = j < k && flag[j] != 0;
            const unsigned long long mask = __ballot(on);
            if (on) act[base + __popcll(mask & ((1ull << lane) - 1ull))] = j;
            base += __popcll(mask);
        }
        if (lane == 0) meta[0] = base;
    }
    __syncthreads();
    const int n = meta[0];
    const bool negative = meta[1] != 0;
    for (int j = tid; j < k; j += kBT) {
        active_all[(size_t)b * k + j] = j < n ? act[j] : -1;
        pi_all[(size_t)b * k + j] = 0.0;
    }
    if (tid == 0) n_active_all[b] = n;
    if (n == 0 || negative) {       // uniform over the workgroup
        for (size_t e = tid; e < (size_t)k * k; e += kBT) T[(e / k) * ld + e % k] = 0.0;
        if (tid == 0) {
            iterations_all[b] = 0;
            err_all[b] = negative ? INFINITY : 0.0;
        }
        return;
    }

    // C2 = (C + alpha) + (C + alpha)' on the active block, c = its row sums before symmetrising, start = row sums of C2
    for (int a = wave; a < n; a += kBW) {
        const size_t ia = (size_t)act[a];
        double cs = 0.0, xs = 0.0;
        for (int q = lane; q < n; q += 64) {
            const size_t iq = (size_t)act[q];
            const double f = (double)C[ia * k + iq] + alpha, g = (double)C[iq * k + ia] + alpha;
            const double s = f + g;
            C2[(size_t)a * n + q] = s;
            cs += f;
            xs += s;
        }
        cs = wave_sum_all(cs);
        xs = wave_sum_all(xs);
        if (lane == 0) { c[a] = cs; xn[a] = xs; }
    }
    __syncthreads();
    {
        const double tot = wave_total(xn, n, lane);
        for (int t = tid; t < n; t += kBT) {
            const double x = xn[t] / tot;
            xc[t] = x;
            v[t] = x > 0.0 ? c[t] / x : 0.0;
        }
    }
    __syncthreads();

    int it = 0;
    double err = INFINITY;
    while (true) {
        for (int a = wave; a < n; a += kBW) {
            const double va = v[a];
            const double* row = C2 + (size_t)a * n;
            double acc = 0.0;
            for (int q = lane; q < n; q += 64) {
                const double c2 = row[q], den = va + v[q];
                if (c2 > 0.0 && den > 0.0) acc += c2 / den;
            }
            acc = wave_sum_all(acc);
            if (lane == 0) xn[a] = acc;
        }
        __syncthreads();
        const double tot = wave_total(xn, n, lane);
        double worst = 0.0;
        for (int t = tid; t < n; t += kBT) {
            const double x = xn[t] / tot, old = xc[t];
            const double mid = 0.5 * (old + x);
            if (mid > 0.0) worst = fmax(worst, fabs(old - x) / mid);
            if (!(x == x)) worst = INFINITY;
            xo[t] = x;
            v[t] = x > 0.0 ? c[t] / x : 0.0;
        }
        worst = wave_max_xor(worst);
        if (lane == 0) red[wave] = worst;
        __syncthreads();
        err = 0.0;
        for (int w = 0; w < kBW; ++w) err = fmax(err, red[w]);
        double* sw = xc; xc = xo; xo = sw;
        ++it;
        // the measure is bounded by 2: above it the iterate is NaN and stays NaN
        if (!(err > maxerr) || !(err <= 4.0) || it >= maxiter) break;
    }

    // T_ab = x_ab / sum_b x_ab with x_ab of the final iterate, packed in the top-left corner; zeros around it
    for (int a = wave; a < n; a += kBW) {
        const double va = v[a];
        const double* row = C2 + (size_t)a * n;
        double acc = 0.0;
        for (int q = lane; q < n; q += 64) {
            const double c2 = row[q], den = va + v[q];
            if (c2 > 0.0 && den > 0.0) acc += c2 / den;
        }
        acc = wave_sum_all(acc);
        for (int q = lane; q < n; q += 64) {
            const double c2 = row[q], den = va + v[q];
            const double f = (c2 > 0.0 && den > 0.0) ? c2 / den : 0.0;
            // a state without any flux keeps a self-loop (cannot happen with alpha > 0)
            T[(size_t)a * ld + q] = acc > 0.0 ? f / acc : (q == a ? 1.0 : 0.0);
        }
    }
    for (size_t e = tid; e < (size_t)k * k; e += kBT) {
        const size_t r = e / k, q = e % k;
        if (r >= (size_t)n || q >= (size_t)n) T[r * ld + q] = 0.0;
    }
    for (int t = tid; t < n; t += kBT) pi_all[(size_t)b * k + t] = xc[t];
    if (tid == 0) {
        iterations_all[b] = it;
        err_all[b] = err;
    }
}

constexpr int kKisThreads = 256;

__global__ __launch_bounds__(kKisThreads) void kis_scores_kernel(const double* __restrict__ vecs, int n_vecs, int k,
                                                                 const double* __restrict__ pi,
                                                                 const int* __restrict__ active,
                                                                 const int* __restrict__ n_active, int k_slow,
                                                                 double* __restrict__ scores, int* __restrict__ info) {
    __shared__ int nan_seen;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = n_active[b];
    if (tid == 0) nan_seen = 0;
    for (int j = tid; j < k; j += kKisThreads) scores[(size_t)b * k + j] = 0.0;
    __syncthreads();
    if (n <= k_slow || n > k) {     // uniform over the workgroup
        if (tid == 0) info[b] = 1;
        return;
    }
    const double* V = vecs + (size_t)b * n_vecs * k;
    for (int a = tid; a < n; a += kKisThreads) {
        double s = 0.0;
        for (int m = 1; m <= k_slow; ++m) {
            const double x = V[(size_t)m * k + a];
            s += x * x;
        }
        const int state = active[(size_t)b * k + a];
        if (!(s == s)) nan_seen = 1;
        else if (state >= 0 && state < k) scores[(size_t)b * k + state] = pi[(size_t)b * k + a] * s;
    }
    __syncthreads();
    if (tid == 0) info[b] = nan_seen ? 2 : 0;
}

}  // namespace

extern "C" {

int msm_reversible_mle_batched_lds_max_n(void) { return kLdsMaxN; }

size_t msm_reversible_mle_batched_scratch_bytes(int k, int batch) {
    if (k <= kLdsMaxN || batch < 1) return 0;
    return (size_t)batch * k * k * sizeof(double);
}

msm_status msm_reversible_mle_batched(msm_ctx* ctx, const int64_t* d_counts, int k, int batch, double alpha, double maxerr,
                                      int maxiter, double* d_T, int64_t t_stride, int ld, double* d_pi,
                                      int32_t* d_active, int32_t* d_n_active, int32_t* d_iterations, double* d_err) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d_counts && d_T && d_pi && d_active && d_n_active && d_iterations && d_err,
                "msm_reversible_mle_batched: NULL pointer");
    MSM_REQUIRE(ctx, k >= 1 && batch >= 1 && ld >= k && (batch == 1 || t_stride >= (int64_t)(k - 1) * ld + k),
                "msm_reversible_mle_batched: bad shape");
    MSM_REQUIRE(ctx, alpha >= 0.0 && maxerr > 0.0 && maxiter >= 1,
                "msm_reversible_mle_batched: need alpha >= 0, maxerr > 0 and maxiter >= 1");
    if (k > kMaxK)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_reversible_mle_batched: k = %d exceeds the LDS tables (%d)", k, kMaxK);
    const bool lds = k <= kLdsMaxN;
    msm_status rs = msm_reserve_scratch(ctx, msm_reversible_mle_batched_scratch_bytes(k, batch));
    if (rs != MSM_OK) return rs;
    const size_t bytes = revmle_lds_bytes(k, lds);
    if (lds) {
        if (bytes > 48 * 1024)
            MSM_HIP(ctx, hipFuncSetAttribute((const void*)revmle_batched_kernel<true>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        hipLaunchKernelGGL(revmle_batched_kernel<true>, dim3((unsigned)batch), dim3(kBT), bytes, ctx->stream,
                           (const long long*)d_counts, k, alpha, maxerr, maxiter, (double*)nullptr, d_T, (size_t)t_stride, ld,
                           d_pi, d_active, d_n_active, d_iterations, d_err);
    } else {
        if (bytes > 48 * 1024)
            MSM_HIP(ctx, hipFuncSetAttribute((const void*)revmle_batched_kernel<false>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        hipLaunchKernelGGL(revmle_batched_kernel<false>, dim3((unsigned)batch), dim3(kBT), bytes, ctx->stream,
                           (const long long*)d_counts, k, alpha, maxerr, maxiter, (double*)ctx->scratch, d_T,
                           (size_t)t_stride, ld, d_pi, d_active, d_n_active, d_iterations, d_err);
    }
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_kis_scores(msm_ctx* ctx, const double* d_vecs, int n_vecs, int k, int batch, const double* d_pi,
                          const int32_t* d_active, const int32_t* d_n_active, int k_slow, double* d_scores,
                          int32_t* d_info) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d_vecs && d_pi && d_active && d_n_active && d_scores && d_info, "msm_kis_scores: NULL pointer");
    MSM_REQUIRE(ctx, k >= 1 && batch >= 1 && k_slow >= 1 && n_vecs >= k_slow + 1,
                "msm_kis_scores: need k >= 1, batch >= 1, k_slow >= 1 and n_vecs >= k_slow + 1");
    hipLaunchKernelGGL(kis_scores_kernel, dim3((unsigned)batch), dim3(kKisThreads), 0, ctx->stream, d_vecs, n_vecs, k, d_pi,
                       d_active, d_n_active, k_slow, d_scores, d_info);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
