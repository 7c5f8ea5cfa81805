// Trajectory bootstrap in batch: resample counts as integer combinations of per-trajectory counts, row-normalise
// the batch, and solve the committor systems of every sample at once.
//
// Reference: UncertaintyQuantifier (S/conformations/uncertainty.py:31-261, _rebuild_msm :506-530) resamples whole
// trajectories with replacement, recounts and rebuilds the MSM per sample, then runs TPTAnalysis on it.  Transition
// counts are additive over trajectories, so the count matrix of a resample is sum_s mult[b, s] * C_s with C_s counted
// once (msm_count_transitions per segment); the TPT numerics are those of msm_reactive_flux (csrc/tpt.hip).
//
// flux_batched_kernel keeps solve_kernel's arithmetic per element: the first row of maximal modulus is the pivot,
// l = a_ik / pivot, a_ij <- fma(-l, a_kj, a_ij), x_k = b_k / u_kk, b_i <- fma(-u_ik, x_k, b_i).  Every element's chain of
// updates is fixed by (n, the system) alone, so the committors have the bits msm_reactive_flux gives for that matrix.
#include <algorithm>

#include "common.h"
#include "wave.h"

namespace {

// ---- C_b = sum_s mult[b, s] * C_s -------------------------------------------------------------------------------
constexpr int kCombineThreads = 256;

// A thread owns one cell: its S per-segment values are read once into registers, then the samples of this
// blockIdx.y stream past (the multiplicities of a sample are wave-uniform loads).  One store per output, no atomics.
template <int S>
__global__ __launch_bounds__(kCombineThreads) void combine_counts_kernel(const long long* __restrict__ seg,
                                                                        const int* __restrict__ mult, int64_t ld_mult,
                                                                        int n_seg, int n_boot, int64_t cells,
                                                                        long long* __restrict__ out, int accumulate) {
    const int64_t c = (int64_t)blockIdx.x * kCombineThreads + threadIdx.x;
    const bool live = c < cells;
    long long v[S];
#pragma unroll
    for (int s = 0; s < S; ++s) v[s] = (live && s < n_seg) ? seg[(size_t)s * cells + c] : 0;
    for (int b = blockIdx.y; b < n_boot; b += gridDim.y) {
        const int* m = mult + (size_t)b * ld_mult;
        long long acc = 0;
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (s < n_seg) acc += (long long)m[s] * v[s];
        if (live) {
            long long* o = out + (size_t)b * cells + c;
            *o = accumulate ? *o + acc : acc;
        }
    }
}

// ---- T = C / row sum over a batch ----------------------------------------------------------------------------------
constexpr int kNormThreads = 256;

// One wave per row of the [batch * k, k] stack: the row sum in int64 (exact), then the IEEE quotient of the two
// integers converted to double (numpy's C / rowsum); an all-zero row stays zero.
__global__ __launch_bounds__(kNormThreads) void row_normalise_batched_kernel(const long long* __restrict__ C, int k,
                                                                            int64_t rows, double* __restrict__ T,
                                                                            long long* __restrict__ rowsum) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kNormThreads / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;                       // wave-uniform
    const long long* c = C + (size_t)row * k;
    long long s = 0;
    for (int j = lane; j < k; j += 64) s += c[j];
    s = wave_sum_down(s);
    s = __shfl(s, 0, 64);
    if (lane == 0) rowsum[row] = s;
    const double rs = (double)s;
    for (int j = lane; j < k; j += 64) T[(size_t)row * k + j] = s > 0 ? (double)c[j] / rs : 0.0;
}

// ---- committors and flux totals, one workgroup per sample --------------------------------------------------------
constexpr int kFluxThreads = 512;
constexpr int kFluxWaves = kFluxThreads / 64;
constexpr size_t kFluxLdsBytes = 128 * 1024;       // W [n, n] and the right-hand side [n] of one system
static_assert(((size_t)MSM_FLUX_LDS_MAX_N * MSM_FLUX_LDS_MAX_N + MSM_FLUX_LDS_MAX_N) * sizeof(double) <= kFluxLdsBytes &&
                  ((size_t)(MSM_FLUX_LDS_MAX_N + 1) * (MSM_FLUX_LDS_MAX_N + 1) + MSM_FLUX_LDS_MAX_N + 1) * sizeof(double) >
                      kFluxLdsBytes,
              "MSM_FLUX_LDS_MAX_N is the largest n whose system fits kFluxLdsBytes");

struct FluxShared {
    double val[kFluxWaves];
    int idx[kFluxWaves];
    int piv;
    int singular;
    double red[kFluxWaves];
};

// W x = r for the workgroup's system (W [n, n] packed, both destroyed); x goes to `x` (global).  Returns 0 or the
// 1-based column without a non-zero pivot, the same in every thread.  The factors below the diagonal are not kept.
__device__ __forceinline__ int flux_solve(double* W, double* r, int n, double* __restrict__ x, FluxShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) sh.singular = 0;
    __syncthreads();                               // the system is complete, the flag is clear
    for (int k = 0; k < n; ++k) {
        // pivot: first row of maximal |W[i][k]|, i >= k
        double best = -1.0;
        int bi = k;
        for (int i = k + tid; i < n; i += kFluxThreads) {
            const double v = fabs(W[(size_t)i * n + k]);
            if (v > best) { best = v; bi = i; }
        }
        wave_argmax_down(best, bi);
        if (lane == 0) { sh.val[wave] = best; sh.idx[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kFluxWaves; ++w)
                if (sh.val[w] > best || (sh.val[w] == best && sh.idx[w] < bi)) { best = sh.val[w]; bi = sh.idx[w]; }
            sh.piv = bi;
            if (!(best > 0.0)) sh.singular = k + 1;
        }
        __syncthreads();
        if (sh.singular) break;
        const int p = sh.piv;
        if (p != k) {                              // columns < k hold nothing that is read again
            for (int j = k + tid; j <= n; j += kFluxThreads) {
                double* a = j < n ? &W[(size_t)k * n + j] : &r[k];
                double* b = j < n ? &W[(size_t)p * n + j] : &r[p];
                const double t = *a; *a = *b; *b = t;
            }
            __syncthreads();
        }
        // a wave per trailing row: l = W[i][k] / pivot, row i <- row i - l * row k, r likewise
        const double pivot = W[(size_t)k * n + k];
        const double rk = r[k];
        for (int i = k + 1 + wave; i < n; i += kFluxWaves) {
            const double l = W[(size_t)i * n + k] / pivot;
            for (int j = k + 1 + lane; j < n; j += 64)
                W[(size_t)i * n + j] = fma(-l, W[(size_t)k * n + j], W[(size_t)i * n + j]);
            if (lane == 0) r[i] = fma(-l, rk, r[i]);
        }
        __syncthreads();
    }
    const int singular = sh.singular;
    if (singular) return singular;
    // back substitution, column-oriented: x_k = r_k / u_kk, then r_i -= u_ik x_k for i < k.  r_k itself is final
    // once step k + 1 is done and is not written again, so one barrier a step suffices.
    for (int k = n - 1; k >= 0; --k) {
        const double xk = r[k] / W[(size_t)k * n + k];
        if (tid == 0) x[k] = xk;
        for (int i = tid; i < k; i += kFluxThreads) r[i] = fma(-W[(size_t)i * n + k], xk, r[i]);
        __syncthreads();
    }
    return 0;
}

// committor_system_kernel's entries (csrc/tpt.hip).  role[i]: 0 intermediate, 1 source (A), 2 sink (B).
__device__ __forceinline__ void flux_system(const double* __restrict__ T, int64_t ldt, const double* __restrict__ pi,
                                            const int* __restrict__ role, int n, int backward, double* W, double* r) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the wave index walks the row of T that is read, so that both systems read T along its rows
    for (int o = wave; o < n; o += kFluxWaves)
        for (int l = lane; l < n; l += 64) {
            const int i = backward ? l : o, j = backward ? o : l;
            double v;
            if (role[i] != 0) v = i == j ? 1.0 : 0.0;
            else if (!backward) v = T[(size_t)i * ldt + j] - (i == j ? 1.0 : 0.0);
            else v = pi[j] * T[(size_t)j * ldt + i] / pi[i] - (i == j ? 1.0 : 0.0);
            W[(size_t)i * n + j] = v;
        }
    for (int i = threadIdx.x; i < n; i += kFluxThreads) r[i] = (backward ? role[i] == 1 : role[i] == 2) ? 1.0 : 0.0;
}

__device__ __forceinline__ void flux_sample(const double* __restrict__ T, int64_t ldt, const double* __restrict__ pi,
                                            const int* __restrict__ role, int n, double* W, double* r,
                                            double* __restrict__ qp, double* __restrict__ qm,
                                            double* __restrict__ totals, int* __restrict__ info, FluxShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bad = 0;
    for (int backward = 0; backward < 2; ++backward) {
        double* q = backward ? qm : qp;
        flux_system(T, ldt, pi, role, n, backward, W, r);
        const int s = flux_solve(W, r, n, q, sh);
        if (s)
            for (int i = tid; i < n; i += kFluxThreads) q[i] = __builtin_nan("");
        if (tid == 0) info[backward] = s;
        bad |= s;
        __syncthreads();                           // W, r and the flag are free again; q is visible to the workgroup
    }
    if (!totals) return;
    // F = sum_{i in A, j not in A} pi_i q-_i T_ij q+_j and Z = sum_i pi_i q-_i: per thread in ascending (i, j), then
    // the waves in ascending order (block_sum_lane0)
    double f = 0.0, z = 0.0;
    if (!bad) {
        for (int i = wave; i < n; i += kFluxWaves) {
            if (role[i] != 1) continue;
            const double w = pi[i] * qm[i];
            for (int j = lane; j < n; j += 64)
                if (role[j] != 1) f += w * T[(size_t)i * ldt + j] * qp[j];
        }
        for (int i = tid; i < n; i += kFluxThreads) z = fma(pi[i], qm[i], z);
    }
    const double F = block_sum_lane0(f, sh.red);
    __syncthreads();
    const double Z = block_sum_lane0(z, sh.red);
    if (tid == 0) {
        const double nan = __builtin_nan("");
        totals[0] = bad ? nan : F;
        totals[1] = bad ? nan : Z;
        totals[2] = bad ? nan : F / Z;
        totals[3] = bad ? nan : Z / F;
    }
}

// kLds: the system lives in dynamic LDS ((n * n + n) doubles); otherwise in slab `blockIdx.x` of `slabs`.
template <bool kLds>
__global__ __launch_bounds__(kFluxThreads) void flux_batched_kernel(const double* __restrict__ T, int64_t t_stride,
                                                                   int64_t ldt, const double* __restrict__ pi,
                                                                   const int* __restrict__ role, int n,
                                                                   double* __restrict__ slabs, double* __restrict__ qp,
                                                                   double* __restrict__ qm, double* __restrict__ totals,
                                                                   int* __restrict__ info) {
    extern __shared__ double flux_lds[];
    __shared__ FluxShared sh;
    const size_t b = blockIdx.x, sys = (size_t)n * n;
    const double* Tb = T + b * t_stride;
    const double* pib = pi + b * n;
    double* tb = totals ? totals + 4 * b : nullptr;
    if constexpr (kLds)
        flux_sample(Tb, ldt, pib, role, n, flux_lds, flux_lds + sys, qp + b * n, qm + b * n, tb, info + 2 * b, sh);
    else
        flux_sample(Tb, ldt, pib, role, n, slabs + b * (sys + n), slabs + b * (sys + n) + sys, qp + b * n, qm + b * n, tb,
                    info + 2 * b, sh);
}

template <int S>
void launch_combine(msm_ctx* ctx, dim3 grid, const int64_t* seg, const int32_t* mult, int64_t ld_mult, int n_seg,
                    int n_boot, int64_t cells, int64_t* out, int accumulate) {
    hipLaunchKernelGGL(combine_counts_kernel<S>, grid, dim3(kCombineThreads), 0, ctx->stream, (const long long*)seg, mult,
                       ld_mult, n_seg, n_boot, cells, (long long*)out, accumulate);
}

}  // namespace

extern "C" {

msm_status msm_combine_counts(msm_ctx* ctx, const int64_t* d_seg_counts, const int32_t* d_mult, int64_t ld_mult, int n_seg,
                              int n_boot, int64_t cells, int64_t* d_counts, int accumulate) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, n_seg >= 1 && n_seg <= MSM_COMBINE_MAX_SEG && n_boot >= 1 && cells >= 1 && ld_mult >= n_seg,
                "msm_combine_counts: bad shape (1 <= n_seg <= %d per call)", MSM_COMBINE_MAX_SEG);
    MSM_REQUIRE(ctx, d_seg_counts && d_mult && d_counts, "msm_combine_counts: NULL pointer");
    const int64_t bx = (cells + kCombineThreads - 1) / kCombineThreads;
    MSM_REQUIRE(ctx, bx <= 0x7fffffff, "msm_combine_counts: too many cells");
    // few cells: the samples are dealt over blockIdx.y until the grid has a few workgroups per CU (the per-segment
    // values of a cell tile are then read once per y, from the L2 after the first)
    const int by = (int)std::min<int64_t>(std::min(n_boot, 65535), std::max<int64_t>(1, (4 * (int64_t)ctx->n_cu) / bx));
    const dim3 grid((unsigned)bx, (unsigned)by);
    if (n_seg <= 4) launch_combine<4>(ctx, grid, d_seg_counts, d_mult, ld_mult, n_seg, n_boot, cells, d_counts, accumulate);
    else if (n_seg <= 8) launch_combine<8>(ctx, grid, d_seg_counts, d_mult, ld_mult, n_seg, n_boot, cells, d_counts, accumulate);
    else if (n_seg <= 16) launch_combine<16>(ctx, grid, d_seg_counts, d_mult, ld_mult, n_seg, n_boot, cells, d_counts, accumulate);
    else launch_combine<MSM_COMBINE_MAX_SEG>(ctx, grid, d_seg_counts, d_mult, ld_mult, n_seg, n_boot, cells, d_counts, accumulate);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_row_normalise_batched(msm_ctx* ctx, const int64_t* d_counts, int k, int batch, double* d_T,
                                     int64_t* d_rowsum) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, k >= 1 && batch >= 1, "msm_row_normalise_batched: bad shape");
    MSM_REQUIRE(ctx, d_counts && d_T && d_rowsum, "msm_row_normalise_batched: NULL pointer");
    const int64_t rows = (int64_t)batch * k, blocks = (rows + kNormThreads / 64 - 1) / (kNormThreads / 64);
    MSM_REQUIRE(ctx, blocks <= 0x7fffffff, "msm_row_normalise_batched: too many rows");
    hipLaunchKernelGGL(row_normalise_batched_kernel, dim3((unsigned)blocks), dim3(kNormThreads), 0, ctx->stream,
                       (const long long*)d_counts, k, rows, d_T, (long long*)d_rowsum);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

size_t msm_reactive_flux_batched_scratch_bytes(int n, int batch, int want_committors) {
    if (n < 1 || batch < 1) return 0;
    const size_t slab = n > MSM_FLUX_LDS_MAX_N ? (size_t)n * n + n : 0;
    return (size_t)batch * (slab + (want_committors ? 0 : 2 * (size_t)n)) * sizeof(double);
}

msm_status msm_reactive_flux_batched(msm_ctx* ctx, const double* d_T, int64_t t_stride, int64_t ldt, const double* d_pi,
                                     const int32_t* d_role, int n, int batch, double* d_qplus, double* d_qminus,
                                     double* d_totals, int32_t* d_info) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, n >= 2 && ldt >= n && batch >= 1 && (batch == 1 || t_stride >= (int64_t)(n - 1) * ldt + n),
                "msm_reactive_flux_batched: bad shape");
    MSM_REQUIRE(ctx, d_T && d_pi && d_role && d_info, "msm_reactive_flux_batched: NULL pointer");
    MSM_REQUIRE(ctx, (d_qplus == nullptr) == (d_qminus == nullptr) && (d_qplus || d_totals),
                "msm_reactive_flux_batched: the committors come together, and without them the totals are required");
    const bool lds = n <= MSM_FLUX_LDS_MAX_N;
    const size_t slab = lds ? 0 : (size_t)n * n + n;
    msm_status rs = msm_reserve_scratch(ctx, msm_reactive_flux_batched_scratch_bytes(n, batch, d_qplus != nullptr));
    if (rs != MSM_OK) return rs;
    double* slabs = (double*)ctx->scratch;
    double* q = slabs + (size_t)batch * slab;      // committors nobody asked for
    double* qp = d_qplus ? d_qplus : q;
    double* qm = d_qminus ? d_qminus : q + (size_t)batch * n;
    if (lds) {
        const size_t bytes = ((size_t)n * n + n) * sizeof(double);
        if (bytes > 48 * 1024)
            MSM_HIP(ctx, hipFuncSetAttribute((const void*)flux_batched_kernel<true>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        hipLaunchKernelGGL(flux_batched_kernel<true>, dim3((unsigned)batch), dim3(kFluxThreads), bytes, ctx->stream, d_T,
                           t_stride, ldt, d_pi, d_role, n, slabs, qp, qm, d_totals, d_info);
    } else {
        hipLaunchKernelGGL(flux_batched_kernel<false>, dim3((unsigned)batch), dim3(kFluxThreads), 0, ctx->stream, d_T,
                           t_stride, ldt, d_pi, d_role, n, slabs, qp, qm, d_totals, d_info);
    }
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
