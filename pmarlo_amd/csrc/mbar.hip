// MBAR (Shirts & Chodera 2008): the streaming pass over the K x N matrix of reduced potentials, the reduced Newton
// system, the weights of unsampled target states.  The contract is in include/msmhip.h and DESIGN.md ("MBAR frame
// weights"); the tests hold it to tests/_mbar_ref.py run in 80-bit floats.
//
// The pass: one lane per frame, rows of u read coalesced.  A workgroup keeps its slab [K, 256 frames] in LDS with a
// row stride of 260 doubles: the lane that owns a frame walks a column (consecutive lanes, consecutive banks), the
// MFMA operand reads of lane (j, g) = (lane & 15, lane >> 4) go to row i0 + j, column c + g, bank pair 4 j + g, and
// the row sums read row `lane` starting at column `lane`, bank pair 5 lane + c: none of the three collides beyond the
// two passes a 64-lane 8-byte access takes anyway.
// Every sum is taken in an order fixed by the launch shape: no floating-point atomics, the same bits on every run.
#include <algorithm>

#include "common.h"
#include "wave.h"

namespace {

constexpr int kT = MSM_MBAR_THREADS;
constexpr int kWaves = kT / 64;
constexpr int kRow = kT + 4;          // slab row stride in doubles
constexpr int kTilesPerWave = 3;      // 10 upper tiles at K = 64 over 4 waves
constexpr int kMaxPerCu = 3;          // the Gram kernel's registers admit 3 workgroups per CU; both kernels share one grid
constexpr size_t kLdsPerCu = 160 * 1024;
static_assert(kT == 256 && kWaves * kTilesPerWave >= 10, "tile spread assumes four waves");

struct PassShape {
    int tiles;            // upper 16 x 16 tiles of G
    int stride;           // doubles of one workgroup's partials: s [K], obj, tiles [tiles][256]
    size_t lds;           // bytes
    int grid;
    int64_t trips;
};

PassShape pass_shape(const msm_ctx* ctx, int K, int64_t N, int want_gram, int max_workgroups) {
    PassShape p;
    const int kt = (K + 15) >> 4;
    p.tiles = kt * (kt + 1) / 2;
    p.stride = K + 1 + (want_gram ? p.tiles * 256 : 0);
    p.lds = ((size_t)K * kRow + 3 * (size_t)K + kT + kWaves) * sizeof(double);
    p.trips = (N + kT - 1) / kT;
    const int per_cu = (int)std::min<size_t>(kMaxPerCu, std::max<size_t>(1, kLdsPerCu / p.lds));
    int64_t cap = (int64_t)ctx->n_cu * per_cu;
    if (max_workgroups > 0) cap = max_workgroups;
    p.grid = (int)std::max<int64_t>(1, std::min<int64_t>(p.trips, cap));
    return p;
}

// tile t of the upper triangle in row-major order -> (ti, tj), ti <= tj < kt
__device__ __forceinline__ void tile_coords(int t, int kt, int& ti, int& tj) {
    ti = 0;
    while (t >= kt - ti) { t -= kt - ti; ++ti; }
    tj = ti + t;
}

template <typename T, bool GRAM>
__global__ __launch_bounds__(kT) void mbar_pass_kernel(const T* __restrict__ u, int K, int64_t N, int64_t ld,
                                                       const double* __restrict__ f, const double* __restrict__ lnN,
                                                       double* __restrict__ logden, double* __restrict__ part,
                                                       int stride, int32_t* __restrict__ status) {
    extern __shared__ double mbar_lds[];
    double* slab = mbar_lds;                  // [K][kRow]
    double* fk = slab + (size_t)K * kRow;     // [K] f_k
    double* lnNk = fk + K;                    // [K] ln N_k
    double* invN = lnNk + K;                  // [K] exp(-ln N_k)
    double* rows = invN + K;                  // [kWaves][64] the waves' row sums at the end
    double* red = rows + kT;                  // [kWaves]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j16 = lane & 15, g = lane >> 4;
    const int kt = (K + 15) >> 4, tiles = kt * (kt + 1) / 2;
    for (int k = tid; k < K; k += kT) {
        fk[k] = f[k];
        lnNk[k] = lnN[k];
        invN[k] = exp(-lnN[k]);
    }
    __syncthreads();

    double s_acc = 0.0, obj_acc = 0.0;
    int bad = 0;
    v4f64 acc[kTilesPerWave];
#pragma unroll
    for (int t = 0; t < kTilesPerWave; ++t) acc[t] = v4f64{0.0, 0.0, 0.0, 0.0};
    double* col = slab + tid;

    const int64_t trips = (N + kT - 1) / kT;
    for (int64_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const int64_t n = trip * kT + tid;
        const bool valid = n < N;
        bool ok = valid;
        double d = 0.0;
        if (valid) {
            const T* __restrict__ un = u + n;
            double m = INFINITY;
            bool frame_bad = false;
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
                const double x = (double)un[(int64_t)k * ld];
                frame_bad |= !(x > -INFINITY);          // NaN or -inf
                col[k * kRow] = x;
                m = x < m ? x : m;
            }
            double M = -INFINITY;
            for (int k = 0; k < K; ++k) {
                const double b = (fk[k] - (col[k * kRow] - m)) + lnNk[k];   // the inner difference is exact at large |u|
                col[k * kRow] = b;
                M = b > M ? b : M;
            }
            ok = !frame_bad && M > -INFINITY && M < INFINITY;
            if (ok) {
                double S = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double e = exp(col[k * kRow] - M);
                    col[k * kRow] = e;
                    S += e;
                }
                d = (M + log(S)) - m;
                const double rS = 1.0 / S;
                for (int k = 0; k < K; ++k) col[k * kRow] = col[k * kRow] * invN[k] * rS;
                obj_acc += d;
            } else {
                d = frame_bad ? NAN : -INFINITY;
                bad |= frame_bad ? MSM_MBAR_BAD_INPUT : MSM_MBAR_BAD_FRAME;
            }
            if (logden) logden[n] = d;
        }
        if (!ok)
            for (int k = 0; k < K; ++k) col[k * kRow] = 0.0;
        __syncthreads();
        // row sums: lane k of a wave adds the wave's 64 columns of row k, four chains of 16, starting at column k
        if (lane < K) {
            const double* row = slab + (size_t)lane * kRow + wave * 64;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 4
            for (int c = 0; c < 64; c += 4) {
                a0 += row[(c + lane) & 63];
                a1 += row[(c + 1 + lane) & 63];
                a2 += row[(c + 2 + lane) & 63];
                a3 += row[(c + 3 + lane) & 63];
            }
            s_acc += (a0 + a1) + (a2 + a3);
        }
        if constexpr (GRAM) {
#pragma unroll
            for (int t = 0; t < kTilesPerWave; ++t) {
                const int tile = wave + kWaves * t;      // wave-uniform
                if (tile < tiles) {
                    int ti, tj;
                    tile_coords(tile, kt, ti, tj);
                    const int ia = ti * 16 + j16, ib = tj * 16 + j16;
                    const double* ra = slab + (size_t)min(ia, K - 1) * kRow;
                    const double* rb = slab + (size_t)min(ib, K - 1) * kRow;
                    const v4f64 c = mfma_tile_acc(kT, g, ia < K, ib < K, [&](int k) { return ra[k]; },
                                                  [&](int k) { return rb[k]; });
                    acc[t] += c;
                }
            }
        }
        __syncthreads();
    }

    double* mine = part + (size_t)blockIdx.x * stride;
    rows[wave * 64 + lane] = s_acc;
    const double obj = block_sum_lane0(obj_acc, red);     // (its barriers also publish `rows`)
    if (tid < K) mine[tid] = ((rows[tid] + rows[64 + tid]) + rows[128 + tid]) + rows[192 + tid];
    if (tid == 0) mine[K] = obj;
    if (bad) atomicOr(status, bad);
    if constexpr (GRAM) {
#pragma unroll
        for (int t = 0; t < kTilesPerWave; ++t) {
            const int tile = wave + kWaves * t;
            if (tile < tiles) {
                double* out = mine + K + 1 + tile * 256;
#pragma unroll
                for (int r = 0; r < 4; ++r) out[(g + 4 * r) * 16 + j16] = acc[t][r];
            }
        }
    }
}

// One wave per output: lane l adds the partials of workgroups l, l + 64, .. in ascending order, then the fixed
// shuffle tree.  Outputs 0 .. K-1: s; K: obj; K + 1 + i K + j (i <= j): G_ij and its mirror image.
__global__ __launch_bounds__(kT) void mbar_reduce_kernel(const double* __restrict__ part, int grid, int stride, int K,
                                                         int want_gram, double* __restrict__ s, double* __restrict__ G,
                                                         double* __restrict__ obj) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int total = K + 1 + (want_gram ? K * K : 0);
    if (o >= total) return;
    int off = o, i = 0, j = 0;
    if (o > K) {
        i = (o - K - 1) / K;
        j = (o - K - 1) % K;
        if (i > j) return;
        const int kt = (K + 15) >> 4, ti = i >> 4, tj = j >> 4;
        const int tile = ti * kt - ti * (ti - 1) / 2 + (tj - ti);
        off = K + 1 + tile * 256 + (i & 15) * 16 + (j & 15);
    }
    double v = 0.0;
    for (int w = lane; w < grid; w += 64) v += part[(size_t)w * stride + off];
    v = wave_sum_down(v);
    if (lane == 0) {
        if (o < K) s[o] = v;
        else if (o == K) obj[0] = v;
        else { G[(size_t)i * K + j] = v; G[(size_t)j * K + i] = v; }
    }
}

template <typename T>
__global__ __launch_bounds__(kT) void mbar_means_kernel(const T* __restrict__ u, int64_t ld,
                                                        const int64_t* __restrict__ off, double* __restrict__ mean) {
    __shared__ double red[kWaves];
    const int k = blockIdx.x;
    const int64_t o0 = off[k], o1 = off[k + 1];
    const T* __restrict__ row = u + (int64_t)k * ld;
    double a = 0.0;
    for (int64_t n = o0 + threadIdx.x; n < o1; n += kT) a += (double)row[n];
    const double tot = block_sum_lane0(a, red);
    if (threadIdx.x == 0) mean[k] = tot / (double)(o1 - o0);
}

__global__ __launch_bounds__(kT) void mbar_newton_kernel(int K, const double* __restrict__ s,
                                                         const double* __restrict__ G, const double* __restrict__ Nk,
                                                         double* __restrict__ H, double* __restrict__ gr) {
    const int R = K - 1;
    for (int p = blockIdx.x * kT + threadIdx.x; p < R * R; p += gridDim.x * kT) {
        const int i = p / R + 1, j = p % R + 1;
        const double off = Nk[i] * Nk[j] * G[(size_t)i * K + j];
        H[p] = i == j ? Nk[i] * s[i] - off : -off;
        if (j == 1) gr[i - 1] = Nk[i] * (s[i] - 1.0);
    }
}

// ---- target states ----------------------------------------------------------------------------------------------
// c_n = -u_tn - d_n.  Launch 1: per workgroup (max_g, sum_n exp(c_n - max_g)) over its frames.  Launch 2: every
// workgroup rebuilds lse = logsumexp_n c_n from those pairs in a fixed order, writes w_n = exp(c_n - lse) and its
// partial sum of w^2.  Launch 3: f_t, ESS_t.
template <typename T>
__device__ __forceinline__ double target_c(const T* __restrict__ ut, const double* __restrict__ logden, int64_t n,
                                           int& bad) {
    const double x = (double)ut[n];
    if (!(x > -INFINITY)) bad |= MSM_MBAR_BAD_INPUT;
    return -x - logden[n];
}

template <typename T>
__global__ __launch_bounds__(kT) void mbar_target_lse_kernel(const T* __restrict__ u, int64_t N, int64_t ld,
                                                             const double* __restrict__ logden,
                                                             double* __restrict__ part, int32_t* __restrict__ status) {
    __shared__ double red[kWaves];
    __shared__ double bc;
    const T* __restrict__ ut = u + (int64_t)blockIdx.y * ld;
    int bad = 0;
    double mx = -INFINITY;
    for (int64_t n = (int64_t)blockIdx.x * kT + threadIdx.x; n < N; n += (int64_t)gridDim.x * kT) {
        const double c = target_c(ut, logden, n, bad);
        mx = c > mx ? c : mx;
    }
    mx = block_max_bcast(mx, red, &bc);
    double a = 0.0;
    if (mx > -INFINITY && mx < INFINITY)
        for (int64_t n = (int64_t)blockIdx.x * kT + threadIdx.x; n < N; n += (int64_t)gridDim.x * kT)
            a += exp(target_c(ut, logden, n, bad) - mx);
    const double tot = block_sum_lane0(a, red);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        o[0] = mx;
        o[1] = tot;
    }
    if (bad) atomicOr(status, bad);
}

// lse of one target from the workgroup pairs: the same bits in every workgroup that calls it
__device__ __forceinline__ double target_lse(const double* __restrict__ pairs, int grid, double* red, double* bc) {
    double mx = -INFINITY;
    for (int w = threadIdx.x; w < grid; w += kT) mx = fmax(mx, pairs[2 * w]);
    mx = block_max_bcast(mx, red, bc);
    if (!(mx > -INFINITY && mx < INFINITY)) return mx;     // no frame reaches the target (or NaN input: flagged)
    double a = 0.0;
    for (int w = threadIdx.x; w < grid; w += kT) {
        const double m = pairs[2 * w];
        if (m > -INFINITY) a += pairs[2 * w + 1] * exp(m - mx);
    }
    __syncthreads();
    const double S = block_sum_bcast(a, red, bc);
    return mx + log(S);
}

template <typename T>
__global__ __launch_bounds__(kT) void mbar_target_write_kernel(const T* __restrict__ u, int64_t N, int64_t ld,
                                                               const double* __restrict__ logden,
                                                               const double* __restrict__ part,
                                                               double* __restrict__ w, double* __restrict__ part2) {
    __shared__ double red[kWaves];
    __shared__ double bc;
    const int t = blockIdx.y;
    const T* __restrict__ ut = u + (int64_t)t * ld;
    const double lse = target_lse(part + (size_t)t * gridDim.x * 2, gridDim.x, red, &bc);
    const bool live = lse > -INFINITY && lse < INFINITY;
    double a = 0.0;
    int bad = 0;
    for (int64_t n = (int64_t)blockIdx.x * kT + threadIdx.x; n < N; n += (int64_t)gridDim.x * kT) {
        const double x = live ? exp(target_c(ut, logden, n, bad) - lse) : 0.0;
        w[(int64_t)t * N + n] = x;
        a += x * x;
    }
    __syncthreads();
    const double tot = block_sum_lane0(a, red);
    if (threadIdx.x == 0) part2[(size_t)t * gridDim.x + blockIdx.x] = tot;
}

__global__ __launch_bounds__(kT) void mbar_target_final_kernel(const double* __restrict__ part,
                                                               const double* __restrict__ part2, int grid,
                                                               double* __restrict__ ft, double* __restrict__ ess,
                                                               int32_t* __restrict__ status) {
    __shared__ double red[kWaves];
    __shared__ double bc;
    const int t = blockIdx.x;
    const double lse = target_lse(part + (size_t)t * grid * 2, grid, red, &bc);
    double a = 0.0;
    for (int w = threadIdx.x; w < grid; w += kT) a += part2[(size_t)t * grid + w];
    __syncthreads();
    const double sq = block_sum_lane0(a, red);
    if (threadIdx.x == 0) {
        ft[t] = -lse;
        ess[t] = 1.0 / sq;
        if (!(lse > -INFINITY && lse < INFINITY)) atomicOr(status, MSM_MBAR_BAD_FRAME);
    }
}

__global__ __launch_bounds__(kT) void mbar_potentials_kernel(const double* __restrict__ energy,
                                                             const double* __restrict__ bias, int64_t ldb,
                                                             const double* __restrict__ beta, int64_t N, int64_t ld,
                                                             double* __restrict__ u) {
    const int k = blockIdx.y;
    const double b = beta[k];
    for (int64_t n = (int64_t)blockIdx.x * kT + threadIdx.x; n < N; n += (int64_t)gridDim.x * kT) {
        const double e = bias ? energy[n] + bias[(int64_t)k * ldb + n] : energy[n];
        u[(int64_t)k * ld + n] = b * e;
    }
}

msm_status check_shape(msm_ctx* ctx, const char* who, int K, int64_t N, int64_t ld, msm_dtype dtype) {
    MSM_REQUIRE(ctx, dtype == MSM_F32 || dtype == MSM_F64, "%s: dtype must be MSM_F32 or MSM_F64", who);
    MSM_REQUIRE(ctx, K >= 1 && N >= 1 && ld >= N, "%s: need K >= 1, N >= 1, ld >= N (K=%d N=%lld ld=%lld)", who, K,
                (long long)N, (long long)ld);
    if (K > MSM_MBAR_MAX_K)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "%s: %d sampled states, at most %d are supported", who, K,
                        MSM_MBAR_MAX_K);
    return MSM_OK;
}

int target_grid(const msm_ctx* ctx, int64_t N) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((N + kT - 1) / kT, (int64_t)ctx->n_cu * 4));
}

}  // namespace

extern "C" {

msm_status msm_mbar_plan(msm_ctx* ctx, int K, int64_t N, msm_dtype dtype, int max_workgroups, int64_t out[4]) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, out != nullptr, "msm_mbar_plan: NULL pointer");
    MSM_REQUIRE(ctx, max_workgroups >= 0, "msm_mbar_plan: max_workgroups must be >= 0 (0: the default)");
    const msm_status rs = check_shape(ctx, "msm_mbar_plan", K, N, N, dtype);
    if (rs != MSM_OK) return rs;
    const PassShape p = pass_shape(ctx, K, N, 1, max_workgroups);
    out[0] = kT;
    out[1] = p.grid;
    out[2] = (int64_t)p.lds;
    out[3] = p.tiles;
    return MSM_OK;
}

msm_status msm_mbar_pass(msm_ctx* ctx, const void* d_u, msm_dtype dtype, int K, int64_t N, int64_t ld,
                         const double* d_f, const double* d_lnN, int want_gram, int max_workgroups, double* d_logden,
                         double* d_s, double* d_G, double* d_obj, int32_t* d_status) {
    if (!ctx) return MSM_ERR_INVALID;
    msm_status rs = check_shape(ctx, "msm_mbar_pass", K, N, ld, dtype);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, max_workgroups >= 0, "msm_mbar_pass: max_workgroups must be >= 0 (0: the default)");
    MSM_REQUIRE(ctx, d_u && d_f && d_lnN && d_s && d_obj && d_status && (d_G || !want_gram),
                "msm_mbar_pass: NULL pointer");
    const PassShape p = pass_shape(ctx, K, N, want_gram, max_workgroups);
    rs = msm_reserve_scratch(ctx, (size_t)p.grid * p.stride * sizeof(double));
    if (rs != MSM_OK) return rs;
    double* part = (double*)ctx->scratch;
#define MSM_MBAR_PASS(T, GRAM)                                                                                        \
    do {                                                                                                              \
        if (p.lds > 48 * 1024)                                                                                        \
            MSM_HIP(ctx, hipFuncSetAttribute((const void*)mbar_pass_kernel<T, GRAM>,                                  \
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));                \
        hipLaunchKernelGGL((mbar_pass_kernel<T, GRAM>), dim3(p.grid), dim3(kT), p.lds, ctx->stream, (const T*)d_u, K, \
                           N, ld, d_f, d_lnN, d_logden, part, p.stride, d_status);                                    \
    } while (0)
    if (dtype == MSM_F32) { if (want_gram) MSM_MBAR_PASS(float, true); else MSM_MBAR_PASS(float, false); }
    else { if (want_gram) MSM_MBAR_PASS(double, true); else MSM_MBAR_PASS(double, false); }
#undef MSM_MBAR_PASS
    MSM_CHECK_LAUNCH(ctx);
    const int outputs = K + 1 + (want_gram ? K * K : 0);
    hipLaunchKernelGGL(mbar_reduce_kernel, dim3(msm_ceil_div(outputs, kWaves)), dim3(kT), 0, ctx->stream,
                       (const double*)part, p.grid, p.stride, K, want_gram ? 1 : 0, d_s, d_G, d_obj);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_mbar_state_means(msm_ctx* ctx, const void* d_u, msm_dtype dtype, int K, int64_t N, int64_t ld,
                                const int64_t* h_offsets, double* d_mean) {
    if (!ctx) return MSM_ERR_INVALID;
    msm_status rs = check_shape(ctx, "msm_mbar_state_means", K, N, ld, dtype);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, d_u && h_offsets && d_mean, "msm_mbar_state_means: NULL pointer");
    MSM_REQUIRE(ctx, h_offsets[0] >= 0 && h_offsets[K] <= N, "msm_mbar_state_means: offsets outside [0, N]");
    for (int k = 0; k < K; ++k)
        MSM_REQUIRE(ctx, h_offsets[k + 1] > h_offsets[k], "msm_mbar_state_means: state %d has no frames", k);
    const void* d_off = nullptr;
    rs = msm_upload_table(ctx, h_offsets, (size_t)(K + 1) * sizeof(int64_t), &d_off);
    if (rs != MSM_OK) return rs;
    if (dtype == MSM_F32)
        hipLaunchKernelGGL(mbar_means_kernel<float>, dim3(K), dim3(kT), 0, ctx->stream, (const float*)d_u, ld,
                           (const int64_t*)d_off, d_mean);
    else
        hipLaunchKernelGGL(mbar_means_kernel<double>, dim3(K), dim3(kT), 0, ctx->stream, (const double*)d_u, ld,
                           (const int64_t*)d_off, d_mean);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_mbar_newton_system(msm_ctx* ctx, int K, const double* d_s, const double* d_G, const double* d_Nk,
                                  double* d_H, double* d_g) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, K >= 2, "msm_mbar_newton_system: the reduced system needs K >= 2 (got %d)", K);
    if (K > MSM_MBAR_MAX_K)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_mbar_newton_system: %d sampled states, at most %d are supported",
                        K, MSM_MBAR_MAX_K);
    MSM_REQUIRE(ctx, d_s && d_G && d_Nk && d_H && d_g, "msm_mbar_newton_system: NULL pointer");
    hipLaunchKernelGGL(mbar_newton_kernel, dim3(msm_ceil_div((int64_t)(K - 1) * (K - 1), kT)), dim3(kT), 0, ctx->stream,
                       K, d_s, d_G, d_Nk, d_H, d_g);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_mbar_weights(msm_ctx* ctx, const void* d_ut, msm_dtype dtype, int T, int64_t N, int64_t ld,
                            const double* d_logden, double* d_ft, double* d_w, double* d_ess, int32_t* d_status) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, dtype == MSM_F32 || dtype == MSM_F64, "msm_mbar_weights: dtype must be MSM_F32 or MSM_F64");
    MSM_REQUIRE(ctx, T >= 1 && T <= 65535 && N >= 1 && ld >= N,
                "msm_mbar_weights: need 1 <= T <= 65535, N >= 1, ld >= N (T=%d N=%lld ld=%lld)", T, (long long)N,
                (long long)ld);
    MSM_REQUIRE(ctx, d_ut && d_logden && d_ft && d_w && d_ess && d_status, "msm_mbar_weights: NULL pointer");
    const int grid = target_grid(ctx, N);
    const msm_status rs = msm_reserve_scratch(ctx, (size_t)T * grid * 3 * sizeof(double));
    if (rs != MSM_OK) return rs;
    double* part = (double*)ctx->scratch;
    double* part2 = part + (size_t)T * grid * 2;
#define MSM_MBAR_TARGETS(T_)                                                                                          \
    do {                                                                                                              \
        hipLaunchKernelGGL(mbar_target_lse_kernel<T_>, dim3(grid, T), dim3(kT), 0, ctx->stream, (const T_*)d_ut, N,   \
                           ld, d_logden, part, d_status);                                                             \
        hipLaunchKernelGGL(mbar_target_write_kernel<T_>, dim3(grid, T), dim3(kT), 0, ctx->stream, (const T_*)d_ut, N, \
                           ld, d_logden, (const double*)part, d_w, part2);                                            \
    } while (0)
    if (dtype == MSM_F32) MSM_MBAR_TARGETS(float); else MSM_MBAR_TARGETS(double);
#undef MSM_MBAR_TARGETS
    hipLaunchKernelGGL(mbar_target_final_kernel, dim3(T), dim3(kT), 0, ctx->stream, (const double*)part,
                       (const double*)part2, grid, d_ft, d_ess, d_status);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_mbar_reduced_potentials(msm_ctx* ctx, const double* d_energy, const double* d_bias, int64_t ldb,
                                       const double* d_beta, int K, int64_t N, int64_t ld, double* d_u) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, K >= 1 && K <= 65535 && N >= 1 && ld >= N && (!d_bias || ldb >= N),
                "msm_mbar_reduced_potentials: need 1 <= K <= 65535, N >= 1, ld >= N, ldb >= N (K=%d N=%lld)", K,
                (long long)N);
    MSM_REQUIRE(ctx, d_energy && d_beta && d_u, "msm_mbar_reduced_potentials: NULL pointer");
    hipLaunchKernelGGL(mbar_potentials_kernel, dim3(target_grid(ctx, N), K), dim3(kT), 0, ctx->stream, d_energy, d_bias,
                       ldb, d_beta, N, ld, d_u);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
