// TRAM (Wu, Paul, Wehmeyer, Noe, PNAS 113, E3221, 2016): the row sums of the multiplier and effective-count updates,
// the streaming frame pass, the free-energy update and the transition matrices.  The contract is in include/msmhip.h
// and DESIGN.md ("TRAM"); the tests hold it to tests/_tram_ref.py run in 80-bit floats.
//
// The pass: frames are grouped by Markov state and every state's range is cut into segments of MSM_TRAM_SEGMENT
// frames.  A workgroup takes one (state, segment) unit per trip, one lane per frame, rows of u read coalesced.  All
// frames of a unit share the Markov state, so the column ln R + f of the [K, m] table is wave-uniform and sits in LDS.
// The unit's r slab [K, 256] goes through LDS with the row stride of mbar.hip (260 doubles: the column walk of a lane
// and the rotated row sums collide no more than a 64-lane 8-byte access does anyway).
// Every sum is taken in an order fixed by the inputs alone: a unit's K sums do not depend on the workgroup that
// forms them, and a second launch adds a state's units in ascending order.  No floating-point atomics.
#include <algorithm>

#include "common.h"
#include "wave.h"

namespace {

constexpr int kT = MSM_TRAM_SEGMENT;
constexpr int kWaves = kT / 64;
constexpr int kRow = kT + 4;          // slab row stride in doubles
constexpr int kMaxPerCu = 4;
constexpr size_t kLdsPerCu = 160 * 1024;
constexpr int kUpdateT = 1024;        // the update's single workgroup
static_assert(kT == 256, "the row sums assume four waves");

struct PassShape {
    size_t lds;
    int grid;
};

PassShape pass_shape(const msm_ctx* ctx, int K, int64_t units, int max_workgroups) {
    PassShape p;
    p.lds = ((size_t)K * kRow + (size_t)K + kT) * sizeof(double);
    const int per_cu = (int)std::min<size_t>(kMaxPerCu, std::max<size_t>(1, kLdsPerCu / p.lds));
    int64_t cap = (int64_t)ctx->n_cu * per_cu;
    if (max_workgroups > 0) cap = max_workgroups;
    p.grid = (int)std::max<int64_t>(1, std::min<int64_t>(units, cap));
    return p;
}

// One wave per row (k, i).  x_j = sign (g_j - g_i); out = sum_j S_ij / (1 + exp(x_j)) + add, lane l adding the
// columns l, l + 64, .. in ascending order, then the fixed shuffle tree.  No exp and no division where S_ij = 0.
__global__ __launch_bounds__(kT) void tram_rows_kernel(int K, int m, const double* __restrict__ S,
                                                       const double* __restrict__ g, const double* __restrict__ f,
                                                       const double* __restrict__ Nki, const double* __restrict__ col,
                                                       int mode, double* __restrict__ out, double* __restrict__ lnout) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (row >= (int64_t)K * m) return;                      // wave-uniform
    const int k = (int)(row / m);
    const double n_i = Nki[row];
    double acc = 0.0;
    if (n_i > 0.0) {
        const double* __restrict__ Srow = S + row * m;
        const double* __restrict__ gk = g + (int64_t)k * m;
        const double gi = g[row];
        for (int j = lane; j < m; j += 64) {
            const double sij = Srow[j];
            if (sij != 0.0) {
                const double x = mode == MSM_TRAM_ROWS_MULTIPLIERS ? gk[j] - gi : gi - gk[j];
                acc += sij / (1.0 + exp(x));
            }
        }
    }
    acc = wave_sum_down(acc);
    if (lane == 0) {
        double o = 0.0;
        if (n_i > 0.0) o = mode == MSM_TRAM_ROWS_MULTIPLIERS ? acc : acc + (n_i - col[row]);
        out[row] = o;
        lnout[row] = o > 0.0 ? log(o) + f[row] : -INFINITY;
    }
}

__global__ __launch_bounds__(kT) void tram_log_multipliers_kernel(int64_t n, const double* __restrict__ f,
                                                                   const double* __restrict__ v,
                                                                   double* __restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (i < n) g[i] = v[i] > 0.0 ? log(v[i]) + f[i] : -INFINITY;
}

template <typename T>
__global__ __launch_bounds__(kT) void tram_pass_kernel(const T* __restrict__ u, int K, int m, int64_t N, int64_t ld,
                                                       const int64_t* __restrict__ off,
                                                       const int64_t* __restrict__ unit_ptr,
                                                       const int32_t* __restrict__ unit_state, int64_t units,
                                                       const double* __restrict__ tab, double* __restrict__ logden,
                                                       double* __restrict__ part, int32_t* __restrict__ status) {
    extern __shared__ double tram_lds[];
    double* slab = tram_lds;                  // [K][kRow]
    double* tk = slab + (size_t)K * kRow;     // [K] ln R_i^k + f_i^k of the unit's state i, -inf for inactive pairs
    double* rows = tk + K;                    // [kWaves][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* colp = slab + tid;
    int bad = 0;

    for (int64_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        // the unit's frames [n0, n1); tables that do not describe frames of [0, N) give an empty unit
        const int i = unit_state[unit];
        int64_t n0 = 0, n1 = 0;
        if (i >= 0 && i < m) {
            const int64_t o0 = off[i], o1 = off[i + 1], q = unit - unit_ptr[i];
            if (o0 >= 0 && o1 <= N && q >= 0 && q <= (o1 - o0) / kT) {
                n0 = o0 + q * kT;
                n1 = n0 + kT < o1 ? n0 + kT : o1;
            }
        }
        if (tid < K) tk[tid] = n1 > n0 ? tab[(int64_t)tid * m + i] : -INFINITY;
        __syncthreads();
        const int64_t n = n0 + tid;
        bool ok = n < n1;
        if (ok) {
            const T* __restrict__ un = u + n;
            double mn = INFINITY;
            bool frame_bad = false;
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
                const double x = (double)un[(int64_t)k * ld];
                frame_bad |= !(x > -INFINITY);          // NaN or -inf
                colp[k * kRow] = x;
                mn = x < mn ? x : mn;
            }
            double M = -INFINITY;
            for (int k = 0; k < K; ++k) {
                const double a = tk[k] - (colp[k * kRow] - mn);     // the inner difference is exact at large |u|
                colp[k * kRow] = a;
                M = a > M ? a : M;
            }
            ok = !frame_bad && M > -INFINITY && M < INFINITY;
            double d;
            if (ok) {
                double Ssum = 0.0;
                for (int k = 0; k < K; ++k) {
                    const double e = exp(colp[k * kRow] - M);
                    colp[k * kRow] = e;
                    Ssum += e;
                }
                d = (M + log(Ssum)) - mn;
                const double rS = 1.0 / Ssum;
                for (int k = 0; k < K; ++k) colp[k * kRow] *= rS;
            } else {
                d = frame_bad ? NAN : -INFINITY;
                bad |= frame_bad ? MSM_MBAR_BAD_INPUT : MSM_MBAR_BAD_FRAME;
            }
            if (logden) logden[n] = d;
        }
        if (!ok)
            for (int k = 0; k < K; ++k) colp[k * kRow] = 0.0;
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
            rows[wave * 64 + lane] = (a0 + a1) + (a2 + a3);
        }
        __syncthreads();
        if (tid < K) part[unit * K + tid] = ((rows[tid] + rows[64 + tid]) + rows[128 + tid]) + rows[192 + tid];
    }
    if (bad) atomicOr(status, bad);
}

// s[k, i] = the partial sums of state i's units, added in ascending unit order.  Lane k of a wave, one wave per state.
__global__ __launch_bounds__(kT) void tram_reduce_kernel(const double* __restrict__ part, int K, int m,
                                                         const int64_t* __restrict__ unit_ptr, int64_t units,
                                                         double* __restrict__ s) {
    const int k = threadIdx.x & 63;
    const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= m || k >= K) return;
    const int64_t p0 = unit_ptr[i], p1 = unit_ptr[i + 1];
    const int64_t u0 = p0 > 0 ? p0 : 0, u1 = p1 < units ? p1 : units;
    double a = 0.0;
#pragma unroll 4
    for (int64_t w = u0; w < u1; ++w) a += part[w * K + k];
    s[(int64_t)k * m + i] = a;
}

// Steps 4 and 5 by one workgroup: f_new = (ln R + f) - ln s on the active pairs, minus its minimum over them;
// err = max |f_new - f_old|; g = ln v + f_new.  Every thread touches its own entries only; min and max are exact.
__global__ __launch_bounds__(kUpdateT) void tram_update_kernel(int64_t n, const double* __restrict__ Nki,
                                                               const double* __restrict__ tab,
                                                               const double* __restrict__ s,
                                                               const double* __restrict__ v, double* __restrict__ f,
                                                               double* __restrict__ g, double* __restrict__ err) {
    __shared__ double red[kUpdateT / 64];
    __shared__ double bc;
    double mn = INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += kUpdateT) {
        if (Nki[i] > 0.0) {
            const double fn = tab[i] - log(s[i]);
            g[i] = fn;
            mn = fmin(mn, fn);
        }
    }
    mn = block_reduce_bcast(mn, red, &bc, INFINITY, op_min{});
    double e = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kUpdateT) {
        if (Nki[i] > 0.0) {
            const double fn = g[i] - mn;
            e = fmax(e, fabs(fn - f[i]));
            f[i] = fn;
            g[i] = v[i] > 0.0 ? log(v[i]) + fn : -INFINITY;
        } else {
            g[i] = -INFINITY;
        }
    }
    __syncthreads();
    e = block_reduce_bcast(e, red, &bc, 0.0, op_max{});
    if (threadIdx.x == 0) err[0] = e;
}

// p_ij = S_ij / (v_i + v_j exp(f_j - f_i)), i != j, of ensemble blockIdx.x + k0.  One wave per row, lanes over the
// columns in ascending order, the fixed shuffle tree.  Launch 1 (P == nullptr) leaves the off-diagonal row sums in
// rowsum [K, m]; launch 2 divides by the largest of them where that exceeds 1 and closes the rows.
__global__ __launch_bounds__(kT) void tram_tmat_kernel(int m, int k0, const double* __restrict__ S,
                                                       const double* __restrict__ Nki, const double* __restrict__ f,
                                                       const double* __restrict__ v, double* __restrict__ rowsum,
                                                       double* __restrict__ P) {
    __shared__ double red[kWaves];
    __shared__ double bc;
    const int k = blockIdx.x + k0, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* __restrict__ Sk = S + (int64_t)k * m * m;
    const double* __restrict__ Nk = Nki + (int64_t)k * m;
    const double* __restrict__ fk = f + (int64_t)k * m;
    const double* __restrict__ vk = v + (int64_t)k * m;
    double* __restrict__ rs = rowsum + (int64_t)k * m;
    double scale = 1.0;
    if (P) {
        double mx = 0.0;
        for (int i = threadIdx.x; i < m; i += kT) mx = fmax(mx, rs[i]);
        mx = block_max_bcast(mx, red, &bc);
        if (mx > 1.0) scale = mx;
    }
    double* __restrict__ Pk = P ? P + (int64_t)blockIdx.x * m * m : nullptr;
    for (int i = wave; i < m; i += kWaves) {
        const bool active = Nk[i] > 0.0;
        const double fi = fk[i], vi = vk[i];
        double acc = 0.0;
        for (int j = lane; j < m; j += 64) {
            double p = 0.0;
            const double sij = Sk[(int64_t)i * m + j];
            if (active && j != i && sij != 0.0 && Nk[j] > 0.0) {
                p = sij / (vi + vk[j] * exp(fk[j] - fi));
                if (scale != 1.0) p /= scale;
            }
            acc += p;
            if (Pk && j != i) Pk[(int64_t)i * m + j] = p;
        }
        acc = wave_sum_down(acc);
        if (lane == 0) {
            if (Pk) Pk[(int64_t)i * m + i] = active ? 1.0 - acc : 0.0;
            else rs[i] = acc;
        }
    }
}

msm_status check_sizes(msm_ctx* ctx, const char* who, int K, int m) {
    MSM_REQUIRE(ctx, K >= 1 && m >= 1, "%s: need K >= 1 and m >= 1 (K=%d m=%d)", who, K, m);
    if (K > MSM_MBAR_MAX_K)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "%s: %d thermodynamic states, at most %d are supported", who, K,
                        MSM_MBAR_MAX_K);
    if (m > MSM_TRAM_MAX_STATES)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "%s: %d Markov states, at most %d are supported", who, m,
                        MSM_TRAM_MAX_STATES);
    return MSM_OK;
}

msm_status check_frames(msm_ctx* ctx, const char* who, int64_t N, int64_t ld, int64_t units, msm_dtype dtype) {
    MSM_REQUIRE(ctx, dtype == MSM_F32 || dtype == MSM_F64, "%s: dtype must be MSM_F32 or MSM_F64", who);
    MSM_REQUIRE(ctx, N >= 1 && ld >= N, "%s: need N >= 1 and ld >= N (N=%lld ld=%lld)", who, (long long)N,
                (long long)ld);
    MSM_REQUIRE(ctx, units >= 1 && units <= N, "%s: need 1 <= units <= N (units=%lld)", who, (long long)units);
    return MSM_OK;
}

void launch_rows(msm_ctx* ctx, int K, int m, const double* d_S, const double* d_g, const double* d_f,
                 const double* d_N, const double* d_col, int mode, double* d_out, double* d_lnout) {
    hipLaunchKernelGGL(tram_rows_kernel, dim3(msm_ceil_div((int64_t)K * m, kWaves)), dim3(kT), 0, ctx->stream, K, m,
                       d_S, d_g, d_f, d_N, d_col, mode, d_out, d_lnout);
}

msm_status launch_pass(msm_ctx* ctx, const void* d_u, msm_dtype dtype, int K, int m, int64_t N, int64_t ld,
                       const int64_t* d_offsets, const int64_t* d_unit_ptr, const int32_t* d_unit_state, int64_t units,
                       const double* d_tab, int max_workgroups, double* d_logden, double* d_s, int32_t* d_status) {
    const PassShape p = pass_shape(ctx, K, units, max_workgroups);
    const msm_status rs = msm_reserve_scratch(ctx, (size_t)units * K * sizeof(double));
    if (rs != MSM_OK) return rs;
    double* part = (double*)ctx->scratch;
#define MSM_TRAM_PASS(T)                                                                                              \
    do {                                                                                                              \
        if (p.lds > 48 * 1024)                                                                                        \
            MSM_HIP(ctx, hipFuncSetAttribute((const void*)tram_pass_kernel<T>,                                        \
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));                \
        hipLaunchKernelGGL(tram_pass_kernel<T>, dim3(p.grid), dim3(kT), p.lds, ctx->stream, (const T*)d_u, K, m, N,   \
                           ld, d_offsets, d_unit_ptr, d_unit_state, units, d_tab, d_logden, part, d_status);          \
    } while (0)
    if (dtype == MSM_F32) MSM_TRAM_PASS(float); else MSM_TRAM_PASS(double);
#undef MSM_TRAM_PASS
    MSM_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(tram_reduce_kernel, dim3(msm_ceil_div(m, kWaves)), dim3(kT), 0, ctx->stream,
                       (const double*)part, K, m, d_unit_ptr, units, d_s);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // namespace

extern "C" {

msm_status msm_tram_plan(msm_ctx* ctx, int K, int m, const int64_t* h_offsets, int max_workgroups, int64_t out[5]) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, h_offsets && out, "msm_tram_plan: NULL pointer");
    MSM_REQUIRE(ctx, max_workgroups >= 0, "msm_tram_plan: max_workgroups must be >= 0 (0: the default)");
    const msm_status rs = check_sizes(ctx, "msm_tram_plan", K, m);
    if (rs != MSM_OK) return rs;
    int64_t units = 0;
    for (int i = 0; i < m; ++i) {
        MSM_REQUIRE(ctx, h_offsets[i + 1] > h_offsets[i], "msm_tram_plan: Markov state %d has no frames", i);
        units += (h_offsets[i + 1] - h_offsets[i] + kT - 1) / kT;
    }
    const PassShape p = pass_shape(ctx, K, units, max_workgroups);
    out[0] = kT;
    out[1] = units;
    out[2] = p.grid;
    out[3] = (int64_t)p.lds;
    out[4] = msm_ceil_div((int64_t)K * m, kWaves);
    return MSM_OK;
}

msm_status msm_tram_rows(msm_ctx* ctx, int K, int m, const double* d_S, const double* d_g, const double* d_f,
                         const double* d_N, const double* d_col, int mode, double* d_out, double* d_lnout) {
    if (!ctx) return MSM_ERR_INVALID;
    const msm_status rs = check_sizes(ctx, "msm_tram_rows", K, m);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, mode == MSM_TRAM_ROWS_MULTIPLIERS || mode == MSM_TRAM_ROWS_COUNTS,
                "msm_tram_rows: mode must be MSM_TRAM_ROWS_MULTIPLIERS or MSM_TRAM_ROWS_COUNTS");
    MSM_REQUIRE(ctx, d_S && d_g && d_f && d_N && d_col && d_out && d_lnout, "msm_tram_rows: NULL pointer");
    MSM_REQUIRE(ctx, d_out != d_g && d_lnout != d_g, "msm_tram_rows: the outputs must not alias d_g");
    launch_rows(ctx, K, m, d_S, d_g, d_f, d_N, d_col, mode, d_out, d_lnout);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_tram_pass(msm_ctx* ctx, const void* d_u, msm_dtype dtype, int K, int m, int64_t N, int64_t ld,
                         const int64_t* d_offsets, const int64_t* d_unit_ptr, const int32_t* d_unit_state,
                         int64_t units, const double* d_tab, int max_workgroups, double* d_logden, double* d_s,
                         int32_t* d_status) {
    if (!ctx) return MSM_ERR_INVALID;
    msm_status rs = check_sizes(ctx, "msm_tram_pass", K, m);
    if (rs != MSM_OK) return rs;
    rs = check_frames(ctx, "msm_tram_pass", N, ld, units, dtype);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, max_workgroups >= 0, "msm_tram_pass: max_workgroups must be >= 0 (0: the default)");
    MSM_REQUIRE(ctx, d_u && d_offsets && d_unit_ptr && d_unit_state && d_tab && d_s && d_status,
                "msm_tram_pass: NULL pointer");
    return launch_pass(ctx, d_u, dtype, K, m, N, ld, d_offsets, d_unit_ptr, d_unit_state, units, d_tab,
                       max_workgroups, d_logden, d_s, d_status);
}

msm_status msm_tram_update(msm_ctx* ctx, int K, int m, const double* d_N, const double* d_tab, const double* d_s,
                           const double* d_v, double* d_f, double* d_g, double* d_err) {
    if (!ctx) return MSM_ERR_INVALID;
    const msm_status rs = check_sizes(ctx, "msm_tram_update", K, m);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, d_N && d_tab && d_s && d_v && d_f && d_g && d_err, "msm_tram_update: NULL pointer");
    hipLaunchKernelGGL(tram_update_kernel, dim3(1), dim3(kUpdateT), 0, ctx->stream, (int64_t)K * m, d_N, d_tab, d_s,
                       d_v, d_f, d_g, d_err);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_tram_iterations(msm_ctx* ctx, const void* d_u, msm_dtype dtype, int K, int m, int64_t N, int64_t ld,
                               const int64_t* d_offsets, const int64_t* d_unit_ptr, const int32_t* d_unit_state,
                               int64_t units, const double* d_S, const double* d_N, const double* d_col, double* d_f,
                               double* d_v, double* d_work, int n_iterations, int max_workgroups, double* d_logden,
                               double* d_err, int32_t* d_status) {
    if (!ctx) return MSM_ERR_INVALID;
    msm_status rs = check_sizes(ctx, "msm_tram_iterations", K, m);
    if (rs != MSM_OK) return rs;
    rs = check_frames(ctx, "msm_tram_iterations", N, ld, units, dtype);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, n_iterations >= 1 && max_workgroups >= 0,
                "msm_tram_iterations: need n_iterations >= 1 and max_workgroups >= 0");
    MSM_REQUIRE(ctx, d_u && d_offsets && d_unit_ptr && d_unit_state && d_S && d_N && d_col && d_f && d_v && d_work &&
                         d_err && d_status, "msm_tram_iterations: NULL pointer");
    const int64_t n = (int64_t)K * m;
    double *g = d_work, *g2 = g + n, *R = g2 + n, *tab = R + n, *s = tab + n;
    hipLaunchKernelGGL(tram_log_multipliers_kernel, dim3(msm_ceil_div(n, kT)), dim3(kT), 0, ctx->stream, n,
                       (const double*)d_f, (const double*)d_v, g);
    for (int it = 0; it < n_iterations; ++it) {
        launch_rows(ctx, K, m, d_S, g, d_f, d_N, d_col, MSM_TRAM_ROWS_MULTIPLIERS, d_v, g2);
        launch_rows(ctx, K, m, d_S, g2, d_f, d_N, d_col, MSM_TRAM_ROWS_COUNTS, R, tab);
        MSM_CHECK_LAUNCH(ctx);
        rs = launch_pass(ctx, d_u, dtype, K, m, N, ld, d_offsets, d_unit_ptr, d_unit_state, units, tab,
                         max_workgroups, it == n_iterations - 1 ? d_logden : nullptr, s, d_status);
        if (rs != MSM_OK) return rs;
        hipLaunchKernelGGL(tram_update_kernel, dim3(1), dim3(kUpdateT), 0, ctx->stream, n, d_N, (const double*)tab,
                           (const double*)s, (const double*)d_v, d_f, g, d_err);
    }
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_tram_transition_matrices(msm_ctx* ctx, int K, int m, const double* d_S, const double* d_N,
                                        const double* d_f, const double* d_v, int k, double* d_rowsum, double* d_P) {
    if (!ctx) return MSM_ERR_INVALID;
    const msm_status rs = check_sizes(ctx, "msm_tram_transition_matrices", K, m);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, k >= -1 && k < K, "msm_tram_transition_matrices: k must be -1 (all) or in [0, %d)", K);
    MSM_REQUIRE(ctx, d_S && d_N && d_f && d_v && d_rowsum && d_P, "msm_tram_transition_matrices: NULL pointer");
    const int k0 = k < 0 ? 0 : k, count = k < 0 ? K : 1;
    hipLaunchKernelGGL(tram_tmat_kernel, dim3(count), dim3(kT), 0, ctx->stream, m, k0, d_S, d_N, d_f, d_v, d_rowsum,
                       (double*)nullptr);
    hipLaunchKernelGGL(tram_tmat_kernel, dim3(count), dim3(kT), 0, ctx->stream, m, k0, d_S, d_N, d_f, d_v, d_rowsum,
                       d_P);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
