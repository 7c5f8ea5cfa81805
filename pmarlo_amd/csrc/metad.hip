// Metadynamics: the sum of Gaussian hills at N frames (value and gradient), the running log-sum-exp of the bias on a
// regular grid that the reweighting offset c(t) is made of, and the append of one hill to a device ledger.  The
// contract is in include/msmhip.h and DESIGN.md ("Metadynamics"); the tests hold the kernels to tests/_metad_ref.py
// run in 80-bit floats.
//
// A hill is a record of 2 d + 1 doubles: centre [d], 1 / sigma [d], height.  Both kernels stage the records through
// LDS in tiles of MSM_METAD_TILE hills; every lane of a wave reads the same record at the same time (one broadcast
// read per word) and adds its own term.  A lane adds its terms in ascending hill index and shares no sum with another
// lane, so a frame's bits depend on its own CVs, its own count and the hills alone.
// All of it is fp64; -ffp-contract=off, so the operation order written here is the order executed.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "wave.h"

namespace {

constexpr int kT = MSM_METAD_THREADS;
constexpr int kWaves = kT / 64;
constexpr int kTile = MSM_METAD_TILE;
static_assert(kT == 256 && MSM_METAD_SCAN_TILE == kT, "one grid point per lane, four waves");

struct HillShape {                        // by value in the kernel arguments
    double period[MSM_METAD_MAX_D];       // 0: the CV is not periodic
    double A, B, cut;                     // term = h (A exp(-dp2) + B) where dp2 < cut
};

struct GridShape {
    double lo[MSM_METAD_GRID_MAX_D], step[MSM_METAD_GRID_MAX_D];
    int bins[MSM_METAD_GRID_MAX_D];
};

struct HillRecord {
    double v[2 * MSM_METAD_MAX_D + 1];
};

// z_i = dp_i / sigma_i of the point s and the record rec; returns dp2 = 1/2 sum z_i^2 (ascending i)
template <int D>
__device__ __forceinline__ double hill_dp2(const double* rec, const double (&s)[D], const HillShape& sh,
                                           double (&z)[D]) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double dp = s[i] - rec[i];
        const double P = sh.period[i];
        if (P > 0.0) dp -= P * rint(dp / P);
        z[i] = dp * rec[D + i];
        q += z[i] * z[i];
    }
    return 0.5 * q;
}

template <int D>
__device__ __forceinline__ void stage_hills(double* tile, const double* __restrict__ hills, int h0, int m) {
    constexpr int R = 2 * D + 1;
    const double* __restrict__ src = hills + (size_t)h0 * R;
    for (int i = threadIdx.x; i < m * R; i += kT) tile[i] = src[i];
}

template <int D, bool GRAD>
__global__ __launch_bounds__(kT) void metad_bias_kernel(const double* __restrict__ cv, int64_t n, int64_t ld,
                                                        const double* __restrict__ hills, int H,
                                                        const int32_t* __restrict__ count, HillShape sh,
                                                        double* __restrict__ bias, double* __restrict__ grad,
                                                        int64_t ldg) {
    constexpr int R = 2 * D + 1;
    __shared__ double tile[kTile * R];
    __shared__ int wg_top;
    const int64_t trips = (n + kT - 1) / kT;
    for (int64_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const int64_t f = trip * kT + threadIdx.x;
        const bool valid = f < n;
        double s[D];
        bool bad = false;
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            s[i] = valid ? cv[f * ld + i] : 0.0;
            bad |= !(fabs(s[i]) < INFINITY);
        }
        if (valid && !bad) cnt = count ? min(max(count[f], 0), H) : H;
        // the workgroup walks the hills any of its frames sees
        if (threadIdx.x == 0) wg_top = 0;
        __syncthreads();
        const int wave_top = wave_reduce_xor(cnt, [](int a, int b) { return max(a, b); });
        if ((threadIdx.x & 63) == 0) atomicMax(&wg_top, wave_top);
        __syncthreads();
        const int top = wg_top;

        double v = 0.0;
        double g[D];
#pragma unroll
        for (int i = 0; i < D; ++i) g[i] = 0.0;
        for (int h0 = 0; h0 < top; h0 += kTile) {
            const int m = min(kTile, top - h0);
            __syncthreads();
            stage_hills<D>(tile, hills, h0, m);
            __syncthreads();
            const int mine = min(m, cnt - h0);
            for (int j = 0; j < mine; ++j) {
                const double* rec = tile + j * R;
                double z[D];
                const double q = hill_dp2<D>(rec, s, sh, z);
                if (q < sh.cut) {
                    const double e = exp(-q);
                    const double h = rec[2 * D];
                    v += h * (sh.A * e + sh.B);
                    if constexpr (GRAD) {
                        const double w = -(h * (sh.A * e));
#pragma unroll
                        for (int i = 0; i < D; ++i) g[i] += w * (z[i] * rec[D + i]);
                    }
                }
            }
        }
        if (valid) {
            bias[f] = bad ? NAN : v;
            if constexpr (GRAD) {
#pragma unroll
                for (int i = 0; i < D; ++i) grad[f * ldg + i] = bad ? NAN : g[i];
            }
        }
        __syncthreads();      // wg_top and the tile are free for the next trip
    }
}

// One checkpoint of the scan: (max, sum exp(a V - max)) of the workgroup's grid points for both exponents.  V >= 0 and
// a >= 0, and rounding is monotone, so max_g (a V_g) = a max_g V_g bit for bit: one maximum serves both exponents.
// `red` is [3 kWaves]; the caller alternates two of them, which makes two barriers enough.
__device__ __forceinline__ void scan_checkpoint(double V, bool valid, double a1, double a2, double* red,
                                                double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double wm = wave_max_xor(valid ? V : -INFINITY);
    if (lane == 0) red[wave] = wm;
    __syncthreads();
    const double mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    double e1 = valid ? exp(a1 * V - a1 * mx) : 0.0;
    double e2 = valid ? exp(a2 * V - a2 * mx) : 0.0;
    wave_sum_down_each(e1, e2);
    if (lane == 0) {
        red[kWaves + wave] = e1;
        red[2 * kWaves + wave] = e2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = a1 * mx;
        out[1] = ((red[kWaves] + red[kWaves + 1]) + red[kWaves + 2]) + red[kWaves + 3];
        out[2] = a2 * mx;
        out[3] = ((red[2 * kWaves] + red[2 * kWaves + 1]) + red[2 * kWaves + 2]) + red[2 * kWaves + 3];
    }
}

// part [tiles, M, 2, 2]: tile t, checkpoint j, exponent, (max, scaled sum).  A tile is kT consecutive grid points,
// whatever the grid of the launch: a workgroup takes tiles blockIdx.x, blockIdx.x + gridDim.x, ..
template <int D>
__global__ __launch_bounds__(kT) void metad_scan_kernel(const double* __restrict__ hills, int H, GridShape gs,
                                                        HillShape sh, const int32_t* __restrict__ ck, int M,
                                                        double a1, double a2, int64_t G, int tiles,
                                                        double* __restrict__ part, double* __restrict__ vgrid) {
    constexpr int R = 2 * D + 1;
    __shared__ double tile[kTile * R];
    __shared__ double red[2][3 * kWaves];
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t gp = (int64_t)t * kT + threadIdx.x;
        const bool valid = gp < G;
        double s[D];
        int64_t r = valid ? gp : 0;
#pragma unroll
        for (int i = D - 1; i >= 0; --i) {
            const int64_t idx = r % gs.bins[i];
            r /= gs.bins[i];
            s[i] = gs.lo[i] + (double)idx * gs.step[i];
        }
        double V = 0.0;
        double* mine = part + (size_t)t * M * 4;
        int j = 0, par = 0;
        for (int h0 = 0; h0 < H; h0 += kTile) {
            const int m = min(kTile, H - h0);
            __syncthreads();
            stage_hills<D>(tile, hills, h0, m);
            __syncthreads();
            for (int jj = 0; jj < m; ++jj) {
                while (j < M && ck[j] == h0 + jj) {          // wave- and workgroup-uniform
                    scan_checkpoint(V, valid, a1, a2, red[par], mine + (size_t)j * 4);
                    par ^= 1;
                    ++j;
                }
                const double* rec = tile + jj * R;
                double z[D];
                const double q = hill_dp2<D>(rec, s, sh, z);
                if (q < sh.cut) V += rec[2 * D] * (sh.A * exp(-q) + sh.B);
            }
        }
        for (; j < M; ++j) {                                 // the checkpoints at H (the host checked the list)
            scan_checkpoint(V, valid, a1, a2, red[par], mine + (size_t)j * 4);
            par ^= 1;
        }
        if (vgrid && valid) vgrid[gp] = V;
        __syncthreads();
    }
}

// lse[j, e] = log sum_g exp(a_e V_{k_j}(g)) from the tiles' pairs, one wave per output: lane l adds the tiles l, l + 64,
// .. in ascending order, then the fixed shuffle tree (the order of mbar_reduce_kernel; a function of `tiles` alone)
__global__ __launch_bounds__(kT) void metad_merge_kernel(const double* __restrict__ part, int tiles, int M,
                                                         double* __restrict__ lse) {
    const int lane = threadIdx.x & 63;
    const int o = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (o >= 2 * M) return;
    const double* __restrict__ p = part + (size_t)o * 2;
    const size_t stride = (size_t)M * 4;
    double mx = -INFINITY;
    for (int t = lane; t < tiles; t += 64) mx = fmax(mx, p[t * stride]);
    mx = wave_max_xor(mx);
    double sum = 0.0;
    for (int t = lane; t < tiles; t += 64) sum += p[t * stride + 1] * exp(p[t * stride] - mx);
    sum = wave_sum_down(sum);
    if (lane == 0) lse[o] = mx + log(sum);
}

// flag |= 1 where a height is negative, NaN or infinite
__global__ __launch_bounds__(kT) void metad_heights_kernel(const double* __restrict__ hills, int H, int R,
                                                           int32_t* __restrict__ flag) {
    bool bad = false;
    for (int h = blockIdx.x * kT + threadIdx.x; h < H; h += gridDim.x * kT) {
        const double x = hills[(size_t)h * R + R - 1];
        bad |= !(x >= 0.0 && x < INFINITY);
    }
    if (bad) atomicOr(flag, 1);
}

// dst [R] = the record; the centre from device memory where `center` is given, the height scaled by
// exp(v_scale * v[0]) where `v` is given (the well-tempered rule, V at the centre still on the device)
__global__ __launch_bounds__(64) void metad_append_kernel(double* __restrict__ dst, int d, HillRecord rec,
                                                          const double* __restrict__ center,
                                                          const double* __restrict__ v, double v_scale) {
    const int i = threadIdx.x, R = 2 * d + 1;
#pragma unroll
    for (int k = 0; k < 2 * MSM_METAD_MAX_D + 1; ++k) {
        if (k != i || k >= R) continue;
        double x = rec.v[k];
        if (center && k < d) x = center[k];
        if (v && k == R - 1) x = x * exp(v_scale * v[0]);
        dst[k] = x;
    }
}

msm_status hill_shape(msm_ctx* ctx, const char* who, int d, int max_d, const double* h_period, int kernel, double cut,
                      HillShape* sh) {
    MSM_REQUIRE(ctx, d >= 1 && d <= max_d, "%s: %d collective variables, 1 to %d are supported", who, d, max_d);
    MSM_REQUIRE(ctx, kernel == MSM_METAD_GAUSSIAN || kernel == MSM_METAD_STRETCHED,
                "%s: kernel must be MSM_METAD_GAUSSIAN or MSM_METAD_STRETCHED", who);
    MSM_REQUIRE(ctx, cut > 0.0 && cut < INFINITY, "%s: the cutoff must be positive and finite", who);
    for (int i = 0; i < MSM_METAD_MAX_D; ++i) sh->period[i] = 0.0;
    for (int i = 0; h_period && i < d; ++i) {
        MSM_REQUIRE(ctx, h_period[i] >= 0.0 && h_period[i] < INFINITY,
                    "%s: period %d must be 0 (not periodic) or positive and finite", who, i);
        sh->period[i] = h_period[i];
    }
    sh->cut = cut;
    sh->A = 1.0;
    sh->B = 0.0;
    if (kernel == MSM_METAD_STRETCHED) {
        sh->A = 1.0 / (1.0 - std::exp(-cut));
        sh->B = -std::exp(-cut) * sh->A;
    }
    return MSM_OK;
}

int bias_grid(const msm_ctx* ctx, int64_t n, int max_workgroups) {
    const int64_t trips = (n + kT - 1) / kT;
    const int64_t cap = max_workgroups > 0 ? max_workgroups : (int64_t)ctx->n_cu * 8;
    return (int)std::max<int64_t>(1, std::min<int64_t>(trips, cap));
}

template <int D>
void launch_bias(msm_ctx* ctx, int grid, const double* d_cv, int64_t n, int64_t ld, const double* d_hills, int H,
                 const int32_t* d_count, const HillShape& sh, double* d_bias, double* d_grad, int64_t ldg) {
    if (d_grad)
        hipLaunchKernelGGL((metad_bias_kernel<D, true>), dim3(grid), dim3(kT), 0, ctx->stream, d_cv, n, ld, d_hills, H,
                           d_count, sh, d_bias, d_grad, ldg);
    else
        hipLaunchKernelGGL((metad_bias_kernel<D, false>), dim3(grid), dim3(kT), 0, ctx->stream, d_cv, n, ld, d_hills,
                           H, d_count, sh, d_bias, d_grad, ldg);
}

}  // namespace

extern "C" {

msm_status msm_metad_plan(msm_ctx* ctx, int64_t n, int H, int d, int max_workgroups, int64_t out[4]) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, out != nullptr, "msm_metad_plan: NULL pointer");
    MSM_REQUIRE(ctx, n >= 1 && H >= 0 && d >= 1 && d <= MSM_METAD_MAX_D && max_workgroups >= 0,
                "msm_metad_plan: need n >= 1, H >= 0, 1 <= d <= %d, max_workgroups >= 0 (0: the default)",
                MSM_METAD_MAX_D);
    out[0] = kT;
    out[1] = kTile;
    out[2] = bias_grid(ctx, n, max_workgroups);
    out[3] = (int64_t)(kTile * (2 * d + 1) * sizeof(double) + sizeof(int));
    return MSM_OK;
}

msm_status msm_metad_bias(msm_ctx* ctx, const double* d_cv, int64_t n, int64_t ld, int d, const double* d_hills, int H,
                          const double* h_period, int kernel, double cut, const int32_t* d_count, int max_workgroups,
                          double* d_bias, double* d_grad, int64_t ldg) {
    if (!ctx) return MSM_ERR_INVALID;
    HillShape sh;
    const msm_status rs = hill_shape(ctx, "msm_metad_bias", d, MSM_METAD_MAX_D, h_period, kernel, cut, &sh);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, n >= 1 && ld >= d && H >= 0 && max_workgroups >= 0 && (!d_grad || ldg >= d),
                "msm_metad_bias: need n >= 1, ld >= d, H >= 0, max_workgroups >= 0, ldg >= d (n=%lld ld=%lld H=%d)",
                (long long)n, (long long)ld, H);
    MSM_REQUIRE(ctx, d_cv && d_bias && (d_hills || H == 0), "msm_metad_bias: NULL pointer");
    const int grid = bias_grid(ctx, n, max_workgroups);
    switch (d) {
#define MSM_METAD_CASE(D)                                                                               \
    case D:                                                                                             \
        launch_bias<D>(ctx, grid, d_cv, n, ld, d_hills, H, d_count, sh, d_bias, d_grad, ldg);           \
        break;
        MSM_METAD_CASE(1) MSM_METAD_CASE(2) MSM_METAD_CASE(3) MSM_METAD_CASE(4)
        MSM_METAD_CASE(5) MSM_METAD_CASE(6) MSM_METAD_CASE(7) MSM_METAD_CASE(8)
#undef MSM_METAD_CASE
    }
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_metad_grid_scan(msm_ctx* ctx, const double* d_hills, int H, int d, const double* h_lo,
                               const double* h_step, const int32_t* h_bins, const double* h_period, int kernel,
                               double cut, const int32_t* h_checkpoints, int M, double a1, double a2,
                               int max_workgroups, double* d_lse, double* d_vgrid) {
    if (!ctx) return MSM_ERR_INVALID;
    HillShape sh;
    msm_status rs = hill_shape(ctx, "msm_metad_grid_scan", d, MSM_METAD_GRID_MAX_D, h_period, kernel, cut, &sh);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, H >= 0 && M >= 1 && max_workgroups >= 0,
                "msm_metad_grid_scan: need H >= 0, M >= 1, max_workgroups >= 0 (H=%d M=%d)", H, M);
    MSM_REQUIRE(ctx, h_lo && h_step && h_bins && h_checkpoints && d_lse && (d_hills || H == 0),
                "msm_metad_grid_scan: NULL pointer");
    MSM_REQUIRE(ctx, a1 >= a2 && a2 >= 0.0 && a1 < INFINITY, "msm_metad_grid_scan: need a1 >= a2 >= 0, finite");
    GridShape gs;
    int64_t G = 1;
    for (int i = 0; i < MSM_METAD_GRID_MAX_D; ++i) {
        gs.lo[i] = 0.0;
        gs.step[i] = 0.0;
        gs.bins[i] = 1;
    }
    for (int i = 0; i < d; ++i) {
        MSM_REQUIRE(ctx, h_bins[i] >= 1 && std::isfinite(h_lo[i]) && std::isfinite(h_step[i]),
                    "msm_metad_grid_scan: axis %d needs bins >= 1 and finite lo, step", i);
        gs.lo[i] = h_lo[i];
        gs.step[i] = h_step[i];
        gs.bins[i] = h_bins[i];
        G *= h_bins[i];
        MSM_REQUIRE(ctx, G <= ((int64_t)1 << 31) - kT, "msm_metad_grid_scan: the grid has too many points");
    }
    for (int j = 0; j < M; ++j)
        MSM_REQUIRE(ctx, h_checkpoints[j] >= (j ? h_checkpoints[j - 1] : 0) && h_checkpoints[j] <= H,
                    "msm_metad_grid_scan: checkpoint %d is not ascending inside [0, %d]", j, H);
    const int tiles = (int)((G + kT - 1) / kT);
    const int cap = max_workgroups > 0 ? max_workgroups : ctx->n_cu * 8;
    const int grid = std::max(1, std::min(tiles, cap));
    const size_t part_bytes = (size_t)tiles * M * 4 * sizeof(double);
    rs = msm_reserve_scratch(ctx, part_bytes + 64);
    if (rs != MSM_OK) return rs;
    double* part = (double*)ctx->scratch;
    int32_t* flag = (int32_t*)((char*)ctx->scratch + part_bytes);
    // the scan's meaning rests on V growing with every hill: a negative (or non-finite) height is refused
    if (H > 0) {
        int32_t h_flag = 0;
        MSM_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int32_t), ctx->stream));
        hipLaunchKernelGGL(metad_heights_kernel, dim3(std::min(msm_ceil_div(H, kT), 64)), dim3(kT), 0, ctx->stream,
                           d_hills, H, 2 * d + 1, flag);
        MSM_CHECK_LAUNCH(ctx);
        MSM_HIP(ctx, hipMemcpyAsync(&h_flag, flag, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        MSM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        MSM_REQUIRE(ctx, h_flag == 0, "msm_metad_grid_scan: a hill has a negative or non-finite height");
    }
    const void* d_ck = nullptr;
    rs = msm_upload_table(ctx, h_checkpoints, (size_t)M * sizeof(int32_t), &d_ck);
    if (rs != MSM_OK) return rs;
#define MSM_METAD_SCAN(D)                                                                                              \
    hipLaunchKernelGGL(metad_scan_kernel<D>, dim3(grid), dim3(kT), 0, ctx->stream, d_hills, H, gs, sh,                 \
                       (const int32_t*)d_ck, M, a1, a2, G, tiles, part, d_vgrid)
    if (d == 1) MSM_METAD_SCAN(1);
    else if (d == 2) MSM_METAD_SCAN(2);
    else MSM_METAD_SCAN(3);
#undef MSM_METAD_SCAN
    MSM_CHECK_LAUNCH(ctx);
    hipLaunchKernelGGL(metad_merge_kernel, dim3(msm_ceil_div(2 * (int64_t)M, kWaves)), dim3(kT), 0, ctx->stream,
                       (const double*)part, tiles, M, d_lse);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_metad_append(msm_ctx* ctx, double* d_hills, int capacity, int index, int d, const double* h_record,
                            const double* d_center, const double* d_v, double v_scale) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d >= 1 && d <= MSM_METAD_MAX_D, "msm_metad_append: %d collective variables, 1 to %d are supported",
                d, MSM_METAD_MAX_D);
    MSM_REQUIRE(ctx, d_hills && h_record, "msm_metad_append: NULL pointer");
    MSM_REQUIRE(ctx, index >= 0 && index < capacity, "msm_metad_append: hill %d does not fit a ledger of capacity %d",
                index, capacity);
    const int R = 2 * d + 1;
    HillRecord rec;
    for (int i = 0; i < 2 * MSM_METAD_MAX_D + 1; ++i) rec.v[i] = i < R ? h_record[i] : 0.0;
    for (int i = d; i < R; ++i)
        MSM_REQUIRE(ctx, h_record[i] >= 0.0 && h_record[i] < INFINITY && (i == R - 1 || h_record[i] > 0.0),
                    "msm_metad_append: 1 / sigma must be positive and the height non-negative, both finite");
    MSM_REQUIRE(ctx, std::isfinite(v_scale), "msm_metad_append: v_scale must be finite");
    hipLaunchKernelGGL(metad_append_kernel, dim3(1), dim3(64), 0, ctx->stream, d_hills + (size_t)index * R, d, rec,
                       d_center, d_v, v_scale);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
