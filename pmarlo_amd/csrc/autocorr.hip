// Per-segment, multi-lag autocorrelation of standardised columns (S/analysis/diagnostics.py:247-351) and the
// side-by-side copy of two column blocks that the canonical correlations start from (:173-221).
//
// Launch sequence of msm_autocorr_lagscan, the same for any number of segments:
//   1. column sums about the segment's first row -> slab -> mean[s][f]
//   2. sums of (x - mean)^2                      -> slab -> 1/sigma[s][f]  (0 marks a masked column)
//   3. per group of kLagsPerLaunch lags: sum z[t] z[t+tau] -> slab -> value[s][l]
// Rows are cut into chunks that never straddle a segment; a workgroup walks chunks grid-stride and
// leaves one slab entry per chunk, and the second kernel of every stage adds a segment's chunks in a
// fixed order: no floating-point atomics, so two calls on the same input give the same bits.
// Everything is centred before it is multiplied, in fp64 whatever the input type.
//
// All three stages are bandwidth-bound.  Stage 3 keeps a tile of standardised rows in LDS; a pair whose
// partner row lies inside the tile is served from there, every other partner is read from global memory,
// so the traffic is about (3 + number of lags longer than the tile) * n * F * sizeof(T).
#include "common.h"
#include "wave.h"

#include <algorithm>
#include <cstring>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileElems = 4096;        // fp64 tile in LDS: 32 KiB, so several workgroups share a CU
constexpr int kLagsPerLaunch = 32;
constexpr int kMaxF = 256;
constexpr int64_t kTargetChunks = 8192;  // slab rows: a few chunks per resident workgroup

// device table, int64: [start n_seg][stop n_seg][first chunk of the segment n_seg + 1][lags n_lag]
struct Tab {
    const int64_t* start;
    const int64_t* stop;
    const int64_t* prefix;
    int n_seg;
};

struct Chunk {
    int seg;
    int64_t a, b;    // the segment
    int64_t r0, r1;  // rows of the chunk
};

__device__ __forceinline__ Chunk find_chunk(const Tab& tb, int64_t c, int64_t chunk_rows) {
    int lo = 0, hi = tb.n_seg - 1;
    while (lo < hi) {  // last segment whose first chunk is <= c (segments without rows own no chunk)
        const int mid = (lo + hi + 1) >> 1;
        if (tb.prefix[mid] <= c) lo = mid; else hi = mid - 1;
    }
    Chunk ch;
    ch.seg = lo;
    ch.a = tb.start[lo];
    ch.b = tb.stop[lo];
    ch.r0 = ch.a + (c - tb.prefix[lo]) * chunk_rows;
    ch.r1 = min(ch.r0 + chunk_rows, ch.b);
    return ch;
}

// ---------------------------------------------------------------------------
// stages 1 and 2: per chunk and column, MODE 0: sum(x - x[a]), MODE 1: sum((x - mean)^2).
// Lanes span the columns of a row (tf = power of two >= F, at most 256), rows are dealt over the rest.
// slab [n_chunks][F]
// ---------------------------------------------------------------------------
template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void autocorr_column_kernel(
    const T* __restrict__ x, int F, int64_t ld, Tab tb, int64_t n_chunks, int64_t chunk_rows, int tf,
    const double* __restrict__ mean, double* __restrict__ slab) {
    __shared__ double red[kThreads];
    const int tid = threadIdx.x;
    const int fx = tid % tf, ry = tid / tf, rp = kThreads / tf;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const Chunk ch = find_chunk(tb, c, chunk_rows);
        double acc = 0.0;
        if (fx < F) {
            const double ref = MODE == 0 ? (double)x[ch.a * ld + fx] : mean[(size_t)ch.seg * F + fx];
            int64_t r = ch.r0 + ry;
            for (; r + 3 * rp < ch.r1; r += 4 * rp) {  // 4 independent loads in flight per lane
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = (double)x[(r + (int64_t)u * rp) * ld + fx];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const double d = v[u] - ref;
                    acc = MODE == 0 ? acc + d : fma(d, d, acc);
                }
            }
            for (; r < ch.r1; r += rp) {
                const double d = (double)x[r * ld + fx] - ref;
                acc = MODE == 0 ? acc + d : fma(d, d, acc);
            }
        }
        __syncthreads();
        red[tid] = acc;
        __syncthreads();
        if (ry == 0 && fx < F) {
            for (int y = 1; y < rp; ++y) acc += red[y * tf + fx];  // fixed order
            slab[(size_t)c * F + fx] = acc;
        }
    }
}

// One workgroup per (segment, 64 columns): 16 groups add the segment's chunks g, g + 16, ..., then the 16
// sums are added in group order.  MODE 0 -> mean, MODE 1 -> 1 / sigma, 0 where the column is masked
// (variance not above the floor, NaN variance included).
template <typename T, int MODE>
__global__ __launch_bounds__(1024) void autocorr_column_reduce_kernel(
    const double* __restrict__ slab, const T* __restrict__ x, int F, int64_t ld, Tab tb, double var_floor,
    double* __restrict__ out) {
    __shared__ double red[16][64];
    const int io = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int s = blockIdx.x;
    const int f = blockIdx.y * 64 + io;
    const int64_t c0 = tb.prefix[s], c1 = tb.prefix[s + 1];
    double acc = 0.0;
    if (f < F)
        for (int64_t c = c0 + g; c < c1; c += 16) acc += slab[(size_t)c * F + f];
    red[g][io] = acc;
    __syncthreads();
    if (g != 0 || f >= F) return;
    double t = 0.0;
    for (int k = 0; k < 16; ++k) t += red[k][io];
    const int64_t a = tb.start[s];
    const double len = (double)(tb.stop[s] - a);
    double r = 0.0;
    if (len > 0.0) {
        if (MODE == 0) {
            r = (double)x[a * ld + f] + t / len;
        } else {
            const double var = t / len;
            r = var > var_floor ? 1.0 / sqrt(var) : 0.0;
        }
    }
    out[(size_t)s * F + f] = r;
}

// ---------------------------------------------------------------------------
// stage 3: slab [n_chunks][kLagsPerLaunch], entry = sum over the chunk's head rows t (t + tau inside the
// segment) and the valid columns of z[t][f] z[t + tau][f].
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void autocorr_lag_kernel(
    const T* __restrict__ x, int F, int64_t ld, Tab tb, int64_t n_chunks, int64_t chunk_rows, int tile_rows,
    const int64_t* __restrict__ lags, int n_lag, const double* __restrict__ mean,
    const double* __restrict__ inv_sigma, double* __restrict__ slab) {
    __shared__ double tile[kTileElems];
    __shared__ double s_mean[kMaxF], s_inv[kMaxF];
    __shared__ double s_acc[kLagsPerLaunch][kWaves];
    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    // element i = row * F + f of a tile; i advances by kThreads
    const int row_tid = tid / F, f_tid = tid - row_tid * F;
    const int row_step = kThreads / F, f_step = kThreads - row_step * F;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const Chunk ch = find_chunk(tb, c, chunk_rows);
        const int64_t seg_len = ch.b - ch.a;
        __syncthreads();  // the previous chunk's tables are read out
        for (int f = tid; f < F; f += kThreads) {
            s_mean[f] = mean[(size_t)ch.seg * F + f];
            s_inv[f] = inv_sigma[(size_t)ch.seg * F + f];
        }
        if (tid < kLagsPerLaunch * kWaves) (&s_acc[0][0])[tid] = 0.0;
        for (int64_t t0 = ch.r0; t0 < ch.r1; t0 += tile_rows) {
            const int rows = (int)min<int64_t>(tile_rows, ch.r1 - t0);
            const int elems = rows * F;  // <= kTileElems
            __syncthreads();
            {
                int row = row_tid, f = f_tid;
                for (int i = tid; i < elems; i += kThreads) {
                    const double v = (double)x[(t0 + row) * ld + f];
                    const double iv = s_inv[f];
                    tile[i] = iv != 0.0 ? (v - s_mean[f]) * iv : 0.0;
                    f += f_step; row += row_step;
                    if (f >= F) { f -= F; ++row; }
                }
            }
            __syncthreads();
            for (int l = 0; l < n_lag; ++l) {
                const int64_t tau = lags[l];
                if (tau >= seg_len) continue;  // same in every lane
                // head rows of this tile whose partner is still inside the segment
                const int64_t lim = ch.b - tau - t0;
                if (lim <= 0) continue;
                const int head_elems = (int)min<int64_t>(rows, lim) * F;
                double acc = 0.0;
                int row = row_tid, f = f_tid;
                if (tau >= rows) {  // every partner comes from global memory
#pragma unroll 4
                    for (int i = tid; i < head_elems; i += kThreads) {
                        const double v = (double)x[(t0 + row + tau) * ld + f];
                        const double iv = s_inv[f];
                        const double z = iv != 0.0 ? (v - s_mean[f]) * iv : 0.0;
                        acc = fma(tile[i], z, acc);
                        f += f_step; row += row_step;
                        if (f >= F) { f -= F; ++row; }
                    }
                } else {
                    const int shift = (int)tau * F;  // tau < rows: shift < kTileElems
                    for (int i = tid; i < head_elems; i += kThreads) {
                        double z;
                        if (i + shift < elems) {
                            z = tile[i + shift];
                        } else {
                            const double v = (double)x[(t0 + row + tau) * ld + f];
                            const double iv = s_inv[f];
                            z = iv != 0.0 ? (v - s_mean[f]) * iv : 0.0;
                        }
                        acc = fma(tile[i], z, acc);
                        f += f_step; row += row_step;
                        if (f >= F) { f -= F; ++row; }
                    }
                }
                acc = wave_sum_down(acc);
                if ((tid & 63) == 0) s_acc[l][wave] += acc;  // a slot belongs to one wave: tiles add in order
            }
        }
        __syncthreads();
        if (tid < n_lag) {
            double t = s_acc[tid][0];
            for (int w = 1; w < kWaves; ++w) t += s_acc[tid][w];
            slab[(size_t)c * kLagsPerLaunch + tid] = t;
        }
    }
}

// One workgroup per segment: 8 groups add the segment's chunks g, g + 8, ..., the 8 sums are added in group
// order and divided by (L - tau) * m.  Also counts the valid columns.
__global__ __launch_bounds__(kThreads) void autocorr_lag_reduce_kernel(
    const double* __restrict__ slab, Tab tb, int F, const int64_t* __restrict__ lags, int n_lag,
    const double* __restrict__ inv_sigma, double* __restrict__ value, int n_lag_total, int lag0,
    int32_t* __restrict__ nvalid) {
    constexpr int kGroups = kThreads / kLagsPerLaunch;
    __shared__ double red[kGroups][kLagsPerLaunch];
    __shared__ int s_valid;
    const int tid = threadIdx.x;
    const int l = tid % kLagsPerLaunch, g = tid / kLagsPerLaunch;
    const int s = blockIdx.x;
    if (tid == 0) s_valid = 0;
    __syncthreads();
    int cnt = 0;
    for (int f = tid; f < F; f += kThreads) cnt += inv_sigma[(size_t)s * F + f] != 0.0 ? 1 : 0;
    if (cnt) atomicAdd(&s_valid, cnt);  // integer: order does not matter
    const int64_t c0 = tb.prefix[s], c1 = tb.prefix[s + 1];
    double acc = 0.0;
    if (l < n_lag)
        for (int64_t c = c0 + g; c < c1; c += kGroups) acc += slab[(size_t)c * kLagsPerLaunch + l];
    red[g][l] = acc;
    __syncthreads();
    const int m = s_valid;
    if (tid == 0 && nvalid) nvalid[s] = m;
    if (g != 0 || l >= n_lag) return;
    double t = 0.0;
    for (int k = 0; k < kGroups; ++k) t += red[k][l];
    const int64_t len = tb.stop[s] - tb.start[s];
    const int64_t tau = lags[l];
    double r = __builtin_nan("");
    if (len > 1 && tau < len && m > 0) r = t / ((double)(len - tau) * (double)m);
    value[(size_t)s * n_lag_total + lag0 + l] = r;
}

template <typename T>
msm_status run_lagscan(msm_ctx* ctx, const T* x, int F, int64_t ld, const Tab& tb, const int64_t* d_lags,
                       int n_lag, int64_t n_chunks, int64_t chunk_rows, int tile_rows, double var_floor,
                       double* d_value, int32_t* d_nvalid) {
    const int n_seg = tb.n_seg;
    double* mean = (double*)ctx->scratch;
    double* inv = mean + (size_t)n_seg * F;
    double* slab = inv + (size_t)n_seg * F;
    int tf = 1;
    while (tf < F) tf <<= 1;
    const int blocks = (int)std::min<int64_t>(n_chunks, (int64_t)ctx->n_cu * 8);
    const dim3 red_grid(n_seg, msm_ceil_div(F, 64));
    if (n_chunks > 0) {
        hipLaunchKernelGGL((autocorr_column_kernel<T, 0>), dim3(blocks), dim3(kThreads), 0, ctx->stream, x, F, ld, tb,
                           n_chunks, chunk_rows, tf, (const double*)nullptr, slab);
        MSM_CHECK_LAUNCH(ctx);
    }
    hipLaunchKernelGGL((autocorr_column_reduce_kernel<T, 0>), red_grid, dim3(1024), 0, ctx->stream,
                       (const double*)slab, x, F, ld, tb, var_floor, mean);
    MSM_CHECK_LAUNCH(ctx);
    if (n_chunks > 0) {
        hipLaunchKernelGGL((autocorr_column_kernel<T, 1>), dim3(blocks), dim3(kThreads), 0, ctx->stream, x, F, ld, tb,
                           n_chunks, chunk_rows, tf, (const double*)mean, slab);
        MSM_CHECK_LAUNCH(ctx);
    }
    hipLaunchKernelGGL((autocorr_column_reduce_kernel<T, 1>), red_grid, dim3(1024), 0, ctx->stream,
                       (const double*)slab, x, F, ld, tb, var_floor, inv);
    MSM_CHECK_LAUNCH(ctx);
    for (int l0 = 0; l0 < n_lag; l0 += kLagsPerLaunch) {
        const int nl = std::min(kLagsPerLaunch, n_lag - l0);
        if (n_chunks > 0) {
            hipLaunchKernelGGL(autocorr_lag_kernel<T>, dim3(blocks), dim3(kThreads), 0, ctx->stream, x, F, ld, tb,
                               n_chunks, chunk_rows, tile_rows, d_lags + l0, nl, (const double*)mean,
                               (const double*)inv, slab);
            MSM_CHECK_LAUNCH(ctx);
        }
        hipLaunchKernelGGL(autocorr_lag_reduce_kernel, dim3(n_seg), dim3(kThreads), 0, ctx->stream,
                           (const double*)slab, tb, F, d_lags + l0, nl, (const double*)inv, d_value, n_lag, l0,
                           d_nvalid);
        MSM_CHECK_LAUNCH(ctx);
    }
    return MSM_OK;
}

// out[t][0 .. pa) = a[t][:], out[t][pa .. pa + pb) = b[t][:], as fp64
template <typename TA, typename TB>
__global__ __launch_bounds__(kThreads) void hstack_kernel(const TA* __restrict__ a, int pa, int64_t lda,
                                                          const TB* __restrict__ b, int pb, int64_t ldb, int64_t n,
                                                          double* __restrict__ out) {
    const int w = pa + pb;
    const int64_t total = n * w;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
        const int64_t t = e / w;
        const int j = (int)(e - t * w);
        out[e] = j < pa ? (double)a[t * lda + j] : (double)b[t * ldb + (j - pa)];
    }
}

template <typename TA, typename TB>
void launch_hstack(msm_ctx* ctx, const void* a, int pa, int64_t lda, const void* b, int pb, int64_t ldb, int64_t n,
                   double* out) {
    const int64_t total = n * (pa + pb);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((total + kThreads - 1) / kThreads,
                                                                    (int64_t)ctx->n_cu * 8));
    hipLaunchKernelGGL((hstack_kernel<TA, TB>), dim3(blocks), dim3(kThreads), 0, ctx->stream, (const TA*)a, pa, lda,
                       (const TB*)b, pb, ldb, n, out);
}

}  // namespace

extern "C" {

msm_status msm_autocorr_lagscan(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                                const int64_t* h_seg_start, const int64_t* h_seg_stop, int n_seg,
                                const int32_t* h_lags, int n_lag, double var_floor, double* d_value,
                                int32_t* d_nvalid) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, dtype == MSM_F32 || dtype == MSM_F64, "msm_autocorr_lagscan: bad dtype");
    MSM_REQUIRE(ctx, n >= 0 && F >= 1 && ld >= F, "msm_autocorr_lagscan: need n >= 0, F >= 1, ld >= F");
    if (F > kMaxF)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_autocorr_lagscan: F = %d exceeds %d columns", F, kMaxF);
    if (n > (int64_t(1) << 31))
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_autocorr_lagscan: more than 2^31 frames");
    MSM_REQUIRE(ctx, n_seg >= 1 && h_seg_start && h_seg_stop, "msm_autocorr_lagscan: need at least one segment");
    MSM_REQUIRE(ctx, n_lag >= 1 && h_lags, "msm_autocorr_lagscan: need at least one lag");
    MSM_REQUIRE(ctx, d_value && (d_x || n == 0), "msm_autocorr_lagscan: NULL pointer");
    MSM_REQUIRE(ctx, var_floor >= 0.0, "msm_autocorr_lagscan: var_floor must be >= 0");
    if (ctx->capturing)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_autocorr_lagscan cannot run under graph capture");
    for (int l = 0; l < n_lag; ++l)
        MSM_REQUIRE(ctx, h_lags[l] >= 1, "msm_autocorr_lagscan: lag %d is %d, must be >= 1", l, (int)h_lags[l]);

    const int tile_rows = kTileElems / F;  // >= 16
    int64_t total_rows = 0;
    for (int s = 0; s < n_seg; ++s) {
        MSM_REQUIRE(ctx, 0 <= h_seg_start[s] && h_seg_start[s] <= h_seg_stop[s] && h_seg_stop[s] <= n,
                    "msm_autocorr_lagscan: segment %d = [%lld, %lld) lies outside [0, %lld]", s,
                    (long long)h_seg_start[s], (long long)h_seg_stop[s], (long long)n);
        total_rows += h_seg_stop[s] - h_seg_start[s];
    }
    // whole tiles per chunk, about kTargetChunks chunks in all
    const int64_t tiles = (total_rows + tile_rows - 1) / tile_rows;
    const int64_t chunk_rows = tile_rows * std::max<int64_t>(1, (tiles + kTargetChunks - 1) / kTargetChunks);
    const size_t tab_len = (size_t)3 * n_seg + 1 + n_lag;
    std::vector<int64_t> tab(tab_len);
    int64_t n_chunks = 0;
    for (int s = 0; s < n_seg; ++s) {
        tab[s] = h_seg_start[s];
        tab[n_seg + s] = h_seg_stop[s];
        tab[2 * (size_t)n_seg + s] = n_chunks;
        n_chunks += (h_seg_stop[s] - h_seg_start[s] + chunk_rows - 1) / chunk_rows;
    }
    tab[3 * (size_t)n_seg] = n_chunks;
    for (int l = 0; l < n_lag; ++l) tab[3 * (size_t)n_seg + 1 + l] = h_lags[l];

    const size_t slab_cols = (size_t)std::max(F, kLagsPerLaunch);
    msm_status rs = msm_reserve_scratch(
        ctx, ((size_t)2 * n_seg * F + (size_t)std::max<int64_t>(n_chunks, 1) * slab_cols) * sizeof(double));
    if (rs != MSM_OK) return rs;
    const void* d_tab = nullptr;
    rs = msm_upload_table(ctx, tab.data(), tab_len * sizeof(int64_t), &d_tab);
    if (rs != MSM_OK) return rs;
    Tab tb;
    tb.start = (const int64_t*)d_tab;
    tb.stop = tb.start + n_seg;
    tb.prefix = tb.stop + n_seg;
    tb.n_seg = n_seg;
    const int64_t* d_lags = tb.prefix + n_seg + 1;
    if (dtype == MSM_F32)
        return run_lagscan<float>(ctx, (const float*)d_x, F, ld, tb, d_lags, n_lag, n_chunks, chunk_rows, tile_rows,
                                  var_floor, d_value, d_nvalid);
    return run_lagscan<double>(ctx, (const double*)d_x, F, ld, tb, d_lags, n_lag, n_chunks, chunk_rows, tile_rows,
                               var_floor, d_value, d_nvalid);
}

msm_status msm_hstack_f64(msm_ctx* ctx, const void* d_a, msm_dtype dtype_a, int pa, int64_t lda, const void* d_b,
                          msm_dtype dtype_b, int pb, int64_t ldb, int64_t n, double* d_out) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, (dtype_a == MSM_F32 || dtype_a == MSM_F64) && (dtype_b == MSM_F32 || dtype_b == MSM_F64),
                "msm_hstack_f64: bad dtype");
    MSM_REQUIRE(ctx, n >= 0 && pa >= 1 && pb >= 1 && lda >= pa && ldb >= pb, "msm_hstack_f64: bad shape");
    if (n == 0) return MSM_OK;
    MSM_REQUIRE(ctx, d_a && d_b && d_out, "msm_hstack_f64: NULL pointer");
    if (dtype_a == MSM_F32 && dtype_b == MSM_F32) launch_hstack<float, float>(ctx, d_a, pa, lda, d_b, pb, ldb, n, d_out);
    else if (dtype_a == MSM_F32) launch_hstack<float, double>(ctx, d_a, pa, lda, d_b, pb, ldb, n, d_out);
    else if (dtype_b == MSM_F32) launch_hstack<double, float>(ctx, d_a, pa, lda, d_b, pb, ldb, n, d_out);
    else launch_hstack<double, double>(ctx, d_a, pa, lda, d_b, pb, ldb, n, d_out);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
