// Mean silhouette coefficient of a clustering (model selection for n_states = "auto").
//
// Reference: _auto_select_n_states (S/markov_state_model/clustering.py:156-233) scores k = 4..20 with
// sklearn.metrics.silhouette_score: s_i = (b_i - a_i) / max(a_i, b_i), a_i = mean Euclidean distance to
// the other members of i's cluster, b_i = smallest mean distance to another cluster, s_i = 0 for
// singleton clusters; the score is the mean of s_i.
//
// Two entry points.
//
// msm_silhouette (k <= 32, points SORTED BY CLUSTER on the host, offsets[k+1]): every thread owns one query point
// and walks the clusters in order, so the per-cluster distance sums sit in registers with static indices; the
// reference points stream through LDS tiles shared by the workgroup.  One launch over all n^2 pairs.
//
// msm_silhouette_samples (any k, labels on the device, frames in their own order): the frames are grouped on the
// device (msm_group_by_label: offsets and members, nothing is sorted or copied), every cluster is cut into segments
// of at most MSM_SIL_SEG_LEN members, and the pair pass runs on a grid of (tile of MSM_SIL_TILE_I query frames) x
// (group of segments).  A workgroup writes, for each of its queries and each of its segments, the sum of the
// distances to that segment's members into a slab [segment][query]; a fold kernel then walks every query's segments
// in cluster order, adds the pieces of a cluster left to right and forms a_i, the running minimum b_i and s_i.
//   * Queries go by in chunks and segments in chunks, so the slab holds at most kSlabBytes (256 MiB) whatever n and k
//     are; the fold carries (sum of the cluster in progress, a_i, b_i) from one segment chunk to the next in the same
//     fp64 words, so where a chunk ends changes no sum.
//   * Launches are cut at max_products (i, j, feature) products, 2^36 by default (the medoid pass's value: a few
//     hundred milliseconds at the rate that pass runs at, short enough for a shared device).  The cut only decides which
//     launch computes a (tile, group); the order of every sum is fixed by the segment list, which follows from the
//     labels alone.  No atomics: the same bytes on every run and for every cut.
//   * Distances are direct differences under the root, sum_f fma(x_if - x_jf, x_if - x_jf, .), as in the medoid
//     pass of representatives.hip, whose register tile this is: a lane owns two queries and 16 of a tile's 64
//     reference rows, the reference words are LDS broadcasts shared by the two.
#include <algorithm>
#include <climits>

#include "common.h"
#include "wave.h"

namespace {

constexpr int kST = 256;
constexpr int kMaxK = 32;
constexpr int kTile = 64;

struct SilOffsets { int64_t off[kMaxK + 1]; };

// The NaN rule of both entry points.  A distance that is not a number (a NaN coordinate, inf - inf) makes the sums it
// enters NaN; the minimum over the other clusters and the maximum in the denominator are compare-selects that keep a
// NaN operand (fmin / fmax would drop it, and a poisoned cluster would silently leave b_i).  Whether another cluster
// exists is read off the counts, never off b_i < inf.  s_i = 0 for the member of a singleton, where no other cluster
// has a member, and where max(a_i, b_i) = 0; otherwise (b_i - a_i) / max(a_i, b_i) as IEEE gives it.  On finite
// input every select takes the operand fmin / fmax took.
__device__ __forceinline__ double nan_min(double run, double v) { return (v < run || v != v) ? v : run; }
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ double sample_value(double a_i, double b_i, int64_t n_own, int64_t n) {
    if (n_own <= 1 || n_own >= n) return 0.0;   // a singleton; no member outside i's cluster
    const double den = nan_max(a_i, b_i);
    return den == 0.0 ? 0.0 : (b_i - a_i) / den;
}

__global__ __launch_bounds__(kST) void silhouette_kernel(const double* __restrict__ x, int64_t n, int d, int64_t ld, int k,
                                                         SilOffsets so, double* __restrict__ s_out) {
    extern __shared__ double tile[];  // [kTile][d]
    const int64_t i = (int64_t)blockIdx.x * kST + threadIdx.x;
    const bool live = i < n;
    const double* xi = x + (live ? i : 0) * ld;
    double acc[kMaxK];
#pragma unroll
    for (int c = 0; c < kMaxK; ++c) acc[c] = 0.0;
#pragma unroll
    for (int c = 0; c < kMaxK; ++c) {
        if (c < k) {
            double a = 0.0;
            for (int64_t j0 = so.off[c]; j0 < so.off[c + 1]; j0 += kTile) {
                const int cnt = (int)min((int64_t)kTile, so.off[c + 1] - j0);
                __syncthreads();
                for (int e = threadIdx.x; e < cnt * d; e += kST) tile[e] = x[(j0 + e / d) * ld + e % d];
                __syncthreads();
                for (int j = 0; j < cnt; ++j) {
                    double d2 = 0.0;
                    const double* xj = tile + j * d;
                    for (int f = 0; f < d; ++f) {
                        const double df = xi[f] - xj[f];
                        d2 = fma(df, df, d2);
                    }
                    a += sqrt(d2);
                }
            }
            acc[c] = a;
        }
    }
    if (!live) return;
    int ci = 0;
#pragma unroll
    for (int c = 0; c < kMaxK; ++c)
        if (c < k && i >= so.off[c] && i < so.off[c + 1]) ci = c;
    double a_i = 0.0, b_i = __builtin_inf();
    int64_t n_ci = 1;
#pragma unroll
    for (int c = 0; c < kMaxK; ++c) {
        if (c < k) {
            const int64_t nc = so.off[c + 1] - so.off[c];
            if (c == ci) { n_ci = nc; a_i = nc > 1 ? acc[c] / (double)(nc - 1) : 0.0; }
            else if (nc > 0) b_i = nan_min(b_i, acc[c] / (double)nc);
        }
    }
    s_out[i] = sample_value(a_i, b_i, n_ci, n);
}

__global__ __launch_bounds__(1024) void mean_kernel(const double* __restrict__ v, int64_t n, double* __restrict__ out) {
    __shared__ double red[16];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) acc += v[i];
    acc = wave_sum_down(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += red[w];
        out[0] = t / (double)n;
    }
}


// ---- any k: segments, partial sums, fold -------------------------------------------------------------------------
constexpr int kT = 256;                       // threads of a workgroup of the pair pass (4 waves)
constexpr int kL = MSM_SIL_SEG_LEN;           // members of a segment at most
constexpr int kTI = MSM_SIL_TILE_I;           // query frames of a workgroup, two per lane
constexpr int kTJ = 64;                       // reference rows staged per tile, kTJ / 4 per wave
constexpr int kJW = kTJ / 4;
constexpr int kDC = 8;                        // features per staged chunk
constexpr int kGroupSegs = 16;                // segments of a group at most (small clusters share a workgroup)
constexpr int kSegChunk = 2048;               // segments of a slab at most
constexpr size_t kSlabBytes = (size_t)1 << 28;
constexpr int64_t kDefaultProducts = (int64_t)1 << 36;
constexpr int kMeanBlocks = 256;
static_assert(kTI == 128 && kT == 256 && kL % kTJ == 0, "tile shapes the pair kernel is written for");

struct SilSeg { int32_t cluster; int32_t start; int32_t len; };   // members[start, start + len) of `cluster`

// Workgroup (x, y) = (query tile t0 + x of the chunk, segment group g0 + y).  Lane l of every wave owns the queries
// 64 r + l (r = 0, 1) of the tile; wave v takes the rows [v * kJW, (v + 1) * kJW) of each staged tile of a segment.
// A lane adds its terms in ascending j; the four wave sums of a query are added in wave order.
// slab[(s - s0) * q_stride + q]: q = query index inside the chunk, s0 = first segment of the chunk.
__global__ __launch_bounds__(kT) void silhouette_pairs_kernel(const double* __restrict__ x, int d, int64_t ld,
                                                              const int32_t* __restrict__ members,
                                                              const SilSeg* __restrict__ segs,
                                                              const int32_t* __restrict__ group_first, int g0, int t0,
                                                              int64_t q0, int qn, int s0, int64_t q_stride,
                                                              double* __restrict__ slab) {
    __shared__ __attribute__((aligned(16))) double xj[kTJ][kDC];
    __shared__ int64_t rowj[kTJ];
    __shared__ double part[4][kTI];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qt = (t0 + (int)blockIdx.x) * kTI;   // first query of the tile, inside the chunk
    const int g = g0 + (int)blockIdx.y;
    const double* xi[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int q = qt + 64 * r + lane;
        xi[r] = x + (q0 + (q < qn ? q : 0)) * ld;   // queries past the end compute and are not stored
    }
    const int s_end = group_first[g + 1];
    for (int s = group_first[g]; s < s_end; ++s) {
        const SilSeg seg = segs[s];
        double acc[2] = {0.0, 0.0};
        for (int j0 = 0; j0 < seg.len; j0 += kTJ) {
            __syncthreads();   // the previous tile's readers (and the previous segment's part readers) are done
            if (threadIdx.x < kTJ) {
                const int j = j0 + threadIdx.x;
                rowj[threadIdx.x] = (int64_t)members[seg.start + (j < seg.len ? j : 0)] * ld;
            }
            double d2[2][kJW];
#pragma unroll
            for (int jj = 0; jj < kJW; ++jj) d2[0][jj] = d2[1][jj] = 0.0;
            for (int f0 = 0; f0 < d; f0 += kDC) {
                __syncthreads();   // rowj is written; the previous chunk's readers are done
                for (int e = threadIdx.x; e < kTJ * kDC; e += kT) {
                    const int j = e / kDC, f = f0 + e % kDC;
                    xj[j][e % kDC] = f < d ? x[rowj[j] + f] : 0.0;
                }
                double a[2][kDC];
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int f = 0; f < kDC; ++f) a[r][f] = f0 + f < d ? xi[r][f0 + f] : 0.0;
                __syncthreads();
#pragma unroll
                for (int fp = 0; fp < kDC; fp += 2) {
                    if (f0 + fp < d) {   // wave-uniform; a chunk's padding costs at most one feature
#pragma unroll
                        for (int jj = 0; jj < kJW; ++jj) {
                            const double b0 = xj[wave * kJW + jj][fp], b1 = xj[wave * kJW + jj][fp + 1];
#pragma unroll
                            for (int r = 0; r < 2; ++r) {
                                const double e0 = a[r][fp] - b0, e1 = a[r][fp + 1] - b1;
                                d2[r][jj] = fma(e1, e1, fma(e0, e0, d2[r][jj]));
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int jj = 0; jj < kJW; ++jj) {
                if (j0 + wave * kJW + jj < seg.len) {   // wave-uniform: a row past the end adds nothing
                    acc[0] += sqrt(d2[0][jj]);
                    acc[1] += sqrt(d2[1][jj]);
                }
            }
        }
        part[wave][lane] = acc[0];
        part[wave][64 + lane] = acc[1];
        __syncthreads();
        if (threadIdx.x < kTI) {
            const int q = qt + threadIdx.x;
            if (q < qn)
                slab[(int64_t)(s - s0) * q_stride + q] =
                    ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
        }
    }
}

// One thread per query of the chunk, over the segments [s0, s1) of a slab.  state f64 [3][q_stride] = (sum of the
// cluster in progress, a_i, min over the other clusters so far); read unless s0 == 0, written unless s1 == n_seg,
// where s_i is formed instead.  A cluster without members has no segment and so takes no part in b_i.
__global__ __launch_bounds__(kT) void silhouette_fold_kernel(const double* __restrict__ slab, const SilSeg* __restrict__ segs,
                                                             const int64_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ labels, int64_t n, int64_t q0,
                                                             int qn, int s0, int s1, int n_seg, int64_t q_stride,
                                                             double* __restrict__ state, double* __restrict__ s_out) {
    const int q = blockIdx.x * kT + threadIdx.x;
    if (q >= qn) return;
    const int ci = labels[q0 + q];
    double cur = 0.0, a_i = 0.0, b_i = __builtin_inf();
    if (s0 > 0) { cur = state[q]; a_i = state[q_stride + q]; b_i = state[2 * q_stride + q]; }
    int c_prev = s0 > 0 ? segs[s0 - 1].cluster : -1;
    auto close = [&](int c) {
        const int64_t nc = offsets[c + 1] - offsets[c];
        if (c == ci) a_i = nc > 1 ? cur / (double)(nc - 1) : 0.0;
        else b_i = nan_min(b_i, cur / (double)nc);
        cur = 0.0;
    };
    for (int s = s0; s < s1; ++s) {
        const int c = segs[s].cluster;   // one address per wave
        if (c != c_prev && c_prev >= 0) close(c_prev);
        cur += slab[(int64_t)(s - s0) * q_stride + q];
        c_prev = c;
    }
    if (s1 < n_seg) {
        state[q] = cur; state[q_stride + q] = a_i; state[2 * q_stride + q] = b_i;
        return;
    }
    if (c_prev >= 0) close(c_prev);
    s_out[q0 + q] = sample_value(a_i, b_i, offsets[ci + 1] - offsets[ci], n);
}

// Mean in two steps over a fixed partition: block b sums v[b * per, (b + 1) * per) (thread t its strided share in
// ascending order, the waves in wave order), then one wave adds the block sums in block order.
__global__ __launch_bounds__(kT) void mean_partial_kernel(const double* __restrict__ v, int64_t n, int64_t per,
                                                          double* __restrict__ partial) {
    __shared__ double red[kT / 64];
    const int64_t lo = (int64_t)blockIdx.x * per, hi = min(n, lo + per);
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kT) acc += v[i];
    const double t = block_sum_lane0(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(64) void mean_final_kernel(const double* __restrict__ partial, int nb, int64_t n,
                                                        double* __restrict__ out) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < nb; b += 64) acc += partial[b];
    acc = wave_sum_down(acc);
    if (threadIdx.x == 0) out[0] = acc / (double)n;
}

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// how the workspace is cut: everything follows from (n, k)
struct SilPlan {
    int seg_chunk;        // segments of a slab at most
    int64_t q_chunk;      // queries of a slab at most (a multiple of kTI)
    size_t off_offsets, off_members, off_state, off_slab, off_mean, bytes;
};

SilPlan sil_plan(int64_t n, int k) {
    SilPlan p;
    const int64_t seg_bound = n / kL + std::min<int64_t>(k, n) + 1;   // sum_c ceil(n_c / kL) is below this
    p.seg_chunk = (int)std::min<int64_t>(seg_bound, kSegChunk);
    const int64_t n_up = (n + kTI - 1) / kTI * kTI;
    const int64_t fit = (int64_t)(kSlabBytes / sizeof(double)) / p.seg_chunk / kTI * kTI;
    p.q_chunk = std::min<int64_t>(n_up, std::max<int64_t>(kTI, fit));
    size_t o = 0;
    p.off_offsets = o; o += align16(((size_t)k + 1) * sizeof(int64_t));
    p.off_members = o; o += align16((size_t)n * sizeof(int32_t));
    p.off_state = o;   o += align16((size_t)3 * p.q_chunk * sizeof(double));
    p.off_slab = o;    o += align16((size_t)p.seg_chunk * p.q_chunk * sizeof(double));
    p.off_mean = o;    o += align16((size_t)kMeanBlocks * sizeof(double));
    p.bytes = o;
    return p;
}

}  // namespace

extern "C" {

msm_status msm_silhouette(msm_ctx* ctx, const double* d_x, int64_t n, int d, int64_t ld, const int64_t* h_offsets, int k,
                          double* d_samples, double* d_score) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, n >= 2 && d >= 1 && d <= 128 && ld >= d, "msm_silhouette: need n >= 2 and 1 <= d <= 128");
    MSM_REQUIRE(ctx, k >= 2 && k <= kMaxK, "msm_silhouette: need 2 <= k <= %d clusters", kMaxK);
    MSM_REQUIRE(ctx, d_x && h_offsets && d_samples && d_score, "msm_silhouette: NULL pointer");
    SilOffsets so;
    for (int c = 0; c <= kMaxK; ++c) so.off[c] = c <= k ? h_offsets[c] : h_offsets[k];
    MSM_REQUIRE(ctx, so.off[0] == 0 && so.off[k] == n, "msm_silhouette: offsets must run from 0 to n");
    for (int c = 0; c < k; ++c) MSM_REQUIRE(ctx, so.off[c + 1] >= so.off[c], "msm_silhouette: offsets must be non-decreasing");
    const int grid = (int)((n + kST - 1) / kST);
    hipLaunchKernelGGL(silhouette_kernel, dim3(grid), dim3(kST), (size_t)kTile * d * sizeof(double), ctx->stream, d_x, n, d,
                       ld, k, so, d_samples);
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_samples, n, d_score);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

size_t msm_silhouette_workspace_bytes(int64_t n, int d, int k) {
    (void)d;
    if (n < 1 || k < 1) return 0;
    return sil_plan(n, k).bytes;
}

msm_status msm_silhouette_samples(msm_ctx* ctx, const double* d_x, int64_t n, int d, int64_t ld, const int32_t* d_labels,
                                  int k, void* d_work, size_t work_bytes, int64_t max_products, double* d_samples,
                                  double* d_score) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d_x && d_labels && d_work && d_samples && d_score, "msm_silhouette_samples: NULL pointer");
    MSM_REQUIRE(ctx, n >= 3 && n <= (int64_t)INT32_MAX, "msm_silhouette_samples: need 3 <= n < 2^31 (got %lld)", (long long)n);
    MSM_REQUIRE(ctx, d >= 1 && d <= MSM_REP_MAX_D && ld >= d, "msm_silhouette_samples: need 1 <= d <= %d and ld >= d (got d = %d)",
                MSM_REP_MAX_D, d);
    MSM_REQUIRE(ctx, k >= 2 && (int64_t)k <= n - 1, "msm_silhouette_samples: need 2 <= k <= n - 1 clusters (got k = %d, n = %lld)",
                k, (long long)n);
    MSM_REQUIRE(ctx, max_products >= 0, "msm_silhouette_samples: max_products must be >= 0 (0 = default)");
    if (ctx->capturing)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_silhouette_samples reads the cluster sizes on the host: not capturable");
    const SilPlan plan = sil_plan(n, k);
    MSM_REQUIRE(ctx, work_bytes >= plan.bytes, "msm_silhouette_samples: the workspace has %zu bytes, "
                "msm_silhouette_workspace_bytes asks for %zu", work_bytes, plan.bytes);
    const int64_t maxp = max_products > 0 ? max_products : kDefaultProducts;
    char* work = (char*)d_work;
    int64_t* offsets = (int64_t*)(work + plan.off_offsets);
    int32_t* members = (int32_t*)(work + plan.off_members);
    double* state = (double*)(work + plan.off_state);
    double* slab = (double*)(work + plan.off_slab);
    double* mean_part = (double*)(work + plan.off_mean);

    msm_status rs = msm_group_by_label(ctx, d_labels, n, k, offsets, members);
    if (rs != MSM_OK) return rs;
    std::vector<int64_t> h_off((size_t)k + 1);
    MSM_HIP(ctx, hipMemcpyAsync(h_off.data(), offsets, h_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    MSM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // a label outside [0, k) belongs to no state, so the states then hold fewer than n frames
    MSM_REQUIRE(ctx, h_off[k] == n, "msm_silhouette_samples: %lld of the %lld labels lie outside [0, %d)",
                (long long)(n - h_off[k]), (long long)n, k);

    // segments in cluster order; groups of consecutive segments with at most kL rows and kGroupSegs segments
    std::vector<SilSeg> segs;
    for (int c = 0; c < k; ++c)
        for (int64_t b = h_off[c]; b < h_off[c + 1]; b += kL)
            segs.push_back({(int32_t)c, (int32_t)b, (int32_t)std::min<int64_t>(kL, h_off[c + 1] - b)});
    const int n_seg = (int)segs.size();
    std::vector<int32_t> group_first{0};
    std::vector<int32_t> group_rows;
    {
        int rows = 0, cnt = 0;
        for (int s = 0; s < n_seg; ++s) {
            if (cnt > 0 && (rows + segs[s].len > kL || cnt == kGroupSegs)) {
                group_first.push_back(s);
                group_rows.push_back(rows);
                rows = cnt = 0;
            }
            rows += segs[s].len;
            ++cnt;
        }
        group_first.push_back(n_seg);
        group_rows.push_back(rows);
    }
    const int n_groups = (int)group_rows.size();
    // one table: segments, then the groups' first segments
    const size_t seg_bytes = align16(segs.size() * sizeof(SilSeg));
    std::vector<char> table(seg_bytes + group_first.size() * sizeof(int32_t));
    std::copy((const char*)segs.data(), (const char*)segs.data() + segs.size() * sizeof(SilSeg), table.begin());
    std::copy((const char*)group_first.data(), (const char*)group_first.data() + group_first.size() * sizeof(int32_t),
              table.begin() + seg_bytes);
    const void* d_tab = nullptr;
    rs = msm_upload_table(ctx, table.data(), table.size(), &d_tab);
    if (rs != MSM_OK) return rs;
    const SilSeg* d_segs = (const SilSeg*)d_tab;
    const int32_t* d_group_first = (const int32_t*)((const char*)d_tab + seg_bytes);

    for (int64_t q0 = 0; q0 < n; q0 += plan.q_chunk) {
        const int qn = (int)std::min<int64_t>(plan.q_chunk, n - q0);
        const int n_tiles = msm_ceil_div(qn, kTI);
        int g = 0;
        while (g < n_groups) {
            // a slab: whole groups with at most seg_chunk segments in all (one group alone never has more)
            int g_end = g + 1;
            while (g_end < n_groups && group_first[g_end + 1] - group_first[g] <= plan.seg_chunk) ++g_end;
            const int s0 = group_first[g], s1 = group_first[g_end];
            // launches of the slab: whole groups x all tiles while that fits the cut, else one group x some tiles
            int gl = g;
            while (gl < g_end) {
                int64_t rows = 0;
                int ge = gl;
                while (ge < g_end && ge - gl < 65535 && (int64_t)n_tiles * kTI * (rows + group_rows[ge]) * d <= maxp)
                    rows += group_rows[ge++];
                if (ge > gl) {
                    hipLaunchKernelGGL(silhouette_pairs_kernel, dim3(n_tiles, ge - gl), dim3(kT), 0, ctx->stream, d_x, d, ld,
                                       members, d_segs, d_group_first, gl, 0, q0, qn, s0, plan.q_chunk, slab);
                    MSM_CHECK_LAUNCH(ctx);
                    gl = ge;
                    continue;
                }
                const int tq = (int)std::max<int64_t>(1, maxp / ((int64_t)kTI * group_rows[gl] * d));
                for (int t0 = 0; t0 < n_tiles; t0 += tq) {
                    hipLaunchKernelGGL(silhouette_pairs_kernel, dim3(std::min(tq, n_tiles - t0), 1), dim3(kT), 0, ctx->stream,
                                       d_x, d, ld, members, d_segs, d_group_first, gl, t0, q0, qn, s0, plan.q_chunk, slab);
                    MSM_CHECK_LAUNCH(ctx);
                }
                ++gl;
            }
            hipLaunchKernelGGL(silhouette_fold_kernel, dim3(msm_ceil_div(qn, kT)), dim3(kT), 0, ctx->stream, slab, d_segs,
                               offsets, d_labels, n, q0, qn, s0, s1, n_seg, plan.q_chunk, state, d_samples);
            MSM_CHECK_LAUNCH(ctx);
            g = g_end;
        }
    }
    const int nb = (int)std::min<int64_t>(kMeanBlocks, msm_ceil_div(n, 4096));
    const int64_t per = (n + nb - 1) / nb;
    hipLaunchKernelGGL(mean_partial_kernel, dim3(nb), dim3(kT), 0, ctx->stream, d_samples, n, per, mean_part);
    hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(64), 0, ctx->stream, mean_part, nb, n, d_score);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
