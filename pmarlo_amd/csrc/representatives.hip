// Representative frames of a state: group frames by label, weighted state centroids, per-member scores
// (distance to the centroid, or the weighted sum of distances to every other member), and the selection.
//
// Reference: RepresentativePicker (S/conformations/representative_picker.py) and _find_representatives
// (S/markov_state_model/_states.py:131-157) walk np.where(labels == s) per state on the host and call
// np.linalg.norm once per member for the medoid.  Here the frames are grouped once, stably (the members of a
// state are in ascending frame order, exactly np.where), and every fp64 sum below is taken in member order
// over a fixed partition, so all outputs are the same bytes from run to run.  No atomics anywhere.
//
// Distances are direct differences sum_f (a_f - b_f)^2: no |a|^2 + |b|^2 - 2 a.b under a square root.
#include <algorithm>
#include <climits>

#include "common.h"
#include "wave.h"

namespace {

constexpr int kT = 256;                           // threads of every workgroup here (4 waves)
constexpr int kChunk = MSM_REP_GROUP_CHUNK;       // frames per grouping chunk
constexpr int kRows = kChunk / kT;                // frames a thread ranks
constexpr int kTI = MSM_REP_TILE_I;               // medoid: i-rows of a task, two per lane
constexpr int kTJ = MSM_REP_TILE_J;               // medoid: j-rows staged per tile, kTJ / 4 per wave
constexpr int kJW = kTJ / 4;
constexpr int kDC = 8;                            // medoid: features per staged chunk
static_assert(kTI == 128 && kTJ % 4 == 0 && kChunk % kT == 0, "tile shapes the kernels are written for");
// medoid launches are cut so that one launch holds at most this many (i, j, feature) products
constexpr int64_t kLaunchProducts = (int64_t)1 << 36;

struct RepTask { int32_t state; int32_t i0; };

// ---- grouping ------------------------------------------------------------------------------------------------
// One workgroup per chunk of kChunk frames.  rank[t] = number of earlier frames of the chunk with t's label; the
// last frame of a label in the chunk writes the chunk's count of it into hist[label][chunk] (zeroed before).
__global__ __launch_bounds__(kT) void group_rank_kernel(const int32_t* __restrict__ labels, int64_t n, int k, int n_chunks,
                                                        int32_t* __restrict__ rank, int32_t* __restrict__ hist) {
    __shared__ int32_t lab[kChunk];
    const int64_t base = (int64_t)blockIdx.x * kChunk;
    const int cnt = (int)min((int64_t)kChunk, n - base);
    for (int e = threadIdx.x; e < kChunk; e += kT) {
        const int32_t s = e < cnt ? labels[base + e] : -1;
        lab[e] = (s >= 0 && s < k) ? s : -1;
    }
    __syncthreads();
    int32_t mine[kRows], before[kRows], after[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) { mine[r] = lab[threadIdx.x + kT * r]; before[r] = 0; after[r] = 0; }
    for (int j = 0; j < cnt; ++j) {
        const int32_t lj = lab[j];   // one address per wave: a broadcast read
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int e = threadIdx.x + kT * r;
            const bool eq = lj == mine[r];
            before[r] += (eq && j < e) ? 1 : 0;
            after[r] |= (eq && j > e) ? 1 : 0;
        }
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int e = threadIdx.x + kT * r;
        if (e < cnt && mine[r] >= 0) {
            rank[base + e] = before[r];
            if (!after[r]) hist[(int64_t)mine[r] * n_chunks + blockIdx.x] = before[r] + 1;
        }
    }
}

// inclusive prefix sum over the wave (a scan, not a reduction: lane l gets v_0 + .. + v_l)
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// One wave per state: hist[s][c] -> number of members of s in the chunks before c; counts[s] = members of s.
__global__ __launch_bounds__(kT) void group_scan_chunks_kernel(int32_t* __restrict__ hist, int k, int n_chunks,
                                                               int64_t* __restrict__ counts) {
    const int s = blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
    if (s >= k) return;   // whole waves leave
    const int lane = threadIdx.x & 63;
    int32_t* row = hist + (int64_t)s * n_chunks;
    int32_t carry = 0;
    for (int c0 = 0; c0 < n_chunks; c0 += 64) {
        const int c = c0 + lane;
        const int32_t v = c < n_chunks ? row[c] : 0;
        const int32_t incl = wave_scan_incl(v);
        if (c < n_chunks) row[c] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) counts[s] = carry;
}

// One wave: offsets[s] = counts[0] + .. + counts[s-1], offsets[k] = total.  counts and offsets may not alias.
__global__ __launch_bounds__(64) void group_offsets_kernel(const int64_t* __restrict__ counts, int k,
                                                           int64_t* __restrict__ offsets) {
    const int lane = threadIdx.x;
    int64_t carry = 0;
    for (int s0 = 0; s0 < k; s0 += 64) {
        const int s = s0 + lane;
        const int64_t v = s < k ? counts[s] : 0;
        const int64_t incl = wave_scan_incl(v);
        if (s < k) offsets[s] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) offsets[k] = carry;
}

__global__ __launch_bounds__(kT) void group_place_kernel(const int32_t* __restrict__ labels, int64_t n, int k, int n_chunks,
                                                         const int32_t* __restrict__ rank, const int32_t* __restrict__ hist,
                                                         const int64_t* __restrict__ offsets, int32_t* __restrict__ members) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (t >= n) return;
    const int32_t s = labels[t];
    if (s < 0 || s >= k) return;
    members[offsets[s] + hist[(int64_t)s * n_chunks + t / kChunk] + rank[t]] = (int32_t)t;
}

// ---- centroids -----------------------------------------------------------------------------------------------
// One workgroup per state.  Thread (r0, f) = (tid / cw, tid % cw) sums column f over the members r0, r0 + R, ..
// in that order (R = kT / cw row lanes, cw = d rounded up to a power of two); the R partial sums are added in
// ascending r0.  The weight sum takes the same partition.
__global__ __launch_bounds__(kT) void state_centroid_kernel(const double* __restrict__ x, int d, int64_t ld,
                                                            const double* __restrict__ w,
                                                            const int64_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ members, int cw,
                                                            double* __restrict__ centroid, double* __restrict__ wsum,
                                                            int32_t* __restrict__ flags) {
    __shared__ double part[kT];
    __shared__ double part_w[kT];
    __shared__ double total_w;
    const int s = blockIdx.x;
    const int64_t o0 = offsets[s];
    const int64_t ns = offsets[s + 1] - o0;
    const int R = kT / cw;
    const int f = threadIdx.x % cw, r0 = threadIdx.x / cw;
    double acc = 0.0, accw = 0.0;
    int bad = 0;
    for (int64_t m = r0; m < ns; m += R) {
        const int64_t t = members[o0 + m];
        const double wt = w ? w[t] : 1.0;
        if (!isfinite(wt)) bad |= MSM_REP_FLAG_NONFINITE;
        if (wt < 0.0) bad |= MSM_REP_FLAG_NEGATIVE;
        accw += wt;
        if (f < d) acc += wt * x[t * ld + f];
    }
    part[threadIdx.x] = acc;       // [r0][f]
    part_w[threadIdx.x] = accw;
    const int any_nonfinite = __syncthreads_or(bad & MSM_REP_FLAG_NONFINITE);
    const int any_negative = __syncthreads_or(bad & MSM_REP_FLAG_NEGATIVE);
    if (threadIdx.x == 0) {
        double tw = 0.0;
        for (int r = 0; r < R; ++r) tw += part_w[r * cw];
        total_w = tw;
        wsum[s] = tw;
        int fl = 0;
        if (ns > 0) {
            if (any_nonfinite) fl |= MSM_REP_FLAG_NONFINITE;
            if (any_negative) fl |= MSM_REP_FLAG_NEGATIVE;
            if (!(tw > 0.0)) fl |= MSM_REP_FLAG_NONPOSITIVE_SUM;
        }
        flags[s] = fl;
    }
    __syncthreads();
    if (r0 == 0 && f < d) {
        double tx = 0.0;
        for (int r = 0; r < R; ++r) tx += part[r * cw + f];
        centroid[(int64_t)s * d + f] = ns > 0 ? tx / total_w : 0.0;
    }
}

// ---- scores --------------------------------------------------------------------------------------------------
// centroid mode: one thread per member, score = |x_i - c_s|_2, the state found through the frame's label
__global__ __launch_bounds__(kT) void centroid_score_kernel(const double* __restrict__ x, int d, int64_t ld,
                                                            const int32_t* __restrict__ labels,
                                                            const int32_t* __restrict__ members, int64_t total,
                                                            const double* __restrict__ centroid,
                                                            double* __restrict__ scores) {
    const int64_t m = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (m >= total) return;
    const int64_t t = members[m];
    const double* xi = x + t * ld;
    const double* c = centroid + (int64_t)labels[t] * d;
    double d2 = 0.0;
    for (int f = 0; f < d; ++f) {
        const double df = xi[f] - c[f];
        d2 = fma(df, df, d2);
    }
    scores[m] = sqrt(d2);
}

// medoid mode: score_i = sum_j w^_j |x_i - x_j|_2 over the members j of i's state, w^ = w / sum w (or 1 / n_s).
// A task is (state, tile of kTI i-rows); lane l of every wave owns the rows i0 + l and i0 + 64 + l.  The members
// go by in tiles of kTJ j-rows, wave v taking the rows [v * kJW, (v + 1) * kJW) of each tile, the features in
// chunks of kDC through LDS: every lane of a wave reads the same x_j word (a broadcast), and the squared distances
// of the 2 x kJW pairs a lane holds stay in registers across the chunks.  A lane adds its j terms in ascending j;
// the four wave sums of a row are added in wave order.
__global__ __launch_bounds__(kT) void medoid_score_kernel(const double* __restrict__ x, int d, int64_t ld,
                                                          const double* __restrict__ w,
                                                          const int64_t* __restrict__ offsets,
                                                          const int32_t* __restrict__ members,
                                                          const double* __restrict__ wsum,
                                                          const RepTask* __restrict__ tasks, double* __restrict__ scores) {
    __shared__ __attribute__((aligned(16))) double xj[kTJ][kDC];
    __shared__ double wj[kTJ];
    __shared__ int64_t rowj[kTJ];
    __shared__ double part[4][kTI];
    const RepTask task = tasks[blockIdx.x];
    const int64_t o0 = offsets[task.state];
    const int ns = (int)(offsets[task.state + 1] - o0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double unit = 1.0 / (double)ns, tw = wsum[task.state];
    const double* xi[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = task.i0 + 64 * r + lane;
        xi[r] = x + (int64_t)members[o0 + (i < ns ? i : 0)] * ld;   // rows past the end compute and are not stored
    }
    double acc[2] = {0.0, 0.0};
    for (int j0 = 0; j0 < ns; j0 += kTJ) {
        __syncthreads();   // the previous tile's readers are done
        if (threadIdx.x < kTJ) {
            const int j = j0 + threadIdx.x;
            const int64_t t = members[o0 + (j < ns ? j : 0)];
            rowj[threadIdx.x] = t * ld;
            wj[threadIdx.x] = j < ns ? (w ? w[t] / tw : unit) : 0.0;   // a row past the end adds +0
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
            const double wt = wj[wave * kJW + jj];
            acc[0] += wt * sqrt(d2[0][jj]);
            acc[1] += wt * sqrt(d2[1][jj]);
        }
    }
    part[wave][lane] = acc[0];
    part[wave][64 + lane] = acc[1];
    __syncthreads();
    if (threadIdx.x < kTI) {
        const int i = task.i0 + threadIdx.x;
        if (i < ns) scores[o0 + i] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
    }
}

// ---- selection -----------------------------------------------------------------------------------------------
// Arg-max over the workgroup, result in every thread: the larger value, the lower index on equal values, NaN never.
__device__ __forceinline__ void block_argmax(double& best, int& bi, double* redv, int* redi) {
    wave_argmax_down(best, bi);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { redv[threadIdx.x >> 6] = best; redi[threadIdx.x >> 6] = bi; }
    __syncthreads();
    best = redv[0];
    bi = redi[0];
    for (int v = 1; v < kT / 64; ++v)
        if (redv[v] > best || (redv[v] == best && redi[v] < bi)) { best = redv[v]; bi = redi[v]; }
}

// One workgroup per listed state: the min(n_reps, n_s) members with the smallest (score, frame), in that order.
// Round r takes the smallest pair above the pair round r - 1 took; the rest of a row is filled with -1.
__global__ __launch_bounds__(kT) void select_smallest_kernel(const int32_t* __restrict__ states,
                                                             const int64_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ members,
                                                             const double* __restrict__ scores, int n_reps,
                                                             int32_t* __restrict__ picks) {
    __shared__ double redv[kT / 64];
    __shared__ int redi[kT / 64];
    const int s = states[blockIdx.x];
    const int64_t o0 = offsets[s];
    const int ns = (int)(offsets[s + 1] - o0);
    int32_t* out = picks + (int64_t)blockIdx.x * n_reps;
    double last_v = 0.0;
    int last_m = -1;
    for (int r = 0; r < n_reps; ++r) {
        double best = -INFINITY;
        int bi = INT_MAX;
        for (int m = threadIdx.x; m < ns; m += kT) {
            const double sc = scores[o0 + m];
            const bool cand = r == 0 ? sc == sc : (sc > last_v || (sc == last_v && m > last_m));
            if (cand && (-sc > best || (-sc == best && m < bi))) { best = -sc; bi = m; }
        }
        block_argmax(best, bi, redv, redi);
        if (bi == INT_MAX) {   // the state is used up: the same in every thread
            for (int q = r + threadIdx.x; q < n_reps; q += kT) out[q] = -1;
            return;
        }
        if (threadIdx.x == 0) out[r] = members[o0 + bi];
        last_v = -best;
        last_m = bi;
    }
}

// One workgroup per listed state, all rounds in one launch: the first pick is the member nearest the centroid
// (scores = centroid distances), then mind_i = min(mind_i, |x_i - x_sel|) with the members already taken at -inf,
// and the next pick is the arg-max of mind, the lowest frame on equal values.  mind is laid out like scores; a
// thread touches only its own members' words, so the rounds need no ordering beyond the barriers of the arg-max.
// A NaN never wins: a member whose distance to a pick is NaN keeps mind = NaN and is never picked; once only such
// members are left the row ends in -1.
__global__ __launch_bounds__(kT) void select_diverse_kernel(const double* __restrict__ x, int d, int64_t ld,
                                                            const int32_t* __restrict__ states,
                                                            const int64_t* __restrict__ offsets,
                                                            const int32_t* __restrict__ members,
                                                            const double* __restrict__ scores, double* __restrict__ mind,
                                                            int n_reps, int32_t* __restrict__ picks) {
    __shared__ double redv[kT / 64];
    __shared__ int redi[kT / 64];
    __shared__ double xs[MSM_REP_MAX_D];
    const int s = states[blockIdx.x];
    const int64_t o0 = offsets[s];
    const int ns = (int)(offsets[s + 1] - o0);
    int32_t* out = picks + (int64_t)blockIdx.x * n_reps;
    const int n_sel = min(n_reps, ns);
    for (int q = n_sel + threadIdx.x; q < n_reps; q += kT) out[q] = -1;
    if (n_sel == 0) return;
    double best = -INFINITY;
    int bi = INT_MAX;
    for (int m = threadIdx.x; m < ns; m += kT) {
        const double sc = scores[o0 + m];
        mind[o0 + m] = INFINITY;
        if (-sc > best || (-sc == best && m < bi)) { best = -sc; bi = m; }
    }
    block_argmax(best, bi, redv, redi);
    if (bi == INT_MAX) bi = 0;   // every distance NaN: np.argmin gives the first
    int sel = bi;
    if (threadIdx.x == 0) out[0] = members[o0 + sel];
    for (int r = 1; r < n_sel; ++r) {
        __syncthreads();   // xs readers of the previous round are done
        const int64_t ts = members[o0 + sel];
        for (int f = threadIdx.x; f < d; f += kT) xs[f] = x[ts * ld + f];
        __syncthreads();
        best = -INFINITY;
        bi = INT_MAX;
        for (int m = threadIdx.x; m < ns; m += kT) {
            double v = mind[o0 + m];
            if (m == sel) v = -INFINITY;
            else if (v != -INFINITY) {
                const double* xi = x + (int64_t)members[o0 + m] * ld;
                double d2 = 0.0;
                for (int f = 0; f < d; ++f) {
                    const double df = xi[f] - xs[f];
                    d2 = fma(df, df, d2);
                }
                const double dist = sqrt(d2);
                v = (dist < v || dist != dist) ? dist : v;   // a NaN distance stays in mind (fmin would drop it)
            }
            mind[o0 + m] = v;
            // a member already taken (-inf) is no candidate, so a round with nothing but NaN left finds no index
            if (v != -INFINITY && (v > best || (v == best && m < bi))) { best = v; bi = m; }
        }
        block_argmax(best, bi, redv, redi);
        if (bi == INT_MAX) {   // every value NaN (NaN features): no index to follow, the same in every thread
            for (int q = r + threadIdx.x; q < n_sel; q += kT) out[q] = -1;
            return;
        }
        sel = bi;
        if (threadIdx.x == 0) out[r] = members[o0 + sel];
    }
}

int pow2_at_least(int d) {
    int c = 1;
    while (c < d) c <<= 1;
    return c;
}

}  // namespace

extern "C" {

msm_status msm_group_by_label(msm_ctx* ctx, const int32_t* d_labels, int64_t n, int k, int64_t* d_offsets,
                              int32_t* d_members) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d_labels && d_offsets && d_members && n >= 1 && k >= 1, "msm_group_by_label: bad arguments");
    if (n > (int64_t)INT32_MAX) return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_group_by_label: more than 2^31 - 1 frames");
    const int n_chunks = msm_ceil_div(n, kChunk);
    // scratch: hist int32 [k][n_chunks] | rank int32 [n] | counts int64 [k]
    const size_t hist_bytes = ((size_t)k * n_chunks * sizeof(int32_t) + 15) & ~(size_t)15;
    const size_t rank_bytes = ((size_t)n * sizeof(int32_t) + 15) & ~(size_t)15;
    msm_status rs = msm_reserve_scratch(ctx, hist_bytes + rank_bytes + (size_t)k * sizeof(int64_t));
    if (rs != MSM_OK) return rs;
    int32_t* hist = (int32_t*)ctx->scratch;
    int32_t* rank = (int32_t*)((char*)ctx->scratch + hist_bytes);
    int64_t* counts = (int64_t*)((char*)ctx->scratch + hist_bytes + rank_bytes);
    MSM_HIP(ctx, hipMemsetAsync(hist, 0, hist_bytes, ctx->stream));
    hipLaunchKernelGGL(group_rank_kernel, dim3(n_chunks), dim3(kT), 0, ctx->stream, d_labels, n, k, n_chunks, rank, hist);
    hipLaunchKernelGGL(group_scan_chunks_kernel, dim3(msm_ceil_div(k, kT / 64)), dim3(kT), 0, ctx->stream, hist, k,
                       n_chunks, counts);
    hipLaunchKernelGGL(group_offsets_kernel, dim3(1), dim3(64), 0, ctx->stream, counts, k, d_offsets);
    hipLaunchKernelGGL(group_place_kernel, dim3(msm_ceil_div(n, kT)), dim3(kT), 0, ctx->stream, d_labels, n, k, n_chunks,
                       rank, hist, d_offsets, d_members);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_state_centroids(msm_ctx* ctx, const double* d_x, int64_t n, int d, int64_t ld, const double* d_w,
                               const int64_t* d_offsets, const int32_t* d_members, int k, double* d_centroid,
                               double* d_wsum, int32_t* d_flags) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d_x && d_offsets && d_members && d_centroid && d_wsum && d_flags && n >= 1 && k >= 1 && d >= 1 &&
                ld >= d, "msm_state_centroids: bad arguments");
    if (d > MSM_REP_MAX_D) return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_state_centroids: d = %d > %d", d, MSM_REP_MAX_D);
    hipLaunchKernelGGL(state_centroid_kernel, dim3(k), dim3(kT), 0, ctx->stream, d_x, d, ld, d_w, d_offsets, d_members,
                       pow2_at_least(d), d_centroid, d_wsum, d_flags);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_state_scores(msm_ctx* ctx, const double* d_x, int64_t n, int d, int64_t ld, const double* d_w,
                            const int32_t* d_labels, const int64_t* d_offsets, const int32_t* d_members, int k,
                            const double* d_centroid, const double* d_wsum, int mode, const int64_t* h_offsets,
                            const int32_t* h_states, int n_states, double* d_scores) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d_x && d_offsets && d_members && d_scores && h_offsets && n >= 1 && k >= 1 && d >= 1 && ld >= d,
                "msm_state_scores: bad arguments");
    MSM_REQUIRE(ctx, mode == MSM_REP_SCORE_CENTROID || mode == MSM_REP_SCORE_MEDOID, "msm_state_scores: unknown mode %d", mode);
    if (d > MSM_REP_MAX_D) return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_state_scores: d = %d > %d", d, MSM_REP_MAX_D);
    const int64_t total = h_offsets[k];
    MSM_REQUIRE(ctx, h_offsets[0] == 0 && total >= 0 && total <= n, "msm_state_scores: offsets must run from 0 to at most n");
    if (mode == MSM_REP_SCORE_CENTROID) {
        MSM_REQUIRE(ctx, d_labels && d_centroid, "msm_state_scores: the centroid mode needs labels and centroids");
        if (total == 0) return MSM_OK;
        hipLaunchKernelGGL(centroid_score_kernel, dim3(msm_ceil_div(total, kT)), dim3(kT), 0, ctx->stream, d_x, d, ld,
                           d_labels, d_members, total, d_centroid, d_scores);
        MSM_CHECK_LAUNCH(ctx);
        return MSM_OK;
    }
    MSM_REQUIRE(ctx, d_wsum && (h_states || n_states == 0) && n_states >= 0, "msm_state_scores: the medoid mode needs the "
                "weight sums and a state list");
    if (ctx->capturing) return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_state_scores builds its task list on the host: not capturable");
    // tasks in list order, cut into launches of at most kLaunchProducts (i, j, feature) products
    std::vector<RepTask> tasks;
    std::vector<int64_t> cost;
    for (int q = 0; q < n_states; ++q) {
        const int s = h_states[q];
        MSM_REQUIRE(ctx, s >= 0 && s < k, "msm_state_scores: state %d outside [0, %d)", s, k);
        const int64_t ns = h_offsets[s + 1] - h_offsets[s];
        MSM_REQUIRE(ctx, ns >= 0 && h_offsets[s + 1] <= total, "msm_state_scores: offsets must be non-decreasing");
        for (int64_t i0 = 0; i0 < ns; i0 += kTI) {
            tasks.push_back({(int32_t)s, (int32_t)i0});
            cost.push_back((int64_t)kTI * ns * d);
        }
    }
    if (tasks.empty()) return MSM_OK;
    const void* d_tab = nullptr;
    msm_status rs = msm_upload_table(ctx, tasks.data(), tasks.size() * sizeof(RepTask), &d_tab);
    if (rs != MSM_OK) return rs;
    const RepTask* d_tasks = (const RepTask*)d_tab;
    size_t first = 0;
    while (first < tasks.size()) {
        size_t last = first;
        int64_t sum = 0;
        while (last < tasks.size() && (last == first || sum + cost[last] <= kLaunchProducts)) sum += cost[last++];
        hipLaunchKernelGGL(medoid_score_kernel, dim3((unsigned)(last - first)), dim3(kT), 0, ctx->stream, d_x, d, ld, d_w,
                           d_offsets, d_members, d_wsum, d_tasks + first, d_scores);
        MSM_CHECK_LAUNCH(ctx);
        first = last;
    }
    return MSM_OK;
}

msm_status msm_state_select(msm_ctx* ctx, const double* d_x, int64_t n, int d, int64_t ld, const int64_t* d_offsets,
                            const int32_t* d_members, int k, const double* d_scores, double* d_mind, int mode,
                            const int32_t* h_states, int n_states, int n_reps, int32_t* d_picks) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d_offsets && d_members && d_scores && d_picks && h_states && n >= 1 && k >= 1 && n_states >= 1 &&
                n_reps >= 1, "msm_state_select: bad arguments");
    MSM_REQUIRE(ctx, mode == MSM_REP_SELECT_SMALLEST || mode == MSM_REP_SELECT_DIVERSE, "msm_state_select: unknown mode %d", mode);
    if (ctx->capturing) return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_state_select uploads its state list: not capturable");
    std::vector<char> seen((size_t)k, 0);
    for (int q = 0; q < n_states; ++q) {
        const int s = h_states[q];
        MSM_REQUIRE(ctx, s >= 0 && s < k, "msm_state_select: state %d outside [0, %d)", s, k);
        MSM_REQUIRE(ctx, !seen[s], "msm_state_select: state %d is listed twice (the states of a call share the mind buffer)", s);
        seen[s] = 1;
    }
    if (mode == MSM_REP_SELECT_DIVERSE) {
        MSM_REQUIRE(ctx, d_x && d_mind && d >= 1 && ld >= d, "msm_state_select: the diverse mode needs the features and a mind buffer");
        if (d > MSM_REP_MAX_D) return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_state_select: d = %d > %d", d, MSM_REP_MAX_D);
    }
    const void* d_tab = nullptr;
    msm_status rs = msm_upload_table(ctx, h_states, (size_t)n_states * sizeof(int32_t), &d_tab);
    if (rs != MSM_OK) return rs;
    const int32_t* d_states = (const int32_t*)d_tab;
    if (mode == MSM_REP_SELECT_SMALLEST)
        hipLaunchKernelGGL(select_smallest_kernel, dim3(n_states), dim3(kT), 0, ctx->stream, d_states, d_offsets, d_members,
                           d_scores, n_reps, d_picks);
    else
        hipLaunchKernelGGL(select_diverse_kernel, dim3(n_states), dim3(kT), 0, ctx->stream, d_x, d, ld, d_states, d_offsets,
                           d_members, d_scores, d_mind, n_reps, d_picks);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
