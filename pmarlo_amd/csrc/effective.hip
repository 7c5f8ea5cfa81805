// Effective count matrix (Noe 2015; deeptime 0.4.5 TransitionCountEstimator(count_mode="effective"),
// deeptime.markov.tools.estimation effective_count_matrix / statistical_inefficiencies): the sliding counts C
// scaled by the statistical inefficiency of every transition's indicator series.  deeptime walks every non-zero
// cell in a Python loop over float arrays; here the loop is integer pair counting over grouped occurrence lists.
// The contract (include/msmhip.h) is this engine's own statement of the documented
// algorithm; parity with deeptime's output is not pinned.
//
// A start frame is a frame t of a segment [start, stop) with t + lag < stop and both labels in [0, k).  Row i is
// the list of its start frames in time order (msm_group_by_label on the masked labels); the start frames of one
// segment form one sub-sequence, a contiguous range [head, end) of row ranks.  Grouping the start frames by
// target and then, stably, by state leaves them sorted by (state, target, time): the occurrence list of cell
// (i, j) is a contiguous slice whose offset is the exclusive prefix sum of C.  Per occurrence three row ranks are
// kept: its own, its sub-sequence's head and end.  With those
//   S_l = occurrence pairs of one sub-sequence at rank distance l,
//   A_l = occurrences with end - 1 - rank >= l,   B_l = occurrences with rank - head >= l,
//   n_l = N_i - (row members with rank - head < l)      (a per-row prefix sum of the head-distance histogram).
// Everything up to the sign of Q_l is integer arithmetic (Q_l in __int128); the histograms are LDS int32 atomics,
// so no result depends on scheduling.  Only the sum of acf_l (1 - l / M_i) is fp64, taken in ascending l by one
// thread.
#include <algorithm>

#include "common.h"
#include "wave.h"

namespace {

constexpr int kT = 256;
constexpr int kB = MSM_EFF_LAG_BLOCK;
static_assert(kB == kT, "one thread per lag of a block");

struct EffState {       // per cell, lives in the work buffer between launches
    double corrsum;
    int32_t next_lag;
    int32_t done;
};

struct EffWork {
    int64_t* seg;        // [2 * n_seg]: starts, then stops - lag (the end of the start frames)
    int32_t* key_i;      // [n] state of a start frame, else -1
    int32_t* key_j;      // [n] target of a start frame, else -1; later the states in target order
    int32_t* mem0;       // [n] start frames by state, time order
    int32_t* mem1;       // [n] start frames by target
    int32_t* mem2;       // [n] positions of mem1 by state: (state, target, time) order
    int32_t* nless;      // [n] row i at off0[i]: head-distance histogram, then its exclusive prefix sum
    int32_t* occ_rank;   // [n] per occurrence in (state, target, time) order: row rank,
    int32_t* occ_head;   //     row rank of the first member of its sub-sequence,
    int32_t* occ_end;    //     one past the row rank of the last
    int64_t* off0;       // [k + 1] row offsets (exclusive prefix sum of N_i)
    int64_t* off1;       // [k + 1]
    int64_t* off2;       // [k + 1]
    int64_t* pairoff;    // [k * k] offset of a cell's occurrence list
    EffState* state;     // [k * k]
    int32_t* row_m;      // [k] M_i
    double* row_num;     // [k] sum_j C_ij si_ij
    int32_t* counter;    // [1] cells a launch left unfinished
};

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

size_t eff_layout(int64_t n, int k, int n_seg, char* base, EffWork* w) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
    const size_t nn = (size_t)std::max<int64_t>(n, 1), kk = (size_t)k * k;
    EffWork t;
    t.seg = (int64_t*)take((size_t)2 * std::max(n_seg, 1) * sizeof(int64_t));
    t.key_i = (int32_t*)take(nn * 4);
    t.key_j = (int32_t*)take(nn * 4);
    t.mem0 = (int32_t*)take(nn * 4);
    t.mem1 = (int32_t*)take(nn * 4);
    t.mem2 = (int32_t*)take(nn * 4);
    t.nless = (int32_t*)take(nn * 4);
    t.occ_rank = (int32_t*)take(nn * 4);
    t.occ_head = (int32_t*)take(nn * 4);
    t.occ_end = (int32_t*)take(nn * 4);
    t.off0 = (int64_t*)take((size_t)(k + 1) * 8);
    t.off1 = (int64_t*)take((size_t)(k + 1) * 8);
    t.off2 = (int64_t*)take((size_t)(k + 1) * 8);
    t.pairoff = (int64_t*)take(kk * 8);
    t.state = (EffState*)take(kk * sizeof(EffState));
    t.row_m = (int32_t*)take((size_t)k * 4);
    t.row_num = (double*)take((size_t)k * 8);
    t.counter = (int32_t*)take(16);
    if (w) *w = t;
    return off;
}

// first index in [lo, hi) with a[index] >= v (hi when there is none)
__device__ __forceinline__ int lower_bound_i32(const int32_t* __restrict__ a, int lo, int hi, int64_t v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the last segment whose first frame is <= t, -1 when t lies before all (seg[s] ascending)
__device__ __forceinline__ int seg_of(const int64_t* __restrict__ seg, int n_seg, int64_t t) {
    int lo = 0, hi = n_seg;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (seg[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__global__ __launch_bounds__(kT) void eff_keys_kernel(const int32_t* __restrict__ labels, int64_t n, int k, int lag,
                                                      const int64_t* __restrict__ seg, int n_seg,
                                                      int32_t* __restrict__ key_i, int32_t* __restrict__ key_j) {
    const int64_t t = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (t >= n) return;
    int32_t a = -1, b = -1;
    const int s = seg_of(seg, n_seg, t);
    if (s >= 0 && t < seg[n_seg + s]) {   // t + lag < stop <= n
        a = labels[t];
        b = labels[t + lag];
        if ((unsigned)a >= (unsigned)k || (unsigned)b >= (unsigned)k) { a = -1; b = -1; }
    }
    key_i[t] = a;
    key_j[t] = b;
}

// the states of the start frames in target order (mem1), -1 past the last start frame
__global__ __launch_bounds__(kT) void eff_keys2_kernel(const int32_t* __restrict__ key_i, const int32_t* __restrict__ mem1,
                                                       const int64_t* __restrict__ off1, int k, int64_t n,
                                                       int32_t* __restrict__ keys2) {
    const int64_t m = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (m >= n) return;
    keys2[m] = m < off1[k] ? key_i[mem1[m]] : -1;
}

// One workgroup per row: pairoff[i][j] = off0[i] + C[i][0] + .. + C[i][j-1]; clears the row's cells, M_i and the
// head-distance histogram.
__global__ __launch_bounds__(kT) void eff_rows_kernel(const int64_t* __restrict__ counts, int k,
                                                      const int64_t* __restrict__ off0, int64_t* __restrict__ pairoff,
                                                      EffState* __restrict__ state, int32_t* __restrict__ trunc,
                                                      int32_t* __restrict__ row_m, int32_t* __restrict__ nless) {
    __shared__ int64_t wave_tot[kT / 64];
    __shared__ int64_t carry_s;
    const int i = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t o0 = off0[i], o1 = off0[i + 1];
    for (int64_t m = o0 + threadIdx.x; m < o1; m += kT) nless[m] = 0;
    if (threadIdx.x == 0) { carry_s = o0; row_m[i] = 0; }
    __syncthreads();
    for (int j0 = 0; j0 < k; j0 += kT) {
        const int j = j0 + threadIdx.x;
        const int64_t c = j < k ? counts[(int64_t)i * k + j] : 0;
        int64_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int64_t before = carry_s;
        for (int w = 0; w < wave; ++w) before += wave_tot[w];
        if (j < k) {
            const int64_t p = (int64_t)i * k + j;
            pairoff[p] = before + incl - c;
            state[p] = EffState{0.0, 0, c > 0 ? 0 : 1};
            trunc[p] = 0;
        }
        __syncthreads();
        if (threadIdx.x == kT - 1) carry_s = before + incl;
        __syncthreads();
    }
}

// One thread per occurrence q (in (state, target, time) order): its row rank and its sub-sequence's rank range,
// the head-distance histogram of its row and M_i.
__global__ __launch_bounds__(kT) void eff_occ_kernel(const int32_t* __restrict__ key_i, const int32_t* __restrict__ mem0,
                                                     const int32_t* __restrict__ mem1, const int32_t* __restrict__ mem2,
                                                     const int64_t* __restrict__ off0, int k, int64_t n,
                                                     const int64_t* __restrict__ seg, int n_seg,
                                                     int32_t* __restrict__ occ_rank, int32_t* __restrict__ occ_head,
                                                     int32_t* __restrict__ occ_end, int32_t* __restrict__ nless,
                                                     int32_t* __restrict__ row_m) {
    const int64_t q = (int64_t)blockIdx.x * kT + threadIdx.x;
    if (q >= n || q >= off0[k]) return;
    const int64_t t = mem1[mem2[q]];
    const int i = key_i[t];
    const int64_t o0 = off0[i];
    const int ni = (int)(off0[i + 1] - o0);
    const int32_t* row = mem0 + o0;
    const int s = seg_of(seg, n_seg, t);
    const int r = lower_bound_i32(row, 0, ni, t);
    const int head = lower_bound_i32(row, 0, r + 1, seg[s]);
    const int end = lower_bound_i32(row, r, ni, seg[n_seg + s]);
    occ_rank[q] = r;
    occ_head[q] = head;
    occ_end[q] = end;
    atomicAdd(&nless[o0 + (r - head)], 1);
    if (r == head) atomicMax(&row_m[i], end - head);   // once per sub-sequence
}

// One workgroup per row: the histogram of head distances becomes its exclusive prefix sum, in place.
__global__ __launch_bounds__(kT) void eff_nless_kernel(const int64_t* __restrict__ off0, int32_t* __restrict__ nless) {
    __shared__ int32_t wave_tot[kT / 64];
    __shared__ int32_t carry_s;
    const int i = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t o0 = off0[i];
    const int64_t ni = off0[i + 1] - o0;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t m0 = 0; m0 < ni; m0 += kT) {
        const int64_t m = m0 + threadIdx.x;
        const int32_t v = m < ni ? nless[o0 + m] : 0;
        int32_t incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int32_t before = carry_s;
        for (int w = 0; w < wave; ++w) before += wave_tot[w];
        if (m < ni) nless[o0 + m] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == kT - 1) carry_s = before + incl;
        __syncthreads();
    }
}

// One workgroup per cell; at most `blocks` lag blocks of kB lags, then the state goes back to the work buffer.
__global__ __launch_bounds__(kT) void eff_ineff_kernel(const int64_t* __restrict__ counts, int k,
                                                       const int64_t* __restrict__ off0,
                                                       const int64_t* __restrict__ pairoff,
                                                       const int32_t* __restrict__ occ_rank,
                                                       const int32_t* __restrict__ occ_head,
                                                       const int32_t* __restrict__ occ_end,
                                                       const int32_t* __restrict__ nless,
                                                       const int32_t* __restrict__ row_m, int blocks,
                                                       EffState* __restrict__ state, int32_t* __restrict__ trunc,
                                                       int32_t* __restrict__ counter) {
    __shared__ int32_t hist_s[kB], hist_a[kB], hist_b[kB];
    __shared__ int32_t scan_a[2][kB], scan_b[2][kB];
    __shared__ double term[kB];
    __shared__ int32_t ge_a, ge_b, first_bad;
    __shared__ int32_t sh_next, sh_done;
    __shared__ double sh_corr;
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    if (state[p].done) return;   // the same in every thread: nothing below has been written yet
    const int i = (int)(p / k);
    const int c = (int)counts[p];
    const int64_t o0 = off0[i];
    const int64_t N = off0[i + 1] - o0;
    const int M = row_m[i];
    const int32_t* __restrict__ rk = occ_rank + pairoff[p];
    const int32_t* __restrict__ hd = occ_head + pairoff[p];
    const int32_t* __restrict__ en = occ_end + pairoff[p];
    const int32_t* __restrict__ nl = nless + o0;
    if (tid == 0) { sh_next = state[p].next_lag; sh_done = 0; sh_corr = state[p].corrsum; }
    __syncthreads();
    for (int blk = 0; blk < blocks; ++blk) {
        const int l0 = sh_next;
        const int L = min(kB, M - l0);   // >= 1: a cell is closed as soon as next_lag reaches M
        hist_s[tid] = 0;
        hist_a[tid] = 0;
        hist_b[tid] = 0;
        if (tid == 0) { ge_a = 0; ge_b = 0; first_bad = kB; }
        __syncthreads();
        int more_a = 0, more_b = 0;
        for (int a = tid; a < c; a += kT) {
            const int ra = rk[a], ea = en[a];
            const int tail = ea - 1 - ra, head = ra - hd[a];
            if (tail >= l0) { if (tail - l0 < kB) atomicAdd(&hist_a[tail - l0], 1); else ++more_a; }
            if (head >= l0) { if (head - l0 < kB) atomicAdd(&hist_b[head - l0], 1); else ++more_b; }
            // partners b >= a of the same sub-sequence (rank < ea) at rank distance in [l0, l0 + kB); ranks grow
            // by at least one per occurrence, so the first lies in [a, a + l0]
            const int64_t lo = (int64_t)ra + l0;
            if (lo < ea) {
                const int lim = (int)min((int64_t)ea, lo + kB);
                // and the one past the last before a + (lim - ra)
                const int b0 = lower_bound_i32(rk, a, (int)min((int64_t)c, (int64_t)a + l0 + 1), lo);
                const int b1 = lower_bound_i32(rk, b0, (int)min((int64_t)c, (int64_t)a + (lim - ra)), lim);
                const int cnt = b1 - b0;
                // the lanes of a wave hold consecutive a: each starts at its own partner, so that in a dense
                // stretch they add to different bins at a time (integer sums: the order changes nothing)
                int u = cnt > 0 ? (tid & 63) % cnt : 0;
                for (int d = 0; d < cnt; ++d) {
                    atomicAdd(&hist_s[rk[b0 + u] - (int)lo], 1);
                    if (++u == cnt) u = 0;
                }
            }
        }
        if (more_a) atomicAdd(&ge_a, more_a);
        if (more_b) atomicAdd(&ge_b, more_b);
        __syncthreads();
        // inclusive suffix sums of the two distance histograms (Hillis-Steele, double buffered)
        scan_a[0][tid] = hist_a[tid];
        scan_b[0][tid] = hist_b[tid];
        __syncthreads();
        int cur = 0;
        for (int off = 1; off < kB; off <<= 1) {
            int32_t va = scan_a[cur][tid], vb = scan_b[cur][tid];
            if (tid + off < kB) { va += scan_a[cur][tid + off]; vb += scan_b[cur][tid + off]; }
            scan_a[cur ^ 1][tid] = va;
            scan_b[cur ^ 1][tid] = vb;
            cur ^= 1;
            __syncthreads();
        }
        if (tid < L) {
            const int l = l0 + tid;
            const int64_t Al = (int64_t)scan_a[cur][tid] + ge_a, Bl = (int64_t)scan_b[cur][tid] + ge_b;
            const int64_t n_l = N - nl[l];
            const __int128 NN = (__int128)N * N;
            const __int128 Q = (__int128)hist_s[tid] * NN - (__int128)c * N * (Al + Bl) + (__int128)c * c * n_l;
            if (Q <= 0) {
                atomicMin(&first_bad, tid);
                term[tid] = 0.0;
            } else {
                // acf_l (1 - l / M) = Q (M - l) / (N^2 n_l M); Q > 0 here, its two halves convert exactly or round once
                const unsigned __int128 uq = (unsigned __int128)Q;
                const double qd = (double)(unsigned long long)(uq >> 64) * 18446744073709551616.0 +
                                  (double)(unsigned long long)uq;
                term[tid] = l == 0 ? 0.0 : (qd * (double)(M - l)) / ((double)N * (double)N * (double)n_l * (double)M);
            }
        }
        __syncthreads();
        if (tid == 0) {
            const int stop = min((int)first_bad, L);
            double cs = sh_corr;
            for (int u = 0; u < stop; ++u) cs += term[u];   // ascending lag; the lag-0 slot holds 0
            sh_corr = cs;
            sh_next = l0 + stop;
            if (first_bad < L || l0 + L >= M) sh_done = 1;
        }
        __syncthreads();
        if (sh_done) break;
    }
    if (tid == 0) {
        state[p] = EffState{sh_corr, sh_next, sh_done};
        if (sh_done) trunc[p] = sh_next;
        else atomicAdd(counter, 1);
    }
}

// One workgroup per row: si and the row's sum_j C_ij si_ij (thread partial sums in ascending j, then a fixed tree).
__global__ __launch_bounds__(kT) void eff_si_kernel(const int64_t* __restrict__ counts, int k,
                                                    const int64_t* __restrict__ off0,
                                                    const EffState* __restrict__ state, double mact,
                                                    double* __restrict__ si, double* __restrict__ row_num) {
    __shared__ double red[kT / 64];
    const int i = blockIdx.x;
    const double N = (double)(off0[i + 1] - off0[i]);
    double part = 0.0;
    for (int j = threadIdx.x; j < k; j += kT) {
        const int64_t p = (int64_t)i * k + j;
        const int64_t c = counts[p];
        double s = 0.0;
        if (c > 0) {
            s = 1.0 / (1.0 + 2.0 * mact * state[p].corrsum * N / (double)c);
            part += (double)c * s;
        }
        si[p] = s;
    }
    const double tot = block_sum_lane0(part, red);
    if (threadIdx.x == 0) row_num[i] = tot;
}

__global__ __launch_bounds__(kT) void eff_apply_kernel(const int64_t* __restrict__ counts, int k,
                                                       const int64_t* __restrict__ off0,
                                                       const double* __restrict__ si,
                                                       const double* __restrict__ row_num, int average,
                                                       double* __restrict__ ceff) {
    __shared__ double w_s;
    const int i = blockIdx.x;
    if (threadIdx.x == 0) {
        double w = 0.0;
        if (average == MSM_EFF_AVERAGE_ROW) {
            const int64_t N = off0[i + 1] - off0[i];
            w = N > 0 ? row_num[i] / (double)N : 0.0;
        } else if (average == MSM_EFF_AVERAGE_ALL) {
            double num = 0.0;
            for (int r = 0; r < k; ++r) num += row_num[r];   // ascending rows, the same in every workgroup
            w = off0[k] > 0 ? num / (double)off0[k] : 0.0;
        }
        w_s = w;
    }
    __syncthreads();
    const double w = w_s;
    for (int j = threadIdx.x; j < k; j += kT) {
        const int64_t p = (int64_t)i * k + j;
        ceff[p] = (average == MSM_EFF_AVERAGE_NONE ? si[p] : w) * (double)counts[p];
    }
}

}  // namespace

extern "C" {

size_t msm_effective_counts_work_bytes(int64_t n, int k, int n_seg) {
    if (n < 0 || k < 1 || n_seg < 0) return 0;
    return eff_layout(n, k, n_seg, nullptr, nullptr);
}

msm_status msm_effective_counts(msm_ctx* ctx, const int32_t* d_labels, int64_t n, const int64_t* h_seg_start,
                                const int64_t* h_seg_stop, int n_seg, int lag, int k, int average, double mact,
                                int blocks_per_launch, void* d_work, size_t work_bytes, double* d_ceff, double* d_si,
                                int64_t* d_counts, int32_t* d_trunc, int64_t* h_launches) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, lag >= 1, "msm_effective_counts: lag must be >= 1 (got %d)", lag);
    MSM_REQUIRE(ctx, n >= 0 && k >= 1 && k <= 46340, "msm_effective_counts: need n >= 0 and 1 <= k <= 46340 (n=%lld k=%d)",
                (long long)n, k);
    if (n > (int64_t)INT32_MAX) return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_effective_counts: more than 2^31 - 1 frames");
    MSM_REQUIRE(ctx, average == MSM_EFF_AVERAGE_ROW || average == MSM_EFF_AVERAGE_ALL || average == MSM_EFF_AVERAGE_NONE,
                "msm_effective_counts: unknown average %d", average);
    MSM_REQUIRE(ctx, mact == mact && mact - mact == 0.0, "msm_effective_counts: mact must be finite");
    MSM_REQUIRE(ctx, blocks_per_launch >= 0, "msm_effective_counts: blocks_per_launch must be >= 0 (0: the default)");
    MSM_REQUIRE(ctx, n_seg >= 0 && (n_seg == 0 || (h_seg_start && h_seg_stop)), "msm_effective_counts: bad segment arrays");
    MSM_REQUIRE(ctx, d_ceff && d_si && d_counts && d_trunc && (d_labels || n == 0), "msm_effective_counts: NULL pointer");
    if (ctx->capturing)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_effective_counts reads its progress on the host: not capturable");
    // segments in ascending order, disjoint, inside [0, n]; those with no pair at this lag are dropped
    std::vector<int64_t> seg_a, seg_e;
    int64_t prev_stop = 0;
    for (int s = 0; s < n_seg; ++s) {
        const int64_t a = h_seg_start[s], b = h_seg_stop[s];
        MSM_REQUIRE(ctx, a >= prev_stop && b >= a && b <= n,
                    "msm_effective_counts: segment %d = [%lld, %lld) is not inside [0, n], ascending and disjoint", s,
                    (long long)a, (long long)b);
        prev_stop = b;
        if (b - a > lag) { seg_a.push_back(a); seg_e.push_back(b - lag); }
    }
    if (n_seg == 0 && n > lag) { seg_a.push_back(0); seg_e.push_back(n - lag); }
    const int ns = (int)seg_a.size();
    const size_t kk = (size_t)k * k;
    if (h_launches) *h_launches = 0;
    if (ns == 0) {   // no pair anywhere
        MSM_HIP(ctx, hipMemsetAsync(d_ceff, 0, kk * sizeof(double), ctx->stream));
        MSM_HIP(ctx, hipMemsetAsync(d_si, 0, kk * sizeof(double), ctx->stream));
        MSM_HIP(ctx, hipMemsetAsync(d_counts, 0, kk * sizeof(int64_t), ctx->stream));
        MSM_HIP(ctx, hipMemsetAsync(d_trunc, 0, kk * sizeof(int32_t), ctx->stream));
        return MSM_OK;
    }
    EffWork w;
    const size_t need = eff_layout(n, k, n_seg, (char*)d_work, &w);
    MSM_REQUIRE(ctx, d_work && work_bytes >= need, "msm_effective_counts: the work buffer holds %zu bytes, %zu are needed",
                work_bytes, need);

    // the sliding counts, by the existing kernel over the caller's own segments
    msm_status rs = msm_count_transitions(ctx, d_labels, n, h_seg_start, h_seg_stop, n_seg, lag, 1, k, d_counts, nullptr);
    if (rs != MSM_OK) return rs;

    std::vector<int64_t> seg_h(seg_a);
    seg_h.insert(seg_h.end(), seg_e.begin(), seg_e.end());
    MSM_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the copy below reads pageable memory)
    MSM_HIP(ctx, hipMemcpy(w.seg, seg_h.data(), seg_h.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    const int n_blocks = msm_ceil_div(n, kT);
    hipLaunchKernelGGL(eff_keys_kernel, dim3(n_blocks), dim3(kT), 0, ctx->stream, d_labels, n, k, lag,
                       (const int64_t*)w.seg, ns, w.key_i, w.key_j);
    MSM_CHECK_LAUNCH(ctx);
    rs = msm_group_by_label(ctx, w.key_i, n, k, w.off0, w.mem0);
    if (rs != MSM_OK) return rs;
    rs = msm_group_by_label(ctx, w.key_j, n, k, w.off1, w.mem1);
    if (rs != MSM_OK) return rs;
    hipLaunchKernelGGL(eff_keys2_kernel, dim3(n_blocks), dim3(kT), 0, ctx->stream, (const int32_t*)w.key_i,
                       (const int32_t*)w.mem1, (const int64_t*)w.off1, k, n, w.key_j);
    MSM_CHECK_LAUNCH(ctx);
    rs = msm_group_by_label(ctx, w.key_j, n, k, w.off2, w.mem2);
    if (rs != MSM_OK) return rs;
    hipLaunchKernelGGL(eff_rows_kernel, dim3(k), dim3(kT), 0, ctx->stream, (const int64_t*)d_counts, k,
                       (const int64_t*)w.off0, w.pairoff, w.state, d_trunc, w.row_m, w.nless);
    hipLaunchKernelGGL(eff_occ_kernel, dim3(n_blocks), dim3(kT), 0, ctx->stream, (const int32_t*)w.key_i,
                       (const int32_t*)w.mem0, (const int32_t*)w.mem1, (const int32_t*)w.mem2, (const int64_t*)w.off0, k,
                       n, (const int64_t*)w.seg, ns, w.occ_rank, w.occ_head, w.occ_end, w.nless, w.row_m);
    hipLaunchKernelGGL(eff_nless_kernel, dim3(k), dim3(kT), 0, ctx->stream, (const int64_t*)w.off0, w.nless);
    MSM_CHECK_LAUNCH(ctx);

    const int blocks = blocks_per_launch > 0 ? blocks_per_launch : MSM_EFF_BLOCKS_PER_LAUNCH;
    int64_t launches = 0;
    for (;;) {
        int32_t left = 0;
        MSM_HIP(ctx, hipMemsetAsync(w.counter, 0, sizeof(int32_t), ctx->stream));
        hipLaunchKernelGGL(eff_ineff_kernel, dim3((unsigned)kk), dim3(kT), 0, ctx->stream, (const int64_t*)d_counts, k,
                           (const int64_t*)w.off0, (const int64_t*)w.pairoff, (const int32_t*)w.occ_rank,
                           (const int32_t*)w.occ_head, (const int32_t*)w.occ_end, (const int32_t*)w.nless,
                           (const int32_t*)w.row_m, blocks, w.state, d_trunc, w.counter);
        MSM_CHECK_LAUNCH(ctx);
        ++launches;
        MSM_HIP(ctx, hipMemcpyAsync(&left, w.counter, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        MSM_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (left == 0) break;
    }
    if (h_launches) *h_launches = launches;
    hipLaunchKernelGGL(eff_si_kernel, dim3(k), dim3(kT), 0, ctx->stream, (const int64_t*)d_counts, k,
                       (const int64_t*)w.off0, (const EffState*)w.state, mact, d_si, w.row_num);
    hipLaunchKernelGGL(eff_apply_kernel, dim3(k), dim3(kT), 0, ctx->stream, (const int64_t*)d_counts, k,
                       (const int64_t*)w.off0, (const double*)d_si, (const double*)w.row_num, average, d_ceff);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
