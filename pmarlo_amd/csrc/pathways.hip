// Dominant reactive pathways A -> B through the net flux: the decomposition
// TPTAnalysis.analyze asks of deeptime (S/conformations/tpt_analysis.py:122-135, pathways(fraction, maxiter)),
// by the rule of markov_state_model/tpt.py::pathway_decomposition / _widest_path.
//
// The rule (include/msmhip.h has it in full): work matrix G of order N = n + 2 with a virtual source n feeding A and
// a virtual sink n + 1 draining B; one path is a max-min Dijkstra n -> n + 1 (pop the not-done node of largest width,
// the lowest index on equal widths; relax width[j] = min(width[i], G[i][j]) when strictly larger); its capacity
// is removed along it, G[a][b] = max(0, G[a][b] - cap), and the decomposition goes on until the requested share of
// the total flux is collected, no path is left, the capacity falls under 1e-14 * total, or maxiter paths were taken.
//
// Arithmetic: only min, max, compares, ONE subtraction (G - cap) and ONE addition (got + cap) touch the data, and the
// three sums that set up G are sequential chains in ascending index.  Nothing here has the shape a * b + c, so no
// operation can be contracted into an FMA (the build has -ffp-contract=off as well): a numpy restatement reproduces
// every bit.  Keep it that way: no fma(), no products of data.
//
// Shape: ONE workgroup of 1024 threads runs the loop of a launch.  Node j belongs to thread j % 1024 (at most three
// nodes a thread at n = 2048); width / prev / done live in LDS and are touched by the owner alone during a search, so
// a pop costs one barrier: the arg-max over (width, index) is wave_argmax_down per wave, one LDS slot per wave, and
// every thread then folds the 16 slots itself (the slots are double-buffered, so the next pop's writes cannot overtake
// a reader).  The popped row of G is read coalesced from global memory.  A launch takes at most `launch_paths` paths
// and leaves its state (G, got, total, path count, status) in the caller's work buffer: the host reads the header
// and launches again while the status is "running".  No spin-wait, no cross-workgroup barrier.
#include <climits>

#include "common.h"
#include "wave.h"

namespace {

constexpr int kPT = 1024;                         // threads of the one workgroup
constexpr int kPwMaxNodes = MSM_PATHWAYS_MAX_N + 2;
constexpr size_t kPwHeaderBytes = 64;             // the header's slot at the front of the work buffer

struct PwHeader {          // first 32 bytes of the work buffer, read back by the host after every launch
    double got;            // flux collected so far
    double total;          // total flux = sum_a G[n][a]
    int32_t n_paths;       // paths taken so far
    int32_t status;        // MSM_PATHWAYS_*
    int32_t bad;           // != 0: the net flux holds a negative, infinite or NaN entry
    int32_t pad;
};
static_assert(sizeof(PwHeader) == 32, "the host reads 32 bytes");

__device__ __forceinline__ double* pw_matrix(void* work) { return (double*)((char*)work + kPwHeaderBytes); }

// Row i of G, one workgroup per row.  The virtual edges are sequential sums in ascending index.
__global__ __launch_bounds__(256) void pw_fill_kernel(const double* __restrict__ net, int64_t ld,
                                                      const int32_t* __restrict__ role, int n, void* work) {
    const int N = n + 2, i = blockIdx.x, tid = threadIdx.x;
    double* row = pw_matrix(work) + (size_t)i * N;
    int bad = 0;
    if (i < n) {
        for (int j = tid; j < n; j += blockDim.x) {
            const double v = net[(size_t)i * ld + j];
            if (!(v >= 0.0) || v == INFINITY) bad = 1;
            row[j] = v;
        }
        if (tid == 0) {
            double s = 0.0;                      // G[i][n+1] = sum_r net[r][i] for a sink i
            if (role[i] == 2)
                for (int r = 0; r < n; ++r) s += net[(size_t)r * ld + i];
            row[n] = 0.0;
            row[n + 1] = s;
        }
    } else if (i == n) {
        for (int a = tid; a < N; a += blockDim.x) {
            double s = 0.0;                      // G[n][a] = sum_j net[a][j] for a source a
            if (a < n && role[a] == 1)
                for (int j = 0; j < n; ++j) s += net[(size_t)a * ld + j];
            row[a] = s;
        }
    } else {
        for (int j = tid; j < N; j += blockDim.x) row[j] = 0.0;
    }
    if (bad) atomicOr(&((PwHeader*)work)->bad, 1);
}

// total = sum_a G[n][a] in ascending a (the entries outside A are +0 and leave the bits alone); fresh counters
__global__ void pw_total_kernel(void* work, int n) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double* row = pw_matrix(work) + (size_t)n * (n + 2);
    double t = 0.0;
    for (int a = 0; a < n; ++a) t += row[a];
    PwHeader* h = (PwHeader*)work;
    h->got = 0.0;
    h->total = t;
    h->n_paths = 0;
    h->status = MSM_PATHWAYS_RUNNING;
}

__global__ __launch_bounds__(kPT) void pathways_kernel(void* work, int n, double fraction, int maxiter, int keep,
                                                       int launch_paths, double* __restrict__ caps,
                                                       int32_t* __restrict__ paths, int32_t* __restrict__ lens) {
    __shared__ double s_width[kPwMaxNodes];
    __shared__ int s_prev[kPwMaxNodes];
    __shared__ int s_list[kPwMaxNodes];           // the path found, sink first
    __shared__ unsigned char s_done[kPwMaxNodes];
    __shared__ double s_val[2][kPT / 64];
    __shared__ int s_idx[2][kPT / 64];
    __shared__ double s_got;
    __shared__ int s_npaths, s_count;

    PwHeader* hdr = (PwHeader*)work;
    double* G = pw_matrix(work);                  // read AND written here: no __restrict__, no const
    const int N = n + 2, src = n, dst = n + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    if (hdr->status != MSM_PATHWAYS_RUNNING) return;
    if (tid == 0) { s_got = hdr->got; s_npaths = hdr->n_paths; }
    const double total = hdr->total;
    const double floor_cap = 1e-14 * total;
    const double target = fraction * total * (1.0 - 1e-14);   // left to right
    __syncthreads();

    int parity = 0;
    for (int taken = 0;; ++taken) {
        // every thread reads the same two LDS words after a barrier: the branches below are uniform
        const double got = s_got;
        const int np = s_npaths;
        int status = MSM_PATHWAYS_RUNNING;
        if (!(total > 0.0)) status = MSM_PATHWAYS_NO_PATH;
        else if (!(got < target)) status = MSM_PATHWAYS_FRACTION;
        else if (np >= maxiter) status = MSM_PATHWAYS_MAXITER;
        if (status != MSM_PATHWAYS_RUNNING || taken >= launch_paths) {
            if (tid == 0) { hdr->got = got; hdr->n_paths = np; hdr->status = status; }
            return;
        }

        // ---- one max-min Dijkstra src -> dst; a thread touches its own nodes only ----
        for (int j = tid; j < N; j += kPT) {
            s_width[j] = j == src ? INFINITY : 0.0;
            s_prev[j] = -1;
            s_done[j] = 0;
        }
        double cap = 0.0;
        bool reached = false;
        for (;;) {
            double best = 0.0;
            int bi = INT_MAX;
            for (int j = tid; j < N; j += kPT)
                if (!s_done[j]) {
                    const double w = s_width[j];
                    if (w > best || (w == best && j < bi)) { best = w; bi = j; }
                }
            wave_argmax_down(best, bi);           // larger width wins, the lower index on equal widths
            if (lane == 0) { s_val[parity][wave] = best; s_idx[parity][wave] = bi; }
            __syncthreads();
            best = s_val[parity][0];
            bi = s_idx[parity][0];
#pragma unroll
            for (int w = 1; w < kPT / 64; ++w) {
                const double ov = s_val[parity][w];
                const int oi = s_idx[parity][w];
                if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
            }
            parity ^= 1;
            if (!(best > 0.0)) break;             // nothing reachable is left: no path
            if (bi == dst) { cap = best; reached = true; break; }
            if ((bi & (kPT - 1)) == tid) s_done[bi] = 1;
            const double* row = G + (size_t)bi * N;
            for (int j = tid; j < N; j += kPT)
                if (!s_done[j]) {
                    const double cand = fmin(best, row[j]);
                    if (cand > s_width[j]) { s_width[j] = cand; s_prev[j] = bi; }
                }
        }
        if (!reached || cap <= floor_cap) {
            if (tid == 0) { hdr->got = got; hdr->n_paths = np; hdr->status = MSM_PATHWAYS_NO_PATH; }
            return;
        }
        __syncthreads();                          // s_prev of every owner is visible

        // ---- remove the capacity along the path, record it ----
        if (tid == 0) {
            int c = 0;
            for (int v = dst; v != src && c < N - 1; v = s_prev[v]) s_list[c++] = v;
            s_list[c++] = src;
            s_count = c;                          // nodes of the path, both virtual ends included
        }
        __syncthreads();
        const int count = s_count, inner = count - 2;
        for (int e = tid; e + 1 < count; e += kPT) {            // edge s_list[e + 1] -> s_list[e]
            const int a = s_list[e + 1], b = s_list[e];
            double* g = &G[(size_t)a * N + b];
            *g = fmax(0.0, *g - cap);
            if (np < keep && e >= 1) paths[(size_t)np * n + (inner - e)] = b;
        }
        if (tid == 0) {
            if (np < keep) lens[np] = inner;
            caps[np] = cap;
            s_got = got + cap;
            s_npaths = np + 1;
        }
        __syncthreads();                          // G, s_got, s_npaths before the next search
    }
}

}  // namespace

extern "C" {

size_t msm_reactive_pathways_work_bytes(int n) {
    if (n < 0) return 0;
    return kPwHeaderBytes + (size_t)(n + 2) * (size_t)(n + 2) * sizeof(double);
}

int msm_reactive_pathways_launch_paths(int n) {
    if (n < 0) return 0;
    const int per = MSM_PATHWAYS_LAUNCH_POPS / (n + 2);
    return per < 1 ? 1 : per;
}

msm_status msm_reactive_pathways_begin(msm_ctx* ctx, const double* d_net, int64_t ldn, const int32_t* d_role, int n,
                                       int maxiter, int keep, void* d_work, double* d_caps, int32_t* d_paths,
                                       int32_t* d_len) {
    if (!ctx) return MSM_ERR_INVALID;
    if (n > MSM_PATHWAYS_MAX_N)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_reactive_pathways: n = %d exceeds the limit of %d states", n,
                        MSM_PATHWAYS_MAX_N);
    MSM_REQUIRE(ctx, n >= 2 && ldn >= n && maxiter >= 0 && keep >= 0, "msm_reactive_pathways_begin: bad shape");
    MSM_REQUIRE(ctx, d_net && d_role && d_work && (maxiter == 0 || d_caps) && (keep == 0 || (d_paths && d_len)),
                "msm_reactive_pathways_begin: NULL pointer");
    MSM_HIP(ctx, hipMemsetAsync(d_work, 0, kPwHeaderBytes, ctx->stream));
    if (keep > 0) {
        MSM_HIP(ctx, hipMemsetAsync(d_paths, 0xFF, (size_t)keep * n * sizeof(int32_t), ctx->stream));
        MSM_HIP(ctx, hipMemsetAsync(d_len, 0, (size_t)keep * sizeof(int32_t), ctx->stream));
    }
    hipLaunchKernelGGL(pw_fill_kernel, dim3(n + 2), dim3(256), 0, ctx->stream, d_net, ldn, d_role, n, d_work);
    hipLaunchKernelGGL(pw_total_kernel, dim3(1), dim3(64), 0, ctx->stream, d_work, n);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_reactive_pathways_run(msm_ctx* ctx, void* d_work, int n, double fraction, int maxiter, int keep,
                                     int launch_paths, double* d_caps, int32_t* d_paths, int32_t* d_len) {
    if (!ctx) return MSM_ERR_INVALID;
    if (n > MSM_PATHWAYS_MAX_N)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "msm_reactive_pathways: n = %d exceeds the limit of %d states", n,
                        MSM_PATHWAYS_MAX_N);
    MSM_REQUIRE(ctx, n >= 2 && maxiter >= 0 && keep >= 0 && launch_paths >= 0, "msm_reactive_pathways_run: bad shape");
    MSM_REQUIRE(ctx, fraction > 0.0 && fraction <= 1.0, "msm_reactive_pathways_run: fraction must be in (0, 1]");
    MSM_REQUIRE(ctx, d_work && (maxiter == 0 || d_caps) && (keep == 0 || (d_paths && d_len)),
                "msm_reactive_pathways_run: NULL pointer");
    if (launch_paths == 0) launch_paths = msm_reactive_pathways_launch_paths(n);
    hipLaunchKernelGGL(pathways_kernel, dim3(1), dim3(kPT), 0, ctx->stream, d_work, n, fraction, maxiter, keep,
                       launch_paths, d_caps, d_paths, d_len);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
