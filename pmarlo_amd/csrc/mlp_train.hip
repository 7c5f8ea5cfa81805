// One training step of a DeepTICA network on the device: the forward pass in training mode, the VAMP-2 loss with
// its closed-form output gradient, the backward pass, and clip + AdamW.  The law: include/msmhip.h
// (msm_vamp2_loss, msm_mlp_loss_grad, msm_adamw_step, and the _weighted entries, whose loss takes per-pair weights:
// other chunk sums, moments and output gradient, the same solve).
//
// Frames are addressed by slot: slots 0 .. m-1 are the t frames of the batch (rows idx_t of the resident array),
// slots m .. 2m-1 the tau frames (rows idx_tau).  As in mlp.hip a workgroup is one wave that owns 16 slots, whose
// rows sit in two LDS images the layers ping-pong between.
//
// The forward pass is the shared walk (mlp_forward_walk, mlp_common.h) with the tape, dropout and the inputs a[l] of
// the Linear layers switched on; what it leaves in the workspace, all fp64 [2m, width]: MlpTape and MlpTrainSlots.
//
// The backward pass works per 16-slot group: the dropout adjoint, then the shared activation and LayerNorm adjoints
// row by row and dA = du . W on the matrix cores (mlp_layer_adjoint, mlp_linear_transposed); du_l (and, where a
// LayerNorm has parameters, dh and dh * xhat) go to the workspace.  Parameter gradients are contractions over the 2m
// slots: the slots are cut into chunks of kChunk = 256 (a constant, so the summation order depends on m alone), one wave
// sums one 16 x 16 tile of dW (or 64 entries of a bias / gamma / beta gradient) over one chunk on the matrix cores,
// and a second kernel adds the chunks in ascending order.  No atomics anywhere: equal inputs give equal bits.
#include "mlp_common.h"

namespace {

constexpr int kStatsHead = 16;          // scalars in front of the four vectors of the stats block
constexpr int kSolveThreads = 256;

// where everything lies in the training workspace (offsets in doubles; -1: absent); travels by value
struct TrainLayout {
    MlpTape tape;
    MlpTrainSlots keep;
    long long y, dy, partial, loss, total;
};

// src[0] + src[stride] + ... (nr terms), added in ascending order; the loads of eight terms go out together, the
// additions keep their order, so the bits are those of the plain loop
__device__ __forceinline__ double ordered_sum(const double* __restrict__ src, size_t stride, int nr) {
    double s = 0.0;
    int r = 0;
    for (; r + 8 <= nr; r += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(r + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; r < nr; ++r) s += src[(size_t)r * stride];
    return s;
}

template <typename T>
__global__ __launch_bounds__(64) void mlp_train_forward_kernel(
    const T* __restrict__ x, int64_t n, int64_t ld, const double* __restrict__ sc_mean,
    const double* __restrict__ sc_scale, const float* __restrict__ params, MlpPlan p,
    const int64_t* __restrict__ idx_t, const int64_t* __restrict__ idx_tau, int m, DropPlan drop, TrainLayout lay,
    double* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mlp_smem[];
    const int lane = threadIdx.x;
    const int j = lane & 15, g = lane >> 4;
    double* img[2];
    img[0] = reinterpret_cast<double*>(mlp_smem);
    img[1] = img[0] + 16 * p.stride[0];
    const int n_out = p.width[p.n_linear];
    const int S2 = 2 * m;
    const int n_groups = (S2 + 15) / 16;
    for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int s0 = grp * 16;
        const int rows = min(16, S2 - s0);
        WAVE_SYNC();   // the previous group's rows have been read
        // the row of x a slot names; one whose index lies outside [0, n) is not read and enters as NaN
        mlp_load_inputs(img[0], p.stride[0], p.width[0], lane, rows, x, ld, sc_mean, sc_scale, [&](int r) {
            const int s = s0 + r;
            const int64_t row = s < m ? idx_t[s] : idx_tau[s - m];
            return row < n ? row : (int64_t)-1;
        });
        int bad;
        const double* cur = mlp_forward_walk<true, true>(p, params, img, lane, rows,
                                                         MlpKeep{&lay.tape, &lay.keep, &drop, ws, (size_t)s0}, &bad);
        if (j < rows) {
            const double qnan = __longlong_as_double(0x7ff8000000000000ll);
            for (int c = g; c < n_out; c += 4) ws[lay.y + (size_t)(s0 + j) * n_out + c] = bad ? qnan : cur[c];
        }
    }
}

__global__ __launch_bounds__(64) void mlp_train_backward_kernel(const float* __restrict__ params, MlpPlan p, int m,
                                                                DropPlan drop, TrainLayout lay,
                                                                double* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mlp_smem[];
    const int lane = threadIdx.x;
    const int j = lane & 15, g = lane >> 4;
    double* img[2];
    img[0] = reinterpret_cast<double*>(mlp_smem);
    img[1] = img[0] + 16 * p.stride[0];
    const int L = p.n_linear;
    const int n_out = p.width[L];
    const int S2 = 2 * m;
    const int n_groups = (S2 + 15) / 16;
    for (int grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        const int s0 = grp * 16;
        const int rows = min(16, S2 - s0);
        const bool mine = j < rows;                          // frame j's slot exists
        const size_t slot = (size_t)min(s0 + j, S2 - 1);     // reads of a slot past 2m are clamped, its writes dropped
        WAVE_SYNC();
        {   // dL/dY of the group; slots past 2m enter as zeros
            const int So = p.stride[L & 1];
            for (int r = 0; r < 16; ++r)
                for (int f = lane; f < n_out; f += 64)
                    img[L & 1][r * So + f] = r < rows ? ws[lay.dy + (size_t)(s0 + r) * n_out + f] : 0.0;
        }
        for (int l = L - 1; l >= 0; --l) {
            const int K = p.width[l], N = p.width[l + 1];
            const int So = p.stride[(l + 1) & 1];
            double* gout = img[(l + 1) & 1] + j * So;        // dL/d(output of layer l), then du_l
            double* gin = img[l & 1] + j * p.stride[l & 1];  // dL/d(input of layer l)
            if (l < L - 1 && drop.on && drop.thr[l + 1]) {
                WAVE_SYNC();
                mlp_dropout(gout, g, N, drop, l + 1, (unsigned)(s0 + j));
            }
            WAVE_SYNC();
            mlp_layer_adjoint<true>(gout, g, p, l, params, lay.tape, &lay.keep, ws, slot, mine);
            WAVE_SYNC();
            save_rows(img[(l + 1) & 1], So, N, rows, ws + lay.keep.du[l] + (size_t)s0 * N, lane);
            if (l == 0 && p.ln_in_off < 0) break;            // nothing upstream of the first Linear has parameters
            mlp_linear_transposed(gout, gin, params + p.w_off[l], K, N, j, g);
        }
        if (p.ln_in_off >= 0) {
            const int F = p.width[0];
            double* gin = img[0] + j * p.stride[0];
            if (drop.on && drop.thr[0]) {
                WAVE_SYNC();
                mlp_dropout(gin, g, F, drop, 0, (unsigned)(s0 + j));
            }
            WAVE_SYNC();
            mlp_layer_norm_adjoint(gin, g, F, ws + lay.tape.z + slot * F, params + p.ln_in_off,
                                   ws + lay.keep.dz + slot * F, ws + lay.keep.dzx + slot * F, mine);
        }
    }
}

// One chunk's share of every parameter gradient: blockIdx.y is the chunk, blockIdx.x the job.  Jobs, in the packed
// order of the parameters: [gamma, beta of the input LayerNorm in blocks of 64 entries;] per Linear its 16 x 16
// tiles of dW, its bias in blocks of 64, [gamma, beta in blocks of 64].  partial [chunks][n_params].
__global__ __launch_bounds__(64) void mlp_train_param_partial_kernel(MlpPlan p, int m, TrainLayout lay, int n_params,
                                                                     const double* __restrict__ ws,
                                                                     double* __restrict__ partial) {
    const int lane = threadIdx.x;
    const int j = lane & 15, g = lane >> 4;
    const int S2 = 2 * m;
    const int r0 = blockIdx.y * kChunk;
    const int nr = min(kChunk, S2 - r0);
    double* __restrict__ out = partial + (size_t)blockIdx.y * n_params;
    int job = blockIdx.x;
    // a column sum: out[off + c] = sum over the chunk's slots of src[slot][c], c in block `cb` of 64 entries
    auto colsum = [&](long long src_off, int w, int off, int cb) {
        const int c = cb * 64 + lane;
        if (c < w) {
            out[off + c] = ordered_sum(ws + src_off + (size_t)r0 * w + c, w, nr);
        }
    };
    if (p.ln_in_off >= 0) {
        const int F = p.width[0], nb = (F + 63) / 64;
        if (job < nb) return colsum(lay.keep.dzx, F, p.ln_in_off, job);
        job -= nb;
        if (job < nb) return colsum(lay.keep.dz, F, p.ln_in_off + F, job);
        job -= nb;
    }
    for (int l = 0; l < p.n_linear; ++l) {
        const int K = p.width[l], N = p.width[l + 1];
        const int tk = (K + 15) / 16, tn = (N + 15) / 16, nb = (N + 63) / 64;
        if (job < tn * tk) {   // dW[n][k] = sum over slots of du[slot][n] a[slot][k]
            const int n0 = (job / tk) * 16, k0 = (job % tk) * 16;
            const double* __restrict__ du = ws + lay.keep.du[l] + (size_t)r0 * N + min(n0 + j, N - 1);
            const double* __restrict__ a = ws + lay.keep.a[l] + (size_t)r0 * K + min(k0 + j, K - 1);
            const v4f64 acc = mfma_tile_acc(
                nr, g, n0 + j < N, k0 + j < K, [&](int r) { return du[(size_t)r * N]; },
                [&](int r) { return a[(size_t)r * K]; });
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int nn = n0 + g + 4 * r;
                if (nn < N && k0 + j < K) out[p.w_off[l] + nn * K + k0 + j] = acc[r];
            }
            return;
        }
        job -= tn * tk;
        if (job < nb) return colsum(lay.keep.du[l], N, p.b_off[l], job);
        job -= nb;
        if (p.ln_off[l] >= 0) {
            if (job < nb) return colsum(lay.keep.dhx[l], N, p.ln_off[l], job);
            job -= nb;
            if (job < nb) return colsum(lay.keep.dh[l], N, p.ln_off[l] + N, job);
            job -= nb;
        }
    }
}

// the jobs of mlp_train_param_partial_kernel (its gridDim.x)
int param_jobs(const MlpPlan& p) {
    int jobs = 0;
    if (p.ln_in_off >= 0) jobs += 2 * ((p.width[0] + 63) / 64);
    for (int l = 0; l < p.n_linear; ++l) {
        const int K = p.width[l], N = p.width[l + 1];
        jobs += ((K + 15) / 16) * ((N + 15) / 16) + ((N + 63) / 64) * (p.ln_off[l] >= 0 ? 3 : 1);
    }
    return jobs;
}

__global__ __launch_bounds__(256) void mlp_train_param_reduce_kernel(const double* __restrict__ partial, int chunks,
                                                                     int n_params, double* __restrict__ grad) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_params) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += partial[(size_t)c * n_params + e];
    grad[e] = s;
}

// ---- VAMP-2 loss -------------------------------------------------------------------------------------------------
// work (doubles): psum [chunks][2 d], pmom [chunks][3][d d], G [3][d d] (G00, Gtt, G0t), mean [2 d],
// then ten d x d matrices for the solve; with weights also wsum [chunks][2] (sum of w', of w'^2) and wtot [2]
// (W, sum of w'^2), -1 without.
struct VampWork {
    long long psum, pmom, G, mean, mats, wsum, wtot, total;
    int chunks;
};

// The moments kernels take one chunk per gridDim.y entry, and gfx950 admits 65536 of them (hipDeviceProp_t's
// maxGridSize[1]): the largest batch of the loss, which is also msm_mlp_loss_grad's 2^24 pairs.
constexpr int64_t kVampMaxPairs = (int64_t)65536 * kChunk;

inline VampWork vamp_work(int m, int d, bool weighted = false) {
    VampWork w;
    w.chunks = (m + kChunk - 1) / kChunk;
    const long long dd = (long long)d * d;
    w.psum = 0;
    w.pmom = w.psum + (long long)w.chunks * 2 * d;
    w.G = w.pmom + (long long)w.chunks * 3 * dd;
    w.mean = w.G + 3 * dd;
    w.mats = w.mean + 2 * d;
    w.total = w.mats + 10 * dd;
    w.wsum = w.wtot = -1;
    if (weighted) {
        w.wsum = w.total;
        w.wtot = w.wsum + (long long)w.chunks * 2;
        w.total = w.wtot + 2;
    }
    return w;
}

// column sums of Y0 (entries 0 .. d-1) and Yt (d .. 2d-1) over one chunk of frames
__global__ __launch_bounds__(128) void vamp2_colsum_kernel(const double* __restrict__ y0, const double* __restrict__ yt,
                                                           int m, int d, int64_t ld, double* __restrict__ psum) {
    const int c = threadIdx.x;
    if (c >= 2 * d) return;
    const int r0 = blockIdx.x * kChunk, nr = min(kChunk, m - r0);
    const double* __restrict__ src = (c < d ? y0 + c : yt + (c - d)) + (size_t)r0 * ld;
    psum[(size_t)blockIdx.x * 2 * d + c] = ordered_sum(src, ld, nr);
}

// the mean of column c (0 .. 2d-1): the chunks' sums in ascending order, over div (m, or the total weight W)
__device__ __forceinline__ double vamp_mean(const double* __restrict__ psum, int chunks, int d, double div, int c) {
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += psum[(size_t)k * 2 * d + c];
    return s / div;
}

// w' of a pair: max(w, 0); a weight that is not finite stays NaN, so that W is NaN and the solve raises its flag
__device__ __forceinline__ double vamp_weight(double w) {
    return fabs(w) <= DBL_MAX ? fmax(w, 0.0) : __longlong_as_double(0x7ff8000000000000ll);
}

// entry q (0: sum of w', 1: sum of w'^2) of the chunks' weight sums, in ascending order
__device__ __forceinline__ double vamp_weight_total(const double* __restrict__ wsum, int chunks, int q) {
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += wsum[(size_t)k * 2 + q];
    return s;
}

// f(0) + f(1) + ... (nr terms) in ascending order, eight terms fetched together as in ordered_sum
template <typename F>
__device__ __forceinline__ double ordered_sum_of(int nr, F f) {
    double s = 0.0;
    int r = 0;
    for (; r + 8 <= nr; r += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = f(r + u);
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; r < nr; ++r) s += f(r);
    return s;
}

// One chunk of pairs under weights: thread c < 2d sums w' Y0 (entries 0 .. d-1) and w' Yt (d .. 2d-1) into psum,
// threads 2d and 2d + 1 sum w' and w'^2 into wsum.  2d + 2 <= 130 threads do anything, and all of them walk one
// loop, w'_r times a second factor (the column's entry, 1, or w'_r), so that a wave holding both kinds of thread does
// not run the chunk twice.
__global__ __launch_bounds__(192) void vamp2_wsum_kernel(const double* __restrict__ y0, const double* __restrict__ yt,
                                                         const double* __restrict__ wts, int m, int d, int64_t ld,
                                                         double* __restrict__ psum, double* __restrict__ wsum) {
    const int c = threadIdx.x;
    if (c >= 2 * d + 2) return;
    const int r0 = blockIdx.x * kChunk, nr = min(kChunk, m - r0);
    const double* __restrict__ wq = wts + r0;
    const bool col = c < 2 * d, sq = c == 2 * d + 1;
    const double* __restrict__ src = col ? (c < d ? y0 + c : yt + (c - d)) + (size_t)r0 * ld : wq;
    const size_t stride = col ? (size_t)ld : 1;
    const double s = ordered_sum_of(nr, [&](int r) {
        const double x = src[(size_t)r * stride];
        return vamp_weight(wq[r]) * (col ? x : sq ? vamp_weight(x) : 1.0);
    });
    if (col) psum[(size_t)blockIdx.x * 2 * d + c] = s;
    else wsum[(size_t)blockIdx.x * 2 + (sq ? 1 : 0)] = s;
}

// One 16 x 16 tile of the centred second moments of one chunk: matrix q = 0: Y0'Y0, 1: Yt'Yt, 2: Y0'Yt.  WEIGHTED:
// the tile of sum_s w'_s (a_s - mean_a)(b_s - mean_b) with the weighted means (the sums over the total weight W instead
// of m); the first operand carries w'_s, the division by W is the solve's.  A row past the chunk's end is fed as zero
// and its weight is not read (mfma_tile_acc asks for row 0 in its place).  Without weights wts and wsum are not read.
template <bool WEIGHTED>
__global__ __launch_bounds__(64) void vamp2_moments_kernel(const double* __restrict__ y0, const double* __restrict__ yt,
                                                           const double* __restrict__ wts, int m, int d, int64_t ld,
                                                           const double* __restrict__ psum,
                                                           const double* __restrict__ wsum, int chunks,
                                                           double* __restrict__ pmom) {
    const int lane = threadIdx.x;
    const int j = lane & 15, g = lane >> 4;
    const int T = (d + 15) / 16;
    const int q = blockIdx.x / (T * T), tile = blockIdx.x % (T * T);
    const int i0 = (tile / T) * 16, c0 = (tile % T) * 16;
    const int r0 = blockIdx.y * kChunk, nr = min(kChunk, m - r0);
    const int ia = min(i0 + j, d - 1), ib = min(c0 + j, d - 1);
    const bool a_tau = q == 1, b_tau = q != 0;
    const double div = WEIGHTED ? vamp_weight_total(wsum, chunks, 0) : (double)m;
    const double ma = vamp_mean(psum, chunks, d, div, ia + (a_tau ? d : 0));
    const double mb = vamp_mean(psum, chunks, d, div, ib + (b_tau ? d : 0));
    const double* __restrict__ A = (a_tau ? yt : y0) + (size_t)r0 * ld + ia;
    const double* __restrict__ B = (b_tau ? yt : y0) + (size_t)r0 * ld + ib;
    const double* __restrict__ wq = WEIGHTED ? wts + r0 : nullptr;
    const v4f64 acc = mfma_tile_acc(
        nr, g, i0 + j < d, c0 + j < d,
        [&](int r) {
            const double a = A[(size_t)r * ld] - ma;
            if constexpr (WEIGHTED) return vamp_weight(wq[r]) * a;
            else return a;
        },
        [&](int r) { return B[(size_t)r * ld] - mb; });
    double* __restrict__ out = pmom + ((size_t)blockIdx.y * 3 + q) * d * d;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + g + 4 * r;
        if (i < d && c0 + j < d) out[i * d + c0 + j] = acc[r];
    }
}

// C (d x d, row-major, global) = op(A) op(B), every thread of the workgroup; barrier at the end
template <bool TA, bool TB>
__device__ __forceinline__ void solve_mm(double* __restrict__ C, const double* A, const double* B, int d, double scale) {
    for (int e = threadIdx.x; e < d * d; e += blockDim.x) {
        const int i = e / d, c = e - i * d;
        double s = 0.0;
        for (int k = 0; k < d; ++k) s += (TA ? A[k * d + i] : A[i * d + k]) * (TB ? B[c * d + k] : B[k * d + c]);
        C[e] = scale * s;
    }
    __syncthreads();
}

// Cyclic Jacobi by the first wave of the workgroup on LDS copies: A (destroyed; its diagonal ends as the
// eigenvalues) and V (eigenvectors in columns), row stride d.  A rotation is skipped when |a_pq| is below 1e-17 of
// the geometric mean of the two diagonal entries; a sweep without a rotation ends the iteration.
__device__ void solve_jacobi(double* A, double* V, int d) {
    const int lane = threadIdx.x;
    if (threadIdx.x < 64) {
        for (int e = lane; e < d * d; e += 64) V[e] = (e / d == e % d) ? 1.0 : 0.0;
        WAVE_SYNC();
        for (int sweep = 0; sweep < 40; ++sweep) {
            int rotated = 0;
            for (int pp = 0; pp < d - 1; ++pp)
                for (int qq = pp + 1; qq < d; ++qq) {
                    const double app = A[pp * d + pp], aqq = A[qq * d + qq], apq = A[pp * d + qq];
                    if (!(fabs(apq) > 1e-17 * sqrt(fabs(app * aqq))) ) continue;   // wave-uniform
                    ++rotated;
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    WAVE_SYNC();
                    if (lane < d) {   // columns p and q
                        const double akp = A[lane * d + pp], akq = A[lane * d + qq];
                        A[lane * d + pp] = c * akp - s * akq;
                        A[lane * d + qq] = s * akp + c * akq;
                        const double vkp = V[lane * d + pp], vkq = V[lane * d + qq];
                        V[lane * d + pp] = c * vkp - s * vkq;
                        V[lane * d + qq] = s * vkp + c * vkq;
                    }
                    WAVE_SYNC();
                    if (lane < d) {   // rows p and q
                        const double apk = A[pp * d + lane], aqk = A[qq * d + lane];
                        A[pp * d + lane] = c * apk - s * aqk;
                        A[qq * d + lane] = s * apk + c * aqk;
                    }
                    WAVE_SYNC();
                    if (lane == 0) A[pp * d + qq] = A[qq * d + pp] = 0.0;
                    WAVE_SYNC();
                }
            if (!rotated) break;
        }
    }
    __syncthreads();
}

// In-place lower Cholesky factor of the LDS matrix M (row stride d), every thread; *ok = 0 when a pivot is not
// positive (LAPACK's potrf criterion, a NaN included).  The strict upper triangle is left as it was.
__device__ void solve_cholesky(double* M, int d, int* ok) {
    if (threadIdx.x == 0) *ok = 1;
    __syncthreads();
    for (int k = 0; k < d; ++k) {
        const double piv = M[k * d + k];
        __syncthreads();
        if (!(piv > 0.0)) {
            if (threadIdx.x == 0) *ok = 0;
            break;   // uniform: every thread read the same pivot
        }
        const double lkk = sqrt(piv);
        for (int i = k + threadIdx.x; i < d; i += blockDim.x) M[i * d + k] = i == k ? lkk : M[i * d + k] / lkk;
        __syncthreads();
        const int rem = d - k - 1;
        for (int e = threadIdx.x; e < rem * rem; e += blockDim.x) {
            const int i = k + 1 + e / rem, c = k + 1 + e % rem;
            if (c <= i) M[i * d + c] -= M[i * d + k] * M[c * d + k];
        }
        __syncthreads();
    }
    __syncthreads();
}

// X (LDS, row stride d) = inverse of the lower factor in L (LDS): thread c solves L x = e_c; barrier at the end
__device__ void solve_lower_inverse(const double* L, double* X, int d) {
    for (int c = threadIdx.x; c < d; c += blockDim.x)
        for (int i = 0; i < d; ++i) {
            double s = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s -= L[i * d + k] * X[k * d + c];
            X[i * d + c] = i < c ? 0.0 : s / L[i * d + i];
        }
    __syncthreads();
}

struct VampOpts {
    double eps, eps_abs, alpha, cond_reg;
};

// Regularised matrix, spectrum, penalty direction and inverse Cholesky factor of one side (q = 0: C00, 1: Ctt).
//   Cq: the covariance (global, overwritten with the regularised matrix), Li: receives the inverse factor (global),
//   P: receives cond_reg (v_max v_max' / l_max - v_min v_min' / l_min), or zeros (global).
// Returns through sh[]: 0 cond, 1 eig min, 2 eig max (clamped), 3 ridge factor c (0 when the trace clamp holds),
// 4 status (0 fine, 1 Cholesky failed after the ladder).
__device__ void solve_side(double* Cq, double* Li, double* P, int d, const VampOpts& o, double* lds, double* sh,
                           int* flag) {
    const double floor_ = 1e-12;
    double* LA = lds;            // d x d
    double* LV = lds + d * d;    // d x d
    if (threadIdx.x == 0) {
        double tr = 0.0;
        for (int i = 0; i < d; ++i) tr += Cq[i * d + i];
        const bool clamped = !(tr >= floor_);
        const double trc = clamped ? floor_ : tr;
        const double mu = trc / (double)d;
        const double ridge = fmax(mu * o.eps, mu * o.eps_abs);   // the diagonal's mean is the trace over d
        sh[5] = o.alpha * mu + ridge;
        sh[3] = clamped ? 0.0 : o.alpha + ridge / mu;
    }
    __syncthreads();
    const double shift = sh[5];
    for (int e = threadIdx.x; e < d * d; e += blockDim.x) {
        const int i = e / d, c = e - i * d;
        const double v = 0.5 * (((1.0 - o.alpha) * Cq[i * d + c] + (i == c ? shift : 0.0)) +
                                ((1.0 - o.alpha) * Cq[c * d + i] + (i == c ? shift : 0.0)));
        LA[e] = v;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < d * d; e += blockDim.x) Cq[e] = LA[e];
    __syncthreads();
    solve_jacobi(LA, LV, d);
    if (threadIdx.x == 0) {
        int imin = 0, imax = 0;
        for (int i = 1; i < d; ++i) {
            if (LA[i * d + i] < LA[imin * d + imin]) imin = i;
            if (LA[i * d + i] > LA[imax * d + imax]) imax = i;
        }
        const double lmin = LA[imin * d + imin], lmax = LA[imax * d + imax];
        sh[1] = fmax(lmin, floor_);
        sh[2] = fmax(lmax, floor_);
        sh[0] = sh[2] / sh[1];
        // the penalty's direction: absent when cond <= 1 (the clamp at 1, and d = 1), each half absent when its
        // eigenvalue sits on the floor
        sh[6] = (sh[0] > 1.0 && lmax > floor_) ? o.cond_reg / lmax : 0.0;
        sh[7] = (sh[0] > 1.0 && lmin > floor_) ? o.cond_reg / lmin : 0.0;
        flag[1] = imin;
        flag[2] = imax;
    }
    __syncthreads();
    {
        const int imin = flag[1], imax = flag[2];
        const double wmax = sh[6], wmin = sh[7];
        for (int e = threadIdx.x; e < d * d; e += blockDim.x) {
            const int i = e / d, c = e - i * d;
            P[e] = wmax * LV[i * d + imax] * LV[c * d + imax] - wmin * LV[i * d + imin] * LV[c * d + imin];
        }
    }
    __syncthreads();
    // the jitter ladder of _stable_cholesky: 1e-8, growth 10, five tries
    double total = 0.0, jitter = 1e-8;
    int ok = 0;
    for (int attempt = 0; attempt < 5 && !ok; ++attempt) {
        for (int e = threadIdx.x; e < d * d; e += blockDim.x) LA[e] = Cq[e] + ((e / d == e % d) ? total : 0.0);
        __syncthreads();
        solve_cholesky(LA, d, flag);
        ok = flag[0];
        __syncthreads();
        if (!ok) {
            total += jitter;
            jitter *= 10.0;
        }
    }
    if (threadIdx.x == 0) sh[4] = ok ? 0.0 : 1.0;
    solve_lower_inverse(LA, LV, d);
    for (int e = threadIdx.x; e < d * d; e += blockDim.x) Li[e] = LV[e];
    __syncthreads();
}

// The small dense algebra of the loss in one workgroup: moments from the chunks' partial sums, both sides'
// regularisation, spectra and inverse Cholesky factors, K = La^-1 C0t Lb^-T, score, penalty, and the three
// gradient matrices G00, Gtt, G0t.  stats: see MSM_VAMP2_* in include/msmhip.h.  Under weights (w.wsum >= 0) the
// moments and the means are divided by the total weight W instead of m; a W that is not positive and finite ends
// the solve with NaN everywhere and stats[10] = 1.
__global__ __launch_bounds__(kSolveThreads) void vamp2_solve_kernel(int m, int d, VampOpts o, VampWork w,
                                                                   double* __restrict__ work,
                                                                   double* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vamp_smem[];
    double* lds = reinterpret_cast<double*>(vamp_smem);   // two d x d matrices
    __shared__ double shA[8], shB[8], shW[2], red[kSolveThreads / 64];
    __shared__ int flag[4];
    const bool weighted = w.wsum >= 0;
    if (threadIdx.x == 0) {
        shW[0] = weighted ? vamp_weight_total(work + w.wsum, w.chunks, 0) : (double)m;
        shW[1] = weighted ? vamp_weight_total(work + w.wsum, w.chunks, 1) : (double)m;
    }
    __syncthreads();
    const double div = shW[0];   // m, or W
    const long long dd = (long long)d * d;
    double* M = work + w.mats;
    double* C00 = M, *Ctt = M + dd, *C0t = M + 2 * dd, *LAi = M + 3 * dd, *LBi = M + 4 * dd, *PA = M + 5 * dd,
            *PB = M + 6 * dd, *K = M + 7 * dd, *T1 = M + 8 * dd, *T2 = M + 9 * dd;
    double* G00 = work + w.G, *Gtt = G00 + dd, *G0t = Gtt + dd;
    const double* psum = work + w.psum;
    const double* pmom = work + w.pmom;
    for (int e = threadIdx.x; e < 3 * dd; e += blockDim.x) {
        double s = 0.0;
        for (int k = 0; k < w.chunks; ++k) s += pmom[(size_t)k * 3 * dd + e];
        M[e] = s / div;
    }
    for (int c = threadIdx.x; c < 2 * d; c += blockDim.x) {
        const double mu = vamp_mean(psum, w.chunks, d, div, c);
        work[w.mean + c] = mu;
        stats[kStatsHead + 2 * kMlpMaxOut + (c < d ? c : kMlpMaxOut + c - d)] = mu;
    }
    __syncthreads();
    if (weighted && !(div > 0.0 && div <= DBL_MAX)) {   // uniform: every thread read the same W
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        for (int e = threadIdx.x; e < 3 * dd; e += blockDim.x) work[w.G + e] = qnan;
        for (int c = threadIdx.x; c < 2 * d; c += blockDim.x) work[w.mean + c] = qnan;
        for (int i = threadIdx.x; i < kStatsHead + 4 * kMlpMaxOut; i += blockDim.x)
            stats[i] = i < 2 || i >= kStatsHead ? qnan : i == 10 ? 1.0 : i == 11 ? div : 0.0;
        if (threadIdx.x == 0) work[w.wtot] = work[w.wtot + 1] = qnan;
        return;
    }
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        stats[kStatsHead + c] = C00[c * d + c];
        stats[kStatsHead + kMlpMaxOut + c] = Ctt[c * d + c];
    }
    __syncthreads();
    solve_side(C00, LAi, PA, d, o, lds, shA, flag);
    solve_side(Ctt, LBi, PB, d, o, lds, shB, flag);
    solve_mm<false, false>(T1, LAi, C0t, d, 1.0);
    solve_mm<false, true>(K, T1, LBi, d, 1.0);       // K = La^-1 C0t Lb^-T
    double part = 0.0;
    for (int e = threadIdx.x; e < dd; e += blockDim.x) part += K[e] * K[e];
    const double score = block_sum_lane0(part, red);
    // G_A = La^-T K K' La^-1 + penalty direction
    solve_mm<false, true>(T1, K, K, d, 1.0);
    solve_mm<true, false>(T2, LAi, T1, d, 1.0);
    solve_mm<false, false>(T1, T2, LAi, d, 1.0);
    for (int e = threadIdx.x; e < dd; e += blockDim.x) PA[e] += T1[e];
    __syncthreads();
    // G_B = Lb^-T K' K Lb^-1 + penalty direction
    solve_mm<true, false>(T1, K, K, d, 1.0);
    solve_mm<true, false>(T2, LBi, T1, d, 1.0);
    solve_mm<false, false>(T1, T2, LBi, d, 1.0);
    for (int e = threadIdx.x; e < dd; e += blockDim.x) PB[e] += T1[e];
    __syncthreads();
    // G0t = -2 La^-T K Lb^-1
    solve_mm<true, false>(T1, LAi, K, d, 1.0);
    solve_mm<false, false>(G0t, T1, LBi, d, -2.0);
    if (threadIdx.x == 0) {
        double ta = 0.0, tb = 0.0;
        for (int i = 0; i < d; ++i) {
            ta += PA[i * d + i];
            tb += PB[i * d + i];
        }
        shA[5] = shA[3] / (double)d * ta;
        shB[5] = shB[3] / (double)d * tb;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < dd; e += blockDim.x) {
        const bool diag = e / d == e % d;
        G00[e] = (1.0 - o.alpha) * PA[e] + (diag ? shA[5] : 0.0);
        Gtt[e] = (1.0 - o.alpha) * PB[e] + (diag ? shB[5] : 0.0);
    }
    if (threadIdx.x == 0) {
        double penalty = 0.0;
        if (o.cond_reg > 0.0) penalty = o.cond_reg * (log(fmax(shA[0], 1.0)) + log(fmax(shB[0], 1.0)));
        const bool failed = shA[4] != 0.0 || shB[4] != 0.0;
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        stats[0] = failed ? qnan : -score + penalty;
        stats[1] = failed ? qnan : score;
        stats[2] = penalty;
        stats[3] = shA[0];
        stats[4] = shB[0];
        stats[5] = shA[1];
        stats[6] = shA[2];
        stats[7] = shB[1];
        stats[8] = shB[2];
        stats[9] = failed ? 1.0 : 0.0;
        for (int i = 10; i < kStatsHead; ++i) stats[i] = 0.0;
        if (weighted) {
            stats[11] = work[w.wtot] = shW[0];
            work[w.wtot + 1] = shW[1];
            stats[12] = shW[0] * shW[0] / shW[1];
        }
    }
}

// dL/dZ0 = (2 Y0c G00 + Ytc G0t') / m, dL/dZt = (2 Ytc Gtt + Y0c G0t) / m with centred outputs; one thread per entry.
// WEIGHTED: pair s carries w'_s / W (wtot[0], left by the solve) instead of 1 / m; else wts and wtot are not read.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void vamp2_grad_kernel(const double* __restrict__ y0, const double* __restrict__ yt,
                                                         const double* __restrict__ wts, int m, int d, int64_t ld,
                                                         const double* __restrict__ G, const double* __restrict__ mean,
                                                         const double* __restrict__ wtot, double* __restrict__ g0,
                                                         double* __restrict__ gt, int64_t ldg) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)m * d) return;
    const int64_t s = e / d;
    const int c = (int)(e - s * d);
    const long long dd = (long long)d * d;
    const double* G00 = G, *Gtt = G + dd, *G0t = G + 2 * dd;
    double a0 = 0.0, b0 = 0.0, at = 0.0, bt = 0.0;
    for (int k = 0; k < d; ++k) {
        const double v0 = y0[s * ld + k] - mean[k], vt = yt[s * ld + k] - mean[d + k];
        a0 += v0 * G00[k * d + c];
        b0 += vt * G0t[c * d + k];
        at += vt * Gtt[k * d + c];
        bt += v0 * G0t[k * d + c];
    }
    if constexpr (WEIGHTED) {
        const double what = vamp_weight(wts[s]) / wtot[0];
        g0[s * ldg + c] = what * (2.0 * a0 + b0);
        gt[s * ldg + c] = what * (2.0 * at + bt);
    } else {
        g0[s * ldg + c] = (2.0 * a0 + b0) / (double)m;
        gt[s * ldg + c] = (2.0 * at + bt) / (double)m;
    }
}

// wts: the pairs' weights [m], or NULL for uniform weights (work is then vamp_work(m, d), else vamp_work(m, d, true))
msm_status vamp2_launch(msm_ctx* ctx, const double* y0, const double* yt, const double* wts, int m, int d, int64_t ld,
                        const VampOpts& o, double* work, double* stats, double* g0, double* gt, int64_t ldg) {
    const VampWork w = vamp_work(m, d, wts != nullptr);
    const int T = (d + 15) / 16;
    const double* wsum = wts ? work + w.wsum : nullptr;
    const double* wtot = wts ? work + w.wtot : nullptr;
    if (wts)
        hipLaunchKernelGGL(vamp2_wsum_kernel, dim3(w.chunks), dim3(192), 0, ctx->stream, y0, yt, wts, m, d, ld,
                           work + w.psum, work + w.wsum);
    else
        hipLaunchKernelGGL(vamp2_colsum_kernel, dim3(w.chunks), dim3(128), 0, ctx->stream, y0, yt, m, d, ld,
                           work + w.psum);
    auto moments = wts ? vamp2_moments_kernel<true> : vamp2_moments_kernel<false>;
    hipLaunchKernelGGL(moments, dim3(3 * T * T, w.chunks), dim3(64), 0, ctx->stream, y0, yt, wts, m, d, ld,
                       work + w.psum, wsum, w.chunks, work + w.pmom);
    const size_t lds = (size_t)2 * d * d * sizeof(double);   // <= 64 KiB
    if (lds > 48 * 1024)
        MSM_HIP(ctx, hipFuncSetAttribute((const void*)vamp2_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)lds));
    hipLaunchKernelGGL(vamp2_solve_kernel, dim3(1), dim3(kSolveThreads), lds, ctx->stream, m, d, o, w, work, stats);
    if (g0) {
        const long long total = (long long)m * d;
        const dim3 grid((unsigned)((total + 255) / 256));
        auto grad = wts ? vamp2_grad_kernel<true> : vamp2_grad_kernel<false>;
        hipLaunchKernelGGL(grad, grid, dim3(256), 0, ctx->stream, y0, yt, wts, m, d, ld, work + w.G, work + w.mean,
                           wtot, g0, gt, ldg);
    }
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

TrainLayout train_layout(const MlpPlan& p, int m, size_t n_params, bool weighted = false) {
    TrainLayout t;
    const long long S2 = 2LL * m;
    const int n_out = p.width[p.n_linear];
    long long off = mlp_tape_layout(p, S2, &t.tape, &t.keep);
    t.y = off;
    off += S2 * n_out;
    t.dy = off;
    off += S2 * n_out;
    t.partial = off;
    off += (long long)((S2 + kChunk - 1) / kChunk) * (long long)n_params;
    t.loss = off;
    off += vamp_work(m, n_out, weighted).total;
    t.total = off;
    return t;
}

// ---- clip + AdamW ------------------------------------------------------------------------------------------------
// out[0] = |g|, out[1] = |g| after the clip, out[2] = 1 when |g| is not finite (the update is then skipped),
// out[3] = the clip coefficient.  One workgroup: thread t sums entries t, t + 1024, ... in ascending order, the
// threads' sums meet in a fixed tree, so the norm depends on n alone.
__global__ __launch_bounds__(1024) void adamw_norm_kernel(const double* __restrict__ grad, int64_t n, double clip,
                                                          double* __restrict__ out) {
    __shared__ double red[16];
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < n; e += 1024) s += grad[e] * grad[e];
    const double total = block_sum_lane0(s, red);
    if (threadIdx.x == 0) {
        const double norm = sqrt(total);
        const bool finite = fabs(norm) <= DBL_MAX;
        const double coef = clip > 0.0 ? fmin(1.0, clip / (norm + 1e-6)) : 1.0;
        out[0] = norm;
        out[1] = norm * coef;
        out[2] = finite ? 0.0 : 1.0;
        out[3] = coef;
    }
}

struct AdamOpts {
    double lr, beta1, beta2, eps, wd, bc1, bc2_sqrt;
};

__global__ __launch_bounds__(256) void adamw_update_kernel(float* __restrict__ prm, const double* __restrict__ grad,
                                                           double* __restrict__ mom, double* __restrict__ var, int64_t n,
                                                           AdamOpts o, const double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || out[2] != 0.0) return;
    const double g = grad[e] * out[3];
    const double mm = o.beta1 * mom[e] + (1.0 - o.beta1) * g;
    const double vv = o.beta2 * var[e] + (1.0 - o.beta2) * (g * g);
    double w = (double)prm[e] * (1.0 - o.lr * o.wd);
    w = w - (o.lr / o.bc1) * (mm / (sqrt(vv) / o.bc2_sqrt + o.eps));
    mom[e] = mm;
    var[e] = vv;
    prm[e] = (float)w;
}

// msm_vamp2_loss (d_w NULL) and msm_vamp2_loss_weighted: one envelope, one set of checks
msm_status vamp2_entry(msm_ctx* ctx, const char* fn, const double* d_y0, const double* d_yt, const double* d_w,
                       int64_t m, int n_out, int64_t ld, double eps, double eps_abs, double alpha, double cond_reg,
                       double* d_work, double* d_stats, double* d_grad0, double* d_gradt, int64_t ldg) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, m >= 1, "%s: %lld frame pairs", fn, (long long)m);
    if (m > kVampMaxPairs)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "%s: %lld frame pairs (at most %lld are supported)", fn, (long long)m,
                        (long long)kVampMaxPairs);
    MSM_REQUIRE(ctx, n_out >= 1, "%s: %d outputs", fn, n_out);
    if (n_out > kMlpMaxOut)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "%s: %d outputs (at most %d are supported)", fn, n_out, kMlpMaxOut);
    MSM_REQUIRE(ctx, ld >= n_out, "%s: row stride %lld for %d outputs", fn, (long long)ld, n_out);
    MSM_REQUIRE(ctx, d_y0 && d_yt && d_work && d_stats, "%s: NULL pointer", fn);
    MSM_REQUIRE(ctx, (d_grad0 == nullptr) == (d_gradt == nullptr), "%s: the two gradients go together", fn);
    MSM_REQUIRE(ctx, !d_grad0 || ldg >= n_out, "%s: gradient row stride %lld for %d outputs", fn, (long long)ldg, n_out);
    const VampOpts o = {eps, std::max(eps_abs, 0.0), std::min(std::max(alpha, 0.0), 1.0), std::max(cond_reg, 0.0)};
    return vamp2_launch(ctx, d_y0, d_yt, d_w, (int)m, n_out, ld, o, d_work, d_stats, d_grad0, d_gradt, ldg);
}

// msm_mlp_train_workspace and its weighted sibling
size_t train_workspace(int64_t m, int n_linear, const int32_t* h_widths, int ln_in, int ln_hidden, int head_activation,
                       bool weighted) {
    if (!h_widths || m < 2 || m > (1 << 24)) return 0;
    MlpPlan p;
    size_t n_params = 0;   // a refusal has nowhere to leave its message (no context): it is reported as 0
    if (mlp_make_plan(nullptr, "msm_mlp_train_workspace", h_widths[0], n_linear, h_widths, 0, ln_in, ln_hidden,
                      head_activation, kMlpAnyParams, &p, &n_params))
        return 0;
    return (size_t)train_layout(p, (int)m, n_params, weighted).total * sizeof(double);
}

}  // namespace

extern "C" {

size_t msm_vamp2_workspace(int64_t m, int n_out) {
    if (m < 1 || n_out < 1 || n_out > kMlpMaxOut || m > kVampMaxPairs) return 0;
    return (size_t)vamp_work((int)m, n_out).total * sizeof(double);
}

msm_status msm_vamp2_loss(msm_ctx* ctx, const double* d_y0, const double* d_yt, int64_t m, int n_out, int64_t ld,
                          double eps, double eps_abs, double alpha, double cond_reg, double* d_work,
                          double* d_stats, double* d_grad0, double* d_gradt, int64_t ldg) {
    return vamp2_entry(ctx, "msm_vamp2_loss", d_y0, d_yt, nullptr, m, n_out, ld, eps, eps_abs, alpha, cond_reg, d_work,
                       d_stats, d_grad0, d_gradt, ldg);
}

size_t msm_vamp2_weighted_workspace(int64_t m, int n_out) {
    if (m < 1 || n_out < 1 || n_out > kMlpMaxOut || m > kVampMaxPairs) return 0;
    return (size_t)vamp_work((int)m, n_out, true).total * sizeof(double);
}

msm_status msm_vamp2_loss_weighted(msm_ctx* ctx, const double* d_y0, const double* d_yt, const double* d_w, int64_t m,
                                   int n_out, int64_t ld, double eps, double eps_abs, double alpha, double cond_reg,
                                   double* d_work, double* d_stats, double* d_grad0, double* d_gradt, int64_t ldg) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, d_w, "msm_vamp2_loss_weighted: NULL pointer");
    return vamp2_entry(ctx, "msm_vamp2_loss_weighted", d_y0, d_yt, d_w, m, n_out, ld, eps, eps_abs, alpha, cond_reg,
                       d_work, d_stats, d_grad0, d_gradt, ldg);
}

size_t msm_mlp_train_workspace(int64_t m, int n_linear, const int32_t* h_widths, int ln_in, int ln_hidden,
                               int head_activation) {
    return train_workspace(m, n_linear, h_widths, ln_in, ln_hidden, head_activation, false);
}

size_t msm_mlp_train_weighted_workspace(int64_t m, int n_linear, const int32_t* h_widths, int ln_in, int ln_hidden,
                                        int head_activation) {
    return train_workspace(m, n_linear, h_widths, ln_in, ln_hidden, head_activation, true);
}

msm_status msm_mlp_loss_grad(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                             const double* d_mean, const double* d_scale, int n_linear, const int32_t* h_widths,
                             int activation, int ln_in, int ln_hidden, int head_activation, const float* d_params,
                             size_t n_params, const int64_t* d_idx_t, const int64_t* d_idx_tau, int64_t m,
                             const double* h_dropout, uint64_t seed, uint64_t step, double eps, double eps_abs,
                             double alpha, double cond_reg, double* d_work, size_t work_bytes, double* d_stats,
                             double* d_grad, double* d_out, int64_t ldo) {
    return msm_mlp_loss_grad_weighted(ctx, d_x, dtype, n, F, ld, d_mean, d_scale, n_linear, h_widths, activation, ln_in,
                                      ln_hidden, head_activation, d_params, n_params, d_idx_t, d_idx_tau, nullptr, m,
                                      h_dropout, seed, step, eps, eps_abs, alpha, cond_reg, d_work, work_bytes, d_stats,
                                      d_grad, d_out, ldo);
}

msm_status msm_mlp_loss_grad_weighted(msm_ctx* ctx, const void* d_x, msm_dtype dtype, int64_t n, int F, int64_t ld,
                                      const double* d_mean, const double* d_scale, int n_linear,
                                      const int32_t* h_widths, int activation, int ln_in, int ln_hidden,
                                      int head_activation, const float* d_params, size_t n_params,
                                      const int64_t* d_idx_t, const int64_t* d_idx_tau, const double* d_w, int64_t m,
                                      const double* h_dropout, uint64_t seed, uint64_t step, double eps, double eps_abs,
                                      double alpha, double cond_reg, double* d_work, size_t work_bytes, double* d_stats,
                                      double* d_grad, double* d_out, int64_t ldo) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, dtype == MSM_F32 || dtype == MSM_F64, "msm_mlp_loss_grad: bad dtype");
    MlpPlan p;
    if (msm_status st = mlp_make_plan(ctx, "msm_mlp_loss_grad", F, n_linear, h_widths, activation, ln_in, ln_hidden,
                                      head_activation, n_params, &p))
        return st;
    const int n_out = p.width[n_linear];
    if (m < 2 || m > (1 << 24))
        return msm_fail(ctx, m < 2 ? MSM_ERR_INVALID : MSM_ERR_UNSUPPORTED,
                        "msm_mlp_loss_grad: %lld frame pairs (2 to %d are supported)", (long long)m, 1 << 24);
    MSM_REQUIRE(ctx, n >= 1 && ld >= F, "msm_mlp_loss_grad: bad shape (n = %lld, ld = %lld)", (long long)n,
                (long long)ld);
    MSM_REQUIRE(ctx, (d_mean == nullptr) == (d_scale == nullptr), "msm_mlp_loss_grad: scaler mean and scale go together");
    MSM_REQUIRE(ctx, d_x && d_params && d_idx_t && d_idx_tau && d_work && d_stats, "msm_mlp_loss_grad: NULL pointer");
    MSM_REQUIRE(ctx, !d_out || ldo >= n_out, "msm_mlp_loss_grad: output row stride %lld for %d outputs",
                (long long)ldo, n_out);
    MSM_REQUIRE(ctx, step <= 0xffffffffull, "msm_mlp_loss_grad: step %llu does not fit the 32-bit counter word",
                (unsigned long long)step);
    DropPlan drop;
    drop.on = 0;
    drop.k0 = (unsigned)seed;
    drop.k1 = (unsigned)(seed >> 32);
    drop.step = (unsigned)step;
    for (int i = 0; i <= kMlpMaxLinear; ++i) {
        drop.thr[i] = 0;
        drop.scale[i] = 1.0;
    }
    if (h_dropout)
        for (int i = 0; i < n_linear; ++i) {   // site 0: inputs, site i: after the activation of Linear i - 1
            const double q = h_dropout[i];
            MSM_REQUIRE(ctx, q >= 0.0 && q < 1.0, "msm_mlp_loss_grad: dropout probability %g at site %d (0 <= p < 1)", q,
                        i);
            drop.thr[i] = (unsigned)floor(q * 4294967296.0);
            drop.scale[i] = 1.0 / (1.0 - q);
            if (drop.thr[i]) drop.on = 1;
        }
    const TrainLayout lay = train_layout(p, (int)m, n_params, d_w != nullptr);
    MSM_REQUIRE(ctx, work_bytes >= (size_t)lay.total * sizeof(double),
                "msm_mlp_loss_grad: workspace of %zu bytes, %zu are needed", work_bytes,
                (size_t)lay.total * sizeof(double));

    MlpLaunch s;
    if (msm_status st = mlp_launch_shape(ctx, mlp_train_kernel_address(false, dtype), p, 2 * m, &s)) return st;
#define MSM_MLP_TRAIN(T)                                                                                              \
    hipLaunchKernelGGL(mlp_train_forward_kernel<T>, dim3(s.grid), dim3(64), s.lds, ctx->stream, (const T*)d_x, n, ld, \
                       d_mean, d_scale, d_params, p, d_idx_t, d_idx_tau, (int)m, drop, lay, d_work)
    if (dtype == MSM_F32) MSM_MLP_TRAIN(float);
    else MSM_MLP_TRAIN(double);
#undef MSM_MLP_TRAIN
    MSM_CHECK_LAUNCH(ctx);
    double* y = d_work + lay.y;
    double* dy = d_work + lay.dy;
    const VampOpts o = {eps, std::max(eps_abs, 0.0), std::min(std::max(alpha, 0.0), 1.0), std::max(cond_reg, 0.0)};
    if (msm_status st = vamp2_launch(ctx, y, y + (size_t)m * n_out, d_w, (int)m, n_out, n_out, o, d_work + lay.loss,
                                     d_stats, d_grad ? dy : nullptr, d_grad ? dy + (size_t)m * n_out : nullptr, n_out))
        return st;
    if (d_out)
        MSM_HIP(ctx, hipMemcpy2DAsync(d_out, (size_t)ldo * sizeof(double), y, (size_t)n_out * sizeof(double),
                                      (size_t)n_out * sizeof(double), (size_t)(2 * m), hipMemcpyDeviceToDevice,
                                      ctx->stream));
    if (!d_grad) return MSM_OK;
    if (msm_status st = mlp_launch_shape(ctx, mlp_train_kernel_address(true, dtype), p, 2 * m, &s)) return st;
    hipLaunchKernelGGL(mlp_train_backward_kernel, dim3(s.grid), dim3(64), s.lds, ctx->stream, d_params, p, (int)m, drop,
                       lay, d_work);
    const int jobs = param_jobs(p);
    const int chunks = (int)((2 * m + kChunk - 1) / kChunk);
    hipLaunchKernelGGL(mlp_train_param_partial_kernel, dim3(jobs, chunks), dim3(64), 0, ctx->stream, p, (int)m, lay,
                       (int)n_params, d_work, d_work + lay.partial);
    hipLaunchKernelGGL(mlp_train_param_reduce_kernel, dim3((unsigned)((n_params + 255) / 256)), dim3(256), 0, ctx->stream,
                       d_work + lay.partial, chunks, (int)n_params, d_grad);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_mlp_launch_plan(msm_ctx* ctx, int kernel, msm_dtype dtype, int64_t rows, int n_linear,
                               const int32_t* h_widths, int ln_in, int ln_hidden, int head_activation, int64_t out[8]) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, out, "msm_mlp_launch_plan: NULL pointer");
    MSM_REQUIRE(ctx, kernel >= MSM_MLP_KERNEL_FORWARD && kernel <= MSM_MLP_KERNEL_TRAIN_BACKWARD,
                "msm_mlp_launch_plan: unknown kernel code %d", kernel);
    MSM_REQUIRE(ctx, dtype == MSM_F32 || dtype == MSM_F64, "msm_mlp_launch_plan: bad dtype");
    MSM_REQUIRE(ctx, h_widths, "msm_mlp_launch_plan: NULL widths");
    MlpPlan p;
    if (msm_status st = mlp_make_plan(ctx, "msm_mlp_launch_plan", h_widths[0], n_linear, h_widths, 0, ln_in, ln_hidden,
                                      head_activation, kMlpAnyParams, &p))
        return st;
    const bool train = kernel == MSM_MLP_KERNEL_TRAIN_FORWARD || kernel == MSM_MLP_KERNEL_TRAIN_BACKWARD;
    const int64_t m = rows / 2;
    if (train) {
        MSM_REQUIRE(ctx, rows >= 0 && rows % 2 == 0, "msm_mlp_launch_plan: %lld slots (a training batch has 2m)",
                    (long long)rows);
        if (m < 2 || m > (1 << 24))
            return msm_fail(ctx, m < 2 ? MSM_ERR_INVALID : MSM_ERR_UNSUPPORTED,
                            "msm_mlp_launch_plan: %lld frame pairs (2 to %d are supported)", (long long)m, 1 << 24);
    } else {
        MSM_REQUIRE(ctx, rows >= 0, "msm_mlp_launch_plan: bad shape (n = %lld)", (long long)rows);
    }
    const void* fn = kernel == MSM_MLP_KERNEL_FORWARD ? mlp_forward_kernel_address(dtype)
                     : kernel == MSM_MLP_KERNEL_VJP   ? mlp_vjp_kernel_address(dtype)
                                                      : mlp_train_kernel_address(kernel == MSM_MLP_KERNEL_TRAIN_BACKWARD, dtype);
    MlpLaunch s;
    if (msm_status st = mlp_launch_shape(ctx, fn, p, rows, &s)) return st;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    out[0] = (int64_t)s.lds;
    out[1] = s.per_cu;
    out[2] = s.grid;
    out[3] = s.n_groups;
    out[4] = s.trips;
    if (train) {
        out[5] = (rows + kChunk - 1) / kChunk;
        out[6] = vamp_work((int)m, p.width[n_linear]).chunks;
        out[7] = param_jobs(p);
    }
    return MSM_OK;
}

msm_status msm_adamw_step(msm_ctx* ctx, float* d_params, const double* d_grad, double* d_m, double* d_v, int64_t n,
                          int64_t step, double lr, double beta1, double beta2, double eps, double weight_decay,
                          double clip, double* d_out) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, n >= 1, "msm_adamw_step: %lld parameters", (long long)n);
    MSM_REQUIRE(ctx, step >= 1, "msm_adamw_step: step %lld (steps count from 1)", (long long)step);
    MSM_REQUIRE(ctx, d_params && d_grad && d_m && d_v && d_out, "msm_adamw_step: NULL pointer");
    MSM_REQUIRE(ctx, beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "msm_adamw_step: betas %g, %g", beta1,
                beta2);
    AdamOpts o;
    o.lr = lr;
    o.beta1 = beta1;
    o.beta2 = beta2;
    o.eps = eps;
    o.wd = weight_decay;
    o.bc1 = 1.0 - std::pow(beta1, (double)step);
    o.bc2_sqrt = std::sqrt(1.0 - std::pow(beta2, (double)step));
    hipLaunchKernelGGL(adamw_norm_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_grad, n, clip, d_out);
    hipLaunchKernelGGL(adamw_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_params,
                       d_grad, d_m, d_v, n, o, d_out);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"

const void* mlp_train_kernel_address(bool backward, msm_dtype dtype) {
    if (backward) return (const void*)mlp_train_backward_kernel;
    return dtype == MSM_F32 ? (const void*)mlp_train_forward_kernel<float>
                            : (const void*)mlp_train_forward_kernel<double>;
}
