// What the DeepTICA network kernels share: inference (mlp.hip), the input gradient (mlp_vjp.hip) and the training
// passes (mlp_train.hip).  Device code plus the host-side plan, tape and launch-shape builders; include after common.h.
//
// A wave owns 16 frames; lane (j, g) = (lane & 15, lane >> 4) works on frame j.  Activation rows sit in LDS as fp64
// [16][stride], two images that the layers ping-pong between.  There is one forward walk over a group
// (mlp_load_inputs, then mlp_forward_walk) and one set of adjoints (mlp_layer_adjoint, mlp_linear_transposed); what a
// kernel adds to them -- a tape for the adjoints, the inputs of the Linear layers, dropout -- is chosen at compile
// time and only inserts stores and row-local factors, so every kernel runs the same arithmetic per frame and the
// outputs of the three forward kernels agree bit for bit.
#pragma once
#include <algorithm>
#include <cfloat>

#include "common.h"
#include "philox.h"
#include "wave.h"

namespace {

constexpr int kMlpMaxWidth = 256;   // F, hidden widths
constexpr int kMlpMaxOut = 64;      // apply_output_transform's limit
constexpr int kMlpMaxLinear = 8;
constexpr int kChunk = MSM_MLP_CHUNK;   // slots per partial sum of a parameter gradient / of a moment (mlp_train.hip)

enum { kActTanh = 0, kActGelu = 1, kActRelu = 2, kActElu = 3, kActSelu = 4, kActLeakyRelu = 5, kActCount = 6 };

// where everything lies in the packed parameters (float offsets; -1: absent); travels by value
struct MlpPlan {
    int n_linear;
    int width[kMlpMaxLinear + 1];
    int w_off[kMlpMaxLinear], b_off[kMlpMaxLinear], ln_off[kMlpMaxLinear];
    int ln_in_off;
    int activation, head_activation;
    int stride[2];   // LDS row strides in doubles of the two images: widest width held, rounded up to 16, plus 2
};

#define WAVE_SYNC() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); __builtin_amdgcn_wave_barrier()

struct op_or {
    __device__ __forceinline__ int operator()(int a, int b) const { return a | b; }
};

constexpr double kSeluScale = 1.0507009873554804934193349852946;
constexpr double kSeluAlpha = 1.6732632423543772848170429916717;

// comparisons that are false for a NaN keep it (torch's relu and leaky_relu do)
__device__ __forceinline__ double mlp_activate(double x, int kind) {
    switch (kind) {
        case kActGelu: return 0.5 * x * (1.0 + erf(x * 0.70710678118654752440));
        case kActRelu: return x < 0.0 ? 0.0 : x;
        case kActElu: return x > 0.0 ? x : expm1(x);
        case kActSelu: return kSeluScale * (x > 0.0 ? x : kSeluAlpha * expm1(x));
        case kActLeakyRelu: return x < 0.0 ? 0.01 * x : x;
        default: return tanh(x);
    }
}

// LayerNorm of frame j's row of `w` entries, by its four lanes (j, g): lane g owns entries g, g + 4, ...; two-pass
// mean and biased variance, eps = 1e-5 inside the root.  The four partial sums meet through the row swaps, which
// leave the same bits in all four lanes.
__device__ __forceinline__ void mlp_layer_norm(double* row, int g, int w, const float* __restrict__ gamma_beta) {
    double s = 0.0;
    for (int f = g; f < w; f += 4) s += row[f];
    const double mean = xrow_reduce(s, op_sum{}) / (double)w;
    double q = 0.0;
    for (int f = g; f < w; f += 4) {
        const double c = row[f] - mean;
        q += c * c;
    }
    const double rstd = 1.0 / sqrt(xrow_reduce(q, op_sum{}) / (double)w + 1e-5);
    for (int f = g; f < w; f += 4)
        row[f] = (row[f] - mean) * rstd * (double)gamma_beta[f] + (double)gamma_beta[w + f];
}

// nxt[c] = bias[c] + sum_k W[c][k] cur[k], c < N, for the wave's 16 frames: out' (16 columns x 16 frames) =
// W (16 x K) . act' (K x 16 frames) per tile of 16 output columns, v_mfma_f64_16x16x4_f64, four tiles (64 columns)
// in flight per pass over K.  Lane (j, g) supplies W[c0 + j][k] and act[frame j][k] for the same k, and acc[r] is
// output column c0 + g + 4 r of frame j; k-step u of a chunk of 16 takes k = k0 + 4 g + u.  The last, partial chunk
// of K feeds zeros (both operands: a stale LDS word next to a zero weight could be a NaN), and output columns past
// N are computed from a clamped row of W and never stored.  cur / nxt: frame j's rows; the caller has made the rows
// of `cur` complete (WAVE_SYNC) before the call.
__device__ __forceinline__ void mlp_linear(const double* cur, double* nxt, const float* __restrict__ W,
                                           const float* __restrict__ bias, int K, int N, int j, int g) {
    for (int n0 = 0; n0 < N; n0 += 64) {
        v4f64 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = n0 + 16 * t + g + 4 * r;
                acc[t][r] = c < N ? (double)bias[c] : 0.0;
            }
        // rows of W at or past N are clamped onto row N - 1: they reach only accumulator entries that are never
        // stored
        const float* wrow[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) wrow[t] = W + (size_t)min(n0 + 16 * t + j, N - 1) * K;
        const int K16 = K & ~15;
        for (int k0 = 0; k0 < K16; k0 += 16) {   // whole chunks: no masks, 16-byte reads of both operands
            const int kb = k0 + 4 * g;
            const double2 b01 = *reinterpret_cast<const double2*>(cur + kb);
            const double2 b23 = *reinterpret_cast<const double2*>(cur + kb + 2);
            const double b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (n0 + 16 * t < N) {   // wave-uniform
                    float w[4];
                    __builtin_memcpy(w, wrow[t] + kb, sizeof(w));   // 4-byte aligned: the compiler picks the width
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)w[u], b[u], acc[t], 0, 0, 0);
                }
            }
        }
        if (K16 < K) {   // the last, partial chunk: both operands zero past K
            const int kb = K16 + 4 * g;
            double b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) b[u] = kb + u < K ? cur[kb + u] : 0.0;   // kb + u < stride always
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (n0 + 16 * t < N) {
                    double a[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) a[u] = kb + u < K ? (double)wrow[t][kb + u] : 0.0;
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc[t], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = n0 + 16 * t + g + 4 * r;
                if (c < N) nxt[c] = acc[t][r];
            }
    }
}

// rows 0 .. rows-1 of an LDS image (row stride S, w entries each) to global rows of w doubles, coalesced
__device__ __forceinline__ void save_rows(const double* img, int S, int w, int rows, double* __restrict__ dst, int lane) {
    for (int r = 0; r < rows; ++r)
        for (int f = lane; f < w; f += 64) dst[(size_t)r * w + f] = img[r * S + f];
}

// The tape: what a forward walk leaves per frame, in a workspace, for the adjoints (offsets in doubles; -1: absent;
// [rows, width] each; travels by value):
//   z     the scaled inputs when an input LayerNorm follows: its adjoint needs the row mean, the root and xhat, which
//         are recomputed from z (three cheap passes over a cached row) rather than stored;
//   u[l]  the output of Linear l when a LayerNorm follows, for the same reason;
//   h[l]  the value the activation is applied to: act'(h).  Storing h instead of recomputing it from u saves a
//         second LayerNorm per row in the backward pass and costs one row of doubles.
struct MlpTape {
    long long z;
    long long h[kMlpMaxLinear], u[kMlpMaxLinear];
};

// What the training passes keep per slot besides the tape:
//   a[l]   the input of Linear l (after LayerNorm, activation and dropout of the layer before): dW_l = du_l' a[l];
//   du[l]  dL/d(output of Linear l);
//   dh[l], dhx[l] (dz, dzx for the input LayerNorm)  dL/d(LayerNorm output) and that times xhat: the beta and gamma
//          gradients are their column sums.
struct MlpTrainSlots {
    long long dz, dzx;
    long long a[kMlpMaxLinear], du[kMlpMaxLinear], dh[kMlpMaxLinear], dhx[kMlpMaxLinear];
};

// The one walk that places them, for `rows` rows each; returns the doubles taken.  Without `train` the tape alone,
// z, then per layer u and h; with it the training workspace, the tape's tensors among the others.
inline long long mlp_tape_layout(const MlpPlan& p, long long rows, MlpTape* t, MlpTrainSlots* train = nullptr) {
    long long off = 0;
    auto take = [&](bool present, long long w) {
        if (!present) return -1LL;
        const long long at = off;
        off += rows * w;
        return at;
    };
    MlpTrainSlots none;
    MlpTrainSlots* x = train ? train : &none;
    const bool tr = train != nullptr, ln_in = p.ln_in_off >= 0;
    t->z = take(ln_in, p.width[0]);
    x->dz = take(tr && ln_in, p.width[0]);
    x->dzx = take(tr && ln_in, p.width[0]);
    for (int l = 0; l < kMlpMaxLinear; ++l) t->h[l] = t->u[l] = x->a[l] = x->du[l] = x->dh[l] = x->dhx[l] = -1;
    for (int l = 0; l < p.n_linear; ++l) {
        const int K = p.width[l], N = p.width[l + 1];
        const bool last = l == p.n_linear - 1;
        const bool act = !last || p.head_activation, ln = !last && p.ln_off[l] >= 0;
        x->a[l] = take(tr, K);
        x->du[l] = take(tr, N);
        if (tr) t->h[l] = take(act, N);    // the training workspace has h ahead of u, the tape alone behind it
        t->u[l] = take(ln, N);
        if (!tr) t->h[l] = take(act, N);
        x->dh[l] = take(tr && ln, N);
        x->dhx[l] = take(tr && ln, N);
    }
    return off;
}

// per dropout site (0: inputs, i + 1: after the activation of Linear i): keep iff word >= thr; kept values times scale
struct DropPlan {
    int on;
    unsigned thr[kMlpMaxLinear + 1];
    double scale[kMlpMaxLinear + 1];
    unsigned k0, k1, step;
};

// Dropout of frame j's row (slot `slot`) at site `site`, forward and adjoint alike: row[f] *= keep ? scale : 0.
// Lane g takes the column blocks g, g + 4, ... of four columns, one Philox call each; the caller synchronises
// the wave before and after (the lanes of a row own other entries outside this function).  Masks are never stored:
// a mask bit is a pure function of (seed, step, site, slot, column), and the backward pass draws it again.
__device__ __forceinline__ void mlp_dropout(double* row, int g, int w, const DropPlan& d, int site, unsigned slot) {
    const Philox rng{d.k0, d.k1};
    const unsigned thr = d.thr[site];
    const double scale = d.scale[site];
    for (int cb = g; 4 * cb < w; cb += 4) {
        uint32_t c[4] = {d.step, (uint32_t)site, slot, (uint32_t)cb};
        rng(c);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = 4 * cb + u;
            if (f < w) row[f] = row[f] * (c[u] >= thr ? scale : 0.0);
        }
    }
}

// The 16 input rows of a group into image 0 (row stride S): Z = (x - mean) / scale in fp64, rounded to fp32 as the
// reference hands it to the network.  row_of(r), asked for r < rows only, names the row of x that enters as row r, or
// is negative: that row is not read and enters as NaN (all outputs of that frame are NaN).  Rows at or past `rows`
// are not read either and enter as zeros.
template <typename T, typename RowOf>
__device__ __forceinline__ void mlp_load_inputs(double* img0, int S, int F, int lane, int rows, const T* __restrict__ x,
                                                int64_t ld, const double* __restrict__ sc_mean,
                                                const double* __restrict__ sc_scale, RowOf row_of) {
    for (int r = 0; r < 16; ++r) {
        const int64_t row = r < rows ? row_of(r) : 0;
        for (int f = lane; f < F; f += 64) {
            double z = 0.0;
            if (r < rows) {
                z = __longlong_as_double(0x7ff8000000000000ll);
                if (row >= 0) {
                    z = (double)x[row * ld + f];
                    if (sc_mean) z = (z - sc_mean[f]) / sc_scale[f];
                    z = (double)(float)z;
                }
            }
            img0[r * S + f] = z;
        }
    }
}

// where a forward walk that keeps something puts it: `ws` + the layouts' offsets, rows from `row0` on (row0 + j is
// also frame j's slot in the dropout counter).  `train` and `drop` only with the training option.
struct MlpKeep {
    const MlpTape* tape;
    const MlpTrainSlots* train;
    const DropPlan* drop;
    double* ws;
    size_t row0;
};

// The forward walk of a group of 16 frames, from "the group's input rows are in image 0" (mlp_load_inputs) to "frame
// j's output row is at the pointer returned": the non-finite flag (`bad`: a non-finite Z anywhere in the frame, all
// of whose outputs are then NaN), the input LayerNorm, and per layer Linear, LayerNorm and activation, the two images
// swapping roles.  What is decided at compile time, and inserts nothing into the arithmetic of a frame:
//   TAPE   z, u[l] and h[l] are written to k.tape (see MlpTape);
//   TRAIN  (with TAPE) dropout by k.drop at every site that has it, and a[l] written to k.train.
// Without either (inference) `k` is not looked at, and there is no WAVE_SYNC beyond the one in front of each Linear.
template <bool TAPE, bool TRAIN>
__device__ __forceinline__ double* mlp_forward_walk(const MlpPlan& p, const float* __restrict__ params,
                                                    double* const* img, int lane, int rows, const MlpKeep& k,
                                                    int* bad_out) {
    static_assert(TAPE || !TRAIN, "the training walk writes the tape");
    const int j = lane & 15, g = lane >> 4;
    const int F = p.width[0], S = p.stride[0];
    WAVE_SYNC();   // the input rows are complete
    if constexpr (TAPE)
        if (k.tape->z >= 0) save_rows(img[0], S, F, rows, k.ws + k.tape->z + k.row0 * F, lane);
    double* cur = img[0] + j * S;   // frame j's row, current and next layer
    double* nxt = img[1] + j * p.stride[1];
    int bad = 0;
    for (int f = g; f < F; f += 4) bad |= !(fabs(cur[f]) <= DBL_MAX);
    *bad_out = xrow_reduce(bad, op_or{});
    if (p.ln_in_off >= 0) mlp_layer_norm(cur, g, F, params + p.ln_in_off);
    if constexpr (TRAIN) {
        if (k.drop->on && k.drop->thr[0]) {
            WAVE_SYNC();
            mlp_dropout(cur, g, F, *k.drop, 0, (unsigned)(k.row0 + j));
        }
        WAVE_SYNC();
        save_rows(img[0], S, F, rows, k.ws + k.train->a[0] + k.row0 * F, lane);
    }
    for (int l = 0; l < p.n_linear; ++l) {
        const int K = p.width[l], N = p.width[l + 1];
        const int Sn = p.stride[(l + 1) & 1];
        const double* image = img[(l + 1) & 1];   // the image `nxt` is a row of
        WAVE_SYNC();   // the rows of `cur` are complete: every lane reads entries other lanes wrote
        mlp_linear(cur, nxt, params + p.w_off[l], params + p.b_off[l], K, N, j, g);
        // lane (j, g) wrote the entries c = g mod 4 of its row and is the one that normalises and activates them; the
        // tape's stores read whole rows, hence their WAVE_SYNC
        const bool last = l == p.n_linear - 1;
        if (!last && p.ln_off[l] >= 0) {
            if constexpr (TAPE) {
                WAVE_SYNC();
                save_rows(image, Sn, N, rows, k.ws + k.tape->u[l] + k.row0 * N, lane);
            }
            mlp_layer_norm(nxt, g, N, params + p.ln_off[l]);
        }
        if (!last || p.head_activation) {
            if constexpr (TAPE) {
                WAVE_SYNC();
                save_rows(image, Sn, N, rows, k.ws + k.tape->h[l] + k.row0 * N, lane);
            }
            for (int f = g; f < N; f += 4) nxt[f] = mlp_activate(nxt[f], p.activation);
        }
        if constexpr (TRAIN)
            if (!last) {
                if (k.drop->on && k.drop->thr[l + 1]) {
                    WAVE_SYNC();
                    mlp_dropout(nxt, g, N, *k.drop, l + 1, (unsigned)(k.row0 + j));
                }
                WAVE_SYNC();
                save_rows(image, Sn, N, rows, k.ws + k.train->a[l + 1] + k.row0 * N, lane);
            }
        double* swap = cur;
        cur = nxt;
        nxt = swap;
    }
    return cur;
}

// ---- the adjoints (mlp_vjp.hip, mlp_train.hip) ----
__device__ __forceinline__ double mlp_activate_grad(double x, int kind) {
    switch (kind) {
        case kActGelu:
            return 0.5 * (1.0 + erf(x * 0.70710678118654752440)) + x * exp(-0.5 * x * x) * 0.39894228040143267794;
        case kActRelu: return x <= 0.0 ? 0.0 : 1.0;
        case kActElu: return x > 0.0 ? 1.0 : exp(x);
        case kActSelu: return kSeluScale * (x > 0.0 ? 1.0 : kSeluAlpha * exp(x));
        case kActLeakyRelu: return x > 0.0 ? 1.0 : 0.01;
        default: {
            const double t = tanh(x);
            return 1.0 - t * t;
        }
    }
}

// LayerNorm adjoint of frame j's row: `grow` holds dL/d(LN output) on entry and dL/d(LN input) on exit; `xin` is
// the row the LayerNorm was applied to (global).  dL/d(output) and dL/d(output) * xhat go to dh / dhx (the beta and
// gamma gradients are their column sums).  Lane g owns entries g, g + 4, ...; `store`: the slot exists.
__device__ __forceinline__ void mlp_layer_norm_adjoint(double* grow, int g, int w, const double* __restrict__ xin,
                                                       const float* __restrict__ gamma, double* __restrict__ dh,
                                                       double* __restrict__ dhx, bool store) {
    double s = 0.0;
    for (int f = g; f < w; f += 4) s += xin[f];
    const double mean = xrow_reduce(s, op_sum{}) / (double)w;
    double q = 0.0;
    for (int f = g; f < w; f += 4) {
        const double c = xin[f] - mean;
        q += c * c;
    }
    const double rstd = 1.0 / sqrt(xrow_reduce(q, op_sum{}) / (double)w + 1e-5);
    double s1 = 0.0, s2 = 0.0;
    for (int f = g; f < w; f += 4) {
        const double xhat = (xin[f] - mean) * rstd;
        const double d = grow[f];
        if (store) {
            dh[f] = d;
            dhx[f] = d * xhat;
        }
        const double dxhat = d * (double)gamma[f];
        grow[f] = dxhat;
        s1 += dxhat;
        s2 += dxhat * xhat;
    }
    s1 = xrow_reduce(s1, op_sum{}) / (double)w;
    s2 = xrow_reduce(s2, op_sum{}) / (double)w;
    for (int f = g; f < w; f += 4) {
        const double xhat = (xin[f] - mean) * rstd;
        grow[f] = rstd * (grow[f] - s1 - xhat * s2);
    }
}

// The adjoint of layer l's activation and LayerNorm on frame j's row: `gout` holds dE/d(output of layer l) on entry
// and du_l on exit; h[l] and u[l] come from the tape's row `row` in `ws`.  KEEP (training): dh and dhx of the row go
// to `train`'s slots when the frame exists (`mine`).  The caller has synchronised the wave: the tape rows are in
// place, and so are the entries of gout other lanes wrote.
template <bool KEEP>
__device__ __forceinline__ void mlp_layer_adjoint(double* gout, int g, const MlpPlan& p, int l,
                                                  const float* __restrict__ params, const MlpTape& tape,
                                                  const MlpTrainSlots* train, double* ws, size_t row, bool mine) {
    const int N = p.width[l + 1];
    const bool last = l == p.n_linear - 1;
    if (!last || p.head_activation) {
        const double* h = ws + tape.h[l] + row * N;
        for (int f = g; f < N; f += 4) gout[f] = gout[f] * mlp_activate_grad(h[f], p.activation);
    }
    if (!last && p.ln_off[l] >= 0) {
        double* dh = nullptr, *dhx = nullptr;
        if constexpr (KEEP) {
            dh = ws + train->dh[l] + row * N;
            dhx = ws + train->dhx[l] + row * N;
        }
        mlp_layer_norm_adjoint(gout, g, N, ws + tape.u[l] + row * N, params + p.ln_off[l], dh, dhx, KEEP && mine);
    }
}

// The transposed Linear, gin[k] = sum_n W[n][k] gout[n], k < K, for the wave's 16 frames: out' (K x 16 frames) =
// W' (K x N) . gout' (N x 16 frames) per tile of 16 entries k on the matrix cores.  gout / gin: frame j's rows; the
// caller has made the rows of `gout` complete (WAVE_SYNC) before the call.
__device__ __forceinline__ void mlp_linear_transposed(const double* gout, double* gin, const float* __restrict__ W,
                                                      int K, int N, int j, int g) {
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int kc = min(k0 + j, K - 1);
        const v4f64 acc = mfma_tile_acc(
            N, g, k0 + j < K, true, [&](int nn) { return (double)W[(size_t)nn * K + kc]; },
            [&](int nn) { return gout[nn]; });
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = k0 + g + 4 * r;
            if (k < K) gin[k] = acc[r];
        }
    }
}

constexpr size_t kMlpAnyParams = ~(size_t)0;   // mlp_make_plan: do not check the parameter count

// The plan of a network from the arguments every entry point takes; `fn` names the entry in the messages.  Checks
// the envelope (MSM_ERR_UNSUPPORTED beyond it, naming the number) and the parameter count, which `needed` receives.
inline msm_status mlp_make_plan(msm_ctx* ctx, const char* fn, int F, int n_linear, const int32_t* h_widths,
                                int activation, int ln_in, int ln_hidden, int head_activation, size_t n_params,
                                MlpPlan* out, size_t* needed = nullptr) {
    MSM_REQUIRE(ctx, h_widths, "%s: NULL widths", fn);
    if (n_linear < 1 || n_linear > kMlpMaxLinear)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "%s: %d Linear layers (1 to %d are supported)", fn, n_linear,
                        kMlpMaxLinear);
    MSM_REQUIRE(ctx, activation >= 0 && activation < kActCount, "%s: unknown activation code %d", fn, activation);
    MSM_REQUIRE(ctx, h_widths[0] == F, "%s: widths[0] = %d but F = %d", fn, (int)h_widths[0], F);
    MlpPlan p;
    p.n_linear = n_linear;
    p.activation = activation;
    p.head_activation = head_activation ? 1 : 0;
    for (int i = 0; i <= kMlpMaxLinear; ++i) p.width[i] = 0;
    for (int i = 0; i < kMlpMaxLinear; ++i) p.w_off[i] = p.b_off[i] = p.ln_off[i] = -1;
    for (int i = 0; i <= n_linear; ++i) {
        const int w = h_widths[i];
        MSM_REQUIRE(ctx, w >= 1, "%s: width %d of layer %d", fn, w, i);
        if (w > kMlpMaxWidth)
            return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "%s: width %d of layer %d (at most %d is supported)", fn, w, i,
                            kMlpMaxWidth);
        p.width[i] = w;
    }
    const int n_out = p.width[n_linear];
    if (n_out > kMlpMaxOut)
        return msm_fail(ctx, MSM_ERR_UNSUPPORTED, "%s: %d outputs (at most %d are supported)", fn, n_out, kMlpMaxOut);
    size_t off = 0;
    p.ln_in_off = -1;
    if (ln_in) {
        p.ln_in_off = 0;
        off = 2 * (size_t)F;
    }
    for (int l = 0; l < n_linear; ++l) {
        const size_t in = p.width[l], o = p.width[l + 1];
        p.w_off[l] = (int)off;
        off += in * o;
        p.b_off[l] = (int)off;
        off += o;
        p.ln_off[l] = -1;
        if (ln_hidden && l + 1 < n_linear) {
            p.ln_off[l] = (int)off;
            off += 2 * o;
        }
    }
    MSM_REQUIRE(ctx, n_params == off || n_params == kMlpAnyParams, "%s: %zu parameters given, the widths need %zu", fn,
                n_params, off);
    if (needed) *needed = off;
    int held[2] = {0, 0};   // layer l reads image l & 1 and writes the other
    for (int i = 0; i <= n_linear; ++i) held[i & 1] = std::max(held[i & 1], p.width[i]);
    for (int i = 0; i < 2; ++i) p.stride[i] = ((held[i] + 15) & ~15) + 2;
    *out = p;
    return MSM_OK;
}

// The launch shape of the four per-frame kernels (mlp_forward_kernel, mlp_vjp_kernel, mlp_train_forward_kernel,
// mlp_train_backward_kernel): one wave per workgroup, a group of 16 rows at a time, one round of workgroups.
struct MlpLaunch {
    size_t lds;         // the two LDS images, bytes (<= 66 KiB)
    int per_cu;         // workgroups resident per CU at that LDS size, at least 1
    int grid;           // min(n_groups, n_cu * per_cu)
    int64_t n_groups;   // ceil(rows / 16)
    int64_t trips;      // ceil(n_groups / grid): from 2 on a workgroup reuses its LDS images
};

// The one place that decides it: every launch site calls this, and msm_mlp_launch_plan reports it.  `kernel`: the
// kernel's host address; `rows`: n, or 2m of a training batch.  Above 48 KiB the kernel's dynamic LDS limit is
// raised here, before the occupancy is asked for.
inline msm_status mlp_launch_shape(msm_ctx* ctx, const void* kernel, const MlpPlan& p, int64_t rows, MlpLaunch* out) {
    MlpLaunch s;
    s.lds = (size_t)16 * (p.stride[0] + p.stride[1]) * sizeof(double);
    if (s.lds > 48 * 1024)
        MSM_HIP(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.lds));
    int per_cu = 0;   // one round of workgroups: as many as are resident at once
    MSM_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, s.lds));
    s.per_cu = std::max(per_cu, 1);
    s.n_groups = (rows + 15) / 16;
    s.grid = (int)std::min<int64_t>(s.n_groups, (int64_t)ctx->n_cu * s.per_cu);
    s.trips = s.grid > 0 ? (s.n_groups + s.grid - 1) / s.grid : 0;
    *out = s;
    return MSM_OK;
}

}  // namespace

// The kernels' host addresses, for msm_mlp_launch_plan (mlp_train.hip): mlp.hip, mlp_vjp.hip, mlp_train.hip
const void* mlp_forward_kernel_address(msm_dtype dtype);
const void* mlp_vjp_kernel_address(msm_dtype dtype);
const void* mlp_train_kernel_address(bool backward, msm_dtype dtype);
