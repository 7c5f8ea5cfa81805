// OPES (on-the-fly probability enhanced sampling, Invernizzi & Parrinello, J. Phys. Chem. Lett. 11, 2731 (2020)): the
// replay of a deposit sequence into a journal of compressed-kernel versions, the bias of N frames against that journal
// (value and gradient) and the bias of one frame against the live kernels, which is the MD step.  The contract is in
// include/msmhip.h and DESIGN.md ("OPES"); the tests hold the kernels to tests/_opes_ref.py run in 80-bit floats.
//
// A kernel is a record of 2 d + 1 doubles: centre [d], sigma [d], height.  The deposit kernel is one wave: every lane
// holds the incoming kernel and the scalar state in registers, the live kernels are spread over the lanes (lane l takes
// the slots l, l + 64, ..), and every cross-lane step is a fixed shuffle tree, so the bits depend on the inputs alone.
// All of it is fp64; -ffp-contract=off, so the operation order written here is the order executed.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"
#include "wave.h"

namespace {

constexpr int kT = MSM_METAD_THREADS;
constexpr int kWaves = kT / 64;
constexpr int kTile = MSM_METAD_TILE;
constexpr int kPD = MSM_OPES_PER_DEPOSIT;
static_assert(kT == 256 && kTile <= kT, "one version's life span per thread while a tile is staged, four waves");

struct OpesShape {                        // by value in the kernel arguments
    double period[MSM_METAD_MAX_D];       // 0: the CV is not periodic
    double sigma0[MSM_METAD_MAX_D];
    double kT, kTp, eps, cut2, v, thr2;   // kTp = kT (1 - 1 / gamma); v = exp(-cutoff^2 / 2)
    double v_empty;                       // kTp log(eps), the bias before the first deposit: one number on every path
    int fixed_sigma;
};

// the minimum image of a - b on axis i, as hill_dp2 of metad.hip forms it
__device__ __forceinline__ double min_image(double a, double b, double P) {
    double dp = a - b;
    if (P > 0.0) dp -= P * rint(dp / P);
    return dp;
}

// z_i = dp_i / sigma_i of the point s and the kernel rec; returns q = sum z_i^2 (ascending i)
template <int D>
__device__ __forceinline__ double kernel_q(const double* rec, const double (&s)[D], const OpesShape& sh,
                                           double (&z)[D]) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        z[i] = min_image(s[i], rec[i], sh.period[i]) / rec[D + i];
        q += z[i] * z[i];
    }
    return q;
}

// sum_k G_k(s) over the live slots k < K by one wave: lane l adds the slots l, l + 64, .. in ascending order, then the
// `down` tree; every lane returns lane 0's bits.  With GRAD also the d sums of dG_k / ds_i.
template <int D, bool GRAD>
__device__ __forceinline__ double live_sum(const double* live, int K, const double (&s)[D], const OpesShape& sh,
                                           double (&g)[D]) {
    constexpr int R = 2 * D + 1;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) g[i] = 0.0;
    for (int k = threadIdx.x & 63; k < K; k += 64) {
        const double* rec = live + (size_t)k * R;
        double z[D];
        const double q = kernel_q<D>(rec, s, sh, z);
        if (q < sh.cut2) {
            const double e = exp(-0.5 * q);
            const double h = rec[2 * D];
            acc += h * (e - sh.v);
            if constexpr (GRAD) {
                const double w = -(h * e);
#pragma unroll
                for (int i = 0; i < D; ++i) g[i] += w * (z[i] / rec[D + i]);
            }
        }
    }
    acc = __shfl(wave_sum_down(acc), 0, 64);
    if constexpr (GRAD) {
#pragma unroll
        for (int i = 0; i < D; ++i) g[i] = __shfl(wave_sum_down(g[i]), 0, 64);
    }
    return acc;
}

// V = kT p log(P / Z + eps), P = acc / W; x = P / Z + eps is returned for the gradient
__device__ __forceinline__ double bias_value(double acc, double W, double Z, const OpesShape& sh, double& x) {
    x = (acc / W) / Z + sh.eps;
    return sh.kTp * log(x);
}
__device__ __forceinline__ double bias_slope(double gacc, double W, double Z, double x, const OpesShape& sh) {
    return sh.kTp * (((gacc / W) / Z) / x);
}

// sum over the live slots k < K, k != hole, of G_x(c_k) + G_k(c_x) for the kernel x = (xc, xs, xh): the terms of the
// double sum behind Z that x takes part in.  One minimum image serves both directions.  Order: that of live_sum.
template <int D>
__device__ __forceinline__ double pair_sum(const double* live, int K, int hole, const double (&xc)[D],
                                           const double (&xs)[D], double xh, const OpesShape& sh) {
    constexpr int R = 2 * D + 1;
    double acc = 0.0;
    for (int k = threadIdx.x & 63; k < K; k += 64) {
        if (k == hole) continue;
        const double* rec = live + (size_t)k * R;
        double qx = 0.0, qk = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double dp = min_image(xc[i], rec[i], sh.period[i]);
            const double zx = dp / xs[i], zk = dp / rec[D + i];
            qx += zx * zx;
            qk += zk * zk;
        }
        const double gx = qx < sh.cut2 ? xh * (exp(-0.5 * qx) - sh.v) : 0.0;
        const double gk = qk < sh.cut2 ? rec[2 * D] * (exp(-0.5 * qk) - sh.v) : 0.0;
        acc += gx + gk;
    }
    return __shfl(wave_sum_down(acc), 0, 64);
}

template <int D>
__device__ __forceinline__ void store_kernel(double* dst, const double (&c)[D], const double (&s)[D], double h) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
        dst[i] = c[i];
        dst[D + i] = s[i];
    }
    dst[2 * D] = h;
}

// One wave consumes up to max_steps deposits from the cursor on.  Nothing is written past `capacity` or `n_records`:
// a full ledger, an unusable record and an unusable state set a status bit and end the launch.
template <int D>
__global__ __launch_bounds__(64) void opes_deposit_kernel(OpesShape sh, double* state, double* live,
                                                          int32_t* slot_version, double* journal, int32_t* death,
                                                          double* per_deposit,
                                                          int capacity, double* records, int n_records,
                                                          const double* cv, int64_t ld, int max_steps, int restart) {
    constexpr int R = 2 * D + 1, RR = 2 * D + 2;
    const int lane = threadIdx.x;
    const double count_d = state[MSM_OPES_STATE_COUNT], K_d = state[MSM_OPES_STATE_LIVE];
    const double cursor_d = restart ? 0.0 : state[MSM_OPES_STATE_CURSOR];
    const double status_d = state[MSM_OPES_STATE_STATUS];
    double W = state[MSM_OPES_STATE_W], W2 = state[MSM_OPES_STATE_W2], S = state[MSM_OPES_STATE_SUM];
    double Z = state[MSM_OPES_STATE_Z];
    int status = status_d >= 0.0 && status_d < 256.0 ? (int)status_d : 0;
    if (!(status_d == 0.0)) return;           // a ledger that refused a deposit consumes nothing until it is cleared
    if (!(count_d >= 0.0 && count_d <= (double)capacity && K_d >= 0.0 && K_d <= count_d && cursor_d >= 0.0 &&
          cursor_d <= (double)n_records)) {
        __syncthreads();
        if (lane == 0) state[MSM_OPES_STATE_STATUS] = (double)(status | MSM_OPES_BAD_STATE);
        return;
    }
    int count = (int)count_d, K = (int)K_d, cursor = (int)cursor_d;
    __syncthreads();                          // every lane has read the state before lane 0 writes it

    for (int step = 0; step < max_steps && cursor < n_records; ++step) {
        const int j = count;                  // the version this deposit gives birth to
        if (j >= capacity) {
            status |= MSM_OPES_FULL;
            break;
        }
        double* rec = records + (size_t)cursor * RR;
        double c[D], sg[D], h, lw;
        bool bad = false;
        if (cv) {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                c[i] = cv[(size_t)cursor * ld + i];
                bad |= !(fabs(c[i]) < INFINITY);
                sg[i] = sh.sigma0[i];
            }
            double V = sh.v_empty;
            if (K > 0 && !bad) {
                double g[D], x;
                const double acc = live_sum<D, false>(live, K, c, sh, g);
                V = bias_value(acc, W, Z, sh, x);
            }
            lw = V / sh.kT;
            h = exp(lw);
        } else {
#pragma unroll
            for (int i = 0; i < D; ++i) {
                c[i] = rec[i];
                sg[i] = rec[D + i];
                bad |= !(fabs(c[i]) < INFINITY);
            }
            h = rec[2 * D];
            lw = rec[2 * D + 1];
        }
        const double w = exp(lw);
        const double Wn = W + w, W2n = W2 + w * w;
        const double neff = ((1.0 + Wn) * (1.0 + Wn)) / (1.0 + W2n);
        if (cv && !sh.fixed_sigma) {
            const double f = pow(neff * (double)(D + 2) / 4.0, -1.0 / (double)(D + 4));
#pragma unroll
            for (int i = 0; i < D; ++i) {
                sg[i] = sh.sigma0[i] * f;
                h = h * (sh.sigma0[i] / sg[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < D; ++i) bad |= !(sg[i] > 0.0 && sg[i] < INFINITY);
        bad |= !(h > 0.0 && h < INFINITY) || !(w > 0.0 && w < INFINITY);
        if (bad) {
            status |= MSM_OPES_BAD_RECORD;
            break;
        }
        W = Wn;
        W2 = W2n;
        if (cv && lane == 0) {                // the record of this deposit, as a KERNELS file would hold it
            store_kernel<D>(rec, c, sg, h);
            rec[2 * D + 1] = lw;
        }

        // compression: the incoming kernel merges into its nearest neighbour while that is closer than the threshold
        int home = -1;                        // the slot the merged kernel will take; its stale record is a hole
        const int K0 = K;
        for (int it = 0; it <= K0; ++it) {    // at most one merge per live kernel
            double best = -INFINITY;
            int bi = INT_MAX;
            for (int k = lane; k < K; k += 64) {
                if (k == home) continue;
                double z[D];
                const double q = kernel_q<D>(live + (size_t)k * R, c, sh, z);
                if (-q > best) {
                    best = -q;
                    bi = k;
                }
            }
            wave_argmax_down(best, bi);       // the smallest q, the lowest slot on equal q
            best = __shfl(best, 0, 64);
            bi = __shfl(bi, 0, 64);
            if (bi == INT_MAX || !(-best < sh.thr2)) break;
            const int t = bi;
            const double* tr = live + (size_t)t * R;
            double tc[D], ts[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                tc[i] = tr[i];
                ts[i] = tr[D + i];
            }
            const double th = tr[2 * D];
            // t leaves the double sum: its pairs with every live kernel, itself counted once
            S -= pair_sum<D>(live, K, home, tc, ts, th, sh) - th * (1.0 - sh.v);
            if (lane == 0) death[slot_version[t]] = j;
            const double hm = th + h;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const double dl = min_image(c[i], tc[i], sh.period[i]);
                const double s2 =
                    (th * (ts[i] * ts[i]) + h * (sg[i] * sg[i])) / hm + ((th * h) / (hm * hm)) * (dl * dl);
                c[i] = tc[i] + (h / hm) * dl;
                sg[i] = sqrt(s2);
            }
            h = hm;
            if (home < 0) {
                home = t;
            } else {                          // a chain merge frees the higher slot; the last live slot fills it
                const int freed = max(home, t), last = K - 1;
                home = min(home, t);
                __syncthreads();              // every lane has read slot `freed`
                if (freed != last && lane == 0) {
#pragma unroll
                    for (int i = 0; i < R; ++i) live[(size_t)freed * R + i] = live[(size_t)last * R + i];
                    slot_version[freed] = slot_version[last];
                }
                K -= 1;
                __syncthreads();
            }
        }
        const int slot = home >= 0 ? home : K;
        if (home < 0) K += 1;
        __syncthreads();
        if (lane == 0) {
            store_kernel<D>(live + (size_t)slot * R, c, sg, h);
            store_kernel<D>(journal + (size_t)j * R, c, sg, h);
            slot_version[slot] = j;
            death[j] = INT_MAX;
        }
        __syncthreads();
        S += pair_sum<D>(live, K, -1, c, sg, h, sh) - h * (1.0 - sh.v);
        Z = S / (W * (double)K);
        if (lane == 0) {
            double* out = per_deposit + (size_t)j * kPD;
            out[0] = W;
            out[1] = Z;
            out[2] = neff;
            out[3] = (double)K;
        }
        count += 1;
        cursor += 1;
    }
    if (lane == 0) {
        state[MSM_OPES_STATE_COUNT] = (double)count;
        state[MSM_OPES_STATE_LIVE] = (double)K;
        state[MSM_OPES_STATE_W] = W;
        state[MSM_OPES_STATE_W2] = W2;
        state[MSM_OPES_STATE_SUM] = S;
        state[MSM_OPES_STATE_Z] = Z;
        state[MSM_OPES_STATE_STATUS] = (double)status;
        state[MSM_OPES_STATE_CURSOR] = (double)cursor;
    }
}

// N frames x the journal.  Frame f with count c sees the versions j < c <= death_j and the state after deposit c - 1.
// One frame per lane, the versions staged through LDS in tiles (centre, 1 / sigma, height; the life span death - j
// beside them), a lane adds in ascending version index.  A tile whose versions all died before the smallest count of
// the workgroup is not staged; its versions would have failed every lane's life-span test.
template <int D, bool GRAD>
__global__ __launch_bounds__(kT) void opes_bias_kernel(const double* __restrict__ cv, int64_t n, int64_t ld,
                                                       const double* __restrict__ versions,
                                                       const int32_t* __restrict__ death,
                                                       const double* __restrict__ per_deposit, int T,
                                                       const int32_t* __restrict__ count,
                                                       const double* __restrict__ state, OpesShape sh, int skip,
                                                       double* __restrict__ bias, double* __restrict__ grad,
                                                       int64_t ldg) {
    constexpr int R = 2 * D + 1;
    if (state) {      // never past the deposits the device has made, whatever the caller believes (a refused deposit)
        const double made = state[MSM_OPES_STATE_COUNT];
        T = made >= 0.0 && made < (double)T ? (int)made : T;
    }
    __shared__ double tile[kTile * R];
    __shared__ int span[kTile];
    __shared__ int tile_death[kWaves];
    __shared__ int wg_top, wg_low;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
        if (valid && !bad) cnt = count ? min(max(count[f], 0), T) : T;
        // the workgroup walks the versions any of its frames can see
        if (threadIdx.x == 0) {
            wg_top = 0;
            wg_low = INT_MAX;
        }
        __syncthreads();
        const int wave_top = wave_reduce_xor(cnt, [](int a, int b) { return max(a, b); });
        const int wave_low = wave_reduce_xor(cnt > 0 ? cnt : INT_MAX, [](int a, int b) { return min(a, b); });
        if (lane == 0) {
            atomicMax(&wg_top, wave_top);
            atomicMin(&wg_low, wave_low);
        }
        __syncthreads();
        const int top = wg_top, low = wg_low;

        double v = 0.0;
        double g[D];
#pragma unroll
        for (int i = 0; i < D; ++i) g[i] = 0.0;
        for (int h0 = 0; h0 < top; h0 += kTile) {
            const int m = min(kTile, top - h0);
            __syncthreads();
            const int dv = (int)threadIdx.x < m ? death[h0 + threadIdx.x] : -1;
            if ((int)threadIdx.x < m) span[threadIdx.x] = dv - (h0 + (int)threadIdx.x);
            const int wave_death = wave_reduce_xor(dv, [](int a, int b) { return max(a, b); });
            if (lane == 0) tile_death[wave] = wave_death;
            __syncthreads();
            const int last_death = max(max(tile_death[0], tile_death[1]), max(tile_death[2], tile_death[3]));
            if (skip && last_death < low) continue;      // workgroup-uniform
            const double* __restrict__ src = versions + (size_t)h0 * R;
            for (int i = threadIdx.x; i < m * R; i += kT) {
                const int col = i % R;
                const double x = src[i];
                tile[i] = col >= D && col < 2 * D ? 1.0 / x : x;
            }
            __syncthreads();
            const int mine = min(m, cnt - h0);
            for (int j = 0; j < mine; ++j) {
                if (cnt - 1 - (h0 + j) >= span[j]) continue;      // the version died before this frame
                const double* rec = tile + j * R;
                double z[D];
                double q = 0.0;
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    z[i] = min_image(s[i], rec[i], sh.period[i]) * rec[D + i];
                    q += z[i] * z[i];
                }
                if (q < sh.cut2) {
                    const double e = exp(-0.5 * q);
                    const double h = rec[2 * D];
                    v += h * (e - sh.v);
                    if constexpr (GRAD) {
                        const double w = -(h * e);
#pragma unroll
                        for (int i = 0; i < D; ++i) g[i] += w * (z[i] * rec[D + i]);
                    }
                }
            }
        }
        if (valid) {
            double V = NAN, x = 1.0, W = 1.0, Z = 1.0;
            if (!bad) {
                if (cnt > 0) {
                    W = per_deposit[(size_t)(cnt - 1) * kPD];
                    Z = per_deposit[(size_t)(cnt - 1) * kPD + 1];
                    V = bias_value(v, W, Z, sh, x);
                } else {
                    V = sh.v_empty;
                }
            }
            bias[f] = V;
            if constexpr (GRAD) {
#pragma unroll
                for (int i = 0; i < D; ++i)
                    grad[f * ldg + i] = bad ? NAN : (cnt > 0 ? bias_slope(g[i], W, Z, x, sh) : 0.0);
            }
        }
        __syncthreads();      // wg_top, wg_low and the tile are free for the next trip
    }
}

// Frames against the live kernels, one wave per frame, K, W and Z read from the device state: the MD step (n = 1)
template <int D, bool GRAD>
__global__ __launch_bounds__(64) void opes_live_kernel(const double* __restrict__ cv, int64_t n, int64_t ld,
                                                       const double* __restrict__ live, int capacity,
                                                       const double* __restrict__ state, OpesShape sh,
                                                       double* __restrict__ bias, double* __restrict__ grad,
                                                       int64_t ldg) {
    const double K_d = state[MSM_OPES_STATE_LIVE];
    const double W = state[MSM_OPES_STATE_W], Z = state[MSM_OPES_STATE_Z];
    const bool usable = K_d >= 0.0 && K_d <= (double)capacity;
    const int K = usable ? (int)K_d : 0;
    for (int64_t f = blockIdx.x; f < n; f += gridDim.x) {
        double s[D];
        bool bad = !usable;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            s[i] = cv[f * ld + i];
            bad |= !(fabs(s[i]) < INFINITY);
        }
        double V = NAN, x = 1.0;
        double g[D];
#pragma unroll
        for (int i = 0; i < D; ++i) g[i] = 0.0;
        if (!bad) {                            // wave-uniform
            if (K > 0) {
                const double acc = live_sum<D, GRAD>(live, K, s, sh, g);
                V = bias_value(acc, W, Z, sh, x);
            } else {
                V = sh.v_empty;
            }
        }
        if (threadIdx.x == 0) {
            bias[f] = V;
            if constexpr (GRAD) {
#pragma unroll
                for (int i = 0; i < D; ++i)
                    grad[f * ldg + i] = bad ? NAN : (K > 0 ? bias_slope(g[i], W, Z, x, sh) : 0.0);
            }
        }
    }
}

msm_status opes_shape(msm_ctx* ctx, const char* who, int d, const double* h_par, bool need_sigma0, OpesShape* sh) {
    MSM_REQUIRE(ctx, d >= 1 && d <= MSM_METAD_MAX_D, "%s: %d collective variables, 1 to %d are supported", who, d,
                MSM_METAD_MAX_D);
    MSM_REQUIRE(ctx, h_par != nullptr, "%s: NULL parameters", who);
    const double kT_ = h_par[MSM_OPES_PAR_KT], p = h_par[MSM_OPES_PAR_PREFACTOR], eps = h_par[MSM_OPES_PAR_EPSILON];
    const double cutoff = h_par[MSM_OPES_PAR_CUTOFF], thr = h_par[MSM_OPES_PAR_THRESHOLD];
    MSM_REQUIRE(ctx, kT_ > 0.0 && kT_ < INFINITY, "%s: kT must be positive and finite", who);
    MSM_REQUIRE(ctx, p > 0.0 && p <= 1.0, "%s: the prefactor 1 - 1 / gamma must lie in (0, 1]", who);
    MSM_REQUIRE(ctx, eps > 0.0 && eps < INFINITY, "%s: epsilon must be positive and finite", who);
    MSM_REQUIRE(ctx, cutoff > 0.0 && cutoff < INFINITY, "%s: the cutoff must be positive and finite", who);
    MSM_REQUIRE(ctx, thr >= 0.0 && thr < INFINITY, "%s: the compression threshold must be >= 0 and finite", who);
    for (int i = 0; i < MSM_METAD_MAX_D; ++i) {
        sh->period[i] = 0.0;
        sh->sigma0[i] = 1.0;
    }
    for (int i = 0; i < d; ++i) {
        const double P = h_par[MSM_OPES_PAR_PERIOD + i], s0 = h_par[MSM_OPES_PAR_SIGMA0 + i];
        MSM_REQUIRE(ctx, P >= 0.0 && P < INFINITY, "%s: period %d must be 0 (not periodic) or positive and finite", who,
                    i);
        MSM_REQUIRE(ctx, !need_sigma0 || (s0 > 0.0 && s0 < INFINITY), "%s: sigma0 %d must be positive and finite", who,
                    i);
        sh->period[i] = P;
        if (need_sigma0) sh->sigma0[i] = s0;
    }
    sh->kT = kT_;
    sh->kTp = kT_ * p;
    sh->eps = eps;
    sh->cut2 = cutoff * cutoff;
    sh->v = std::exp(-0.5 * sh->cut2);
    sh->thr2 = thr * thr;
    sh->v_empty = sh->kTp * std::log(eps);
    sh->fixed_sigma = h_par[MSM_OPES_PAR_FIXED_SIGMA] != 0.0;
    return MSM_OK;
}

int opes_bias_grid(const msm_ctx* ctx, int64_t n, int max_workgroups) {
    const int64_t trips = (n + kT - 1) / kT;
    const int64_t cap = max_workgroups > 0 ? max_workgroups : (int64_t)ctx->n_cu * 8;
    return (int)std::max<int64_t>(1, std::min<int64_t>(trips, cap));
}

int opes_live_grid(const msm_ctx* ctx, int64_t n, int max_workgroups) {
    const int64_t cap = max_workgroups > 0 ? max_workgroups : (int64_t)ctx->n_cu * 8;
    return (int)std::max<int64_t>(1, std::min<int64_t>(n, cap));
}

template <int D>
void launch_opes_bias(msm_ctx* ctx, int grid, const double* d_cv, int64_t n, int64_t ld, const double* d_versions,
                      const int32_t* d_death, const double* d_pd, int T, const int32_t* d_count,
                      const double* d_state, const OpesShape& sh, int skip, double* d_bias, double* d_grad, int64_t ldg) {
    if (d_grad)
        hipLaunchKernelGGL((opes_bias_kernel<D, true>), dim3(grid), dim3(kT), 0, ctx->stream, d_cv, n, ld, d_versions,
                           d_death, d_pd, T, d_count, d_state, sh, skip, d_bias, d_grad, ldg);
    else
        hipLaunchKernelGGL((opes_bias_kernel<D, false>), dim3(grid), dim3(kT), 0, ctx->stream, d_cv, n, ld, d_versions,
                           d_death, d_pd, T, d_count, d_state, sh, skip, d_bias, d_grad, ldg);
}

template <int D>
void launch_opes_live(msm_ctx* ctx, int grid, const double* d_cv, int64_t n, int64_t ld, const double* d_live,
                      int capacity, const double* d_state, const OpesShape& sh, double* d_bias, double* d_grad,
                      int64_t ldg) {
    if (d_grad)
        hipLaunchKernelGGL((opes_live_kernel<D, true>), dim3(grid), dim3(64), 0, ctx->stream, d_cv, n, ld, d_live,
                           capacity, d_state, sh, d_bias, d_grad, ldg);
    else
        hipLaunchKernelGGL((opes_live_kernel<D, false>), dim3(grid), dim3(64), 0, ctx->stream, d_cv, n, ld, d_live,
                           capacity, d_state, sh, d_bias, d_grad, ldg);
}

}  // namespace

extern "C" {

msm_status msm_opes_plan(msm_ctx* ctx, int64_t n, int T, int d, int max_workgroups, int64_t out[6]) {
    if (!ctx) return MSM_ERR_INVALID;
    MSM_REQUIRE(ctx, out != nullptr, "msm_opes_plan: NULL pointer");
    MSM_REQUIRE(ctx, n >= 1 && T >= 0 && d >= 1 && d <= MSM_METAD_MAX_D && max_workgroups >= 0,
                "msm_opes_plan: need n >= 1, T >= 0, 1 <= d <= %d, max_workgroups >= 0 (0: the default)",
                MSM_METAD_MAX_D);
    out[0] = kT;
    out[1] = kTile;
    out[2] = opes_bias_grid(ctx, n, max_workgroups);
    out[3] = (int64_t)(kTile * (2 * d + 1) * sizeof(double) + (kTile + kWaves + 2) * sizeof(int));
    out[4] = 64;
    out[5] = opes_live_grid(ctx, n, max_workgroups);
    return MSM_OK;
}

msm_status msm_opes_deposit(msm_ctx* ctx, int d, const double* h_par, double* d_state, double* d_live,
                            int32_t* d_slot_version, double* d_journal, int32_t* d_death, double* d_per_deposit,
                            int capacity, double* d_records, int n_records, const double* d_cv, int64_t ld,
                            int max_steps, int restart) {
    if (!ctx) return MSM_ERR_INVALID;
    OpesShape sh;
    const msm_status rs = opes_shape(ctx, "msm_opes_deposit", d, h_par, d_cv != nullptr, &sh);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, capacity >= 1 && n_records >= 0 && max_steps >= 1 && (!d_cv || ld >= d),
                "msm_opes_deposit: need capacity >= 1, n_records >= 0, max_steps >= 1, ld >= d (capacity=%d "
                "n_records=%d max_steps=%d)", capacity, n_records, max_steps);
    MSM_REQUIRE(ctx, d_state && d_live && d_slot_version && d_journal && d_death && d_per_deposit &&
                         (d_records || n_records == 0),
                "msm_opes_deposit: NULL pointer");
    if (n_records == 0) return MSM_OK;
    switch (d) {
#define MSM_OPES_CASE(D)                                                                                           \
    case D:                                                                                                        \
        hipLaunchKernelGGL(opes_deposit_kernel<D>, dim3(1), dim3(64), 0, ctx->stream, sh, d_state, d_live,         \
                           d_slot_version, d_journal, d_death, d_per_deposit, capacity, d_records, n_records,      \
                           d_cv, ld, max_steps, restart);                                                          \
        break;
        MSM_OPES_CASE(1) MSM_OPES_CASE(2) MSM_OPES_CASE(3) MSM_OPES_CASE(4)
        MSM_OPES_CASE(5) MSM_OPES_CASE(6) MSM_OPES_CASE(7) MSM_OPES_CASE(8)
#undef MSM_OPES_CASE
    }
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

msm_status msm_opes_bias(msm_ctx* ctx, const double* d_cv, int64_t n, int64_t ld, int d, const double* h_par,
                         const double* d_kernels, const int32_t* d_death, const double* d_per_deposit, int T,
                         const int32_t* d_count, const double* d_state, int flags, int max_workgroups, double* d_bias,
                         double* d_grad, int64_t ldg) {
    if (!ctx) return MSM_ERR_INVALID;
    OpesShape sh;
    const msm_status rs = opes_shape(ctx, "msm_opes_bias", d, h_par, false, &sh);
    if (rs != MSM_OK) return rs;
    MSM_REQUIRE(ctx, n >= 1 && ld >= d && T >= 0 && max_workgroups >= 0 && (!d_grad || ldg >= d) &&
                         (flags & ~MSM_OPES_NO_SKIP) == 0,
                "msm_opes_bias: need n >= 1, ld >= d, T >= 0, max_workgroups >= 0, ldg >= d, known flags (n=%lld "
                "ld=%lld T=%d)", (long long)n, (long long)ld, T);
    MSM_REQUIRE(ctx, d_cv && d_bias, "msm_opes_bias: NULL pointer");
    const bool live = d_death == nullptr;
    if (live) {
        MSM_REQUIRE(ctx, d_kernels && d_state && !d_count && T >= 1,
                    "msm_opes_bias: the live form needs the live kernels, their capacity, the state and no counts");
    } else {
        MSM_REQUIRE(ctx, (d_kernels && d_per_deposit) || T == 0, "msm_opes_bias: NULL pointer");
    }
    const int grid = live ? opes_live_grid(ctx, n, max_workgroups) : opes_bias_grid(ctx, n, max_workgroups);
    const int skip = (flags & MSM_OPES_NO_SKIP) ? 0 : 1;
    switch (d) {
#define MSM_OPES_CASE(D)                                                                                           \
    case D:                                                                                                        \
        if (live)                                                                                                  \
            launch_opes_live<D>(ctx, grid, d_cv, n, ld, d_kernels, T, d_state, sh, d_bias, d_grad, ldg);           \
        else                                                                                                       \
            launch_opes_bias<D>(ctx, grid, d_cv, n, ld, d_kernels, d_death, d_per_deposit, T, d_count, d_state,    \
                                sh, skip, d_bias, d_grad, ldg);                                                    \
        break;
        MSM_OPES_CASE(1) MSM_OPES_CASE(2) MSM_OPES_CASE(3) MSM_OPES_CASE(4)
        MSM_OPES_CASE(5) MSM_OPES_CASE(6) MSM_OPES_CASE(7) MSM_OPES_CASE(8)
#undef MSM_OPES_CASE
    }
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // extern "C"
