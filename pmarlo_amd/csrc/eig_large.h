// Device-wide symmetric eigensolver for orders 256 < n <= 2048 (block Jacobi) and the TICA / one-sided solves built on
// it.  Part of eig.hip's translation unit (included after its anonymous namespace: it reuses jacobi_eigh, pivot_pair,
// rank_order and mfma_tile_acc); nothing at or below order 256 comes through here.
//
// Method.  The matrix is cut into blocks of width b = 32 (zero-padded to nb = ceil(n / 32) whole blocks).  One sweep
// is a round-robin tournament over block pairs (pivot_pair on block indices: nb - 1 rounds of nb / 2 disjoint pairs,
// one block sitting out when nb is odd).  A round is three plain launches on the context's stream:
//   (1) bj_pivot_kernel: one workgroup per pair gathers its 64 x 64 pivot submatrix into the LDS, diagonalises it
//       with jacobi_eigh (order 64: the pipelined variant), tightens Q's orthogonality by one Newton-Schulz step and
//       leaves Q (64 x 64) and the 64 new diagonal entries diag(Q'SQ) in global memory;
//   (2) bj_apply_right_kernel: A <- A Q on the pair's two block columns, V <- V Q;
//   (3) bj_apply_left_kernel:  A <- Q' A on the pair's two block rows; the pivot blocks themselves are written as
//       diag(new diagonal) and exact zeros (the scalar code annihilates its pivot exactly, rotate_block).
// (2) and (3) are (n x 64)(64 x 64) products on v_mfma_f64_16x16x4_f64, one workgroup per (pair, 32 rows or columns).
// The two triangles of A then agree to rounding only ((Q'A)Q against Q'(AQ)); the pivot gather reads one of them.
// Stream order is the only synchronisation: no barrier across workgroups, no atomics.  Convergence is a device flag:
// ahead of every sweep bj_offnorm_kernel / bj_converge_kernel evaluate jacobi_converged's test (||off||_F <= n eps
// ||A||_F) with a fixed summation order and either set ctl[0] or count the sweep in ctl[1].  The host enqueues the
// schedule of all kBjSweeps = 40 sweeps; every kernel reads the flag first and returns when it is set.
//
// Padding.  Padded rows and columns of A are exact zeros.  jacobi_rotation skips a pivot with apq == 0, so Q has unit
// rows and columns there, the products reproduce the zeros exactly and padding never couples to the matrix; it is
// dropped by index at the end.  The second eigensolve of the TICA solve works the same way on the leading rank x rank
// part (the rank is read from device memory; block pairs entirely past it are skipped).
#pragma once

namespace {

constexpr int kBjB = 32;              // block width
constexpr int kBjP = 2 * kBjB;        // order of a pivot problem
constexpr int kBjLd = kBjP + 1;       // its LDS row stride
constexpr int kBjMaxOrder = 2048;
constexpr int kBjSweeps = 40;         // the cap every caller of jacobi_eigh passes
constexpr int kBjQld = 80;            // LDS row stride of Q in the apply kernels (lane groups 32 banks apart)
constexpr int kBjPld = 66;            // ... of the row panel of bj_apply_right_kernel
constexpr int kBjApplyThreads = 128;  // two waves: 32 rows (right) or 32 columns (left) per workgroup
constexpr int kBjCtlDone = 0, kBjCtlSweeps = 1, kBjCtlRank = 2;

// Pair i of round `round` over nb blocks; false when the pair has nothing to do: one side is the padding player of
// an odd block count, or both blocks lie past the active order.
__device__ __forceinline__ bool bj_pair(int round, int i, int nb, int active, int& p, int& q) {
    pivot_pair(round, i, nb + (nb & 1), p, q);
    return q < nb && (p < q ? p : q) * kBjB < active;
}
// global index of local index k of the pair: 0..31 -> block p, 32..63 -> block q
__device__ __forceinline__ int bj_global(int p, int q, int k) { return (k < kBjB ? p : q) * kBjB + (k & (kBjB - 1)); }

// ctl: done = 0, sweeps = 0; V = I (when given)
__global__ void bj_init_kernel(int* ctl, double* V, int npad) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e == 0) { ctl[kBjCtlDone] = 0; ctl[kBjCtlSweeps] = 0; }
    if (V && e < (size_t)npad * npad) V[e] = (e / npad == e % npad) ? 1.0 : 0.0;
}

// partial sums of the convergence test over the rows of one block: part[2 blk] = off^2, part[2 blk + 1] = diag^2
__global__ __launch_bounds__(256) void bj_offnorm_kernel(const double* __restrict__ A, int npad, int n,
                                                         const int* __restrict__ ctl, double* __restrict__ part) {
    __shared__ double red[4];
    if (ctl[kBjCtlDone]) return;
    const int r0 = blockIdx.x * kBjB;
    double off = 0.0, dia = 0.0;
    for (int e = threadIdx.x; e < kBjB * npad; e += blockDim.x) {
        const int r = r0 + e / npad, c = e % npad;
        if (r < n && c < n) {
            const double v = A[(size_t)r * npad + c];
            if (r == c) dia = fma(v, v, dia); else off = fma(v, v, off);
        }
    }
    off = block_sum_lane0(off, red);
    dia = block_sum_lane0(dia, red);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = off; part[2 * blockIdx.x + 1] = dia; }
}

// the test of jacobi_converged on the partial sums, in block order: sets the flag or counts the sweep about to run
__global__ void bj_converge_kernel(const double* __restrict__ part, int nb, int n, const int* __restrict__ d_active,
                                   int* ctl) {
    if (threadIdx.x != 0 || ctl[kBjCtlDone]) return;
    double off = 0.0, dia = 0.0;
    for (int b = 0; b < nb; ++b) { off += part[2 * b]; dia += part[2 * b + 1]; }
    const int active = d_active ? *d_active : n;
    const double tol = (double)active * 2.220446049250313e-16;
    if (off <= tol * tol * (dia + off) || off == 0.0) ctl[kBjCtlDone] = 1;
    else ctl[kBjCtlSweeps] += 1;
}

// launch 1 of a round: Q and the new diagonal of every pair
__global__ __launch_bounds__(kEigThreads) void bj_pivot_kernel(const double* __restrict__ A, int npad, int nb, int n,
                                                              int round, const int* __restrict__ ctl,
                                                              const int* __restrict__ d_active,
                                                              double* __restrict__ Qg, double* __restrict__ dnew) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ JacobiShared sh;
    if (ctl[kBjCtlDone]) return;
    int p, q;
    if (!bj_pair(round, blockIdx.x, nb, d_active ? *d_active : n, p, q)) return;
    const int tid = threadIdx.x, nt = blockDim.x;
    double* S = reinterpret_cast<double*>(smem_raw);
    double* Q = S + kBjP * kBjLd;
    double* W = Q + kBjP * kBjLd;
    // one triangle of the pivot submatrix, mirrored: S is symmetric bit for bit
    auto gather = [&]() {
        for (int e = tid; e < kBjP * kBjP; e += nt) {
            const int i = e / kBjP, j = e - i * kBjP;
            const int lo = i < j ? i : j, hi = i < j ? j : i;
            S[i * kBjLd + j] = A[(size_t)bj_global(p, q, lo) * npad + bj_global(p, q, hi)];
        }
        __syncthreads();
    };
    gather();
    jacobi_eigh(S, Q, kBjP, kBjLd, &sh, kBjSweeps);
    __syncthreads();
    // One Newton-Schulz step, W = Q (3 I - Q'Q) / 2: the few 1e-15 by which the product of a solve's rotations misses
    // orthogonality add up over the hundreds of pivot problems a column passes through; squared, they do not.  Unit
    // rows and columns of Q (padding, skipped pivots) give unit rows and columns of W exactly.
    mfma_mm<true, false>(S, Q, Q, kBjP, kBjP, kBjP, kBjLd);
    for (int e = tid; e < kBjP * kBjP; e += nt) {
        const int i = e / kBjP, j = e - i * kBjP;
        S[i * kBjLd + j] = 0.5 * ((i == j ? 3.0 : 0.0) - S[i * kBjLd + j]);
    }
    __syncthreads();
    mfma_mm<false, false>(W, Q, S, kBjP, kBjP, kBjP, kBjLd);
    // the new diagonal that goes with W: diag(W' S0 W), S0 gathered again (A does not change during this launch)
    gather();
    mfma_mm<false, false>(Q, S, W, kBjP, kBjP, kBjP, kBjLd);
    double* Qo = Qg + (size_t)blockIdx.x * kBjP * kBjP;
    for (int e = tid; e < kBjP * kBjP; e += nt) Qo[e] = W[(e / kBjP) * kBjLd + (e % kBjP)];
    if (tid < kBjP) {
        double d = 0.0;
        for (int k = 0; k < kBjP; ++k) d = fma(W[k * kBjLd + tid], Q[k * kBjLd + tid], d);
        dnew[blockIdx.x * kBjP + tid] = d;
    }
}

__device__ __forceinline__ void bj_load_q(double* Qs, const double* __restrict__ Qg, int pair) {
    const double* src = Qg + (size_t)pair * kBjP * kBjP;
    for (int e = threadIdx.x; e < kBjP * kBjP; e += blockDim.x) Qs[(e / kBjP) * kBjQld + (e % kBjP)] = src[e];
}

// launch 2: M <- M Q on the two block columns of the pair, M = A (blockIdx.z == 0) or V.  A workgroup owns 32 rows:
// it stages its 32 x 64 panel in the LDS, then writes the same entries, so the update is in place.
__global__ __launch_bounds__(kBjApplyThreads) void bj_apply_right_kernel(double* A, double* V, int npad, int nb, int n,
                                                                        int round, const int* __restrict__ ctl,
                                                                        const int* __restrict__ d_active,
                                                                        const double* __restrict__ Qg) {
    __shared__ double Qs[kBjP * kBjQld];
    __shared__ double Ps[kBjB * kBjPld];
    if (ctl[kBjCtlDone]) return;
    int p, q;
    if (!bj_pair(round, blockIdx.y, nb, d_active ? *d_active : n, p, q)) return;
    double* M = blockIdx.z ? V : A;
    const int r0 = blockIdx.x * kBjB;
    bj_load_q(Qs, Qg, blockIdx.y);
    for (int e = threadIdx.x; e < kBjB * kBjP; e += blockDim.x) {
        const int r = e / kBjP, k = e - r * kBjP;
        Ps[r * kBjPld + k] = M[(size_t)(r0 + r) * npad + bj_global(p, q, k)];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, rw = (threadIdx.x >> 6) * 16;
    const int j = lane & 15, g = lane >> 4;
    double a[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) a[u] = Ps[(rw + j) * kBjPld + 4 * u + g];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int c0 = 16 * t;
        v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 16; ++u)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], Qs[(4 * u + g) * kBjQld + c0 + j], acc, 0, 0, 0);
        const int col = bj_global(p, q, c0 + j);
#pragma unroll
        for (int r = 0; r < 4; ++r) M[(size_t)(r0 + rw + g + 4 * r) * npad + col] = acc[r];
    }
}

// launch 3: A <- Q' A on the two block rows of the pair.  A wave owns 16 columns: it reads its 64 x 16 panel into
// registers before the first store, so the update is in place.  Inside the pivot blocks the result is known: the new
// diagonal and exact zeros.
__global__ __launch_bounds__(kBjApplyThreads) void bj_apply_left_kernel(double* A, int npad, int nb, int n, int round,
                                                                       const int* __restrict__ ctl,
                                                                       const int* __restrict__ d_active,
                                                                       const double* __restrict__ Qg,
                                                                       const double* __restrict__ dnew) {
    __shared__ double Qs[kBjP * kBjQld];
    if (ctl[kBjCtlDone]) return;
    int p, q;
    if (!bj_pair(round, blockIdx.y, nb, d_active ? *d_active : n, p, q)) return;
    bj_load_q(Qs, Qg, blockIdx.y);
    __syncthreads();
    const int lane = threadIdx.x & 63, c0 = blockIdx.x * kBjB + (threadIdx.x >> 6) * 16;
    const int j = lane & 15, g = lane >> 4;
    double b[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) b[u] = A[(size_t)bj_global(p, q, 4 * u + g) * npad + c0 + j];
    const int cb = c0 / kBjB;
    const bool pivot = cb == p || cb == q;
    const int lc = (cb == p ? 0 : kBjB) + ((c0 + j) & (kBjB - 1));   // local column inside the pivot blocks
    const double* dn = dnew + blockIdx.y * kBjP;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i0 = 16 * t;
        v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < 16; ++u)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Qs[(4 * u + g) * kBjQld + i0 + j], b[u], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lr = i0 + g + 4 * r;
            const double v = pivot ? (lr == lc ? dn[lr] : 0.0) : acc[r];
            A[(size_t)bj_global(p, q, lr) * npad + c0 + j] = v;
        }
    }
}

// C = opA opB, all three npad x npad with row stride npad (npad a multiple of 32: no ragged tiles), one 16 x 16 tile
// per wave, 2 x 2 tiles per workgroup.  C must not alias A or B.
template <bool TA, bool TB>
__global__ __launch_bounds__(256) void bj_gemm_kernel(double* __restrict__ C, const double* __restrict__ A,
                                                      const double* __restrict__ B, int npad) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int i0 = blockIdx.y * 32 + (wave >> 1) * 16, c0 = blockIdx.x * 32 + (wave & 1) * 16;
    const size_t ai = i0 + j, bj = c0 + j, ld = npad;
    const v4f64 acc = mfma_tile_acc(
        npad, g, true, true, [&](int k) { return TA ? A[k * ld + ai] : A[ai * ld + k]; },
        [&](int k) { return TB ? B[bj * ld + k] : B[k * ld + bj]; });
#pragma unroll
    for (int r = 0; r < 4; ++r) C[(size_t)(i0 + g + 4 * r) * ld + c0 + j] = acc[r];
}

// dst = (src + src') / 2 over the padded matrix
__global__ void bj_sym_kernel(const double* __restrict__ src, double* __restrict__ dst, int npad) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)npad * npad) return;
    const size_t i = e / npad, j = e % npad;
    dst[e] = 0.5 * (src[e] + src[j * npad + i]);
}

// Sign of the largest-magnitude entry (first occurrence) of a strided column of n entries, the rule of
// canonical_signs; every thread of the workgroup (256 threads) calls and gets the result.
__device__ __forceinline__ double bj_column_sign(const double* __restrict__ col, size_t stride, int n, double* sbest,
                                                 double* sval, int* sidx) {
    double best = -1.0, val = 0.0;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double v = col[i * stride];
        if (fabs(v) > best) { best = fabs(v); bi = i; val = v; }
    }
    wave_argmax_xor(best, bi, val);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sbest[threadIdx.x >> 6] = best; sval[threadIdx.x >> 6] = val; sidx[threadIdx.x >> 6] = bi; }
    __syncthreads();
    best = sbest[0]; val = sval[0]; bi = sidx[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
        if (sbest[w] > best || (sbest[w] == best && sidx[w] < bi)) { best = sbest[w]; val = sval[w]; bi = sidx[w]; }
    return val < 0.0 ? -1.0 : 1.0;
}

// ---- msm_eigh -----------------------------------------------------------------------------------------------------
// A = symmetric part of the input, zero-padded
__global__ void bj_load_sym_kernel(const double* __restrict__ Ain, int n, double* __restrict__ A, int npad) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)npad * npad) return;
    const size_t i = e / npad, j = e % npad;
    A[e] = (i < (size_t)n && j < (size_t)n) ? 0.5 * (Ain[i * n + j] + Ain[j * n + i]) : 0.0;
}

// One workgroup: the diagonal of A ranked ascending (descending: by value, or by magnitude with by_abs) over the first
// `count` indices; order[] and the sorted values out.  T (optional): the pair count of a moments block, T <= 0 gives
// zeros.  sweeps_out (optional) <- ctl[sweeps].
template <bool descending, bool by_abs>
__global__ __launch_bounds__(kEigThreads) void bj_sort_kernel(const double* __restrict__ A, int npad, int n,
                                                             const int* __restrict__ d_count, int* __restrict__ order,
                                                             double* __restrict__ ev, double* __restrict__ out_sorted,
                                                             const int* __restrict__ ctl, int* __restrict__ sweeps_out,
                                                             const double* __restrict__ T) {
    __shared__ double key[kBjMaxOrder];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int count = d_count ? *d_count : n;
    for (int i = tid; i < n; i += nt) {
        const double v = i < count ? A[(size_t)i * npad + i] : 0.0;
        key[i] = v;
        if (ev) ev[i] = v;
        order[i] = i;   // a NaN key ranks nowhere: no slot is left unwritten
    }
    __syncthreads();
    rank_order<descending>(count, order, [&](int i) { return by_abs ? fabs(key[i]) : key[i]; });
    __syncthreads();
    if (out_sorted) {
        const bool zero = T && !(*T > 0.0);
        for (int j = tid; j < n; j += nt) out_sorted[j] = zero ? 0.0 : key[order[j]];
    }
    if (tid == 0 && sweeps_out) *sweeps_out = ctl[kBjCtlSweeps];
}

// out[i][j] = V[i][order[j]], n x n packed
__global__ void bj_gather_cols_kernel(const double* __restrict__ V, int npad, int n, const int* __restrict__ order,
                                      double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)n * n) return;
    const size_t i = e / n, j = e % n;
    out[e] = V[i * npad + order[j]];
}

// ---- msm_tica_solve -----------------------------------------------------------------------------------------------
// C00 -> A, C0t -> B1 (both zero-padded), the means out: tica_solve_kernel's build_cov.  T <= 0: zeros.
__global__ void bjt_cov_kernel(const double* __restrict__ mom, const double* __restrict__ scale, int n, int npad,
                               double* __restrict__ A, double* __restrict__ B1, double* __restrict__ out_mean) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)npad * npad) return;
    const size_t i = e / npad, j = e % npad, nn = n;
    const double* M00 = mom;
    const double* M0t = mom + nn * nn;
    const double* sx = M0t + nn * nn;
    const double* sy = sx + nn;
    const double T = sy[nn];
    double c00 = 0.0, c0t = 0.0;
    if (i < nn && j < nn) {
        const bool live = T > 0.0;
        const double w = 2.0 * T;
        const double isi = scale ? 1.0 / scale[i] : 1.0, isj = scale ? 1.0 / scale[j] : 1.0;
        const double mi = live ? (sx[i] + sy[i]) / w * isi : 0.0, mj = live ? (sx[j] + sy[j]) / w * isj : 0.0;
        if (live) {
            const double ss = isi * isj, mm = mi * mj;
            c00 = 0.5 * (M00[i * nn + j] + M00[j * nn + i]) / w * ss - mm;
            c0t = (M0t[i * nn + j] + M0t[j * nn + i]) / w * ss - mm;
        }
        if (j == 0) out_mean[i] = mi;
    }
    A[e] = c00;
    B1[e] = c0t;
}

// spd_inv_split's cut on the eigenvalues of C00 (the diagonal of A): order by |s| descending, epsilon raised to
// -s_min + 1e-16 when C00 has a negative eigenvalue, rank = #{|s| >= epsilon}; T <= 0 gives rank 0.
__global__ __launch_bounds__(kEigThreads) void bjt_rank_kernel(const double* __restrict__ A, int npad, int n,
                                                              const double* __restrict__ T, double epsilon,
                                                              double* __restrict__ ev, int* __restrict__ order,
                                                              int* ctl, int* __restrict__ out_rank) {
    __shared__ double key[kBjMaxOrder];
    __shared__ double red[kEigThreads / 64], bc[2];
    const int tid = threadIdx.x, nt = blockDim.x;
    double mn = INFINITY;
    for (int i = tid; i < n; i += nt) {
        const double v = A[(size_t)i * npad + i];
        key[i] = v;
        ev[i] = v;
        order[i] = i;
        mn = fmin(mn, v);
    }
    __syncthreads();
    rank_order<true>(n, order, [&](int i) { return fabs(key[i]); });
    const double evmin = block_reduce_bcast(mn, red, &bc[0], INFINITY, op_min{});
    double eps = epsilon;
    if (evmin < 0.0) eps = fmax(eps, -evmin + 1e-16);
    double cnt = 0.0;
    for (int i = tid; i < n; i += nt) cnt += fabs(key[i]) >= eps ? 1.0 : 0.0;
    cnt = block_sum_bcast(cnt, red, &bc[1]);   // a count: exact
    if (tid == 0) {
        const int rank = *T > 0.0 ? (int)cnt : 0;
        ctl[kBjCtlRank] = rank;
        *out_rank = rank;
    }
}

// Column j of L = V[:, order[j]] with its canonical sign, over sqrt(s); columns from the rank on and the padding
// are zero.  One workgroup (256 threads) per column.
__global__ __launch_bounds__(256) void bjt_whiten_kernel(const double* __restrict__ V, int npad, int n,
                                                         const double* __restrict__ ev, const int* __restrict__ order,
                                                         const int* __restrict__ ctl, double* __restrict__ L) {
    __shared__ double sbest[4], sval[4];
    __shared__ int sidx[4];
    const int j = blockIdx.x, rank = ctl[kBjCtlRank];
    if (j >= rank) {
        for (int i = threadIdx.x; i < npad; i += blockDim.x) L[(size_t)i * npad + j] = 0.0;
        return;
    }
    const int c = order[j];
    const double sgn = bj_column_sign(V + c, npad, n, sbest, sval, sidx);
    const double root = sqrt(ev[c]);
    for (int i = threadIdx.x; i < npad; i += blockDim.x)
        L[(size_t)i * npad + j] = i < n ? (V[(size_t)i * npad + c] * sgn) / root : 0.0;
}

// Output column j: solver column order2[j] of R = L Rt with its canonical sign and the kinetic-map factor; zeros
// from keep = min(n_lead, rank) on.  One workgroup (256 threads) per column.
__global__ __launch_bounds__(256) void bjt_finish_kernel(const double* __restrict__ R, int npad, int n,
                                                         const double* __restrict__ ev2,
                                                         const int* __restrict__ order2, const int* __restrict__ ctl,
                                                         int kinetic_map, int n_lead, double* __restrict__ out_eig,
                                                         double* __restrict__ out_W) {
    __shared__ double sbest[4], sval[4];
    __shared__ int sidx[4];
    const int j = blockIdx.x, rank = ctl[kBjCtlRank];
    const int keep = n_lead > 0 && n_lead < rank ? n_lead : rank;
    if (j >= keep) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) out_W[(size_t)i * n + j] = 0.0;
        if (threadIdx.x == 0) out_eig[j] = 0.0;
        return;
    }
    const int c = order2[j];
    const double sgn = bj_column_sign(R + c, npad, n, sbest, sval, sidx);
    const double lam = ev2[c];
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        double v = R[(size_t)i * npad + c] * sgn;
        if (kinetic_map) v *= lam;
        out_W[(size_t)i * n + j] = v;
    }
    if (threadIdx.x == 0) out_eig[j] = lam;
}

// ---- msm_onesided_tica_eigenvalues --------------------------------------------------------------------------------
// C0 -> A, Ct -> B1 (zero-padded): the head of onesided_eig_kernel.  T <= 0: zeros.
__global__ void bjo_cov_kernel(const double* __restrict__ mom, int n, int npad, double* __restrict__ A,
                               double* __restrict__ B1) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)npad * npad) return;
    const size_t i = e / npad, j = e % npad, nn = n;
    const double* M00 = mom;
    const double* M0t = mom + nn * nn;
    const double* sx = M0t + nn * nn;
    const double* sy = sx + nn;
    const double T = sy[nn];
    double c0 = 0.0, ct = 0.0;
    if (i < nn && j < nn && T > 0.0) {
        const double den = T - 1.0 > 1.0 ? T - 1.0 : 1.0;
        c0 = (0.5 * (M00[i * nn + j] + M00[j * nn + i]) - sx[i] * sx[j] / T) / den;
        ct = (M0t[i * nn + j] - sx[i] * sy[j] / T) / den;
    }
    A[e] = c0;
    B1[e] = ct;
}

// P = V diag(w^-1/4), w = the diagonal of A clipped at `clip` (S = P P'); zero-padded
__global__ void bjo_scale_kernel(const double* __restrict__ V, const double* __restrict__ A, int n, int npad,
                                 double clip, double* __restrict__ P) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)npad * npad) return;
    const size_t i = e / npad, j = e % npad;
    double v = 0.0;
    if (i < (size_t)n && j < (size_t)n) {
        const double w = A[j * npad + j];
        v = V[e] / sqrt(sqrt(w > clip ? w : clip));
    }
    P[e] = v;
}

// ---- host side ----------------------------------------------------------------------------------------------------
struct BjWork {
    int n, nb, npad, m;
    double* mat[5];            // npad x npad each; mat[0] = A, mat[1] = V
    double *Q, *dnew, *part, *ev, *ev2;
    int *order, *order2, *ctl;
};

size_t bj_scratch_bytes(int n, int nmats) {
    const size_t nb = (n + kBjB - 1) / kBjB, npad = nb * kBjB, m = (nb + 1) / 2;
    return (nmats * npad * npad + m * kBjP * kBjP + m * kBjP + 2 * nb + 2 * npad) * sizeof(double) +
           (2 * npad + 8) * sizeof(int) + 64;
}

BjWork bj_layout(void* scratch, int n, int nmats) {
    BjWork wk;
    wk.n = n; wk.nb = (n + kBjB - 1) / kBjB; wk.npad = wk.nb * kBjB; wk.m = (wk.nb + 1) / 2;
    double* base = (double*)scratch;
    const size_t mat = (size_t)wk.npad * wk.npad;
    for (int i = 0; i < 5; ++i) wk.mat[i] = i < nmats ? base + i * mat : nullptr;
    wk.Q = base + nmats * mat;
    wk.dnew = wk.Q + (size_t)wk.m * kBjP * kBjP;
    wk.part = wk.dnew + (size_t)wk.m * kBjP;
    wk.ev = wk.part + 2 * wk.nb;
    wk.ev2 = wk.ev + wk.npad;
    wk.order = (int*)(wk.ev2 + wk.npad);
    wk.order2 = wk.order + wk.npad;
    wk.ctl = wk.order2 + wk.npad;
    return wk;
}

inline unsigned bj_grid(size_t items, int threads) { return (unsigned)((items + threads - 1) / threads); }

// Eigenpairs of the symmetric matrix in mat[0] (zero-padded): the diagonal of mat[0] and, with want_v, the columns of
// mat[1], in solver order; ctl[sweeps] = sweeps taken.  d_active (device, optional): the order of the leading part
// that is not padding.  Enqueues the whole fixed schedule; returns without waiting.
msm_status bj_solve(msm_ctx* ctx, const BjWork& wk, bool want_v, const int* d_active) {
    const size_t lds = 3 * (size_t)kBjP * kBjLd * sizeof(double);   // S, Q and the Newton-Schulz work matrix
    MSM_HIP(ctx, hipFuncSetAttribute((const void*)bj_pivot_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    double *A = wk.mat[0], *V = want_v ? wk.mat[1] : nullptr;
    const size_t elems = (size_t)wk.npad * wk.npad;
    hipLaunchKernelGGL(bj_init_kernel, dim3(want_v ? bj_grid(elems, 256) : 1), dim3(256), 0, ctx->stream, wk.ctl, V, wk.npad);
    const int rounds = wk.nb + (wk.nb & 1) - 1;
    const dim3 right(wk.npad / kBjB, wk.m, want_v ? 2 : 1), left(wk.npad / kBjB, wk.m);
    for (int sweep = 0; sweep < kBjSweeps; ++sweep) {
        hipLaunchKernelGGL(bj_offnorm_kernel, dim3(wk.nb), dim3(256), 0, ctx->stream, A, wk.npad, wk.n, wk.ctl, wk.part);
        hipLaunchKernelGGL(bj_converge_kernel, dim3(1), dim3(64), 0, ctx->stream, wk.part, wk.nb, wk.n, d_active, wk.ctl);
        for (int round = 0; round < rounds; ++round) {
            hipLaunchKernelGGL(bj_pivot_kernel, dim3(wk.m), dim3(kEigThreads), lds, ctx->stream, A, wk.npad, wk.nb, wk.n,
                               round, wk.ctl, d_active, wk.Q, wk.dnew);
            hipLaunchKernelGGL(bj_apply_right_kernel, right, dim3(kBjApplyThreads), 0, ctx->stream, A, V, wk.npad, wk.nb,
                               wk.n, round, wk.ctl, d_active, wk.Q);
            hipLaunchKernelGGL(bj_apply_left_kernel, left, dim3(kBjApplyThreads), 0, ctx->stream, A, wk.npad, wk.nb,
                               wk.n, round, wk.ctl, d_active, wk.Q, wk.dnew);
        }
        MSM_CHECK_LAUNCH(ctx);
    }
    return MSM_OK;
}

template <bool TA, bool TB>
void bj_gemm(msm_ctx* ctx, const BjWork& wk, double* C, const double* A, const double* B) {
    hipLaunchKernelGGL((bj_gemm_kernel<TA, TB>), dim3(wk.npad / 32, wk.npad / 32), dim3(256), 0, ctx->stream, C, A, B, wk.npad);
}

msm_status bj_eigh(msm_ctx* ctx, const double* d_a, int n, double* d_w, double* d_v, int* d_sweeps) {
    msm_status rs = msm_reserve_scratch(ctx, bj_scratch_bytes(n, 2));
    if (rs != MSM_OK) return rs;
    const BjWork wk = bj_layout(ctx->scratch, n, 2);
    const size_t elems = (size_t)wk.npad * wk.npad;
    hipLaunchKernelGGL(bj_load_sym_kernel, dim3(bj_grid(elems, 256)), dim3(256), 0, ctx->stream, d_a, n, wk.mat[0], wk.npad);
    rs = bj_solve(ctx, wk, d_v != nullptr, nullptr);
    if (rs != MSM_OK) return rs;
    hipLaunchKernelGGL((bj_sort_kernel<false, false>), dim3(1), dim3(kEigThreads), 0, ctx->stream, wk.mat[0], wk.npad, n,
                       (const int*)nullptr, wk.order, (double*)nullptr, d_w, wk.ctl, d_sweeps, (const double*)nullptr);
    if (d_v)
        hipLaunchKernelGGL(bj_gather_cols_kernel, dim3(bj_grid((size_t)n * n, 256)), dim3(256), 0, ctx->stream, wk.mat[1],
                           wk.npad, n, wk.order, d_v);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

// The steps of tica_solve_kernel's eigen path (spd_inv_split, whitened eigenproblem, generic tail), one or more
// launches each; the rank stays on the device (ctl[rank]) and every grid is sized for F.
msm_status bj_tica_solve(msm_ctx* ctx, const double* d_moments, const double* d_scale, int F, double epsilon,
                         int kinetic_map, double* d_eigvals, double* d_coeffs, double* d_mean, int* d_rank, int n_lead) {
    msm_status rs = msm_reserve_scratch(ctx, bj_scratch_bytes(F, 5));
    if (rs != MSM_OK) return rs;
    const BjWork wk = bj_layout(ctx->scratch, F, 5);
    double *A = wk.mat[0], *V = wk.mat[1], *B1 = wk.mat[2], *L = wk.mat[3], *B3 = wk.mat[4];
    const size_t elems = (size_t)wk.npad * wk.npad;
    const double* d_T = d_moments + 2 * (size_t)F * F + 2 * F;
    const int* d_active = wk.ctl + kBjCtlRank;
    hipLaunchKernelGGL(bjt_cov_kernel, dim3(bj_grid(elems, 256)), dim3(256), 0, ctx->stream, d_moments, d_scale, F, wk.npad,
                       A, B1, d_mean);
    rs = bj_solve(ctx, wk, true, nullptr);   // C00 = V S V'
    if (rs != MSM_OK) return rs;
    hipLaunchKernelGGL(bjt_rank_kernel, dim3(1), dim3(kEigThreads), 0, ctx->stream, A, wk.npad, F, d_T, epsilon, wk.ev,
                       wk.order, wk.ctl, d_rank);
    hipLaunchKernelGGL(bjt_whiten_kernel, dim3(wk.npad), dim3(256), 0, ctx->stream, V, wk.npad, F, wk.ev, wk.order, wk.ctl, L);
    bj_gemm<false, false>(ctx, wk, B3, B1, L);   // C0t L
    bj_gemm<true, false>(ctx, wk, V, L, B3);     // L' C0t L
    hipLaunchKernelGGL(bj_sym_kernel, dim3(bj_grid(elems, 256)), dim3(256), 0, ctx->stream, V, A, wk.npad);
    MSM_CHECK_LAUNCH(ctx);
    rs = bj_solve(ctx, wk, true, d_active);
    if (rs != MSM_OK) return rs;
    hipLaunchKernelGGL((bj_sort_kernel<true, true>), dim3(1), dim3(kEigThreads), 0, ctx->stream, A, wk.npad, F, d_active,
                       wk.order2, wk.ev2, (double*)nullptr, wk.ctl, (int*)nullptr, (const double*)nullptr);
    bj_gemm<false, false>(ctx, wk, B1, L, V);    // R = L Rt, columns in solver order
    hipLaunchKernelGGL(bjt_finish_kernel, dim3(F), dim3(256), 0, ctx->stream, B1, wk.npad, F, wk.ev2, wk.order2, wk.ctl,
                       kinetic_map, n_lead, d_eigvals, d_coeffs);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

// onesided_eig_kernel's two eigensolves and three products on the device-wide parts
msm_status bj_onesided(msm_ctx* ctx, const double* d_moments, int F, double clip, double* d_eigvals) {
    msm_status rs = msm_reserve_scratch(ctx, bj_scratch_bytes(F, 5));
    if (rs != MSM_OK) return rs;
    const BjWork wk = bj_layout(ctx->scratch, F, 5);
    double *A = wk.mat[0], *V = wk.mat[1], *Ct = wk.mat[2], *P = wk.mat[3], *S = wk.mat[4];
    const size_t elems = (size_t)wk.npad * wk.npad;
    const dim3 eg(bj_grid(elems, 256));
    const double* d_T = d_moments + 2 * (size_t)F * F + 2 * F;
    hipLaunchKernelGGL(bjo_cov_kernel, eg, dim3(256), 0, ctx->stream, d_moments, F, wk.npad, A, Ct);
    rs = bj_solve(ctx, wk, true, nullptr);
    if (rs != MSM_OK) return rs;
    hipLaunchKernelGGL(bjo_scale_kernel, eg, dim3(256), 0, ctx->stream, V, A, F, wk.npad, clip, P);
    bj_gemm<false, true>(ctx, wk, S, P, P);     // S = P P'
    bj_gemm<false, false>(ctx, wk, V, S, Ct);   // S Ct
    bj_gemm<false, false>(ctx, wk, P, V, S);    // (S Ct) S'   (S is symmetric)
    hipLaunchKernelGGL(bj_sym_kernel, eg, dim3(256), 0, ctx->stream, P, A, wk.npad);
    MSM_CHECK_LAUNCH(ctx);
    rs = bj_solve(ctx, wk, false, nullptr);
    if (rs != MSM_OK) return rs;
    hipLaunchKernelGGL((bj_sort_kernel<true, false>), dim3(1), dim3(kEigThreads), 0, ctx->stream, A, wk.npad, F,
                       (const int*)nullptr, wk.order, (double*)nullptr, d_eigvals, wk.ctl, (int*)nullptr, d_T);
    MSM_CHECK_LAUNCH(ctx);
    return MSM_OK;
}

}  // namespace
