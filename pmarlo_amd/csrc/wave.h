// Cross-lane and workgroup reductions shared by every kernel of libmsmhip.so, and two workgroup idioms more than one
// file uses (rank_order, mfma_tile_acc).  Device-only; include after common.h.
//
// What all of it rests on:
//   * a wave is 64 lanes (gfx9); "lane" is threadIdx.x & 63, "wave" is threadIdx.x >> 6, and every lane of the wave
//     is active at the call (a shuffle that reads an inactive lane returns garbage);
//   * the build has -ffp-contract=off and no fast-math, so the combining order written here is the order executed:
//     results are fixed bit for bit by (offset sequence, operand order `op(mine, theirs)`);
//   * for a sum, lane 0 of the `down` tree and lane 0 of the `xor` butterfly hold the same bits; no other lane does;
//   * fmax / fmin ignore a NaN operand and canonicalise; the bare v_max_f64 family (hw_*) does neither (never-NaN operands);
//   * v_permlane16_swap / v_permlane32_swap exist on gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// Combiners, called as op(mine, theirs).
struct op_sum {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct op_max {   // fmax: a NaN operand is ignored
    __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};
struct op_min {   // fmin: a NaN operand is ignored
    __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
};

// The bare v_max_f64 / v_min_f64 / v_max_f32: one instruction, no canonicalising v_max x, x in front (fmax() adds one
// per operand that the compiler cannot prove canonical).  A NaN operand loses; the operands are never NaN at the sites.
//   hw_*      plain asm: the compiler may move, merge or drop it (the tridiagonal solver and the filter's running
//             maxima want it scheduled freely).
//   hw_*_pin  asm volatile: stays where it is written relative to other volatile asm.  The k-means kernels read MFMA
//             results with it and pad the MFMA -> VALU hazard by hand, which only holds if it does not move.
__device__ __forceinline__ double hw_max_f64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double hw_min_f64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float hw_max_f32(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double hw_max_f64_pin(double a, double b) {
    double r;
    asm volatile("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// Shuffle reductions (ds_bpermute: six dependent trips through the LDS crossbar, any type __shfl takes).
// Result in lane 0 only (other lanes hold partial garbage); offsets 32, 16, .., 1; v = op(v, lane + off's v).
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce_down(T v, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_down(v, off, 64));
    return v;
}
// Result in every lane; offsets 32, 16, .., 1; v = op(v, lane ^ off's v).  For a sum the lanes agree only up to
// rounding order (lane 0 matches wave_reduce_down bit for bit); for max / min they agree exactly.
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce_xor(T v, Op op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    return v;
}
// Named forms: double, int, unsigned, (unsigned) long long for the sums; double (fmax / fmin) for max / min.
template <typename T> __device__ __forceinline__ T wave_sum_down(T v) { return wave_reduce_down(v, op_sum{}); }
template <typename T> __device__ __forceinline__ T wave_sum_xor(T v) { return wave_reduce_xor(v, op_sum{}); }
template <typename T> __device__ __forceinline__ T wave_max_down(T v) { return wave_reduce_down(v, op_max{}); }
template <typename T> __device__ __forceinline__ T wave_min_down(T v) { return wave_reduce_down(v, op_min{}); }
template <typename T> __device__ __forceinline__ T wave_max_xor(T v) { return wave_reduce_xor(v, op_max{}); }

// Independent reductions in one loop: the shuffles of a step are issued together, so k values cost about one
// reduction's latency, not k (the compiler does not always interleave separate calls).  Per value the arithmetic is
// exactly that of the single form.
template <typename... T>
__device__ __forceinline__ void wave_sum_down_each(T&... v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ((v += __shfl_down(v, off, 64)), ...);
}
__device__ __forceinline__ void wave_minmax_xor(double& mn, double& mx) {   // fmin / fmax, every lane
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { mn = fmin(mn, __shfl_xor(mn, off, 64)); mx = fmax(mx, __shfl_xor(mx, off, 64)); }
}

// Arg-max of (value, index) pairs: the larger value wins, the lower index on equal values; a NaN value never wins.
// `down`: offsets 32 .. 1, lane 0.  `xor`: offsets 1 .. 32, every lane; `carry` travels with the winner.
__device__ __forceinline__ void wave_argmax_down(double& best, int& bi) {
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(best, off, 64);
        const int oi = __shfl_down(bi, off, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
}
__device__ __forceinline__ void wave_argmax_xor(double& best, int& bi, double& carry) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double ob = __shfl_xor(best, off, 64), oc = __shfl_xor(carry, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; carry = oc; }
    }
}

// Workgroup reductions.  `red` is LDS, one slot per wave (blockDim.x / 64, a multiple of 64 threads); every thread
// of the workgroup calls.  The wave results (wave_reduce_down) are combined by thread 0 in ascending wave order
// starting from the identity, so the result depends on blockDim.x but never on timing.
// Total in thread 0 only (0.0 elsewhere).  Two barriers; `red` may be reused after the next barrier of the caller.
__device__ __forceinline__ double block_sum_lane0(double v, double* red) {
    v = wave_sum_down(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    return t;
}
// Result in every thread, through the LDS word `bc`.  Three barriers.
template <typename Op>
__device__ __forceinline__ double block_reduce_bcast(double v, double* red, double* bc, double identity, Op op) {
    v = wave_reduce_down(v, op);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = identity;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t = op(t, red[i]);
        *bc = t;
    }
    __syncthreads();
    return *bc;
}
__device__ __forceinline__ double block_sum_bcast(double v, double* red, double* bc) {
    return block_reduce_bcast(v, red, bc, 0.0, op_sum{});
}
__device__ __forceinline__ double block_max_bcast(double v, double* red, double* bc) {
    return block_reduce_bcast(v, red, bc, -INFINITY, op_max{});
}

// Rank by counting: order[r] = the index whose key(i) is the r-th largest (descending) or smallest, equal keys in
// index order (stable).  Index i is ranked by thread i, i + blockDim.x, ...: the result is a function of the keys
// alone.  No barrier: the caller synchronises before `order` is read.
template <bool descending, typename Key>
__device__ __forceinline__ void rank_order(int n, int* order, Key key) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double a = key(i);
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double b = key(j);
            rank += (descending ? b > a : b < a) || (b == a && j < i);
        }
        order[rank] = i;
    }
}
// The same with equal keys ordered by tie(i) in the same direction first, then by index.
template <bool descending, typename Key, typename Tie>
__device__ __forceinline__ void rank_order(int n, int* order, Key key, Tie tie) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double a = key(i), ta = tie(i);
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double b = key(j), tb = tie(j);
            rank += (descending ? b > a : b < a) ||
                    (b == a && ((descending ? tb > ta : tb < ta) || (tb == ta && j < i)));
        }
        order[rank] = i;
    }
}

// VALU-only reductions: DPP moves inside the rows of 16 lanes, then the two row swaps of gfx950.  No LDS crossbar:
// a step is one v_mov_dpp (two for a 64-bit payload) plus the combiner.  Every lane ends with the result; for a sum
// all lanes hold the same bits (both partners of a step add the same two values).  T has 4 or 8 bytes.
typedef unsigned wave_v2u32 __attribute__((ext_vector_type(2)));
// lane i gets x of the lane that DPP control CTRL names (always a valid lane for the controls used here, so the
// result does not depend on bound_ctrl).  BC is bound_ctrl all the same: with BC = false the compiler first writes
// the `old` value 0 to the destination, one v_mov_b32 per move, and the k-means filter was tuned with those in place.
template <int CTRL, bool BC = true, typename T>
__device__ __forceinline__ T mov_dpp(T x) {
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, BC));
    } else {
        const long long b = __builtin_bit_cast(long long, x);
        const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xF, 0xF, BC);
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xF, 0xF, BC);
        return __builtin_bit_cast(T, ((long long)hi << 32) | (unsigned)lo);
    }
}

// over aligned groups of 8 lanes: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror; x = op(x, partner's x)
template <bool BC = true, typename T, typename Op>
__device__ __forceinline__ T row8_reduce(T x, Op op) {
    x = op(x, mov_dpp<0xB1, BC>(x));
    x = op(x, mov_dpp<0x4E, BC>(x));
    x = op(x, mov_dpp<0x141, BC>(x));
    return x;
}
// over each row of 16 lanes: row8_reduce, then row_mirror
template <bool BC = true, typename T, typename Op>
__device__ __forceinline__ T row_reduce(T x, Op op) {
    x = row8_reduce<BC>(x, op);
    return op(x, mov_dpp<0x140, BC>(x));
}
// over the 4 lanes (j, j + 16, j + 32, j + 48): v_permlane16_swap, then v_permlane32_swap; x = op(kept, swapped)
template <int STEP>
__device__ __forceinline__ wave_v2u32 row_swap(unsigned u) {
    if constexpr (STEP == 0) return __builtin_amdgcn_permlane16_swap(u, u, false, false);
    else return __builtin_amdgcn_permlane32_swap(u, u, false, false);
}
template <int STEP, typename T, typename Op>
__device__ __forceinline__ T xrow_step(T x, Op op) {
    if constexpr (sizeof(T) == 4) {
        const wave_v2u32 r = row_swap<STEP>(__builtin_bit_cast(unsigned, x));
        return op(__builtin_bit_cast(T, (unsigned)r[0]), __builtin_bit_cast(T, (unsigned)r[1]));
    } else {
        const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
        const wave_v2u32 rl = row_swap<STEP>((unsigned)b), rh = row_swap<STEP>((unsigned)(b >> 32));
        return op(__builtin_bit_cast(T, ((unsigned long long)rh[0] << 32) | rl[0]),
                  __builtin_bit_cast(T, ((unsigned long long)rh[1] << 32) | rl[1]));
    }
}
template <typename T, typename Op>
__device__ __forceinline__ T xrow_reduce(T x, Op op) { return xrow_step<1>(xrow_step<0>(x, op), op); }
// whole wave, result in every lane
template <bool BC = true, typename T, typename Op>
__device__ __forceinline__ T wave_reduce_valu(T x, Op op) { return xrow_reduce(row_reduce<BC>(x, op), op); }

__device__ __forceinline__ double wave_sum_all(double x) { return wave_reduce_valu(x, op_sum{}); }
// the k-means filter's forms (BC = false, see mov_dpp); operands never NaN (hw_max_f32 / hw_max_f64_pin)
__device__ __forceinline__ int min_i32(int a, int b) { return min(a, b); }
__device__ __forceinline__ float xrow_max_f32(float x) { return xrow_reduce(x, hw_max_f32); }
__device__ __forceinline__ float wave_max_f32(float x) { return wave_reduce_valu<false>(x, hw_max_f32); }
__device__ __forceinline__ double wave_max_f64(double x) { return wave_reduce_valu<false>(x, hw_max_f64_pin); }
__device__ __forceinline__ int xrow_min_i32(int x) { return xrow_reduce(x, min_i32); }
__device__ __forceinline__ int wave_min_i32(int x) { return wave_reduce_valu<false>(x, min_i32); }

// Lane `lane`'s 64-bit value to every lane: two v_readlane_b32 (the value lands in SGPRs); `lane` is wave-uniform.
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

typedef double v4f64 __attribute__((ext_vector_type(4)));   // accumulator of v_mfma_f64_16x16x4_f64

// One 16 x 16 tile of C = opA opB on the fp64 matrix cores by one wave: lane (j, g) = (lane & 15, lane >> 4) supplies
// a(k) = opA(i0 + j, k) and b(k) = opB(k, c0 + j), k < inner, through loadA(k) / loadB(k), which read clamped
// (in-range) addresses; aok / bok say whether the lane's row of opA / column of opB lies inside the matrix, and what
// lies outside is fed as zero.  acc[r] ends up as entry (i0 + g + 4 r, c0 + j) of the tile.
template <typename LoadA, typename LoadB>
__device__ __forceinline__ v4f64 mfma_tile_acc(int inner, int g, bool aok, bool bok, LoadA loadA, LoadB loadB) {
    v4f64 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < inner; k0 += 16) {   // four instructions per trip: their operand reads go out together
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool kok = k0 + 4 * u + g < inner;
            const int k = kok ? k0 + 4 * u + g : 0;
            a[u] = loadA(k);
            b[u] = loadB(k);
            if (!(aok && kok)) a[u] = 0.0;
            if (!(bok && kok)) b[u] = 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    return acc;
}
