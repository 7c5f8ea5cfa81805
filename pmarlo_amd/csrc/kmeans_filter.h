// Certified fp16 matrix-core FILTER + certified fp32 candidate pick for the k-means score table (d <= 10).
// Included by kmeans.hip inside its anonymous namespace (uses FitState, to_fixed, load_as_f64).
//
// The label of a frame is the arg-max over the k centres of the PINNED fp64 score
//     m_j = fl(dot_j - h_j),  dot_j = ascending-feature fma chain of c_j[f] * z[f],  h_j = |c_j|^2 / 2
// (strict '>' over ascending j; kmeans.hip states why this is sklearn's arg-min).  An all-fp64 scan costs
// three v_mfma_f64_16x16x4 (64 cycles each) per 16 centres x 16 frames.  This kernel gets the same labels,
// bit for bit, from ONE v_mfma_f32_16x16x32_f16 (16 cycles) per 16 centres x 16 frames:
//
// 1. FILTER.  Frames are scaled by 2^e_x (one power of two per shard), centres by 2^e_c (one per launch), so that
//    every scaled coordinate v' has |v'| < 2^13 (Scales, below).  v' is split into two fp16 numbers,
//    v' = vh + vl + r with |r| <= 2^-22 |v'| (a part that would be subnormal is left out: Range).  One instruction
//    (31 of its 32 product slots, filter_slot) evaluates, per centre and frame,
//        u'_j = sum_f (ch xh + ch xl + cl xh)  +  C_j  +  kappa |c'_j| |x'|,   C_j >= -(1 - kappa) h'_j
//    with h'_j = 2^(e_x + e_c) h_j and C_j the fp32 C operand, rounded up: the scaled score plus
//    kappa (|x'||c'_j| + h'_j) >= kappa S'_j, S'_j = sum_f |x'_f c'_jf| + h'_j.  u_j = 2^-(e_x + e_c) u'_j is an
//    UPPER BOUND of the pinned score m_j (the scales are powers of two: every relative bound carries over exactly):
//      dropped split terms   <= 12.01 x 2^-24 S_j  (cl xl, and the residuals r of both sides)
//      accumulation          <= 34.3 x 2^-24 S_j: the instruction sums its 32 products and C with an error of at
//                               most 33 x 2^-24 of the largest term, in any slot order, plus the final rounding
//                               (measured on MI355X, tests/test_gpu_mfma_rule_f16.py: worst observed 8.5 x 2^-24
//                               of the largest term; a term of 2^-24 of the largest vanishes; the last bits depend
//                               on the slot order; fp16 subnormal inputs are kept, not flushed -- the filter never
//                               hands one over, so it does not depend on that)
//      fp64 chain of m_j     <= 12 x 2^-53 S_j, fp64 rounding of (1 - kappa) h_j <= 2^-53 h_j
//    and kappa = 52 x 2^-24 covers their sum with 5.6 x 2^-24 S_j to spare.  The C operand and both factors of the
//    kappa slot are rounded up, which only raises u.  (The bf16 form this replaces split every coordinate three ways:
//    6 d + 4 slots, two instructions per tile at d > 4, an 80-byte frame image and kappa = 80 x 2^-24.)
// 2. Per lane (4 accumulator rows of a frame) only the largest PAIR maximum of u, the runner-up pair maximum and
//    the pair index are tracked (max3 tree, med3, max, compare, select: 8 VALU per 8 scores).
// 3. CANDIDATE PICK.  The 8 centres of the winning lane's winning pair are scored in fp32 from an fp32 copy of the
//    centre table (s_j: the same chain in fp32, unscaled; |s_j - exact_j| <= 14.1 x 2^-24 S_j, and
//    S_j <= |z||c_j| + h_j), E = 20 x 2^-24 max_j (max(|z|, 1) |c_j| + h_j) + 1e-30.  With jw = arg-max s_j and
//    R = the largest u outside the 8 (runner-up pair of the winning lane, best pairs of the frame's other three lanes,
//    brought back to unscaled units): if s_jw - E exceeds every other s_j + E AND R, then m_jw > m_j for every other
//    centre: the label is jw, exactly as the all-fp64 scan gives it, and no fp64 arithmetic was needed.  (The pinned
//    distance, when asked for, is the fp64 chain of that one centre.)
// 4. Otherwise (about 0.2 % of the frames: near-ties, duplicate centres, NaN / out-of-range input) the wave scores ALL
//    centres for that frame in fp32 from the same LDS table, lane l rows l, l + 64, ...: no centre with
//    s_j < max s - 2 E can hold the pinned maximum, so when one centre is left it is the label; else the pinned fp64
//    scores of the few rows in that band decide (lowest index on ties, as the all-fp64 scan).  Only frames or tables
//    that fail the range guard take the plain scan of all centres in fp64 (rows from global memory).
//
// Scales.  e_x puts a bound on max |x| of the shard into [2^12, 2^13): msm_kmeans_pack_bounded takes the bound from
// the caller (the bench chain hands over max |Y| of the projection, slot 2 of the fit state), msm_kmeans_pack finds
// it with a pass of its own (filter_absmax_kernel, coordinates that pass the unscaled guard only); e_x travels in the
// word after the image rows.  e_c does the same for max |c| of the centre table, per launch and workgroup.  A frame
// is only ever compared across centres, so shards need no common e_x.
// Range: scaled parts below 2^-14 (fp16 subnormal) are LEFT OUT of the operands and the bound pays for them: a frame
// adds twice what it left out (a whole |v'| or a residual |v' - vh|, each < 2^-14), divided by kappa, to its |x'|
// slot; a centre adds twice its left-out sum to its kappa |c'_j| slot -- either covers the dropped products with
// room for the accumulation error of the slot itself.  Both slots are at least 2^-14.  Frames or centres with
// |v| > 1e18, |v'| > 2^14, inf or NaN fail the guard: the frame (for a centre: every frame) takes step 4; so does
// every frame when a centre's |C| would exceed 2^100.
// Row sums.  The kappa slot of a centre holds any fp16 number >= kappa |c'_j| + 2 tiny_j, tiny_j the sum of what the
// split left out of the row: step 1 asks for nothing more, so neither sum needs a fixed order.  The four lanes
// (j, j + 16, j + 32, j + 48) of a row add |c'_jf|^2 and the left-out parts over features q, q + 4, q + 8 each and
// combine them with the row swaps (filter_stage_build).  Every term is non-negative, so an fp64 sum of the ten in ANY
// order is within 10 x 2^-53 relative of the exact sum; the square root, the product with kappa and the final sum add
// a few 2^-53 more; the factor 1 + 2^-20 (kUp20d) in front of the round-up to fp16 covers all of it a hundred million
// times over.  The order may therefore move the last bit of the slot (up or down one fp16 step on a row that sits within
// 2^-20 of a step; the labels cannot change, only which frames near a tie take step 4).  What carries the bits of a
// label or a distance keeps its order: h_j (the serial chain over ascending features, in lane j), C, the fp32 table,
// the operand images.
//
// Schedule.  One workgroup of kFilterWaves waves per CU builds the centre tables in its LDS and then takes units of
// 64 frames: tile loop (matrix pipe + top-two bookkeeping), the loads of the next unit's images and of this unit's
// coordinates, the cross-lane step, the candidate pick, the commit, step 4 for what is left.  The d <= 10 accumulate
// passes keep a frame's fp64 coordinates only until their fp32 copy for the pick is made: a certified frame that moves
// its member sums (every frame in the first pass, under 10 % after two) reads its row again, L2-warm, all loads ahead
// of the first atomic; step 4 reads the row of its frame wave-uniformly, next to the fp64 rows of the two best centres.
// That takes the fp64 no-whitening build from 132 VGPRs to 122: 16 waves without scratch memory (filter_waves); the first
// unit's images travel across the staging of the tables, which holds 24 registers (filter_stage_fetch).  (Step 4 as a scan of all
// centres in fp64, rows from global memory, cost 25-30 us per pass for 0.2 % of the frames, in place or queued for the
// end of the workgroup's units alike: ~10 us of a wave per frame, and the slowest workgroup has 20 of them.  Scoring
// the eight candidates in fp64 before step 4, one lane and one row at a time, halves the frames that reach step 4 and
// still loses 6 us per pass: eight dependent trips to the L2 per occurrence.)  What the SIMD can do (tools/probe/bf16_mix_probe.hip): a matrix instruction keeps the
// matrix pipe for 16 cycles and the VALU port for 8, a VALU instruction the port for 4; the bf16 tile loop (16 + 34 per
// iteration) was balanced between the two; with one instruction per tile the VALU port bounds it.  Tried and dropped: scoring the candidates of unit i - 1 inside the tile
// loop of unit i (same time: the port is the limit either way, and the state costs 12 of 16 waves).
#pragma once
#include "f16_split.h"

typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v4f32 __attribute__((ext_vector_type(4)));

// waves per workgroup (= per CU): one instruction per tile and one 16-byte B operand per frame group keep the assign
// passes within the 128 VGPRs of 16 waves.  The d <= 10 accumulate passes drop the ten fp64 coordinates once the fp32
// copy for the candidate pick is made and read the row again for the frames that move their member sums (kReloadZ in
// the kernel): on fp64 frames without whitening (`plain`: the bench step) that fits 16 waves too, 122 VGPRs; on fp32
// frames or with whitening the 16-wave build still spills 24-60 bytes per lane, so those run 12 waves (a kernel with
// ANY scratch memory ran 25 us longer per pass)
#ifdef MSM_KMF_WAVES
__host__ __device__ constexpr int filter_waves(int, bool, bool) { return MSM_KMF_WAVES; }
#else
__host__ __device__ constexpr int filter_waves(int dp, bool heavy, bool plain) { return dp == 10 && heavy && !plain ? 12 : 16; }
#endif
constexpr int kFilterMaxD = 10;
constexpr int kFilterCloseCH = 5;                                // prologue close: k d <= 5 x 1024 elements in one round of loads
constexpr int kFilterRowQ = 3;                                   // uint4 per frame image (48 bytes)
constexpr double kFilterHi = 1e18;                               // unscaled range guard (the fp32 pick)
constexpr double kFilterScaledHi = 16384.0;                      // 2^14: scaled range guard (fp16 operands)
constexpr int kFilterScaleTop = 13;                              // a scale puts the largest |v| into [2^12, 2^13)
constexpr double kFilterKappa = 52.0 * 5.9604644775390625e-08;   // 52 x 2^-24
constexpr float kPickEps = 20.0f * 5.9604644775390625e-08f;      // 20 x 2^-24
constexpr float kPickFloor = 1e-30f;
constexpr float kUp20 = 1.0f + 9.5367431640625e-07f;             // 1 + 2^-20
constexpr double kUp20d = 1.0 + 9.5367431640625e-07;

// the exponent e of a power-of-two scale 2^e that puts amax into [2^12, 2^13) (0 for a zero or non-finite bound;
// clamped to +-60 so that 2^-(e_x + e_c) stays a normal fp32 number)
__host__ __device__ inline int filter_scale_exp(double amax) {
    if (!(amax > 0.0) || !(amax <= 1.7976931348623157e308)) return 0;
    const int q = ilogb(amax) + 1;   // amax = m 2^q, m in [0.5, 1) (frexp's out-parameter costs scratch memory)
    const int e = kFilterScaleTop - q;
    return e < -60 ? -60 : (e > 60 ? 60 : e);
}

// f16_round, f16_ceil, f16_bits, f16_split2 (the two-term fp16 split of a scaled coordinate, with what it leaves out
// added to `tiny`), f32_up and kF16MinNormal: f16_split.h, integer arithmetic on the bit pattern of the double

// K slot of product term t (0 = ch xh, 1 = ch xl, 2 = cl xh), feature f.  Quarter q of the instruction (slots
// 8 q .. 8 q + 7) reads piece filter_piece(q) of the 48-byte frame image
//     [xh0..7 | xl0..7 | xh8 xh9 xl8 xl9 xh8 xh9 0 |x|]
// so that quarters 0 and 2 share piece 0: q0 = ch xh, q1 = ch xl, q2 = cl xh (features 0..7), q3 = features 8, 9 of
// the three terms, an empty slot and kappa |c_j| against |x| (slot 31).  -(1 - kappa) h_j is the C operand.
__host__ __device__ constexpr int filter_slot(int t, int f) { return f < 8 ? 8 * t + f : 24 + 2 * t + (f - 8); }
constexpr int kFilterSlotNorm = 31;
__device__ __forceinline__ int filter_piece(int q) { return q == 3 ? 2 : (q & 1); }

// max3 / med3 are written with compiler-visible builtins (hipcc then pads the MFMA -> VALU read hazard itself;
// it does not inside inline asm).  fmaxf(fmaxf(a, b), c) becomes ONE v_max3_f32 with no canonicalising v_max x, x
// when `a` is already the result of a VALU maximum, which is why the pair maximum below starts from b2.
__device__ __forceinline__ float max3_f32(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
__device__ __forceinline__ float med3_f32(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }
// hw_max_f32 (wave.h) where a maximum is loop-carried: fmaxf() costs an extra canonicalising v_max per call, and
// med3(a, b, +inf) is folded back into it

// ---------------------------------------------------------------------------------------------------------
// Frame images: row t = the B operands of frame t (3 uint4, layout as filter_slot) in scaled units x' = 2^e_x x; the
// |x| slot is rounded up (it meets kappa |c_j|) and is +inf when the frame fails the range guard.  The image holds
// whole units of 64 rows and then one uint4 [max |x| bound (f64) | e_x (i32) | pad]: e_x follows from the bound
// `absmax` (>= max |x| over the shard, whitened when mean / stdv are given), one scale per shard.  One thread per frame.
// ---------------------------------------------------------------------------------------------------------
// Both sides of the kernel go through the LDS so that the memory system only ever sees consecutive lanes on
// consecutive 16-byte pieces: a lane reading its own 8 D-byte row or writing its own image row touched 64
// cache lines per instruction.  `dense`: rows back to back (ld == D) on a 16-byte boundary.
template <typename T, int D>
__global__ __launch_bounds__(256) void kmeans_pack_kernel(const T* __restrict__ x, int64_t n, int64_t ld,
                                                         const double* __restrict__ mean,
                                                         const double* __restrict__ stdv, const double* absmax,
                                                         uint4* __restrict__ image, int dense) {
    constexpr int RQ = kFilterRowQ;
    constexpr int kOutStride = RQ;                      // uint4 per staged image row (odd: bank spread)
    constexpr int kInBytes = 256 * D * (int)sizeof(T);  // a workgroup's rows, back to back
    constexpr int kOutBytes = 256 * kOutStride * 16;
    __shared__ __attribute__((aligned(16))) unsigned char stage[kOutBytes > kInBytes ? kOutBytes : kInBytes];
    const int64_t t0 = (int64_t)blockIdx.x * 256;
    const int64_t t = t0 + threadIdx.x;
    const int rows = (int)(n - t0 < 256 ? n - t0 : 256);
    // the image is padded to whole units of 64 rows: rows beyond n are written as frames that fail the range guard
    const int64_t n_pad = (n + 63) & ~(int64_t)63;
    const int rows_out = (int)(n_pad - t0 < 256 ? n_pad - t0 : 256);
    const int ex = filter_scale_exp(*absmax);
    if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<int*>(image + n_pad * RQ)[2] = ex;
    double v[D];
    if (dense) {
        // rows * D * sizeof(T) bytes from x + t0 * D, 16 bytes per lane and trip (the tail of the last workgroup by element)
        const unsigned char* src = reinterpret_cast<const unsigned char*>(x + t0 * D);
        const int nbytes = rows * D * (int)sizeof(T);
        for (int b = threadIdx.x * 16; b + 16 <= nbytes; b += 256 * 16)
            *reinterpret_cast<uint4*>(stage + b) = *reinterpret_cast<const uint4*>(src + b);
        if (threadIdx.x < (nbytes & 15) / (int)sizeof(T)) {
            const int e = (nbytes & ~15) / (int)sizeof(T) + threadIdx.x;
            reinterpret_cast<T*>(stage)[e] = reinterpret_cast<const T*>(src)[e];
        }
        __syncthreads();
        const T* row = reinterpret_cast<const T*>(stage) + threadIdx.x * D;
#pragma unroll
        for (int f = 0; f < D; ++f) v[f] = threadIdx.x < rows ? (double)row[f] : 0.0;
        __syncthreads();   // the staging area is reused for the images
    } else {
        const T* row = x + (t < n ? t : n - 1) * ld;
#pragma unroll
        for (int f = 0; f < D; ++f) v[f] = load_as_f64(row + f);
    }
    bool ok = t < n;
#pragma unroll
    for (int f = 0; f < D; ++f) {
        if (mean) v[f] = (v[f] - mean[f]) / stdv[f];
        ok = ok && fabs(v[f]) <= kFilterHi;           // false for NaN
        v[f] = ldexp(v[f], ex);                       // exact
        ok = ok && fabs(v[f]) <= kFilterScaledHi;
    }
    unsigned short hi[D], lo[D];
    double q = 0.0, tiny = 0.0;
#pragma unroll
    for (int f = 0; f < D; ++f) {
        hi[f] = lo[f] = 0;
        if (ok) {
            q = fma(v[f], v[f], q);
            f16_split2(v[f], hi[f], lo[f], tiny);
        }
    }
    // |x'| rounded up, plus twice what the left-out parts can contribute against kappa |c_j| (header, "Range")
    const unsigned short xn =
        ok ? f16_bits(f16_ceil(fmax((sqrt(q) + 2.0 * tiny / kFilterKappa) * kUp20d, kF16MinNormal))) : 0x7C00;
    unsigned short s[8 * RQ];
#pragma unroll
    for (int i = 0; i < 8 * RQ; ++i) s[i] = 0;
#pragma unroll
    for (int f = 0; f < D; ++f) {
        if (f < 8) {
            s[f] = hi[f];
            s[8 + f] = lo[f];
        } else {
            s[16 + f - 8] = s[20 + f - 8] = hi[f];
            s[18 + f - 8] = lo[f];
        }
    }
    s[23] = xn;
    uint4* mine = reinterpret_cast<uint4*>(stage) + threadIdx.x * kOutStride;
#pragma unroll
    for (int c = 0; c < RQ; ++c)
        mine[c] = make_uint4(s[8 * c + 0] | ((unsigned)s[8 * c + 1] << 16), s[8 * c + 2] | ((unsigned)s[8 * c + 3] << 16),
                             s[8 * c + 4] | ((unsigned)s[8 * c + 5] << 16), s[8 * c + 6] | ((unsigned)s[8 * c + 7] << 16));
    __syncthreads();
    uint4* dst = image + t0 * RQ;
    for (int c = threadIdx.x; c < rows_out * RQ; c += 256)
        dst[c] = reinterpret_cast<const uint4*>(stage)[(c / RQ) * kOutStride + (c % RQ)];
}

// ---------------------------------------------------------------------------------------------------------
// Centre side, once per launch and workgroup (one wave per 16-centre tile) into the kernel's LDS:
//   img   [n_tiles][64] uint4           A operands in scaled units c' = 2^e_c c, lane-major
//   tab   [n_tiles * 16][RF] f32        fp32 centre coordinates zero-padded to DP features, then h_j, then |c_j|
//                                       rounded up (padding rows: 0, 3e38, -3e38), rows 16-byte aligned: step 3
//   cz    [n_tiles * 16] f32            C operand: -(1 - kappa) h_j 2^(e_x + e_c) rounded up (padding rows: -3e38)
//   hs    [n_tiles * 16] f64            h_j (+inf for padding rows): step 4 and the pinned distance
//   any_bad                             a centre failed the range guard: every frame takes the exhaustive scan
// DP = 4 (d <= 4) or 10 (d <= 10): the features of the fp32 table and of the frame coordinates.
// ---------------------------------------------------------------------------------------------------------
template <int DP>
struct FilterShape {
    static constexpr int RF = DP == 4 ? 8 : 12;                             // floats per table row
    static constexpr int kTileBytes = 1024 + 16 * RF * 4 + 16 * 4 + 16 * 8;  // image + table rows + C + h of one tile
};
__host__ __device__ constexpr int filter_dp(int d) { return d <= 4 ? 4 : 10; }

// One wave stages one 16-centre tile in two steps, so that a wave with several tiles has the global loads of all of
// them in flight before it builds the first (the build is ~300 instructions; one load round trip under load is as long):
//   filter_stage_fetch: the tile's 16 x d coordinates, one coalesced load per 64 elements (element e = row e / d,
//                       feature e % d), at most kStageRegs per lane;
//                       and features q, q + 4, q + 8 of row lane & 15 (q = lane >> 4): the row side, kStageRowQ per lane;
//   filter_stage_build: fp16 pairs into the A operands, fp32 coordinates into the table rows; then the row side.  Its
//                       bound part (range guard, |c'_j|^2, what the split leaves out) is summed by the four lanes of a
//                       row, each over its own features, and combined with the row swaps of wave.h; lane j of the first
//                       sixteen collects the row's coordinates from the other three by the same swaps and runs the
//                       fp64 chain over ascending features for h_j (the bits of every other h_j in the library), C,
//                       the kappa slot and the table's last two columns.
constexpr int kStageRegs = (16 * kFilterMaxD + 63) / 64;
// i / d for 0 <= i < 8192 (a tile's 160 elements; the close's kFilterCloseCH x 1024), 1 <= d <= 10 without the
// integer-division sequence: (i + 0.5) / d is at least 0.05 away from every integer, fp32 rounding moves it by less
// than 0.002
__device__ __forceinline__ int stage_row(int i, int d) { return (int)(((float)i + 0.5f) * (1.0f / (float)d)); }
// x of lane (j, qs) = j + 16 qs in lane j < 16 (the other lanes get some lane's x): v_permlane32_swap brings rows 2, 3
// to rows 0, 1, v_permlane16_swap row 1 to row 0 (row_swap, wave.h)
__device__ __forceinline__ double xrow_to_first(double x, int qs) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    if (qs & 2) {
        lo = row_swap<1>(lo)[1];
        hi = row_swap<1>(hi)[1];
    }
    if (qs & 1) {
        lo = row_swap<0>(lo)[1];
        hi = row_swap<0>(hi)[1];
    }
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <int DP>
constexpr int kStageRowQ = (DP + 3) / 4;   // features of a row per lane when its four lanes (j, j + 16, j + 32, j + 48) share them
template <int DP>
__device__ __forceinline__ void filter_stage_fetch(int tile, int lane, const double* __restrict__ centers, int k, int d,
                                                   double (&c)[kStageRegs], double (&rq)[kStageRowQ<DP>]) {
#pragma unroll
    for (int u = 0; u < kStageRegs; ++u) {
        const int i = lane + 64 * u;
        const int r = stage_row(i, d), j = tile * 16 + r;
        c[u] = (i < 16 * d && j < k) ? centers[(size_t)tile * 16 * d + i] : 0.0;
    }
    // the row side: features q, q + 4, q + 8 of row lane & 15 (zeros beyond d and k leave every chain and sum unchanged)
    const int jq = tile * 16 + (lane & 15);
#pragma unroll
    for (int m = 0; m < kStageRowQ<DP>; ++m) {
        const int f = (lane >> 4) + 4 * m;
        rq[m] = (jq < k && f < d) ? centers[(size_t)jq * d + f] : 0.0;
    }
}
// ec: the centres' scale exponent; exc = e_x + e_c (the scale of the C operand)
template <int DP>
__device__ __forceinline__ void filter_stage_build(int tile, int lane, unsigned short* simg, const double (&c)[kStageRegs],
                                                   const double (&rq)[kStageRowQ<DP>], int k, int d, int ec, int exc,
                                                   float* __restrict__ tab, float* __restrict__ cz, double* __restrict__ hs,
                                                   int* __restrict__ any_bad) {
    using S = FilterShape<DP>;
    for (int i = lane; i < 64 * 4; i += 64) reinterpret_cast<unsigned*>(simg)[i] = 0u;
    for (int i = lane; i < 16 * S::RF; i += 64) tab[(size_t)tile * 16 * S::RF + i] = 0.0f;   // pads beyond d
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // one wave, LDS in order: only the compiler must not reorder
    auto slot_addr = [&](int i, int sl) { return ((sl >> 3) * 16 + i) * 8 + (sl & 7); };   // fp16 element of row i, slot sl
#pragma unroll
    for (int u = 0; u < kStageRegs; ++u) {
        const int i = lane + 64 * u;
        const int r = stage_row(i, d), f = i - r * d, j = tile * 16 + r;
        if (i < 16 * d && j < k) {
            tab[(size_t)j * S::RF + f] = (float)c[u];
            const double w = ldexp(c[u], ec);
            if (fabs(w) <= kFilterScaledHi) {            // (else the row lanes below fail the range guard)
                unsigned short ch, cl;
                double tiny = 0.0;                       // (the row lanes add it up for the kappa slot)
                f16_split2(w, ch, cl, tiny);
                simg[slot_addr(r, filter_slot(0, f))] = ch;
                simg[slot_addr(r, filter_slot(1, f))] = ch;
                simg[slot_addr(r, filter_slot(2, f))] = cl;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // the bound side of row lane & 15, dealt over its four lanes by feature: the range guard, |c'_j|^2 and what
    // f16_split2 leaves out of the row (header, "Row sums"); zeros beyond d and in padding rows add nothing
    double aw = 0.0, tiny = 0.0;
    int ok_q = 1;
#pragma unroll
    for (int m = 0; m < kStageRowQ<DP>; ++m) {
        const double cf = rq[m];
        const double w = ldexp(cf, ec);
        if (!(fabs(cf) <= kFilterHi && fabs(w) <= kFilterScaledHi)) ok_q = 0;   // NaN fails
        aw = fma(w, w, aw);
        const bool whole = !(fabs(w) >= kF16MinNormal);
        const double r = whole ? fabs(w) : fabs(w - f16_round(w));
        if (whole || !(r >= kF16MinNormal)) tiny += r;
    }
    aw = xrow_reduce(aw, op_sum{});
    tiny = xrow_reduce(tiny, op_sum{});
    const bool ok_row = xrow_min_i32(ok_q) != 0;   // (a row that fails has garbage in aw and tiny: neither is used)
    // |c_j|^2 in lane j < 16: the serial chain over ascending features, feature f from lane (j, f & 3)
    double a = 0.0;
#pragma unroll
    for (int f = 0; f < DP; ++f) {
        const double cf = xrow_to_first(rq[f >> 2], f & 3);
        a = fma(cf, cf, a);
    }
    int bad_row = 0;
    if (lane < 16) {
        const int j = tile * 16 + lane;
        float* row = tab + (size_t)j * S::RF;
        double h = __builtin_inf();
        if (j < k) {
            h = 0.5 * a;
            const double cval = ldexp(-(h - kFilterKappa * h), exc);
            const bool ok = ok_row && fabs(cval) <= 0x1p100;
            if (!ok) bad_row = 1;
            cz[j] = ok ? f32_up(cval) : 0.0f;
            if (ok)
                simg[slot_addr(lane, kFilterSlotNorm)] =
                    f16_bits(f16_ceil(fmax((kFilterKappa * sqrt(aw) + 2.0 * tiny) * kUp20d, kF16MinNormal)));
            row[DP] = (float)h;
            row[DP + 1] = (float)(sqrt(a) * kUp20d);
        } else {
            cz[j] = -3.0e38f;            // a padding centre never holds a maximum
            row[DP] = 3.0e38f;           // score -3e38 ...
            row[DP + 1] = -3.0e38f;      // ... and an S bound <= 0 (the pick multiplies this by max(|z|, 1))
        }
        hs[j] = h;
    }
    const bool bad = __any(bad_row != 0);
    if (bad && lane == 0) atomicOr(any_bad, 1);
}

// The filter's cross-lane steps are on the VALU (wave.h): xrow_* over the 4 lanes (j, j + 16, j + 32, j + 48) that share
// a frame, wave_* over the whole wave.  A butterfly of __shfl_xor would be six trips through the LDS crossbar, ~1 us.

// max |v| over the coordinates that pass the unscaled range guard (whitened when mean / stdv are given) into *out_bits
// (non-negative doubles order like their bits): the bound of the frames' scale when the caller has none to give
template <typename T>
__global__ __launch_bounds__(256) void filter_absmax_kernel(const T* __restrict__ x, int64_t n, int d, int64_t ld,
                                                           const double* __restrict__ mean, const double* __restrict__ stdv,
                                                           unsigned long long* __restrict__ out_bits) {
    double m = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n * d; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / d;
        const int f = (int)(i - r * d);
        double v = load_as_f64(x + r * ld + f);
        if (mean) v = (v - mean[f]) / stdv[f];
        if (fabs(v) <= kFilterHi) m = fmax(m, fabs(v));
    }
    m = wave_max_f64(m);
    __shared__ double wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmax(fmax(wm[0], wm[1]), fmax(wm[2], wm[3]));
        if (m > 0.0) atomicMax(out_bits, (unsigned long long)__double_as_longlong(m));
    }
}

template <typename T, int DP, bool WHITEN>
__device__ __forceinline__ void filter_load_frame(const T* __restrict__ x, int64_t ld, int d, bool vec_rows,
                                                  const double* __restrict__ mean, const double* __restrict__ stdv,
                                                  int64_t t, double (&z)[DP]) {
    const T* row = x + t * ld;
    if (vec_rows) {
        const double2* r2 = reinterpret_cast<const double2*>(row);
#pragma unroll
        for (int f2 = 0; f2 < DP / 2; ++f2) {
            const double2 v = r2[f2];
            z[2 * f2] = v.x;
            z[2 * f2 + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int f = 0; f < DP; ++f) {
            const double v = load_as_f64(row + (f < d ? f : d - 1));
            z[f] = f < d ? v : 0.0;
        }
    }
    if constexpr (WHITEN) {
#pragma unroll
        for (int f = 0; f < DP; ++f) {
            const int fc = f < d ? f : d - 1;
            const double w = (z[f] - mean[fc]) / stdv[fc];
            z[f] = f < d ? w : 0.0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// LDS of the main kernel: img | tab | hs | lsum [k][d], lcnt [k] u64 (ACCUM) | cen [k][d] f64 (CLOSE)
// centres <- sums / counts, shift2, n_iter, done: what kmeans_update_kernel (kmeans.hip) does, by one workgroup of MT
// threads, with the additions of shift2 in the order of that kernel's 1024 threads (virtual thread v takes the
// elements v, v + 1024, ...; 64 consecutive virtual threads add up by the same shuffles; the sixteen partial sums in
// order), so the two ways of closing an iteration give the same bits.  sums / counts were last written by other
// workgroups' atomics: read them with device-scope loads.
template <int MT>
__device__ __forceinline__ void filter_close_iteration(const unsigned long long* sums, const unsigned long long* counts, int k,
                                                       int d, double* centers, FitState* st) {
    __shared__ double red[16];
    const int tid = threadIdx.x;
    const double inv_scale = st->inv_scale;
    for (int v0 = 0; v0 < 1024; v0 += MT) {
        const int v = v0 + tid;
        if (v < 1024) {                 // whole waves: MT and 1024 are multiples of 64
            double acc = 0.0;
            constexpr int CH = 4;       // elements in flight per thread: the loads of a chunk before the arithmetic of any
            for (int i0 = v; i0 < k * d; i0 += 1024 * CH) {
                long long cnt[CH], sm[CH];
                double old[CH];
#pragma unroll
                for (int c = 0; c < CH; ++c) {
                    const int i = i0 + c * 1024;
                    cnt[c] = 0;
                    if (i < k * d) {
                        cnt[c] = (long long)__hip_atomic_load(&counts[i / d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        sm[c] = (long long)__hip_atomic_load(&sums[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        old[c] = centers[i];
                    }
                }
#pragma unroll
                for (int c = 0; c < CH; ++c)
                    if (cnt[c] > 0) {
                        const double c_new = (double)sm[c] * inv_scale / (double)cnt[c];
                        const double dlt = c_new - old[c];
                        acc = fma(dlt, dlt, acc);
                        centers[i0 + c * 1024] = c_new;
                    }
            }
            // wave_sum_down (wave.h) written out: the call moves the red[] address ahead of the last shuffle and adds an s_waitcnt
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
            if ((v & 63) == 0) red[v >> 6] = acc;
        }
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < 16; ++i) t += red[i];
        st->shift2 = t;
        st->n_iter += 1.0;
        if (t <= st->tol2) st->done = 1.0;
    }
}

// ---------------------------------------------------------------------------------------------------------
// CL = FilterCloseArgs (CLOSE; msm_kmeans_lloyd_pass_deferred / msm_kmeans_assign_closing, fp64 frames without whitening): the
// launch closes the Lloyd iteration of its PREDECESSOR in its own prologue (every workgroup for itself, from the member sums
// the kernel boundary has ordered), keeps the fp64 centre table in the LDS, and ends with its flush: no workgroup
// waits for another.  The member sums rotate through three buffers so that no workgroup reads what another one of
// the same launch adds to: `sums_in` / `counts_in` (complete, read only), `sums` / `counts` (zero when the launch
// begins; receive sums_in + this launch's moves), `sums_clear` / `counts_clear` (zeroed for the next launch).  The
// LAST workgroup (the one with the fewest units) writes everything global that is not a flush: centers_out, the
// fit state, the carry of sums_in and the clear.  `centers` are then the centres BEFORE the pending close, never written
// in this launch.  CL = FilterNoClose: the kernel as it was, with the ticket close in its epilogue where upd_centers is given.
struct FilterNoClose {
    static constexpr bool kClose = false;
};
struct FilterCloseArgs {
    static constexpr bool kClose = true;
    double* centers_out;
    const unsigned long long* sums_in;
    const unsigned long long* counts_in;
    unsigned long long* sums_clear;
    unsigned long long* counts_clear;
    int close_pending;
};
template <typename T, int DP, int NF, bool ACCUM, bool WHITEN, typename CL = FilterNoClose>
__global__ __launch_bounds__(64 * filter_waves(DP, ACCUM, sizeof(T) == 8 && !WHITEN)) void kmeans_filter_kernel(
    const T* __restrict__ x, int64_t n, int d, int64_t ld, int k, const double* __restrict__ mean,
    const double* __restrict__ stdv, const uint4* __restrict__ image, const double* __restrict__ centers,
    int32_t* __restrict__ labels,
    double* __restrict__ mindist, const FitState* __restrict__ st, unsigned long long* __restrict__ sums,
    unsigned long long* __restrict__ counts, unsigned long long* __restrict__ n_scanned, double* upd_centers,
    unsigned int* __restrict__ ticket, int first_pass, CL cl) {
    constexpr bool CLOSE = CL::kClose;
    // first_pass (delta mode): no frame is booked under a centre yet -- every previous label counts as -1 and `labels`
    // is only written, so the fit needs neither a fill of the label buffer nor the pass over it (a kernel argument:
    // uniform, it stays in a scalar register)
    using S = FilterShape<DP>;
    constexpr int kFilterWaves = filter_waves(DP, ACCUM, sizeof(T) == 8 && !WHITEN);
    constexpr int kMT = 64 * kFilterWaves, RF = S::RF, RQ = kFilterRowQ;
    // the d <= 10 accumulate passes keep only the fp32 copy of a frame's coordinates after the candidate pick; the few
    // frames that move their member sums read their fp64 row once more (filter_waves)
    constexpr bool kReloadZ = ACCUM && DP == 10;
    static_assert(NF == 4, "one frame group per lane quarter: a unit is 64 frames, one per lane in the candidate pick");
    static_assert(!CLOSE || (kMT == 1024 && sizeof(T) == 8 && !WHITEN), "the prologue close is kmeans_update_kernel's 1024 threads");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    // CLOSE: the workgroup that writes the global results of the close; with the rounded-up deal of units it has the fewest
    const bool closer = CLOSE && blockIdx.x == gridDim.x - 1;
    // CLOSE: carry the complete member sums into this launch's buffer (atomics: other workgroups are adding their moves
    // to it) and clear the buffer of the next launch
    auto close_housekeeping = [&]() {
      if constexpr (CLOSE) {
        if (cl.close_pending && cl.sums_in) {
            for (int i = threadIdx.x; i < k * d; i += kMT) {
                const unsigned long long v = cl.sums_in[i];
                if (v) atomicAdd(&sums[i], v);
            }
            for (int i = threadIdx.x; i < k; i += kMT) {
                const unsigned long long v = cl.counts_in[i];
                if (v) atomicAdd(&counts[i], v);
            }
        }
        if (cl.sums_clear) {
            for (int i = threadIdx.x; i < k * d; i += kMT) cl.sums_clear[i] = 0ull;
            for (int i = threadIdx.x; i < k; i += kMT) cl.counts_clear[i] = 0ull;
        }
      }
    };
    if constexpr (ACCUM) {
        // (CLOSE: the closing workgroup of THIS launch may set `done` while a late workgroup arrives here; that one
        // returns now, the others a few lines down when they find the same shift -- nothing differs)
        if (st->done != 0.0) {
            if constexpr (CLOSE) {
                // converged in an earlier launch: nothing is computed, the buffers keep their rotation
                if (closer) {
                    if (cl.close_pending && cl.centers_out != centers)
                        for (int i = threadIdx.x; i < k * d; i += kMT) cl.centers_out[i] = centers[i];
                    close_housekeeping();
                }
            }
            return;
        }
    }
    const int k16 = (k + 15) & ~15;
    const int n_tiles = ((k16 / 16) + 1) & ~1;            // even: the loop takes tile pairs
    uint4* img = reinterpret_cast<uint4*>(smem_raw);
    float* tab = reinterpret_cast<float*>(img + (size_t)n_tiles * 64);
    float* cz = tab + (size_t)n_tiles * 16 * RF;
    double* hs = reinterpret_cast<double*>(cz + (size_t)n_tiles * 16);
    unsigned long long* lsum = reinterpret_cast<unsigned long long*>(hs + (size_t)n_tiles * 16);
    unsigned long long* lcnt = lsum + (ACCUM ? (size_t)k * d : 0);
    // CLOSE: cen [k][d] f64, the centres of this launch -- every fp64 centre coordinate the kernel reads comes from here
    // (centers_out is being written during the launch)
    double* cen = reinterpret_cast<double*>(lcnt + (ACCUM ? (size_t)k : 0));
    const double* crows = CLOSE ? cen : centers;
    __shared__ int unit_ctr;
    __shared__ int any_bad;
    __shared__ unsigned long long cmax_bits;
    // CLOSE: the high word of max |c| per wave, from the close (the scale needs the exponent alone; 1 stands for a
    // subnormal maximum, which has the scale of any other number below 2^-47).  Words, not doubles: the static LDS of
    // the kernel stays inside the 256 bytes filter_lds_bytes_close leaves for it
    __shared__ int wave_cmax_hi[CLOSE ? 16 : 1];
    // (the wave number through readfirstlane: the compiler then knows that unit numbers are uniform and addresses the
    // image and coordinate loads as scalar base + lane offset + immediate, not with a 64-bit register pair per load)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j16 = lane & 15, q = lane >> 4;
    const double scale = ACCUM ? st->scale : 0.0;
    if (tid == 0) {
        unit_ctr = kFilterWaves;
        any_bad = 0;
        cmax_bits = 0ull;
    }
    KSTAMP_INIT
    if constexpr (ACCUM) {
        for (int i = tid; i < k * (d + 1); i += kMT) lsum[i] = 0ull;
    }
    if constexpr (CLOSE) {
        // ---- the close of the previous launch's iteration: the arithmetic of filter_close_iteration<1024> (thread =
        // virtual thread, elements tid, tid + 1024, ... in ascending order, the same shuffles, the sixteen partial sums in
        // order), by every workgroup for itself: same inputs, same bits on every CU.  All loads go out before any
        // arithmetic: one round trip (kFilterCloseCH x 1024 elements; the host sends larger tables elsewhere)
        __shared__ double red[16];
        constexpr int CH = kFilterCloseCH;
        static_assert(CH * 1024 <= 8192, "stage_row");
        long long cnt[CH], sm[CH];
        double old[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = tid + c * 1024;
            cnt[c] = 0;
            sm[c] = 0;
            old[c] = 0.0;
            if (i < k * d) {
                old[c] = centers[i];
                if (cl.close_pending) {
                    cnt[c] = (long long)cl.counts_in[stage_row(i, d)];
                    sm[c] = (long long)cl.sums_in[i];
                }
            }
        }
        const double inv_scale = st ? st->inv_scale : 0.0;   // (no state: an assign launch with nothing to close)
        double acc = 0.0, cm = 0.0;   // cm: max |c| of the closed table, for the centres' scale below
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int i = tid + c * 1024;
            if (i < k * d) {
                double cv = old[c];
                if (cnt[c] > 0) {
                    const double c_new = (double)sm[c] * inv_scale / (double)cnt[c];
                    const double dlt = c_new - old[c];
                    acc = fma(dlt, dlt, acc);
                    cv = c_new;
                }
                cen[i] = cv;
                cm = fmax(cm, fabs(cv));
                if (closer && cl.centers_out != centers) cl.centers_out[i] = cv;
            }
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        cm = wave_max_f64(cm);
        if (lane == 0) {
            red[wave] = acc;
            const int hw = (int)(__double_as_longlong(cm) >> 32);
            wave_cmax_hi[wave] = hw == 0 && cm > 0.0 ? 1 : hw;
        }
        __syncthreads();
        if (cl.close_pending) {
            double t = 0.0;
            for (int i = 0; i < 16; ++i) t += red[i];
            // an assign launch behind a fit that had converged before: the close above gave the centres it was handed
            // (same sums, same arithmetic) and the fit state stays.  Only the closing workgroup looks at `done` here:
            // it is the one that writes it
            FitState* stw = const_cast<FitState*>(st);
            if (closer && tid == 0 && (ACCUM || stw->done == 0.0)) {
                stw->shift2 = t;
                stw->n_iter += 1.0;
                if (t <= stw->tol2) stw->done = 1.0;
            }
            if constexpr (ACCUM) {
                if (closer) close_housekeeping();
                if (t <= st->tol2) return;   // converged: no units, no flush -- what the next launch of the ticket chain does
            }
        } else if constexpr (ACCUM) {
            if (closer) close_housekeeping();
        }
    } else {
        __syncthreads();
    }
    KSTAMP_VM(8);   // stamps 8-12: the prologue (diagnostic builds only; they drain the loads each phase waits for)
    constexpr int kUnit = 16 * NF;   // 64 frames
    const int64_t n_units = (n + kUnit - 1) / kUnit;
    const int64_t units_per_block = (n_units + gridDim.x - 1) / gridDim.x;
    const int64_t u_begin = (int64_t)blockIdx.x * units_per_block;
    const int64_t u_end = min(n_units, u_begin + units_per_block);
    // image piece of this lane: quarter q reads piece filter_piece(q) of its frame's row
    const int voff = j16 * RQ + filter_piece(q);
    // the frames' scale 2^e_x, in the word after the image rows (kmeans_pack_kernel)
    const int ex = reinterpret_cast<const int*>(image + (size_t)((n + 63) & ~(int64_t)63) * RQ)[2];

    int64_t unit = u_begin + wave;
    v8h b[NF];
    // (the image holds whole units of rows, msm_kmeans_image_bytes: no clamping at the end of the shard, and the loads
    // are scalar base + lane offset + immediate)
    auto load_images = [&](int64_t un) {
        const uint4* ub = image + un * (kUnit * RQ);
#pragma unroll
        for (int u = 0; u < NF; ++u) b[u] = __builtin_bit_cast(v8h, ub[voff + u * 16 * RQ]);
    };
    // the first unit's images travel while the tables are built (the staging of two tiles holds 24 registers since the
    // row side takes its coordinates from the lanes of the row: the images' 16 fit beside them at 16 waves)
    if (unit < u_end) load_images(unit);

    // ---- centre tables, built by every workgroup for itself: wave w stages tiles w, w + W, ... straight into the
    // LDS (a separate staging launch + 113 KB of copies per workgroup did the same for 4.7 us more per pass);
    // padding tiles too (their rows carry the -3e38 sentinel); two tiles per trip, both fetched before either is built.
    // The centres' scale 2^e_c comes first: max |c| over the table (non-negative doubles order like their bits; NaN
    // loses, an infinite coordinate fails the range guard anyway).  (Taking it from the fetched tiles instead kept
    // their registers alive across the barrier: scratch memory.)  CLOSE: the close had every coordinate in a register and
    // left the sixteen wave maxima behind its barrier: no second pass over the table, no barrier of its own.
    double cmax;
    if constexpr (CLOSE) {
        const int hw = wave_reduce_valu<false>(wave_cmax_hi[lane & 15], [](int a, int b) { return max(a, b); });
        cmax = __longlong_as_double((long long)hw << 32);
    } else {
        double cm = 0.0;
        for (int i = tid; i < k * d; i += kMT) cm = fmax(cm, fabs(crows[i]));
        cm = wave_max_f64(cm);
        if (lane == 0 && cm > 0.0) atomicMax(&cmax_bits, (unsigned long long)__double_as_longlong(cm));
        __syncthreads();
        cmax = __longlong_as_double((long long)cmax_bits);
    }
    // (uniform values through readfirstlane: scalar registers, not VGPRs, for the rest of the kernel)
    const int ec = __builtin_amdgcn_readfirstlane(filter_scale_exp(cmax));
    const int exc = ex + ec;
    KSTAMP_VM(9);
    for (int t = wave; t < n_tiles; t += 2 * kFilterWaves) {
        const int t2 = t + kFilterWaves;
        double c0[kStageRegs], c1[kStageRegs], q0[kStageRowQ<DP>], q1[kStageRowQ<DP>];
        filter_stage_fetch<DP>(t, lane, crows, k, d, c0, q0);
        if (t2 < n_tiles) filter_stage_fetch<DP>(t2, lane, crows, k, d, c1, q1);
        KSTAMP_VM(10);
        filter_stage_build<DP>(t, lane, reinterpret_cast<unsigned short*>(img + (size_t)t * 64), c0, q0, k, d, ec, exc, tab,
                               cz, hs, &any_bad);
        if (t2 < n_tiles)
            filter_stage_build<DP>(t2, lane, reinterpret_cast<unsigned short*>(img + (size_t)t2 * 64), c1, q1, k, d, ec, exc,
                                   tab, cz, hs, &any_bad);
        KSTAMP(11);
    }
    __syncthreads();
    // the upper bounds come out in units of 2^-(e_x + e_c): R goes back to the units of the fp32 scores with this
    const float inv_scale_u = __int_as_float((127 - exc) << 23);   // 2^-exc, |exc| <= 120: built in a scalar register
    const bool all_scan = __builtin_amdgcn_readfirstlane(any_bad) != 0;
    KSTAMP(0);

    KSTAMP_VM(12);
    unsigned long long my_scans = 0;
    // 16-byte loads of a frame's coordinates: fp64 rows of exactly DP features on 16-byte boundaries
    const bool vec_rows = sizeof(T) == 8 && d == DP && ((ld * sizeof(T)) & 15) == 0 && (((uintptr_t)x) & 15) == 0;
    const int iters = n_tiles / 2;
    constexpr int kNone = 0x7fffffff;

    auto load_frame = [&](int64_t t, double (&z)[DP]) { filter_load_frame<T, DP, WHITEN>(x, ld, d, vec_rows, mean, stdv, t, z); };
    // pinned fp64 score of centre c for the frame z: the ascending-feature chain; `crow` = the centre's coordinates
    auto score64 = [&](const double* crow, int c, const double (&z)[DP]) {
        double a = 0.0;
#pragma unroll
        for (int f = 0; f < DP; ++f)
            if (f < d) a = fma(crow[f], z[f], a);
        return a - hs[c];
    };
    auto write_label = [&](int64_t t, int bidx, double bm, const double (&z)[DP]) {
        labels[t] = bidx;
        if (mindist) {
            double zsq = 0.0;
#pragma unroll
            for (int f = 0; f < DP; ++f) zsq = fma(z[f], z[f], zsq);
            const double md = -2.0 * bm + zsq;
            mindist[t] = md > 0.0 ? md : 0.0;
        }
    };
    // ---- what a scan leaves behind: the label (delta mode: the move of the frame's contribution) or label + distance
    auto commit_scan = [&](int64_t t, int sbi, double sbest, const double (&zz)[DP], int old_s) {
        if constexpr (ACCUM) {
            if (!labels || old_s != sbi) {
                // lane f adds feature f (written out per feature: picked by lane number, the coordinates became an
                // array in scratch memory)
#pragma unroll
                for (int f = 0; f < DP; ++f) {
                    if (f < d && lane == f) {
                        const unsigned long long fx = (unsigned long long)to_fixed(zz[f], scale);
                        atomicAdd(&lsum[(size_t)sbi * d + f], fx);
                        if (old_s >= 0) atomicAdd(&lsum[(size_t)old_s * d + f], 0ull - fx);
                    }
                }
                if (lane == 0) {
                    atomicAdd(&lcnt[sbi], 1ull);
                    if (old_s >= 0) atomicAdd(&lcnt[old_s], ~0ull);
                    if (labels) labels[t] = sbi;
                }
            }
        } else {
            if (lane == 0) write_label(t, sbi, sbest, zz);
        }
    };
    // ---- the plain form of step 4: the pinned fp64 scores of ALL centres, lane l takes centres l, l + 64, ..., rows from
    // the global table (40 KB, L2-resident; CLOSE: from cen[] in the LDS), one round trip per 64 centres: only for frames (or centre tables) outside
    // the range the fp32 scores are certified for, and for bands too crowded for the bookkeeping of the fp32 scan
    auto scan_frame = [&](int64_t t) {
        double zz[DP];
        load_frame(t, zz);
        double sbest = -__builtin_inf();
        int sbi = kNone;
        for (int c = lane; c < k; c += 64) {
            const double sc = score64(crows + (size_t)c * d, c, zz);
            if (sc > sbest) { sbest = sc; sbi = c; }   // ascending c per lane: the first maximum stays
        }
        // wave_argmax_xor (wave.h) written out: as a call, every specialisation of the kernel gets a different branch layout
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double ob = __shfl_xor(sbest, off, 64);
            const int oi = __shfl_xor(sbi, off, 64);
            if (ob > sbest || (ob == sbest && oi < sbi)) { sbest = ob; sbi = oi; }
        }
        if (sbi >= k) { sbi = 0; sbest = -__builtin_inf(); }   // every score NaN: label 0, as the fp64 kernel
        int old_s = -1;
        if constexpr (ACCUM) {
            if (labels && !first_pass) old_s = labels[t];
        }
        commit_scan(t, sbi, sbest, zz, old_s);
#ifdef MSM_KMF_DIAG_COUNT   // diagnostic builds count one kind of event: 1 = plain scans, 2 = bands resolved in fp64
        if (MSM_KMF_DIAG_COUNT == 1) ++my_scans;
#else
        ++my_scans;
#endif
    };

    while (unit < u_end) {
        int nt = 0;
        if (lane == 0) nt = atomicAdd(&unit_ctr, 1);
        const int64_t nxt = u_begin + __builtin_amdgcn_readfirstlane(nt);
        KSTAMP_VM(1);
        // ---- filter: pair maxima of the upper bounds, top two per lane
        float b1[NF], b2[NF];
        int bp[NF];
#pragma unroll
        for (int u = 0; u < NF; ++u) { b1[u] = -__builtin_inff(); b2[u] = -__builtin_inff(); bp[u] = 0; }
#ifdef MSM_KMF_DIAG_NOTILE   // timing experiments only (tools/build_variant.sh): wrong results
        for (int it = 0; it < (iters < 9 ? iters : 9); ++it) {
#else
        for (int it = 0; it < iters; ++it) {
#endif
            const int jt = 2 * it;
            const v8h aa = __builtin_bit_cast(v8h, img[(jt + 0) * 64 + lane]);
            const v8h ab = __builtin_bit_cast(v8h, img[(jt + 1) * 64 + lane]);
            // C: -(1 - kappa) h of this lane's four centres (rows 4 q .. 4 q + 3 of the tile), shared by the frame groups
            const v4f32 ca = *reinterpret_cast<const v4f32*>(cz + (jt + 0) * 16 + 4 * q);
            const v4f32 cb = *reinterpret_cast<const v4f32*>(cz + (jt + 1) * 16 + 4 * q);
            v4f32 acca[NF], accb[NF];
#pragma unroll
            for (int u = 0; u < NF; ++u) {
                acca[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(aa, b[u], ca, 0, 0, 0);
                accb[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ab, b[u], cb, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < NF; ++u) {
                // m = max(b2, pair maximum): b2 <= b1, so the top-two update below is the same as with the bare
                // pair maximum, and every v_max3 takes an already canonical first operand
                float m = max3_f32(b2[u], acca[u][0], acca[u][1]);
                m = max3_f32(m, acca[u][2], acca[u][3]);
                m = max3_f32(m, accb[u][0], accb[u][1]);
                m = max3_f32(m, accb[u][2], accb[u][3]);
                const bool better = m > b1[u];
                b2[u] = med3_f32(b1[u], b2[u], m);
                b1[u] = hw_max_f32(b1[u], m);
                bp[u] = better ? jt : bp[u];
            }
        }
        KSTAMP(2);
        // the range guard of this lane's frames (the |x| slot: last element of the last piece, lane quarter 3), before
        // the images of the next unit replace them
        bool guard[NF];
#pragma unroll
        for (int u = 0; u < NF; ++u) guard[u] = q == 3 && __builtin_bit_cast(unsigned short, b[u][7]) == 0x7C00;
        // ---- the loads of the next round go out now: the next unit's images, this unit's coordinates (lane = frame:
        // lane (q, j16) takes frame j16 of group q)
        if (nxt < u_end) load_images(nxt);
        const int64_t f0 = unit * kUnit + lane;
        const bool fok = f0 < n;
        const int64_t fr = fok ? f0 : n - 1;
        // delta mode: the previous label goes out BEFORE the coordinates -- loads return in order
        int old = -1;
        if constexpr (ACCUM) {
            if (labels && !first_pass) old = labels[fr];
        }
        double z[DP];
        load_frame(fr, z);
        // ---- the winning lane, its pair and the bound R on everything outside its 8 candidates, per frame
        // lane (q, j16) keeps the values of group u = q, the frame it refines (selected here, one group at a time:
        // picked out of per-group arrays afterwards, the arrays were indexed by q and went to scratch memory)
        int cd = kNone;
        float Ru = __builtin_inff();
#ifdef MSM_KMF_DIAG_NOCROSS
        cd = bp[0] | (q << 16);
        Ru = b2[0] + b1[1] + b1[2] + b1[3] + b2[1] + b2[2] + b2[3] + (guard[0] | guard[1] | guard[2] | guard[3] ? 1.f : 0.f) + (float)(bp[1] + bp[2] + bp[3]);
#else
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            const float M1 = xrow_max_f32(b1[u]);
            // lowest holder lane q and its pair, in one minimum: (q << 16) | pair
            const int code_u = xrow_min_i32(b1[u] == M1 ? ((q << 16) | bp[u]) : kNone);
            const int gs = code_u >> 16;
            float r = q == gs ? b2[u] : b1[u];
            if (guard[u]) r = __builtin_inff();     // an infinite R refuses the certificate
            const float R_u = xrow_max_f32(r);
            cd = q == u ? code_u : cd;
            Ru = q == u ? R_u : Ru;
        }
#endif
        // R in the units of the fp32 scores: a power of two, exact unless the result is subnormal; the 2^-149 added
        // before the one rounding keeps it an upper bound there too (infinities stay)
        Ru = __builtin_fmaf(Ru, inv_scale_u, 1.40129846e-45f);
        KSTAMP(3);
        // ---- step 3, one frame per lane: its eight candidates (rows 4 gs .. 4 gs + 3 of both tiles of the winning
        // pair) scored in fp32 one after the other: best and second-best score, the index of the best, the largest S bound
        const int gs = cd >> 16, pstar = cd & 0xffff;
        const int base = min(pstar * 16 + 4 * gs, n_tiles * 16 - 20);   // (the clamp only meets the "no candidate" code)
        float pz[DP];
        float qz = 0.f;
#pragma unroll
        for (int f = 0; f < DP; ++f) {
            pz[f] = (float)z[f];
            qz = __builtin_fmaf(pz[f], pz[f], qz);
        }
        const bool z_bad = !(qz < __builtin_inff());   // NaN or overflow: the bare v_max / v_med3 below drop NaN operands
        // max(|z|, 1) rounded up: the S bound of a row is |c_j| max(|z|, 1) + h_j (padding rows: (1 - this) 3e38 <= 0)
        const float zn = hw_max_f32(__builtin_amdgcn_sqrtf(qz) * kUp20, 1.0f);
        float s1 = -__builtin_inff(), s2 = -__builtin_inff(), sbmax = 0.f;
        int i1 = 0;
#ifndef MSM_KMF_DIAG_NOPICK
        const float* p_row = tab + (size_t)base * RF;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float4* r4 = reinterpret_cast<const float4*>(p_row + ((c & 3) + 16 * (c >> 2)) * RF);
            float a = 0.f, h, cn;
            if constexpr (DP == 4) {
                const float4 r0 = r4[0], r1 = r4[1];
                a = __builtin_fmaf(r0.x, pz[0], a);
                a = __builtin_fmaf(r0.y, pz[1], a);
                a = __builtin_fmaf(r0.z, pz[2], a);
                a = __builtin_fmaf(r0.w, pz[3], a);
                h = r1.x;
                cn = r1.y;
            } else {
                const float4 r0 = r4[0], r1 = r4[1], r2 = r4[2];
                a = __builtin_fmaf(r0.x, pz[0], a);
                a = __builtin_fmaf(r0.y, pz[1], a);
                a = __builtin_fmaf(r0.z, pz[2], a);
                a = __builtin_fmaf(r0.w, pz[3], a);
                a = __builtin_fmaf(r1.x, pz[4], a);
                a = __builtin_fmaf(r1.y, pz[5], a);
                a = __builtin_fmaf(r1.z, pz[6], a);
                a = __builtin_fmaf(r1.w, pz[7], a);
                a = __builtin_fmaf(r2.x, pz[8], a);
                a = __builtin_fmaf(r2.y, pz[9], a);
                h = r2.z;
                cn = r2.w;
            }
            const float s = a - h;
            sbmax = hw_max_f32(sbmax, __builtin_fmaf(zn, cn, h));
            const bool better = s > s1;             // ties keep the earlier candidate; s2 = s1 then refuses the certificate
            s2 = med3_f32(s1, s2, s);
            s1 = hw_max_f32(s1, s);
            i1 = better ? c : i1;
        }
#endif
        // one error bound for the eight: E >= E_j.  s1 - s2 > 2 E puts s_jw - E_jw above every other s_j + E_j
        const float e = __builtin_fmaf(kPickEps, sbmax, kPickFloor);
        const int jw = base + (i1 & 3) + 16 * (i1 >> 2);
        const bool certified = !all_scan && !z_bad && cd != kNone && jw < k && s1 - s2 > 2.0f * e && s1 - e > Ru;
        const int lab = jw;
#if defined(MSM_KMF_DIAG_NOSCAN) || defined(MSM_KMF_DIAG_NOQUEUE)
        unsigned long long todo = 0;
#else
        unsigned long long todo = __ballot(fok && !certified);   // one bit per frame
#endif
        KSTAMP(4);
#ifdef MSM_KMF_DIAG_NOCOMMIT
        if (fok && certified && cd == 12345) {
#else
        if (fok && certified) {
#endif
            if constexpr (ACCUM) {
                // delta mode (labels != NULL): the sums follow the frames that CHANGED centre since the last pass
                // (integer sums: the same bits as a full re-accumulation); else every frame is added
                if (!labels || old != lab) {
                    // kReloadZ: the row this wave read for the pick a moment ago, once more (all its loads before the
                    // first atomic); the registers of z[] were free from the fp32 conversion on
                    double zm[DP];
                    if constexpr (kReloadZ) {
                        load_frame(f0, zm);
                    } else {
#pragma unroll
                        for (int f = 0; f < DP; ++f) zm[f] = z[f];
                    }
#pragma unroll
                    for (int f = 0; f < DP; ++f) {
                        if (f < d) {
                            const unsigned long long fx = (unsigned long long)to_fixed(zm[f], scale);
                            atomicAdd(&lsum[(size_t)lab * d + f], fx);
                            if (old >= 0) atomicAdd(&lsum[(size_t)old * d + f], 0ull - fx);
                        }
                    }
                    atomicAdd(&lcnt[lab], 1ull);
                    if (old >= 0) atomicAdd(&lcnt[old], ~0ull);
                    if (labels) labels[f0] = lab;
                }
            } else {
                // the pinned distance, when asked for: the fp64 chain of the one winning centre (row from the global table; CLOSE: cen[])
                if (mindist) write_label(f0, lab, score64(crows + (size_t)lab * d, lab, z), z);
                else labels[f0] = lab;
            }
        }
        KSTAMP(5);
        // ---- step 4 for the frames without a certificate, one after the other, by the whole wave
        while (todo) {
            const int jf = __builtin_ctzll(todo);
            todo &= todo - 1;
            // the 64-bit readlane pairs (readlane_f64 of wave.h) written out, here and below: calls change the SGPR spills of this loop
            const int64_t t = ((int64_t)__builtin_amdgcn_readlane((int)(f0 >> 32), jf) << 32) |
                              (unsigned)__builtin_amdgcn_readlane((int)f0, jf);
            const bool plain = all_scan || __builtin_amdgcn_readlane((int)(z_bad || !(Ru < __builtin_inff())), jf) != 0;
            if (plain) {
                scan_frame(t);
                continue;
            }
            // (a) fp32 scores of ALL centres from the LDS table, lane l takes rows l, l + 64, ...: per lane the best two rows
            // and the third-best score; over the wave the best score, the largest S bound and from them the band
            // [top - 2 E, top] outside of which no centre can hold the pinned maximum
            float zf[DP];
#pragma unroll
            for (int f = 0; f < DP; ++f) zf[f] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pz[f]), jf));
            const float znj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(zn), jf));
            float t1 = -__builtin_inff(), t2 = -__builtin_inff(), t3 = -__builtin_inff(), sbl = 0.f;
            int c1 = 0, c2 = 0;
            for (int c = lane; c < n_tiles * 16; c += 64) {
                const float4* r4 = reinterpret_cast<const float4*>(tab + (size_t)c * RF);
                float a = 0.f, h, cn;
                if constexpr (DP == 4) {
                    const float4 r0 = r4[0], r1 = r4[1];
                    a = __builtin_fmaf(r0.x, zf[0], a);
                    a = __builtin_fmaf(r0.y, zf[1], a);
                    a = __builtin_fmaf(r0.z, zf[2], a);
                    a = __builtin_fmaf(r0.w, zf[3], a);
                    h = r1.x;
                    cn = r1.y;
                } else {
                    const float4 r0 = r4[0], r1 = r4[1], r2 = r4[2];
                    a = __builtin_fmaf(r0.x, zf[0], a);
                    a = __builtin_fmaf(r0.y, zf[1], a);
                    a = __builtin_fmaf(r0.z, zf[2], a);
                    a = __builtin_fmaf(r0.w, zf[3], a);
                    a = __builtin_fmaf(r1.x, zf[4], a);
                    a = __builtin_fmaf(r1.y, zf[5], a);
                    a = __builtin_fmaf(r1.z, zf[6], a);
                    a = __builtin_fmaf(r1.w, zf[7], a);
                    a = __builtin_fmaf(r2.x, zf[8], a);
                    a = __builtin_fmaf(r2.y, zf[9], a);
                    h = r2.z;
                    cn = r2.w;
                }
                const float sc = a - h;
                sbl = hw_max_f32(sbl, __builtin_fmaf(znj, cn, h));
                if (sc > t1) { t3 = t2; t2 = t1; c2 = c1; t1 = sc; c1 = c; }
                else if (sc > t2) { t3 = t2; t2 = sc; c2 = c; }
                else t3 = hw_max_f32(t3, sc);
            }
            // the fp64 rows of this lane's two best centres go out now: (b) wants them one round trip later, for the
            // few lanes inside the band
            double rowa[DP], rowb[DP];
            {
                const double* ca = crows + (size_t)(c1 < k ? c1 : 0) * d;
                const double* cb = crows + (size_t)(c2 < k ? c2 : 0) * d;
#pragma unroll
                for (int f = 0; f < DP; ++f) {
                    rowa[f] = f < d ? ca[f] : 0.0;
                    rowb[f] = f < d ? cb[f] : 0.0;
                }
            }
            // kReloadZ: the frame's fp64 coordinates travel with those rows (wave-uniform, as in scan_frame)
            double zz[DP];
            if constexpr (kReloadZ) load_frame(t, zz);
            const float top = wave_max_f32(t1), sbw = wave_max_f32(sbl);
            const float band = top - 2.0f * __builtin_fmaf(kPickEps, sbw, kPickFloor);
            const unsigned long long in1 = __ballot(t1 >= band);
            if (__any(t3 >= band) || in1 == 0ull) {   // three of one lane's rows in the band (or NaN): the plain scan decides
                scan_frame(t);
                continue;
            }
            // the frame's previous label is in lane jf's registers, and so are its fp64 coordinates unless kReloadZ
            if constexpr (!kReloadZ) {
#pragma unroll
                for (int f = 0; f < DP; ++f) {
                    const long long bits = __double_as_longlong(z[f]);
                    zz[f] = __longlong_as_double((long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(bits >> 32), jf) << 32) |
                                                             (unsigned)__builtin_amdgcn_readlane((int)bits, jf)));
                }
            }
            const int old_t = __builtin_amdgcn_readlane(old, jf);
            int sbi;
            double sbest = 0.0;
            const bool two = __any(t2 >= band) || __builtin_popcountll(in1) > 1;
            if (!two && !(mindist && !ACCUM)) {
                sbi = __builtin_amdgcn_readlane(c1, __builtin_ctzll(in1));   // one centre in the band: it is the pinned arg-max
            } else {
                // (b) the pinned fp64 scores of the rows in the band decide (rows from the global table)
                double m1 = -__builtin_inf();
                int i1b = kNone;
                auto chain = [&](const double (&row)[DP], int c) {   // zeros beyond d leave the chain unchanged
                    double a = 0.0;
#pragma unroll
                    for (int f = 0; f < DP; ++f) a = fma(row[f], zz[f], a);
                    return a - hs[c];
                };
                if (t1 >= band && c1 < k) { m1 = chain(rowa, c1); i1b = c1; }
                if (t2 >= band && c2 < k) {
                    const double m2 = chain(rowb, c2);
                    if (m2 > m1 || (m2 == m1 && c2 < i1b)) { m1 = m2; i1b = c2; }
                }
                sbest = wave_max_f64(m1);
                sbi = wave_min_i32(m1 == sbest ? i1b : kNone);    // lowest index on ties, as the all-fp64 scan
                if (sbi >= k) {   // cannot happen for finite input; the plain scan has the rule for it
                    scan_frame(t);
                    continue;
                }
            }
            commit_scan(t, sbi, sbest, zz, old_t);
#ifdef MSM_KMF_DIAG_COUNT
            if (MSM_KMF_DIAG_COUNT == 2 && two) ++my_scans;
#else
            ++my_scans;
#endif
        }
        KSTAMP(6);
        unit = nxt;
    }
    KSTAMP(7);
    if (n_scanned && lane == 0 && my_scans) atomicAdd(n_scanned, my_scans);
    if constexpr (ACCUM) {
        __syncthreads();
        for (int i = tid; i < k * d; i += kMT)
            if (lsum[i]) atomicAdd(&sums[i], lsum[i]);
        for (int i = tid; i < k; i += kMT)
            if (lcnt[i]) atomicAdd(&counts[i], lcnt[i]);
        // The workgroup that finishes LAST closes the Lloyd iteration (centres <- sums / counts, shift, convergence flag)
        // instead of a one-workgroup launch of its own after this one: every other workgroup has then added its member
        // sums and read the old centres for the last time.
        if constexpr (!CLOSE)   // (CLOSE: the launch ends with its flush; the next one closes the iteration)
        if (upd_centers) {
            // Ordering without a device-wide fence (__threadfence() = buffer_wbl2: a write-back of the XCD's whole L2 by
            // every workgroup, +45 us per launch, measured): the member sums travel as atomics, which are resolved at
            // the device's coherence point, and every wave waits for the acknowledgement of its own (vmcnt) before the
            // workgroup takes its ticket; the closing workgroup reads them with device-scope loads, and nothing in
            // this launch has read sums / counts before, so no cache holds an older copy.
            __shared__ int is_last;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                is_last = t == gridDim.x - 1;
                if (is_last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
            }
            __syncthreads();
            if (is_last) filter_close_iteration<kMT>(sums, counts, k, d, upd_centers, const_cast<FitState*>(st));
        }
    }
    KSTAMP_FLUSH
}

// LDS bytes of the filter kernel; 0 when the shape does not fit (the fp64 kernel runs instead).  The member
// sums of an accumulate pass must fit the LDS too.
static inline size_t filter_lds_bytes(int k, int d, bool accum) {
    if (d > kFilterMaxD) return 0;
    const int k16 = (k + 15) & ~15;
    const int n_tiles = ((k16 / 16) + 1) & ~1;
    const size_t tile_bytes = filter_dp(d) == 4 ? FilterShape<4>::kTileBytes : FilterShape<10>::kTileBytes;
    const size_t total = (size_t)n_tiles * tile_bytes + (accum ? (size_t)k * (d + 1) * sizeof(unsigned long long) : 0);
    const size_t cap = 160 * 1024 - 64;   // static __shared__ words of the kernel (two ints, one u64)
    return total <= cap ? total : 0;
}
// the same for the deferred chain's flavour: the fp64 centre table on top, and the close's sixteen partial sums
static inline size_t filter_lds_bytes_close(int k, int d, bool accum) {
    const size_t base = filter_lds_bytes(k, d, accum);
    if (!base) return 0;
    const size_t total = base + (size_t)k * d * sizeof(double);
    const size_t cap = 160 * 1024 - 256;
    return total <= cap ? total : 0;
}
