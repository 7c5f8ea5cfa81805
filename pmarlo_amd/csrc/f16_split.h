// fp16 numbers of the normal range from fp64, on the bit pattern of the double: what the k-means filter
// (kmeans_filter.h) builds its operands with.  No ilogb / ldexp / rint: the exponent field is read where it stands,
// rounding is an add and a mask on the 64-bit pattern (a carry out of the fraction moves into the exponent field,
// which is the next binade), and the only floating-point operation is the exact subtraction that gives a residual.
// Host and device: tests/test_filter_split_bits.py compiles this header with the host compiler and compares every
// function, bit for bit, with the fp64 library forms it replaced.
//
// Domain (what the filter hands over): finite doubles, |v| <= 2^14; f16_round / f16_ceil / f16_bits want
// 2^-14 <= |v| <= 2^16 (normal doubles, so the exponent field is never 0 or 2047); f32_up wants |v| < 2^127.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MSM_F16_FN __host__ __device__ __forceinline__
#else
#define MSM_F16_FN inline
#endif

constexpr double kF16MinNormal = 6.103515625e-05;   // 2^-14

MSM_F16_FN uint64_t f16s_bits(double v) { return __builtin_bit_cast(uint64_t, v); }
MSM_F16_FN double f16s_from_bits(uint64_t b) { return __builtin_bit_cast(double, b); }
MSM_F16_FN double f16s_abs(double v) { return f16s_from_bits(f16s_bits(v) & 0x7fffffffffffffffull); }

// an fp16 number keeps 11 significant bits: the leading one and the top 10 of the double's 52 fraction bits
constexpr uint64_t kF16DropMask = (1ull << 42) - 1;

// nearest fp16 number, ties to even (the bit above the dropped 42 decides a tie); the sign bit rides along
MSM_F16_FN double f16_round(double v) {
    const uint64_t b = f16s_bits(v);
    return f16s_from_bits((b + ((1ull << 41) - 1) + ((b >> 42) & 1ull)) & ~kF16DropMask);
}
// smallest fp16 number >= v, v >= 2^-14 (positive: rounding the magnitude up)
MSM_F16_FN double f16_ceil(double v) { return f16s_from_bits((f16s_bits(v) + kF16DropMask) & ~kF16DropMask); }
// the fp16 pattern of v, v an fp16 number of the normal range (exact): sign, exponent rebiased by 1023 - 15, the ten
// fraction bits -- all of them in the high word.  (2^16 comes out as 0x7C00, the pattern a conversion gives it.)
MSM_F16_FN unsigned short f16_bits(double v) {
    const uint32_t h = (uint32_t)(f16s_bits(v) >> 32);
    return (unsigned short)(((h >> 16) & 0x8000u) | (((h >> 10) & 0x1fffffu) - (1008u << 10)));
}
// two-term fp16 split of a scaled coordinate |v| <= 2^14: v = hi + lo + r with |r| <= 2^-22 |v|.  A part that would
// be subnormal is left out (zero) and what it leaves behind is added to `tiny` (the bound pays for it, kmeans_filter.h
// "Range")
MSM_F16_FN void f16_split2(double v, unsigned short& hi, unsigned short& lo, double& tiny) {
    hi = lo = 0;
    const double av = f16s_abs(v);
    if (!(av >= kF16MinNormal)) {
        tiny += av;
        return;
    }
    const double h = f16_round(v);
    const double r = v - h;   // exact
    hi = f16_bits(h);
    const double ar = f16s_abs(r);
    if (!(ar >= kF16MinNormal)) {
        tiny += ar;
        return;
    }
    lo = f16_bits(f16_round(r));
}
// smallest fp32 >= v, |v| < 2^127.  Inside fp32's normal range: the pattern truncated to 23 fraction bits (towards
// zero), one step up for a positive v that lost bits (a carry moves into the exponent field).  Below 2^-126 (zero
// included) the result is an fp32 subnormal or zero: the conversion and one comparison, as before.
MSM_F16_FN float f32_up(double v) {
    const uint64_t b = f16s_bits(v);
    const uint32_t e = (uint32_t)(b >> 52) & 0x7ffu;
    if (e >= 1023u - 126u && e < 1023u + 127u) {
        const uint32_t t = ((uint32_t)(b >> 32) & 0x80000000u) |
                           (uint32_t)(((b & 0x7fffffffffffffffull) >> 29) - (896ull << 23));   // exponent rebiased by 1023 - 127
        const bool up = !(b >> 63) && (b & ((1ull << 29) - 1)) != 0;
        return __builtin_bit_cast(float, t + (up ? 1u : 0u));
    }
    float f = (float)v;
    if ((double)f < v) f = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) + (f >= 0.0f ? 1u : ~0u));
    return f;
}
