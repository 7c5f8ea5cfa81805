// Counter-based random numbers shared by the posterior samplers (posterior.hip, revposterior.hip).
// Device-only; include after common.h.
//
// Philox4x32-10 (Salmon et al., SC'11) keyed by the seed: a variate is a pure function of (key, counter), so it
// does not depend on the launch geometry, the batch it is drawn in, or any other variate.  Gamma variates come from
// Marsaglia & Tsang's squeeze method (ACM TOMS 26, 2000) for shape >= 1 and the boost G(a) = G(a + 1) U^(1/a)
// below; they are returned as logarithms, so that a shape of 1e-3 (U^1000) cannot underflow.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

struct Philox {
    uint32_t k0, k1;
    __device__ __forceinline__ void round(uint32_t (&c)[4], uint32_t a, uint32_t b) const {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ a;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ b;
        const uint32_t n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    }
    __device__ __forceinline__ void operator()(uint32_t (&c)[4]) const {
        uint32_t a = k0, b = k1;
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            round(c, a, b);
            a += 0x9E3779B9u;
            b += 0xBB67AE85u;
        }
    }
};

// 64 random bits -> double in (0, 1): 53 bits, never 0 or 1
__device__ __forceinline__ double unit_open(uint32_t hi, uint32_t lo) {
    const uint64_t v = (((uint64_t)hi << 32) | lo) >> 11;
    return ((double)v + 0.5) * 1.1102230246251565e-16;  // 2^-53
}

// log of a Gamma(shape, 1) variate; cell identity = (col, row, sample).  The fourth counter word is
// base + 2 * attempt (+ 1), attempt < 64: a caller that draws several variates for one cell gives each its own
// base, 128 apart.
__device__ inline double log_gamma_variate(const Philox& rng, double shape, uint32_t col, uint32_t row, uint32_t sample,
                                           uint32_t base = 0) {
    const bool boost = shape < 1.0;
    const double a = boost ? shape + 1.0 : shape;
    const double d = a - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    double lg = 0.0;
    uint32_t attempt = 0;
    for (;;) {
        uint32_t r[4] = {col, row, sample, base + 2 * attempt};
        rng(r);
        const double u1 = unit_open(r[0], r[1]), u2 = unit_open(r[2], r[3]);
        uint32_t q[4] = {col, row, sample, base + 2 * attempt + 1};
        rng(q);
        const double u3 = unit_open(q[0], q[1]), u4 = unit_open(q[2], q[3]);
        ++attempt;
        const double x = sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);  // Box-Muller
        const double t = 1.0 + c * x;
        if (t <= 0.0) continue;
        const double v = t * t * t;
        const double x2 = x * x;
        const double lv = log(v);
        if (u3 < 1.0 - 0.0331 * x2 * x2 || log(u3) < 0.5 * x2 + d * (1.0 - v + lv) || attempt >= 64) {
            lg = log(d) + lv;
            if (boost) lg += log(u4) / shape;
            break;
        }
    }
    return lg;
}
