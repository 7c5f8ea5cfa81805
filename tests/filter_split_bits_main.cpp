// Host check of pmarlo_amd/csrc/f16_split.h (tests/test_filter_split_bits.py compiles and runs this): the integer
// forms of f16_round, f16_ceil, f16_bits, f16_split2 and f32_up against the fp64 library forms they replaced,
// restated below, bit for bit.  Exit status 0 and "mismatches 0" when every input agrees.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../pmarlo_amd/csrc/f16_split.h"

namespace ref {
double f16_round(double v) {
    const int q = std::ilogb(v) + 1;
    return std::ldexp(std::rint(std::ldexp(v, 11 - q)), q - 11);
}
double f16_ceil(double v) {
    const int q = std::ilogb(v) + 1;
    return std::ldexp(std::ceil(std::ldexp(v, 11 - q)), q - 11);
}
// the pattern of an fp16 number of the normal range (what the conversion fp64 -> fp32 -> fp16 gives: both steps exact)
unsigned short f16_bits(double v) {
    int q;
    const double m = std::frexp(std::fabs(v), &q);                  // |v| = m 2^q, m in [0.5, 1)
    const int frac = (int)std::ldexp(m, 11) - 1024;                 // the ten bits behind the leading one
    return (unsigned short)((std::signbit(v) ? 0x8000 : 0) | ((q + 14) << 10) | frac);
}
void f16_split2(double v, unsigned short& hi, unsigned short& lo, double& tiny) {
    hi = lo = 0;
    if (!(std::fabs(v) >= kF16MinNormal)) {
        tiny += std::fabs(v);
        return;
    }
    const double h = f16_round(v);
    const double r = v - h;
    hi = f16_bits(h);
    if (!(std::fabs(r) >= kF16MinNormal)) {
        tiny += std::fabs(r);
        return;
    }
    lo = f16_bits(f16_round(r));
}
float f32_up(double v) {
    float f = (float)v;
    if ((double)f < v) {
        uint32_t b;
        std::memcpy(&b, &f, 4);
        b += f >= 0.0f ? 1u : ~0u;
        std::memcpy(&f, &b, 4);
    }
    return f;
}
}   // namespace ref

static uint64_t bits(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
static uint32_t bits(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }

static long long n_inputs = 0, n_bad = 0;
static void fail(const char* what, double v) {
    if (++n_bad <= 20) std::printf("MISMATCH %s at %a\n", what, v);
}

static void check(double v) {
    ++n_inputs;
    const double a = std::fabs(v);
    if (a >= kF16MinNormal) {
        const double r0 = ref::f16_round(v), r1 = f16_round(v);
        if (bits(r0) != bits(r1)) fail("f16_round", v);
        else if (a <= 65504.0 && ref::f16_bits(r0) != f16_bits(r1)) fail("f16_bits", v);
        if (v > 0.0) {
            const double c0 = ref::f16_ceil(v), c1 = f16_ceil(v);
            if (bits(c0) != bits(c1)) fail("f16_ceil", v);
            else if (c0 <= 65504.0 && ref::f16_bits(c0) != f16_bits(c1)) fail("f16_bits(f16_ceil)", v);
        }
    }
    for (const double t0 : {0.0, 0x1.23456789abcdep-20}) {
        unsigned short h0, l0, h1, l1;
        double t_ref = t0, t_new = t0;
        ref::f16_split2(v, h0, l0, t_ref);
        f16_split2(v, h1, l1, t_new);
        if (h0 != h1) fail("f16_split2 hi", v);
        if (l0 != l1) fail("f16_split2 lo", v);
        if (bits(t_ref) != bits(t_new)) fail("f16_split2 tiny", v);
    }
    if (bits(ref::f32_up(v)) != bits(f32_up(v))) fail("f32_up", v);
}
// v, its neighbours one and two fp64 steps away on both sides
static void check_around(double v, int steps) {
    check(v);
    double up = v, dn = v;
    for (int i = 0; i < steps; ++i) {
        up = std::nextafter(up, INFINITY);
        dn = std::nextafter(dn, -INFINITY);
        check(up);
        check(dn);
    }
}

int main() {
    // every fp16 number of the normal range, both signs; the midpoint to the next one (the largest: to 2^16)
    for (int s = 0; s < 2; ++s)
        for (int e = 1; e <= 30; ++e)
            for (int m = 0; m < 1024; ++m) {
                const double v = std::ldexp(1024.0 + m, e - 25), nx = std::ldexp(1025.0 + m, e - 25);
                const double sg = s ? -1.0 : 1.0;
                check_around(sg * v, 2);
                check_around(sg * 0.5 * (v + nx), 1);
            }
    // below the normal range: [2^-30, 2^-14), the zeros, and the edges of the split's domain
    uint64_t sd = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { sd = sd * 6364136223846793005ull + 1442695040888963407ull; return sd; };
    for (int e = -30; e < -14; ++e) {
        check_around(std::ldexp(1.0, e), 2);
        check_around(-std::ldexp(1.0, e), 2);
        for (int i = 0; i < 256; ++i) {
            const double v = std::ldexp(1.0 + (double)(next() >> 11) * 0x1p-53, e);
            check(v);
            check(-v);
        }
    }
    check(0.0);
    check(-0.0);
    check_around(16384.0, 2);
    check_around(-16384.0, 2);
    // seeded random doubles, exponents -20 .. 14, both signs
    for (int i = 0; i < 1000000; ++i) {
        const uint64_t r = next();
        const int e = -20 + (int)((r >> 3) % 35);
        const double v = std::ldexp(1.0 + (double)(next() >> 12) * 0x1p-52, e);
        check((r & 1) ? -v : v);
    }
    std::printf("inputs %lld mismatches %lld\n", n_inputs, n_bad);
    return n_bad ? 1 : 0;
}
