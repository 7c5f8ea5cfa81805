"""The hardware rule the fp16 k-means filter's certificate rests on (pmarlo_amd/csrc/kmeans_filter.h, step 1):
v_mfma_f32_16x16x32_f16 sums its 32 products and C with an error of at most 33 x 2^-24 of the largest term, in
any order of the slots.  The filter never hands the instruction a subnormal fp16 number (such parts are left out of
the operands and paid for in the bound), so the result does not depend on how the instruction treats them; the
last test records that treatment all the same.  The numbers were measured on one MI355X through the same C ABI
(msm_mfma_f16_probe); this file repeats the measurement on every box the suite runs on."""

from __future__ import annotations

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _f16_bits(x: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float16)).view(np.uint16)


def _f16_val(bits: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float64)


def _exact(a_bits, b_bits, c):
    """Products of two fp16 numbers are exact in float64; math.fsum gives the correctly rounded sum."""
    a, b = _f16_val(a_bits), _f16_val(b_bits)
    t = a.shape[0]
    out = np.empty((t, 16, 16))
    big = np.empty((t, 16, 16))
    for s in range(t):
        for i in range(16):
            for j in range(16):
                terms = list(a[s, i, :] * b[s, :, j]) + [float(c[s, i, j])]
                out[s, i, j] = math.fsum(terms)
                big[s, i, j] = max(abs(v) for v in terms)
    return out, big


def _normal_operands(rng, shape, spread):
    """fp16 numbers of either sign, magnitudes 2^-spread .. 2^spread around 1 (normal fp16 for spread <= 13)."""
    return _f16_bits(rng.normal(size=shape) * np.exp2(rng.uniform(-spread, spread, size=shape)))


def test_accumulation_error_bound(engine):
    """Random operands over a wide range of magnitudes and signs, C included: |D - exact| <= 33 x 2^-24 x the
    largest term (the filter assumes 34.3 per instruction: the bound plus the final rounding)."""
    rng = np.random.default_rng(2026)
    t = 24
    worst = 0.0
    for spread in (0.0, 3.0, 6.0, 12.0):
        a = _normal_operands(rng, (t, 16, 32), spread)
        b = _normal_operands(rng, (t, 32, 16), spread)
        c = (rng.normal(size=(t, 16, 16)) * np.exp2(rng.uniform(-2 * spread, 2 * spread, size=(t, 16, 16)))).astype(np.float32)
        got = engine.mfma_f16_probe(a, b, c).astype(np.float64)
        want, big = _exact(a, b, c)
        worst = max(worst, float((np.abs(got - want) / (big * U)).max()))
    assert worst <= 33.0, f"accumulation error {worst:.2f} x 2^-24 of the largest term exceeds the filter's bound"


def test_any_slot_order_stays_inside_the_bound(engine):
    """The filter orders its 32 slots for the 48-byte frame image (kmeans_filter.h, filter_slot); the bound must
    hold for every order, whatever the bits of one order are."""
    rng = np.random.default_rng(8)
    t = 8
    a = _normal_operands(rng, (t, 16, 32), 10.0)
    b = _normal_operands(rng, (t, 32, 16), 10.0)
    c = (rng.normal(size=(t, 16, 16)) * 1e4).astype(np.float32)
    want, big = _exact(a, b, c)
    worst = 0.0
    for trial in range(5):
        perm = np.arange(32) if trial == 0 else rng.permutation(32)
        got = engine.mfma_f16_probe(a[:, :, perm], b[:, perm, :], c).astype(np.float64)
        worst = max(worst, float((np.abs(got - want) / (big * U)).max()))
    assert worst <= 33.0, f"a slot order gives {worst:.2f} x 2^-24 of the largest term"


def test_cancellation_against_c(engine):
    """Products that cancel C to a few bits (the filter's score against -(1 - kappa) h in the C operand): the error
    is still measured against the largest term, not against the small result."""
    rng = np.random.default_rng(9)
    t = 8
    a = _normal_operands(rng, (t, 16, 32), 4.0)
    b = _normal_operands(rng, (t, 32, 16), 4.0)
    exact_ab = np.einsum("tik,tkj->tij", _f16_val(a), _f16_val(b))
    c = (-exact_ab * (1.0 + 1e-6 * rng.normal(size=exact_ab.shape))).astype(np.float32)
    got = engine.mfma_f16_probe(a, b, c).astype(np.float64)
    want, big = _exact(a, b, c)
    worst = float((np.abs(got - want) / (big * U)).max())
    assert worst <= 33.0, f"cancellation against C: {worst:.2f} x 2^-24 of the largest term"


def test_subnormal_inputs_are_flushed_or_kept_exactly(engine):
    """An fp16 subnormal operand times 1.0 comes out either exactly (kept) or as zero (flushed), the same way for
    every subnormal pattern.  The filter does not rely on either (it never hands over a subnormal)."""
    t = 1
    pats = np.array([0x0001, 0x0002, 0x0155, 0x03FF, 0x8001, 0x83FF] + [0x0001 << (i % 10) for i in range(10)], np.uint16)
    a = np.zeros((t, 16, 32), np.uint16)
    b = np.zeros((t, 32, 16), np.uint16)
    a[0, :, 0] = pats
    b[0, 0, :] = 0x3C00                                    # 1.0
    got = engine.mfma_f16_probe(a, b, np.zeros((t, 16, 16), np.float32)).astype(np.float64)[0, :, 0]
    val = _f16_val(pats)
    kept = bool(np.array_equal(got, val))
    flushed = bool(np.all(got == 0.0))
    assert kept or flushed, (got, val)
    # a subnormal product of two normal numbers (2^-14 x 2^-14 = 2^-28) is a normal fp32 number and stays exact
    a2 = np.zeros((t, 16, 32), np.uint16)
    b2 = np.zeros((t, 32, 16), np.uint16)
    a2[0, :, 0] = 0x0400                                   # 2^-14, the smallest normal fp16
    b2[0, 0, :] = 0x0400
    got2 = engine.mfma_f16_probe(a2, b2, np.zeros((t, 16, 16), np.float32))
    assert np.all(got2[0, :, 0] == np.float32(2.0 ** -28))


def test_filter_shaped_operands(engine):
    """The filter's own operand shape (two-way fp16 splits of scaled d = 10 coordinates, slots ch xh, ch xl, cl xh and
    kappa |c| |x|, -(1 - kappa) h in C): |u - exact| <= 34.3 x 2^-24 S, S = sum |x'_f c'_f| + |h'|."""
    rng = np.random.default_rng(12)
    t, d = 16, 10

    def split2(v):
        hi = np.asarray(v, np.float64).astype(np.float16).astype(np.float64)
        lo = (np.asarray(v, np.float64) - hi).astype(np.float16).astype(np.float64)
        return _f16_bits(hi), _f16_bits(lo)

    cc = rng.normal(size=(t, 16, d)) * 2000.0            # scaled centres, |c'| < 2^13
    xx = rng.normal(size=(t, 16, d)) * 2000.0            # scaled frames
    h = 0.5 * (cc ** 2).sum(-1)
    (ch, cl), (xh, xl) = split2(cc), split2(xx)
    A = np.zeros((t, 16, 32), np.uint16)
    B = np.zeros((t, 32, 16), np.uint16)
    pairs = [(ch, xh), (ch, xl), (cl, xh)]
    slot = 0
    for cp, xp in pairs:
        for f in range(d):
            A[:, :, slot] = cp[:, :, f]
            B[:, slot, :] = xp[:, :, f]
            slot += 1
    c = np.repeat((-h)[:, :, None], 16, axis=2).astype(np.float32)
    got = engine.mfma_f16_probe(A, B, c).astype(np.float64)
    want = np.einsum("tik,tkj->tij", _f16_val(A), _f16_val(B)) + c.astype(np.float64)
    S = np.einsum("tif,tjf->tij", np.abs(cc), np.abs(xx)) + h[:, :, None]
    err = np.abs(got - want) / (S * U)
    assert float(err.max()) <= 34.3, f"accumulation error {float(err.max()):.1f} x 2^-24 S exceeds the filter's bound"
