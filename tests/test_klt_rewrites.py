"""CPU proofs of the arithmetic rewrites in k_klt3 (ygz_slam_amd/csrc/klt.hip): each replaces a computation of the reference arithmetic
by a cheaper one that gives the same bits, and each is checked here over every float it can see or over >= 10^8 random floats.
These tests check the arithmetic identities on NumPy restatements of the device macros, not the compiled code: test_macros_are_the_proven_ones
only pins the macro text to what is proven here.  The device outputs themselves are held to the parent build's bits by
tests/test_gpu_klt_bitexact.py."""
import os
import re

import numpy as np

CHUNK = 1 << 24
KLT_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ygz_slam_amd", "csrc", "klt.hip")


def test_macros_are_the_proven_ones():
    """the restatements below follow these definitions; a change of a constant or a comparison in klt.hip has to come with a new proof"""
    src = re.sub(r"\s+", " ", open(KLT_HIP).read())
    for text in ("#define KLT_ABS_LT_001(x) (fabsf(x) <= 0.01f)",
                 "{ return __builtin_fma((double)dx, (double)dx, (double)dy * (double)dy); }",
                 "#define KLT_WBITS(x) __float_as_uint(__builtin_fmaf((x), 16384.f, 12582912.f))",
                 "wtop = KLT_DXP(w00_, w01_);",
                 "wbot = KLT_DXP(w10_, 16384u - (w00_ + w01_ + w10_));",
                 "#define KLT_DXP(a, b) __builtin_amdgcn_perm((b), (a), 0x05040100u)"):
        assert text in src, text


def _floats(lo_bits, hi_bits):
    """every float32 whose bit pattern lies in [lo_bits, hi_bits), in chunks"""
    for b in range(lo_bits, hi_bits, CHUNK):
        yield np.arange(b, min(b + CHUNK, hi_bits), dtype=np.uint32).view(np.float32)


def test_abs_lt_001_is_a_float_compare():
    """KLT_ABS_LT_001: (double)fabsf(x) < 0.01  <=>  fabsf(x) <= 0.01f: every float within 2^23 patterns of 0.01f, NaN and inf, and
    10^8 random floats"""
    c = np.float32(0.01)
    assert float(c) < 0.01 and float(np.nextafter(c, np.float32(1))) > 0.01         # 0.01f is the largest float below 0.01
    cb = int(c.view(np.uint32))
    rng = np.random.default_rng(5)
    xs = [f for f in _floats(cb - (1 << 23), cb + (1 << 23))] + [np.array([np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32)]
    xs += [rng.integers(0, 1 << 32, 10_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32) for _ in range(10)]
    for x in xs:
        with np.errstate(invalid="ignore"):
            assert np.array_equal(np.abs(x).astype(np.float64) < 0.01, np.abs(x) <= c)


def test_squared_step_is_one_fma():
    """klt_norm2_d: (double)x * x is exact for every float x (<= 48 significant bits, inside the normal FP64 range), so
    fma(dx, dx, dy * dy) rounds the same exact sum as dx * dx + dy * dy does.  Exactness over 10^8 random finite floats of every exponent
    and over all floats of one binade (every significand)."""
    rng = np.random.default_rng(7)
    n = 0
    while n < 100_000_000:
        x = rng.integers(0, 1 << 32, 10_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
        x = x[np.isfinite(x)]
        d = x.astype(np.float64)
        assert np.array_equal(d * d, (x.astype(np.longdouble) * x.astype(np.longdouble)).astype(np.float64))
        assert np.array_equal((d * d).astype(np.longdouble), x.astype(np.longdouble) * x.astype(np.longdouble))
        n += len(x)
    for f in _floats(0x3F800000, 0x3F800000 + (1 << 23)):                          # [1, 2): every significand
        d = f.astype(np.float64)
        assert np.array_equal((d * d).astype(np.longdouble), f.astype(np.longdouble) * f.astype(np.longdouble))


def _wbits(x):
    """KLT_WBITS: fma(x, 16384, 1.5 * 2^23) as float bits.  x * 16384 is exact (checked), so the float add of it rounds the same sum."""
    t = x * np.float32(16384)
    assert np.array_equal(t.astype(np.float64), x.astype(np.float64) * 16384)
    return (t + np.float32(12582912.0)).view(np.uint32)


def test_weight_bits_are_rounded_weights():
    """KLT_WBITS(x) == 0x4B400000 + cv_round_f(x * 16384) (round to nearest even): every float of [0.5, 1] and of [2^-16, 2^-13) (where
    x * 16384 has ties), and 10^8 random floats of [0, 1]"""
    rng = np.random.default_rng(3)
    xs = list(_floats(0x3F000000, 0x3F800001)) + list(_floats(0x37800000, 0x39000000))
    xs += [rng.integers(0, 0x3F800001, 10_000_000, dtype=np.uint32).view(np.float32) for _ in range(10)]
    for x in xs:
        b = _wbits(x)
        r = np.rint(x.astype(np.float64) * 16384)                                  # rint: ties to even, as __float2int_rn
        assert np.array_equal(b - np.uint32(0x4B400000), r.astype(np.uint32))


def test_packed_weights_match_klt_weights():
    """KLT_WEIGHTS_P against KLT_WEIGHTS (the parent's packing) over 3 x 10^7 random (a, b) in [0, 1) (10^8 weights) and every float
    a of [0.5, 1) against its mirror"""
    rng = np.random.default_rng(11)

    def ref(a, b):
        f32 = np.float32
        ia, ib = f32(1) - a, f32(1) - b
        iw00 = np.rint((ia * ib) * f32(16384)).astype(np.int64)
        iw01 = np.rint((a * ib) * f32(16384)).astype(np.int64)
        iw10 = np.rint((ia * b) * f32(16384)).astype(np.int64)
        iw11 = 16384 - iw00 - iw01 - iw10
        return ((iw00 & 0xffff) | (iw01 << 16)) & 0xffffffff, ((iw10 & 0xffff) | ((iw11 & 0xffff) << 16)) & 0xffffffff

    def new(a, b):
        ia, ib = np.float32(1) - a, np.float32(1) - b
        w00, w01, w10 = _wbits(ia * ib), _wbits(a * ib), _wbits(ia * b)
        wtop = (w00 & 0xffff) | ((w01 & 0xffff) << 16)                            # KLT_DXP(w00, w01): the low halves
        wbot = (w10 & 0xffff) | (((np.uint32(16384) - (w00 + w01 + w10)) & 0xffff) << 16)      # KLT_DXP(w10, 16384 - (...))
        return wtop.astype(np.int64), wbot.astype(np.int64)

    with np.errstate(over="ignore"):
        for _ in range(3):
            a = rng.random(10_000_000, dtype=np.float32)
            b = rng.random(10_000_000, dtype=np.float32)
            for u, v in zip(ref(a, b), new(a, b)):
                assert np.array_equal(u, v)
        for a in _floats(0x3F000000, 0x3F800000):
            for u, v in zip(ref(a, a[::-1]), new(a, a[::-1])):
                assert np.array_equal(u, v)
