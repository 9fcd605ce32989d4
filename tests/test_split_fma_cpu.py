"""Operand split of csrc/mfma_split.h (split8 / split_row / stage_split / stage_rm): the form that feeds the f16 high half straight
into a mixed-precision FMA against the earlier form that converted it back to f32 first, restated in numpy and compared bit for bit.

    earlier:  hi = f16(x);  lo = f16((x - f32(hi)) * 2^11)
    now:      hi = f16(x);  lo = f16(fma(f32(hi), -2^11, x * 2^11))

Both residuals are exact in f32 (x - hi needs at most the bits of x below the f16 rounding point, the scaling is a power of two), so
the two forms round the same number to f16.  The FMA is evaluated here in float64 and the test also asserts that its float64 value IS
an f32 number: whichever way the hardware rounds the intermediate (v_fma_mix_f32 + convert, or v_fma_mixlo_f16 in one step), the
result is the same.  With the per-row power-of-two scaling of the adjoint rows (split_row<SCALED>) the row is scaled first in both forms.

Outside what the engine feeds it the two forms part only where x * 2^11 overflows f32 (|x| > 1.6e35): hi is already +-inf there in both.
"""
import numpy as np

LO_SCALE = np.float32(2048.0)


def _f16(x):
    with np.errstate(over="ignore"):
        return x.astype(np.float16)


def split_parent(x):
    x = x.astype(np.float32)
    hi = _f16(x)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = _f16((x - hi.astype(np.float32)) * LO_SCALE)
    return hi, lo


def split_fma(x, check_exact=True):
    x = x.astype(np.float32)
    hi = _f16(x)
    with np.errstate(invalid="ignore", over="ignore"):
        xs = x * LO_SCALE                                          # f32, exact (power of two)
        wide = hi.astype(np.float64) * -2048.0 + xs.astype(np.float64)   # both terms exact in f64; so is the sum (asserted below)
        r32 = wide.astype(np.float32)
    if check_exact:
        fin = np.isfinite(wide)
        assert np.array_equal(r32[fin].astype(np.float64), wide[fin]), "the fused residual is not an f32 number"
    return hi, _f16(r32)


def row_scale(x):
    """split_row<SCALED>: the power of two that brings the row's largest |x| into [1, 2) (row_exponent: rows of zeros keep 1)."""
    m = np.abs(x).max(axis=1)
    e = np.frexp(m)[1] - 1
    ok = (m > 0) & (m < 3.0e38)
    e = np.where(ok, np.clip(e, -125, 125), 0)
    return np.ldexp(np.float32(1.0), -e).astype(np.float32)[:, None]


def _bits(a):
    return a.view(np.uint16)


def _assert_same(x):
    h0, l0 = split_parent(x)
    h1, l1 = split_fma(x)
    assert np.array_equal(_bits(h0), _bits(h1))
    bad = np.nonzero(_bits(l0) != _bits(l1))[0]
    assert bad.size == 0, f"{bad.size} low halves differ, first x = {x.ravel()[bad[0]]!r}"
    return h0, l0


def _random_values(n, seed):
    rng = np.random.default_rng(seed)
    mag = np.exp(rng.uniform(np.log(1e-8), np.log(1e4), n))
    return (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def hand_picked():
    two = lambda e: np.float32(2.0) ** np.float32(e)   # noqa: E731
    v = [0.0, -0.0, 1.0, -1.0,
         # f16 rounding ties (halfway between two f16 neighbours: to even) and their f32 neighbours
         1.0 + two(-11), 1.0 + 3 * two(-11), 1.0 + two(-11) + two(-23), 1.0 + two(-11) - two(-23), 2049.0, 2051.0, 4098.0, -(1.0 + two(-11)),
         0.1, 1.0 / 3.0, 3.14159274,
         # low halves in the f16 subnormals (|lo| < 2^-14 after the 2^11 scaling), ties at half the smallest subnormal included
         two(-10) + two(-33), two(-13) + two(-36), two(-13) + 3 * two(-36), two(-12) + 5 * two(-35), -(two(-10) + two(-33)),
         # high halves in the f16 subnormals, or flushed to zero by the rounding
         1e-5, 6.1e-5, 5.96e-8, 2.98e-8, 2.9802322e-8, 3.1e-8, 1e-8, 1e-12, 1e-30, -1e-6,
         # the top of the f16 range: the largest finite f16, the largest f32 that still rounds to it, 1e4 (the sampled range's end) and
         # the first values that round to infinity (the plain forward path has no row scaling: its operands must stay below this)
         65504.0, 65519.996, 1e4, 9999.999, 65520.0, 1e5, -65520.0]
    return np.array(v, dtype=np.float32)


def test_random_values_split_bit_identically():
    x = _random_values(1_000_000, 7)
    hi, lo = _assert_same(x)
    # the split does what it is for: hi + lo / 2^11 reproduces x to ~2^-22 relative wherever the low half is a normal f16
    rec = hi.astype(np.float64) + lo.astype(np.float64) / 2048.0
    normal = np.abs(x) > 1e-3
    assert np.max(np.abs(rec[normal] - x[normal]) / np.abs(x[normal])) < 2.0 ** -21


def test_hand_picked_values_split_bit_identically():
    x = hand_picked()
    hi, lo = _assert_same(x)
    assert np.isinf(hi[-1]) and np.isinf(lo[-1])          # out of range: both forms give infinities, the same ones
    # the subnormal-low-half cases really are subnormal (or rounded to zero) in f16
    k = list(x).index(np.float32(2.0) ** -10 + np.float32(2.0) ** -33)
    assert 0 < abs(float(lo[k])) < 2.0 ** -14


def test_row_scaled_split_is_bit_identical():
    """SCALED rows (adjoint operands, 1e-3 .. 1e-7 and below): scaled by the row's power of two, then split."""
    rng = np.random.default_rng(11)
    x = _random_values(1_000_000, 13).reshape(-1, 64)
    x *= np.exp(rng.uniform(np.log(1e-9), 0.0, (x.shape[0], 1))).astype(np.float32)      # rows of very different magnitude
    x = np.concatenate([x, np.zeros((1, 64), np.float32), np.resize(hand_picked(), (3, 64))])
    down = row_scale(x)
    xs = x * down
    fin = np.isfinite(xs).all(axis=1)
    assert np.abs(xs[fin]).max() < 2.0                    # the scaled rows sit in [-2, 2]
    _assert_same(xs.ravel())
    # the scaling itself is exact: scaling back reproduces the row
    up = (np.float32(1.0) / down).astype(np.float32)
    assert np.array_equal((xs * up)[fin], x[fin])


def test_forms_part_only_where_the_scaled_value_overflows():
    """Documented limit: beyond |x| = f32_max / 2^11 the fused form's x * 2^11 is infinite; hi is +-inf there in either form."""
    x = np.array([1.0e35, 3.0e38, -3.0e38], dtype=np.float32)
    h0, _ = split_parent(x)
    h1, _ = split_fma(x, check_exact=False)
    assert np.isinf(h0).all() and np.array_equal(_bits(h0), _bits(h1))
