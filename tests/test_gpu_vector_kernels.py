"""The solvers' vector kernels (csrc/tomo_ctx.hip: k_vec<...>, k_residual_scale, k_update, k_dot, tomo_vec_update_acc; csrc/tomo_reg.hip:
k_soft_threshold) against numpy, element by element, at the sizes where a grid-stride kernel can go wrong: 0, 1, one block +- 1, exactly
one sweep of the capped grid (2048 x 256 = 524 288 threads; 4096 x 256 for the soft threshold), one element into the second sweep, and a
ragged third sweep.  float32 outputs are compared BIT FOR BIT with numpy's float32 expression (the two fmaf kernels: on exactly
representable data, and to half a unit in the last place of the float64 value otherwise), float64 sums to 1e-12 relative."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = [0, 1, 255, 256, 257, 524288, 524289, 1048581]
GUARD = f32(-123.25)


@pytest.fixture()
def be():
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    ctx = _lib.Context()
    b = HipBackend.__new__(HipBackend)
    b.ctx, b.lib = ctx, ctx.lib
    yield b
    ctx.close()


def _put(be, host, off=0):
    """`host` on the device, `off` floats past an allocation's start and followed by a guard float; the view keeps its base alive."""
    host = np.asarray(host, f32)
    base = be.ctx.to_device(np.concatenate([np.full(off, GUARD), host, np.full(1, GUARD)]))
    return base.view(off, host.size)


def _get(view):
    """The view's values, after checking that the floats around it still hold the guard value."""
    whole = view._base.download()
    off = whole.size - 1 - view.size
    assert np.all(whole[:off] == GUARD) and whole[-1] == GUARD, "a kernel wrote outside its n elements"
    return whole[off:off + view.size]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same_bits(got, want):
    return got.dtype == f32 and want.dtype == f32 and np.array_equal(_bits(got), _bits(want))


def _same_bits_or_nan(got, want):
    nan = np.isnan(want)
    return got.dtype == f32 and want.dtype == f32 and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _exact(rng, n):
    """14 significant bits between 2^-10 and 2^4 (tests/test_gpu_multires.py): with a scalar of a small power-of-two denominator,
    s x + y is a float32 number, so a fused and an unfused evaluation agree and both equal numpy."""
    return (rng.integers(1, 2 ** 14, n) / 2 ** 10).astype(f32)


def _d(v):
    return np.asarray(v, np.float64)


def _close(got, want):
    return abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("n", SIZES)
def test_fill_sub_mul(be, n):
    rng = np.random.default_rng(n % 1000)
    a, b = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    A, B, O = _put(be, a), _put(be, b), _put(be, np.zeros(n))
    be.fill(O, 0.1)
    assert _same_bits(_get(O), np.full(n, f32(0.1)))
    be.sub(O, A, B)
    assert _same_bits(_get(O), a - b)
    be.mul(A, B)
    assert _same_bits(_get(A), a * b)
    assert _same_bits(_get(B), b)


@pytest.mark.parametrize("n", SIZES)
def test_axpy_xpay(be, n):
    rng = np.random.default_rng(n % 1000 + 1)
    s = 0.375
    x, y = _exact(rng, n), _exact(rng, n)
    X, Y = _put(be, x), _put(be, y)
    be.axpy(Y, X, s)                                 # y += s x
    assert _same_bits(_get(Y), y + f32(s) * x)
    Y = _put(be, y)
    be.xpay(Y, X, s)                                 # y = x + s y
    assert _same_bits(_get(Y), x + f32(s) * y)
    assert _same_bits(_get(X), x)
    # any data: ONE rounding of the exact s x + y (fmaf), i.e. within half a unit in the last place of the float64 value
    s = 0.3
    x, y = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    for name, p, q in (("axpy", x, y), ("xpay", y, x)):          # result = s p + q, written to y
        X, Y = _put(be, x), _put(be, y)
        getattr(be, name)(Y, X, s)
        got = _get(Y)
        want = _d(f32(s)) * _d(p) + _d(q)
        ulp = np.maximum(2.0 ** (np.frexp(np.abs(want))[1] - 24.0), 2.0 ** -149)
        slack = 2.0 ** -51 * (np.abs(_d(f32(s)) * _d(p)) + np.abs(_d(q)))       # the float64 value's own two roundings
        err = np.abs(_d(got) - want)
        print("%s n=%d: largest error %.3f units in the last place" % (name, n, float(np.max(err / ulp)) if n else 0.0))
        assert got.dtype == f32 and np.all(err <= 0.5 * ulp + slack)


def _specials(rng, n, extra):
    """standard_normal with `extra` at the front and (where there is room) again at the end, in the last sweep."""
    v = rng.standard_normal(n).astype(f32)
    extra = np.asarray(extra, f32)
    if n >= 2 * extra.size:
        v[:extra.size] = extra
        v[-extra.size:] = extra[::-1]
    elif n >= 1:
        v[0] = extra[n % extra.size]
    return v


@pytest.mark.parametrize("n", SIZES)
def test_recip_guard(be, n):
    rng = np.random.default_rng(n % 1000 + 2)
    thresh = 0.25
    v = _specials(rng, n, [0.0, -0.0, np.inf, -np.inf, np.nan, thresh, np.nextafter(f32(thresh), f32(0)), -3.0, 1e-30, 3e38, 1e-40])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = f32(1) / v
    V = _put(be, v)
    be.recip_guard(V)                                # strict: 0 where v == 0 (either sign), else the IEEE quotient
    assert _same_bits_or_nan(_get(V), np.where(v == 0, f32(0), inv))
    V = _put(be, v)
    be.recip_guard(V, thresh)                        # threshold: 0 where v < thresh (negatives, -inf), else the IEEE quotient
    assert _same_bits_or_nan(_get(V), np.where(v < f32(thresh), f32(0), inv))


@pytest.mark.parametrize("n", SIZES)
def test_residual_scale(be, n):
    rng = np.random.default_rng(n % 1000 + 3)
    b, ax, w = (rng.standard_normal(n).astype(f32) for _ in range(3))
    B, AX, W = _put(be, b), _put(be, ax), _put(be, w)
    r = b - ax
    want = float(np.sum(_d(r) ** 2))
    for dw, out in ((W, w * r), (None, r)):
        O = _put(be, np.zeros(n))
        s = be.residual_scale(B, AX, dw, O)
        assert _same_bits(_get(O), out)
        assert _close(s, want), (s, want)
    assert _same_bits(_get(B), b) and _same_bits(_get(AX), ax)


def _update_model(rec, bp, v, positivity, gt):
    r = rec + (bp * v if v is not None else bp)      # product and sum each rounded to float32
    if positivity:
        r = np.where(r < 0, f32(0), r)
    return r, (float(np.sum(_d(gt - r) ** 2)) if gt is not None else None)


@pytest.mark.parametrize("n", SIZES)
def test_update(be, n):
    rng = np.random.default_rng(n % 1000 + 4)
    rec, bp, v, gt = (rng.standard_normal(n).astype(f32) for _ in range(4))
    BP, V, GT = _put(be, bp), _put(be, v), _put(be, gt)
    for use_v in (True, False):
        for positivity in (True, False):
            for use_gt in (True, False):
                want, want_err = _update_model(rec, bp, v if use_v else None, positivity, gt if use_gt else None)
                R = _put(be, rec)
                err = be.update(R, BP, V if use_v else None, positivity=positivity, gt=GT if use_gt else None)
                assert _same_bits(_get(R), want), (use_v, positivity, use_gt)
                if use_gt:
                    assert _close(err, want_err), (err, want_err)
                else:
                    assert err is None
    assert _same_bits(_get(BP), bp) and _same_bits(_get(V), v) and _same_bits(_get(GT), gt)


@pytest.mark.parametrize("n", SIZES)
def test_update_acc_over_slabs(be, n):
    """Three slabs of one buffer, the middle one empty: the bits of `rec` and the error sum of the single call."""
    rng = np.random.default_rng(n % 1000 + 5)
    rec, bp, v, gt = (rng.standard_normal(n).astype(f32) for _ in range(4))
    BP, V, GT = _put(be, bp), _put(be, v), _put(be, gt)
    R1 = _put(be, rec)
    one = be.update(R1, BP, V, positivity=True, gt=GT)
    want, want_err = _update_model(rec, bp, v, True, gt)
    assert _same_bits(_get(R1), want) and _close(one, want_err)
    k = n // 3
    for _ in range(2):                               # the second pass: a new first=True restarts the sum
        R = _put(be, rec)
        for i, (o, m) in enumerate(((0, k), (k, 0), (k, n - k))):
            be.update_acc(R.view(o, m), BP.view(o, m), V.view(o, m), positivity=True, gt=GT.view(o, m), first=(i == 0))
        got = be.update_acc_fetch()
        assert _close(got, one), (got, one)
        assert _same_bits(_get(R), want)


@pytest.mark.parametrize("n", SIZES)
def test_dot_diff_sumsq_dot_acc(be, n):
    rng = np.random.default_rng(n % 1000 + 6)
    a, b = (1.0 + rng.standard_normal(n)).astype(f32), (1.0 + rng.standard_normal(n)).astype(f32)
    A, B = _put(be, a), _put(be, b)
    dot, dif = float(np.sum(_d(a) * _d(b))), float(np.sum(_d(a - b) ** 2))
    got_dot, got_dif = be.dot(A, B), be.diff_sumsq(A, B)
    assert _close(got_dot, dot) and _close(got_dif, dif), (got_dot, dot, got_dif, dif)
    be.acc_zero(0, 8)
    be.dot_acc(A, B, 3)
    be.dot_acc(A, B, 5, diff=True)
    be.dot_acc(A, B, 3, diff=True)                   # adds to what slot 3 holds
    acc = be.acc_fetch(2, 5)
    assert acc[0] == 0.0 and acc[2] == 0.0 and acc[4] == 0.0
    assert _close(acc[1], dot + dif) and _close(acc[3], dif), (acc, dot, dif)
    if n == 0:
        assert got_dot == 0.0 and got_dif == 0.0 and acc[1] == 0.0 and acc[3] == 0.0


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 257, 1048576, 1048581])
def test_soft_threshold(be, n, off):
    from oracle import oracle as orc
    rng = np.random.default_rng(n % 1000 + 7)
    lam = f32(0.6)
    inf = f32(np.inf)
    x = _specials(rng, n, [lam, -lam, np.nextafter(lam, inf), np.nextafter(-lam, -inf), np.nextafter(lam, -inf), np.nextafter(-lam, inf),
                           0.0, -0.0, np.inf, -np.inf, np.nan])
    with np.errstate(invalid="ignore"):
        want = orc.soft_thresholding(x, lam)
    assert want.dtype == f32 and not np.any(np.isnan(want))
    X, O = _put(be, x, off), _put(be, np.full(n, 9.0), off)
    be.soft_threshold(O, X, float(lam))
    assert _same_bits(_get(O), want)
    assert _same_bits_or_nan(_get(X), x)
