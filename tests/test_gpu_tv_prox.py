"""The TV proximal step on the GPU (csrc/tomo_reg.hip: tomo_tv_denoise_fista and tomo_tv_prox_det, tomo_tv_norm_3d) against the stepwise
numpy model of tests/tv_model.py, on the case table that tests/test_tv_model.py qualifies: axes of length 2, nz at 255 / 256 / 257 / 513
(the z-chunk boundary), 524 320 voxels (a second sweep of the fixed reduction grid, all 2048 partials), stops decided by the dual gap.

  - iterations: exactly the model's (the stop margin of every case is far above float32's effect on a gap);
  - cases A-C: `new` and the gap within K x what float32 costs the MODEL (d32 = |float32 model - float64 model|, never less than one
    rounding of the input's magnitude) of the float64 model -- the device rounds the same operations as the float32 model, it may not
    sit a large factor farther out;
  - cases E (no projection: adds and products only): `new` equal to the float32 model BIT FOR BIT -- a product contracted into an FMA
    anywhere in the iteration fails it -- and the gap within one last place per square root plus the reordering of the float64 sums.

Every test prints the figure it asserts on."""
import numpy as np
import pytest

import tv_model as tm

pytestmark = pytest.mark.gpu

# Measured on the MI355X, |gpu - m64| / d32 over the 19 cases A-C x both entry points: 0.69 to 1.34 (A 0.69-1.34, B 0.89-1.02,
# C 0.94-1.16; DESIGN.md section 4, "The TV proximal step against a float32 model").  K is the smallest power of two that is at least
# twice the largest ratio; the gap bound takes the same K (largest measured |gap_gpu - gap_m64|: 3.2 x its unit, on the 8 voxels of 2x2x2).
K = 4
EPS32 = 2.0 ** -23
ENTRIES = ("tv_denoise_fista", "tv_prox_det")


@pytest.fixture()
def be():
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    ctx = _lib.Context()
    b = HipBackend.__new__(HipBackend)
    b.ctx, b.lib = ctx, ctx.lib
    yield b
    ctx.close()


def _run(be, entry, im, **kw):
    d_im, out = be.ctx.to_device(im), be.ctx.empty(im.shape)
    it, gap = getattr(be, entry)(d_im, out, im.shape, **kw)
    return out.download(), it, gap


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sumsq(im):
    return float(np.sum(im.astype(np.float64) ** 2))


@pytest.mark.parametrize("case", tm.INEXACT, ids=[tm.case_id(c) for c in tm.INEXACT])
def test_new_and_gap_within_float32_of_the_float64_model(be, case):
    im, kw = tm.case_input(case), tm.params(case)
    new64, it64, gap64, _, _, tv64 = tm.case_model(case, np.float64)
    new32, it32, gap32 = tm.case_model(case, np.float32)[:3]
    d32 = float(np.max(np.abs(new32 - new64)))
    unit = max(d32, EPS32 * float(np.max(np.abs(im))))
    gunit = max(abs(gap32 - gap64), EPS32 * kw["weight"] * tv64 / _sumsq(im))
    for entry in ENTRIES:
        got, it, gap = _run(be, entry, im, **kw)
        dn, dg = float(np.max(np.abs(got - new64))), abs(gap - gap64)
        print("%s %s: %d iterations (model %d); new: d32 %.2e, |gpu - m64| %.2e = %.2f x d32 (%.3f of the bound); gap %.6e: |m32 - m64| %.2e, "
              "|gpu - m64| %.2e (%.3f of the bound)" % (tm.case_id(case), entry, it, it64, d32, dn, dn / d32 if d32 else float("inf"), dn / (K * unit), gap, abs(gap32 - gap64),
                                                     dg, dg / (K * gunit)))
        assert it == it64 == it32
        assert got.dtype == np.float32 and dn <= K * unit
        assert dg <= K * gunit


@pytest.mark.parametrize("case", tm.EXACT, ids=[tm.case_id(c) for c in tm.EXACT])
def test_exact_regime_equals_the_float32_model_bit_for_bit(be, case):
    im, kw = tm.case_input(case), tm.params(case)
    new32, it32, gap32, _, worst, tv32 = tm.case_model(case, np.float32)
    assert worst < 0.5
    gbound = EPS32 * kw["weight"] * tv32 / _sumsq(im) + 4.0 * im.size * 2.0 ** -53
    for entry in ENTRIES:
        got, it, gap = _run(be, entry, im, **kw)
        differ = int(np.sum(_bits(got) != _bits(new32)))
        print("%s %s: %d of %d values differ from the float32 model in their bits (largest difference %.2e); gap %.9e, |gpu - m32| %.2e "
              "(bound %.2e)" % (tm.case_id(case), entry, differ, im.size, float(np.max(np.abs(got - new32))), gap, abs(gap - gap32), gbound))
        assert it == it32
        assert np.array_equal(_bits(got), _bits(new32)), "%d of %d values differ" % (differ, im.size)
        assert abs(gap - gap32) <= gbound


@pytest.mark.parametrize("shape", [tm.BIG, (5, 4, 255)])
def test_tv_prox_det_is_a_function_of_the_input_bits(be, shape):
    """Same bits and same gap over two calls, after a call on a larger volume (the workspace regrown, another layout's values left in
    it), and on a fresh context."""
    from tomography_alignment_amd import _lib
    case = ("B", shape)
    im, kw = tm.case_input(case), tm.params(case)
    first, it1, gap1 = _run(be, "tv_prox_det", im, **kw)
    again, it2, gap2 = _run(be, "tv_prox_det", im, **kw)
    assert it1 == it2 == tm.case_model(case, np.float64)[1]
    assert np.array_equal(_bits(first), _bits(again)) and gap1 == gap2
    larger = (shape[0], shape[1] + 1, shape[2] + 3)
    _run(be, "tv_prox_det", tm.flat(larger), weight=0.4, niter=2, eps=0.0, check_gap_frequency=1)
    after, it3, gap3 = _run(be, "tv_prox_det", im, **kw)
    assert it3 == it1 and np.array_equal(_bits(first), _bits(after)) and gap3 == gap1
    ctx2 = _lib.Context()
    be2 = type(be).__new__(type(be))
    be2.ctx, be2.lib = ctx2, ctx2.lib
    fresh, it4, gap4 = _run(be2, "tv_prox_det", im, **kw)
    ctx2.close()
    assert it4 == it1 and np.array_equal(_bits(first), _bits(fresh)) and gap4 == gap1
    print("tv_prox_det %s: %d iterations, gap %.17g on four calls" % (shape, it1, gap1))


@pytest.mark.parametrize("shape", tm.SHAPES, ids=["%dx%dx%d" % s for s in tm.SHAPES])
def test_tv_norm_3d(be, shape):
    from oracle import oracle as orc
    x = tm.block(shape)
    want = float(np.linalg.norm(orc.tv_gradient(x.astype(np.float64))))
    got = be.tv_norm_3d(be.ctx.to_device(x), shape)
    print("tv_norm_3d %s: %.9e, relative difference from float64 %.2e" % (shape, got, abs(got - want) / want))
    assert abs(got - want) <= 1e-6 * want
    assert be.tv_norm_3d(be.ctx.to_device(np.full(shape, 0.37, np.float32)), shape) == 0.0


@pytest.mark.parametrize("shape", [(1, 4, 4), (4, 1, 4), (4, 4, 1)])
def test_an_axis_of_length_one_is_refused(be, shape):
    from tomography_alignment_amd import _lib
    d_im = be.ctx.to_device(np.ones(shape, np.float32))
    for entry in ENTRIES:
        out = be.ctx.to_device(np.full(shape, 7.0, np.float32))
        with pytest.raises(_lib.TomoError):
            getattr(be, entry)(d_im, out, shape, weight=0.5, niter=3)
        assert np.array_equal(out.download(), np.full(shape, 7.0, np.float32))
    with pytest.raises(_lib.TomoError):
        be.tv_norm_3d(d_im, shape)


def test_degenerate_parameters(be):
    shape = (5, 4, 255)
    im = tm.flat(shape)
    for entry in ENTRIES:
        got, it, gap = _run(be, entry, im, weight=2.0, niter=0)
        assert it == 0 and gap == 0.0 and np.array_equal(_bits(got), _bits(im))
        # 3 iterations, a gap check every 4th: only iteration 0 is checked, and its iterate is what comes back
        kw = dict(weight=2.0, niter=3, eps=0.0, check_gap_frequency=4)
        new32, it32, gap32, gaps, worst, tv32 = tm.denoise_fista(im, dtype=np.float32, **kw)
        assert it32 == 3 and len(gaps) == 1 and worst < 0.5
        assert np.array_equal(new32, tm.denoise_fista(im, weight=2.0, niter=1, eps=0.0, check_gap_frequency=1, dtype=np.float32)[0])
        got, it, gap = _run(be, entry, im, **kw)
        assert it == 3 and np.array_equal(_bits(got), _bits(new32))
        assert abs(gap - gap32) <= EPS32 * 2.0 * tv32 / _sumsq(im) + 4.0 * im.size * 2.0 ** -53
