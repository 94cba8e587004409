"""preprocess.remove_outlier / median_filter on the GPU (k_outlier of libtomo_prep.so) against the numpy model of tests/outlier_model.py,
bit for bit (np.array_equal of the raw bits, so NaNs and the two zeros compare) and count for count.

The kernel's work-group tile is 64 columns x 32 rows (OUT_TW x OUT_TH in csrc/prep/tomo_prep.hip), a lane per column; its grid spans at
most 65535 frames and strides over the rest.  The shapes are the smallest at which each path can go wrong: the minimum (1, size, size),
odd columns (3, 9, 13), more than one tile in each direction (2, 33, 70), three ragged tiles in both (1, 67, 131), and 65537 frames."""
import numpy as np
import pytest

import outlier_model as om

from tomography_alignment_amd import _lib, _prep_lib, preprocess
from tomography_alignment_amd._binding import TomoError
from tomography_alignment_amd.examples import generate_data
from tomography_alignment_amd.examples import preprocess as ex_pre

pytestmark = pytest.mark.gpu

MARGIN = 1e-3                # no finite d of the model lies within this (relative) of a finite, nonzero dif
NANS = np.array([0x7fc00000, 0x7fc00001, 0xffc12345, 0x7f800001, 0xffffffff], np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def pre(ctx):
    p = preprocess.Preprocessor(ctx)
    yield p
    p.close()


def make_frames(shape, dtype, seed=0):
    """Frames with what the order and the decision can get wrong.  uint16: the full range with 0 and 65535 side by side (a signed
    compare sorts them the other way round), the last frame of a stack of several holding 0..3 only (ties everywhere).  float32: -0.0
    and +0.0, both infinities, NaNs of different payloads and signs, and a window with more than half NaN."""
    rng = np.random.default_rng([seed, shape[0], shape[1], shape[2], np.dtype(dtype).itemsize])
    n, rows, cols = shape
    if dtype == np.uint16:
        a = rng.integers(0, 65536, shape).astype(np.uint16)
        flat = a.reshape(-1)
        flat[::5] = 0
        flat[1::5] = 65535
        flat[2::5] = 32768
        flat[3::5] = 32767
        if n > 1:
            a[-1] = rng.integers(0, 4, (rows, cols))
        return a
    a = (rng.standard_normal(shape) * 1000).astype(np.float32)
    flat = a.reshape(-1)
    flat[::7] = -0.0
    flat[1::7] = 0.0
    flat[3::11] = np.inf
    flat[5::13] = -np.inf
    flat[2::9] = NANS[np.arange(flat[2::9].size) % NANS.size]
    a[0, :min(rows, 3), :min(cols, 3)] = NANS[1]                     # nine NaNs: every window that holds five of them has a NaN median
    a[0, 1, 1] = NANS[2]
    return a


def pick_dif(a, size, two_sided, start):
    """The first of start * 1.01^j whose margin on the model is at least MARGIN (the decisions then do not hinge on a rounding)."""
    dif = float(np.float32(start))
    d = om.distance(a, size, two_sided)[1]
    for _ in range(200):
        if om.dif_margin(d, dif) >= MARGIN:
            return dif
        dif = float(np.float32(dif * 1.01))
    raise AssertionError("no dif with a margin near %r" % start)


def gpu(ctx, pre, a, mode, size, dif=0.0, two_sided=False, in_place=False, budget=None):
    """(bits of the result, counts or None) of a device-to-device call; every buffer is freed."""
    d = ctx.to_device(a, a.dtype)
    out = d if in_place else None
    try:
        if mode == om.MEDIAN:
            r, c = pre.median_filter(d, size=size, out=out, max_scratch_bytes=budget), None
        else:
            r, c = pre.remove_outlier(d, dif, size=size, two_sided=two_sided, out=out, max_scratch_bytes=budget, return_count=True)
        assert isinstance(r, _lib.DeviceArray) and r.dtype == a.dtype and r.shape == a.shape and (r is d) == in_place
        host = r.download()
    finally:
        d.free()
        if not in_place:
            r.free()
    return om.bits(host), c


SHAPES = [(3, 9, 13), (2, 33, 70), (1, 67, 131)]
CASES = [(s, size) for size in (3, 5, 7) for s in [(1, size, size)] + SHAPES]


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("shape, size", CASES)
def test_equals_the_model_bit_for_bit(ctx, pre, shape, size, dtype):
    a = make_frames(shape, dtype)
    mid = 20000.0 if dtype == np.uint16 else 700.0
    got, _ = gpu(ctx, pre, a, om.MEDIAN, size)
    assert np.array_equal(got, om.bits(om.median_filter(a, size)))
    for two_sided in (False, True):
        for dif in (0.0, pick_dif(a, size, two_sided, mid), np.inf):
            margin = om.dif_margin(om.distance(a, size, two_sided)[1], dif)
            assert margin >= MARGIN, (dif, margin)
            ref, ref_count = om.remove_outlier(a, dif, size, two_sided)
            got, count = gpu(ctx, pre, a, om.OUTLIER, size, dif, two_sided)
            assert np.array_equal(got, om.bits(ref)), (dif, two_sided)
            assert count.dtype == np.int64 and np.array_equal(count, ref_count), (dif, two_sided, count, ref_count)
            if dif == np.inf and dtype == np.uint16:
                assert not count.any() and np.array_equal(got, a)


@pytest.mark.parametrize("size", [3, 5, 7])
def test_uint16_difference_equal_to_dif_replaces(ctx, pre, size):
    """uint16 differences are exact: a pixel exactly dif above (below) its median is replaced, one count less is kept."""
    a = np.full((2, 2 * size, 2 * size + 1), 1000, np.uint16)
    a[0, size, size], a[0, 1, 1] = 1000 + 4321, 1000 + 4320
    a[1, size, size], a[1, 0, 2 * size] = 1000 - 321, 65535
    for dif, two_sided in ((4321.0, False), (321.0, True), (64535.0, False)):
        ref, ref_count = om.remove_outlier(a, dif, size, two_sided)
        got, count = gpu(ctx, pre, a, om.OUTLIER, size, dif, two_sided)
        assert np.array_equal(got, ref) and np.array_equal(count, ref_count)
    assert list(om.remove_outlier(a, 4321.0, size)[1]) == [1, 1] and list(om.remove_outlier(a, 321.0, size, True)[1]) == [2, 2]
    assert list(om.remove_outlier(a, 64535.0, size)[1]) == [0, 1]


def test_more_frames_than_the_grid_spans(ctx, pre):
    a = make_frames((65537, 3, 3), np.uint16)
    ref, ref_count = om.remove_outlier(a, 20000.0, 3)
    got, count = gpu(ctx, pre, a, om.OUTLIER, 3, 20000.0)
    assert np.array_equal(got, ref) and np.array_equal(count, ref_count)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
def test_in_place_and_batched_equal_out_of_place(ctx, pre, dtype):
    shape, size = (3, 33, 70), 5
    a = make_frames(shape, dtype)
    frame_bytes = shape[1] * shape[2] * np.dtype(dtype).itemsize
    code = _prep_lib.U16 if dtype == np.uint16 else _prep_lib.F32
    assert [_prep_lib.outlier_batch(33, 70, code, 3, b) for b in (0, frame_bytes, 2 * frame_bytes + 1)] == [3, 1, 2]
    dif = pick_dif(a, size, True, 500.0)
    for mode in (om.OUTLIER, om.MEDIAN):
        ref, ref_count = gpu(ctx, pre, a, mode, size, dif, True)
        assert np.array_equal(ref, om.bits(om.apply(a, size, mode, dif, True)[0]))
        whole, whole_count = gpu(ctx, pre, a, mode, size, dif, True, in_place=True, budget=0)
        assert np.array_equal(whole, ref)
        for budget in (frame_bytes, 2 * frame_bytes + 1):                # batches of 1 and of 2 frames on n = 3
            got, count = gpu(ctx, pre, a, mode, size, dif, True, in_place=True, budget=budget)
            assert np.array_equal(got, whole)
            if mode == om.OUTLIER:
                assert np.array_equal(count, ref_count) and np.array_equal(whole_count, ref_count)


def test_host_and_device_conventions_and_no_leaks(ctx, pre):
    a = make_frames((2, 33, 70), np.float32)
    ref, ref_count = om.remove_outlier(a, np.inf, 3)
    before = len(ctx._arrays)
    host, count = pre.remove_outlier(a, np.inf, return_count=True)                       # numpy in, numpy out
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and np.array_equal(om.bits(host), om.bits(ref))
    assert np.array_equal(count, ref_count) and len(ctx._arrays) == before
    img = pre.median_filter(a[1], size=5)                                                # one 2-D image
    assert img.shape == a[1].shape and np.array_equal(om.bits(img), om.bits(om.median_filter(a[1], 5)))
    assert np.array_equal(om.bits(preprocess.median_filter(a, size=7, ctx=ctx)), om.bits(om.median_filter(a, 7)))
    assert np.array_equal(om.bits(preprocess.remove_outlier(a, 0.0, two_sided=True, ctx=ctx)), om.bits(om.remove_outlier(a, 0.0, 3, True)[0]))
    assert len(ctx._arrays) == before
    d = ctx.to_device(a, np.float32)
    o = ctx.zeros(a.shape, np.float32)
    r = pre.remove_outlier(d, np.inf, out=o)                 # device in, device out, enqueued on the context's stream: the download,
    assert r is o                                            # which that stream orders behind it, sees the result
    assert np.array_equal(om.bits(o.download()), om.bits(ref)) and np.array_equal(om.bits(d.download()), om.bits(a))
    with pytest.raises(ValueError, match="overlap"):
        pre.median_filter(d, out=_shifted(d))
    d.free()
    o.free()
    del d, o, r
    assert len(ctx._arrays) == before


def _shifted(d):
    """A DeviceArray of d's size that starts one value into d: partial overlap."""
    v = d.view(0, d.size)
    v.ptr = type(d.ptr)(d.ptr.value + d.dtype.itemsize)
    v.shape = d.shape
    return v


def test_bad_arguments_fail_in_the_library_without_launching(ctx, pre):
    a = make_frames((2, 9, 13), np.uint16)
    d, o = ctx.to_device(a, np.uint16), ctx.zeros(a.shape, np.uint16)
    pre.median_filter(d, out=d)                               # makes the handle
    ref = d.download()
    st, h = ctx.stream(), pre.handle
    good = dict(dtype=_prep_lib.U16, n=2, rows=9, cols=13, size=3, mode=_prep_lib.OUTLIER, dif=1.0)
    bad = [dict(dtype=2), dict(mode=2), dict(size=4), dict(size=9), dict(size=1), dict(rows=2), dict(cols=2), dict(n=0), dict(dif=-1.0),
           dict(dif=float("nan")), dict(rows=1 << 16, cols=1 << 15), dict(rows=9, size=7, cols=6)]
    for kw in bad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(TomoError, match="tomo_prep_outlier"):
            h.outlier(st, d.ptr, o.ptr, **args)
    with pytest.raises(TomoError, match="overlap"):
        h.outlier(st, d.ptr, d.ptr.value + 2, **good)
    with pytest.raises(TomoError, match="NULL"):
        h.outlier(st, d.ptr, None, **good)
    ctx.sync()
    assert not o.download().any() and np.array_equal(d.download(), ref)
    h.outlier(st, d.ptr, o.ptr, **dict(good, mode=_prep_lib.MEDIAN2D, dif=float("nan")))      # MEDIAN2D ignores dif
    assert np.array_equal(o.download(), om.median_filter(ref, 3))
    d.free()
    o.free()


def test_median_mode_counts_the_pixels_whose_bits_changed(ctx, pre):
    a = make_frames((3, 9, 13), np.float32)
    ref, ref_count = om.apply(a, 3, om.MEDIAN)
    d, o, c = ctx.to_device(a, np.float32), ctx.empty(a.shape, np.float32), ctx.to_device(np.full(3, 77, np.uint32), np.uint32)
    pre._ready(d)
    pre.handle.outlier(ctx.stream(), d.ptr, o.ptr, _prep_lib.F32, 3, 9, 13, 3, _prep_lib.MEDIAN2D, d_count=c.ptr)
    assert np.array_equal(om.bits(o.download()), om.bits(ref))
    assert np.array_equal(c.download(), ref_count) and ref_count.sum() > np.isnan(a).sum()       # the call cleared the 77s first
    for b in (d, o, c):
        b.free()


SEED = 16         # of the end-to-end data, picked by om.removes_exactly_the_zingers at the pipeline's window (3), which the test asserts.
#                   The object is a Shepp-Logan phantom with sharp rims, not the smooth object the threshold of 3000 counts was chosen
#                   on (tests/test_outlier.py): at 32 pixels a rim pixel can differ from its 3 x 3 median by more than that.  Of the
#                   seeds 0 ... 31 the check holds for 13, 16, 19 and 23 (16 with the widest gap: the largest d of a clean pixel is 2798,
#                   the smallest of a zinger 5593); at a window of 5 it holds for none (23 - 60 clean pixels lie 3000 above their median).


@pytest.fixture(scope="module")
def raw32():
    """(clean, data): generate_data.make at 32^3 x 24 angles without and with 4 zingers per frame, same seed."""
    return generate_data.make(32, 24, seed=SEED, raw=True), generate_data.make(32, 24, seed=SEED, raw=True, zingers=4)


def test_end_to_end_zingers_are_removed_exactly(ctx, pre, raw32):
    clean, data = raw32
    mask = data["zinger_mask"]
    assert np.array_equal(data["counts"] != clean["counts"], mask)
    assert om.removes_exactly_the_zingers(clean, data, 3000.0, 3)     # what SEED was picked by
    out = om.remove_outlier(data["counts"], 3000.0, 3)[0]
    got, count = pre.remove_outlier(data["counts"], 3000.0, return_count=True)
    assert np.array_equal(got != data["counts"], mask) and np.all(count == 4)
    assert np.array_equal(got, out)

    p_clean = ex_pre.run(clean, ctx=ctx)["projections"]
    p_left = ex_pre.run(data, ctx=ctx)["projections"]
    removed = ex_pre.run(data, ctx=ctx, zinger_dif=3000)
    assert "zinger_mask" not in removed and "counts" not in removed
    p_removed = removed["projections"]
    e_left, e_removed = float(np.abs(p_left - p_clean).sum()), float(np.abs(p_removed - p_clean).sum())
    print("L1 error of the projections against the zinger-free run: %.6g with the zingers left in, %.6g with them removed" % (e_left, e_removed))
    assert e_removed < e_left

    # without zinger_dif the calls are the earlier ones: normalize, then the sorting pass
    sino = pre.normalize(clean["counts"], clean["flats"], clean["darks"])
    earlier = (pre.remove_stripe_sorting(sino, size=21) / np.float32(clean["mu"])).astype(np.float32)
    assert np.array_equal(p_clean, earlier)
    assert np.array_equal(ex_pre.run(clean, ctx=ctx, zinger_dif=None, zinger_size=5)["projections"], p_clean)
