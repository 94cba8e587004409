"""morphology on the GPU (libtomo_morph.so) against the model of tests/morph_model.py, bit for bit: distance_sq for both borders and
distance on every shape of morph_model.GPU_SHAPES and every mask of morph_model.masks (no background, one background voxel in each
corner, one foreground voxel, random, slabs, a checkerboard, a ball), the root on chosen integers, erode / dilate / open / close over
the r2 list and both border values, fill_holes with its count, outputs given and in place, unaligned pointers, every result again
under a line limit of 8 (the second path on every axis longer than that) with equal bytes, repeats and a second handle, one larger run
against scipy, the handle's lifetime, the refusals, and align_rigid.run(segment=True, morphology=True) end to end.  Every test prints
what it measured."""
import json
import os

import numpy as np
import pytest

import morph_model as mm
import seg_model as sm
import vol_model as vm

from tomography_alignment_amd import _lib, _morph_lib, morphology
from tomography_alignment_amd.examples import align_rigid, generate_data

pytestmark = pytest.mark.gpu

SHAPES = mm.GPU_SHAPES
IDS = ["%dx%dx%d" % s for s in SHAPES]
BORDERS = ("ignore", "background")
BALL_SHAPES = [(1, 1, 1), (1, 1, 7), (5, 1, 1), (7, 1, 3), (5, 5, 3), (3, 5, 5), (3, 5, 32), (33, 5, 3), mm.CROSSING]
BALL_MASKS = ("zeros", "ones", "one foreground voxel", "bernoulli 0.9", "slabs", "ball")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def mo(ctx):
    m = morphology.Morphology(ctx)
    yield m
    m.close()


@pytest.fixture(scope="module")
def mo8(ctx):
    m = morphology.Morphology(ctx, line_limit=8)
    yield m
    m.close()


_D2 = {}


def _d2(shape, name, mask, border, inverse=False):
    """The model's distance_sq, computed once per mask and handed out read-only."""
    key = (shape, name, border, inverse)
    if key not in _D2:
        d = mm.distance_sq(mask == 0 if inverse else mask, border)
        d.setflags(write=False)
        _D2[key] = d
    return _D2[key]


def _offset(ctx, a):
    """a on the device one element past a 16-byte boundary (one byte for uint8): the guarded single accesses whatever nz is."""
    big = ctx.empty(a.size + 16, a.dtype)
    v = big.view(1, a.size)
    v.upload(a)
    return big, v


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _take(d, shape):
    h = d.download().reshape(shape)
    d.free()
    return h


# ------------------------------------------------------------------------------------------------------------------------ distances

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_distances_are_the_models(ctx, mo, mo8, shape):
    wrong = top = 0
    masks = mm.masks(shape)
    for name, m in masks.items():
        d = ctx.to_device(m, np.uint8)
        for border in BORDERS:
            ref = _d2(shape, name, m, border)
            got = _take(mo.distance_sq(d, border), shape)
            got8 = _take(mo8.distance_sq(d, border), shape)
            root = _take(mo.distance(d, border), shape)
            root8 = _take(mo8.distance(d, border), shape)
            bad = int(np.count_nonzero(got != ref)) + int(np.count_nonzero(_bits(root) != _bits(mm.root(ref))))
            wrong += bad
            top = max(top, int(ref[ref < mm.INF].max(initial=0)))
            assert got.dtype == np.int32 and root.dtype == np.float32 and bad == 0, (name, border)
            assert got8.tobytes() == got.tobytes() and root8.tobytes() == root.tobytes(), (name, border, "line limit 8")
        d.free()
    ones = masks["ones"]
    assert (mo.distance_sq(ones) == mm.INF).all() and np.isposinf(mo.distance(ones)).all()               # host in, host out
    assert int(mo.distance_sq(ones, "background").max()) == ((min(shape) + 1) // 2) ** 2
    print("%s: %d masks x 2 borders, distance_sq and distance on both paths: %d voxels differ, largest finite d2 %d" % (shape, len(masks), wrong, top))


def test_distances_through_unaligned_pointers_and_into_given_outputs(ctx, mo, mo8):
    for shape in ((5, 6, 8), mm.CROSSING):
        m = mm.bernoulli(shape, 0.9, 5)
        big, off = _offset(ctx, m)
        d = ctx.to_device(m.astype(bool), np.bool_)                        # a bool mask
        for border in BORDERS:
            ref = _d2(shape, "bernoulli 0.9 seed 5", m, border)
            for who in (mo, mo8):
                assert np.array_equal(_take(who.distance_sq(off, border, shape=shape), shape), ref)
                assert np.array_equal(_take(who.distance_sq(d, border), shape), ref)
                for dtype, call, want in ((np.int32, who.distance_sq, ref), (np.float32, who.distance, mm.root(ref))):
                    d_out = ctx.empty(m.size + 16, dtype)
                    for k in (0, 1):
                        d_out.upload(np.full(m.size + 16, 77, dtype))
                        o = d_out.view(k, m.size)
                        assert call(d, border, out=o, shape=shape) is o
                        rest = d_out.download()
                        diff = int(np.count_nonzero(rest[k:k + m.size].reshape(shape).view(np.uint32) != want.view(np.uint32)))
                        print("%s %s %s into an output %d elements past a 16-byte boundary: %d differ" % (shape, border, np.dtype(dtype).name, k, diff))
                        assert diff == 0 and (rest[:k] == 77).all() and (rest[k + m.size:] == 77).all()
                    d_out.free()
            host = np.full(shape, 7, np.int32)
            assert mo.distance_sq(m, border, out=host) is host and np.array_equal(host, ref)
        assert np.array_equal(morphology.distance_sq(d, "background").download(), _d2(shape, "bernoulli 0.9 seed 5", m, "background"))
        with pytest.raises(ValueError):
            mo.distance_sq(d, out=np.zeros(shape, np.int32))              # a host output for a device mask
        big.free(), d.free()


def test_the_passes_alone_chain_to_the_transform(ctx, mo, mo8):
    shape = mm.CROSSING
    m = mm.bernoulli(shape, 0.9, 5)
    d, d_a, d_b = ctx.to_device(m, np.uint8), ctx.empty(shape, np.int32), ctx.empty(shape, np.int32)
    for border in (0, 1):
        ref = _d2(shape, "bernoulli 0.9 seed 5", m, BORDERS[border])
        mo._ready(d), mo8._ready(d)
        mo.handle.line_pass(ctx.stream(), d.ptr, *shape, 2, border, d_a.ptr)
        mo.handle.line_pass(ctx.stream(), d_a.ptr, *shape, 1, border, d_a.ptr)        # in place
        mo.handle.line_pass(ctx.stream(), d_a.ptr, *shape, 0, border, d_b.ptr)
        assert np.array_equal(d_b.download(), ref)
        mo8.handle.line_pass(ctx.stream(), d.ptr, *shape, 2, border, d_a.ptr)
        with pytest.raises(_lib.TomoError, match="cannot run in place"):
            mo8.handle.line_pass(ctx.stream(), d_a.ptr, *shape, 1, border, d_a.ptr)
        mo8.handle.line_pass(ctx.stream(), d_a.ptr, *shape, 1, border, d_b.ptr)
        mo8.handle.line_pass(ctx.stream(), d_b.ptr, *shape, 0, border, d_a.ptr)
        assert np.array_equal(d_a.download(), ref)
    with pytest.raises(_lib.TomoError, match="axis must be"):
        mo.handle.line_pass(ctx.stream(), d.ptr, *shape, 3, 0, d_a.ptr)
    d.free(), d_a.free(), d_b.free()
    print("z, y, x alone, in place and into a second buffer, on both paths: the transform")


def test_the_root_is_correctly_rounded(ctx, mo):
    k = np.unique(np.concatenate([np.arange(1, 4097), np.arange(4097, 28378, 13), [28377, 16383, 16384, 23170]])).astype(np.int64)
    chosen = np.concatenate([[0, 1, 2, 3, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 3 * 16383 ** 2, mm.INF - 1, mm.INF], k * k, k * k - 1, k * k + 1])
    assert chosen.max() <= mm.INF and chosen.min() >= 0 and 28376 ** 2 < 3 * 16383 ** 2 < 28377 ** 2
    d2 = chosen.astype(np.int32)
    ref = mm.root(d2)
    got = mo.root(d2)
    d = ctx.to_device(d2, np.int32)
    dev = mo.root(d)
    f = ctx.empty(d2.shape, np.float32)
    mo.handle.root(ctx.stream(), d.ptr, d.size, f.ptr)
    diff = int(np.count_nonzero(_bits(got) != _bits(ref))) + int(np.count_nonzero(_bits(dev.download()) != _bits(ref)))
    diff += int(np.count_nonzero(_bits(f.download()) != _bits(ref)))
    print("%d integers up to 2^31 - 1 (k^2, k^2 +- 1 for k up to 28377, 2^24 +- 1, 3 * 16383^2, INF): %d roots differ from float32(sqrt(float64))"
          % (d2.size, diff))
    assert diff == 0 and np.isposinf(got[d2 == mm.INF]).all() and got[0] == 0
    mo.handle.root(ctx.stream(), d.ptr, d.size, d.ptr)                    # in place
    assert np.array_equal(d.download().view(np.uint32), _bits(ref))
    d.free(), dev.free(), f.free()


# ------------------------------------------------------------------------------------------------------------------------- the ball

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_erosion_and_dilation_are_the_models(ctx, mo, mo8, shape):
    wrong = calls = 0
    for name, m in mm.masks(shape).items():
        d = ctx.to_device(m, np.uint8)
        inv = _d2(shape, name, m, "ignore", inverse=True)
        for r2 in mm.R2:
            for who in (mo, mo8):
                for bv in (0, 1):
                    ref = (_d2(shape, name, m, "ignore" if bv else "background") > r2).astype(np.uint8)
                    got = _take(who.erode(d, r2, bv), shape)
                    wrong += int(np.count_nonzero(got != ref))
                    assert got.dtype == np.uint8 and np.array_equal(got, ref), (name, r2, bv)
                got = _take(who.dilate(d, r2), shape)
                wrong += int(np.count_nonzero(got != (inv <= r2)))
                assert np.array_equal(got, (inv <= r2).astype(np.uint8)), (name, r2)
                calls += 3
        d.free()
    print("%s: %d erosions and dilations over r2 in %s, both border values, both paths: %d voxels differ" % (shape, calls, mm.R2, wrong))


@pytest.mark.parametrize("shape", BALL_SHAPES, ids=["%dx%dx%d" % s for s in BALL_SHAPES])
def test_opening_and_closing_are_the_models(ctx, mo, mo8, shape):
    calls = 0
    masks = mm.masks(shape)
    for name in BALL_MASKS:
        m = masks[name]
        d = ctx.to_device(m, np.uint8)
        for r2 in mm.R2:
            for bv in (0, 1):
                ref_o, ref_c = mm.open_(m, r2, bv), mm.close_(m, r2, bv)
                for who in (mo, mo8):
                    assert np.array_equal(_take(who.open(d, r2, bv), shape), ref_o), (name, r2, bv, "open")
                    assert np.array_equal(_take(who.close_ball(d, r2, bv), shape), ref_c), (name, r2, bv, "close")
                    calls += 2
        d.free()
    m = masks["slabs"]
    assert np.array_equal(morphology.open(m, 2), mm.open_(m, 2)) and np.array_equal(morphology.close(m, 2, 1), mm.close_(m, 2, 1))
    print("%s: %d openings and closings over r2 in %s, both border values, both paths: equal the model's" % (shape, calls, mm.R2))


def test_the_ball_in_place_through_unaligned_pointers_and_huge_r2(ctx, mo, mo8):
    shape = mm.CROSSING
    m = mm.masks(shape)["bernoulli 0.99"]
    m200 = (m * 200).astype(np.uint8)                                      # any non-zero byte is foreground
    for who in (mo, mo8):
        for call, ref in ((lambda a, **k: who.erode(a, 5, 0, **k), mm.erode(m, 5, 0)), (lambda a, **k: who.erode(a, 5, 1, **k), mm.erode(m, 5, 1)),
                          (lambda a, **k: who.dilate(a, 5, **k), mm.dilate(m, 5)), (lambda a, **k: who.open(a, 5, **k), mm.open_(m, 5)),
                          (lambda a, **k: who.close_ball(a, 5, 1, **k), mm.close_(m, 5, 1))):
            d = ctx.to_device(m200, np.uint8)
            assert call(d, out=d) is d and np.array_equal(d.download(), ref)                             # in place
            big, off = _offset(ctx, m200)
            assert call(off, out=off, shape=shape) is off and np.array_equal(off.download().reshape(shape), ref)
            host = m200.copy()
            assert call(host, out=host) is host and np.array_equal(host, ref)
            assert np.array_equal(call(m.astype(bool)), ref)
            d.free(), big.free()
    ones = np.ones((5, 6, 7), np.uint8)
    for r2 in (3 * 16383 ** 2, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 40):
        assert mo.erode(ones, r2, 1).all() and not mo.erode(ones, r2, 0).any()      # no background anywhere is farther than every r2
        assert not mo.dilate(np.zeros((5, 6, 7), np.uint8), r2).any()
        one = np.zeros((5, 6, 7), np.uint8)
        one[2, 3, 4] = 1
        assert mo.dilate(one, r2).all()
    print("in place, one byte past a 16-byte boundary, host in place, bool masks; r2 up to 2^40: equal the model's")


# --------------------------------------------------------------------------------------------------------------------- hole filling

def test_fill_holes_is_the_models(ctx, mo):
    cases = [("nested shells", mm.nested_shells((9, 10, 11))), ("nested shells, crossing", mm.nested_shells(mm.CROSSING)),
             ("corner hole", mm.corner_hole((5, 6, 7))), ("no holes: a ball", mm.solid_ball((5, 6, 7))),
             ("no background", np.ones((3, 4, 5), np.uint8)), ("no foreground", np.zeros((3, 4, 5), np.uint8)),
             ("bernoulli 0.9", mm.bernoulli(mm.CROSSING, 0.9, 3)), ("one voxel", np.ones((1, 1, 1), np.uint8))]
    for name, m in cases:
        ref, count = mm.fill_holes(m)
        m200 = (m * 200).astype(np.uint8)
        got, n = mo.fill_holes(m200, return_count=True)
        d = ctx.to_device(m200, np.uint8)
        d_got, d_n = mo.fill_holes(d, return_count=True)
        print("%s %s: %d voxels filled, the model %d" % (name, m.shape, n, count))
        assert got.dtype == np.uint8 and np.array_equal(got, ref) and n == d_n == count
        assert np.array_equal(d_got.download(), ref) and np.array_equal(d.download(), m200)
        assert mo.fill_holes(d, out=d) is d and np.array_equal(d.download(), ref)                       # in place
        big, off = _offset(ctx, m200)
        assert np.array_equal(_take(mo.fill_holes(off, shape=m.shape), m.shape), ref)
        d.free(), d_got.free(), big.free()
    assert mm.fill_holes(cases[3][1])[1] == 0 and mm.fill_holes(cases[2][1])[1] == 7 and mm.fill_holes(cases[0][1])[1] > 100
    assert np.array_equal(morphology.fill_holes(cases[2][1]), mm.fill_holes(cases[2][1])[0])
    labels = np.array([0, 1, 2, 3, -1, 4, 2 ** 31 - 1, 2], np.int32)      # select skips labels outside 0 ... n
    d_l, d_t, d_m = ctx.to_device(labels, np.int32), ctx.to_device(np.array([0, 1, 0, 1], np.uint8), np.uint8), ctx.to_device(np.full(8, 9, np.uint8), np.uint8)
    mo.handle.select(ctx.stream(), d_l.ptr, 8, 3, d_t.ptr, d_m.ptr)
    assert d_m.download().tolist() == [9, 1, 9, 1, 9, 9, 9, 9]
    d_l.free(), d_t.free(), d_m.free()


# ---------------------------------------------------------------------------------------------------------- determinism, scipy, lifetime

def test_results_do_not_depend_on_the_run_or_the_handle(ctx, mo):
    shape = mm.CROSSING
    m = mm.bernoulli(shape, 0.9, 9)
    d = ctx.to_device(m, np.uint8)
    with morphology.Morphology(ctx) as other:
        first = None
        for who, runs in ((mo, 10), (other, 1)):
            for _ in range(runs):
                got = (_take(who.distance_sq(d, "background"), shape).tobytes(), _take(who.distance(d), shape).tobytes(),
                       _take(who.open(d, 3), shape).tobytes(), _take(who.fill_holes(d), shape).tobytes())
                first = first or got
                assert got == first
    d.free()
    print("ten runs on one handle and one on a second: equal bytes")


def test_a_larger_volume_against_scipy(ctx, mo):
    ndimage = pytest.importorskip("scipy.ndimage")
    shape = (96, 80, 112)
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    m = ((np.sin(x / 7.0) + np.sin(y / 5.0) + np.sin(z / 9.0) > -0.4) & (np.random.default_rng(2).random(shape) < 0.999)).astype(np.uint8)
    edt = ndimage.distance_transform_edt(m)
    d = ctx.to_device(m, np.uint8)
    d2 = _take(mo.distance_sq(d), shape)
    dist = _take(mo.distance(d), shape)
    print("%s, %.1f %% foreground: largest distance %.3f, scipy's %.3f" % (shape, 100.0 * m.mean(), float(dist.max()), float(edt.max())))
    assert np.array_equal(d2, np.rint(edt * edt).astype(np.int64)) and np.array_equal(_bits(dist), _bits(edt.astype(np.float32)))
    s = mm.ball(12)
    assert np.array_equal(_take(mo.erode(d, 12), shape), ndimage.binary_erosion(m, s))
    assert np.array_equal(_take(mo.erode(d, 12, 1), shape), ndimage.binary_erosion(m, s, border_value=1))
    assert np.array_equal(_take(mo.dilate(d, 12), shape), ndimage.binary_dilation(m, s))
    assert np.array_equal(_take(mo.open(d, 12), shape), ndimage.binary_opening(m, s))
    assert np.array_equal(_take(mo.close_ball(d, 12), shape), ndimage.binary_closing(m, s))
    filled, n = mo.fill_holes(d, return_count=True)
    ref = ndimage.binary_fill_holes(m)
    assert np.array_equal(_take(filled, shape), ref) and n == int(ref.sum()) - int(m.sum())
    d.free()


def test_handle_lifetime_and_refusals(ctx):
    h = _morph_lib.MorphHandle(ctx.device)
    st = ctx.stream()
    m = mm.bernoulli((4, 8, 12), 0.8, 23)
    d_m, d_o, d_b = ctx.to_device(m, np.uint8), ctx.empty(m.shape, np.int32), ctx.to_device(m, np.uint8)
    idle = h.device_bytes()
    with pytest.raises(_morph_lib.MorphUnsupported, match="nothing was launched"):
        h.distance_sq(st, d_m.ptr, _morph_lib.MAX_DIM + 1, 8, 12, 0, d_o.ptr)
    with pytest.raises(_morph_lib.MorphUnsupported, match="nothing was launched"):
        h.erode(st, d_m.ptr, 4, 8, _morph_lib.MAX_DIM + 1, 1, 0, d_b.ptr)
    with pytest.raises(_morph_lib.MorphUnsupported, match="2\\^31 - 1 voxels"):
        h.dilate(st, d_m.ptr, 2048, 1024, 1024, 1, d_b.ptr)
    with pytest.raises(_lib.TomoError, match="border must be"):
        h.distance_sq(st, d_m.ptr, 4, 8, 12, 2, d_o.ptr)
    with pytest.raises(_lib.TomoError, match="misaligned"):
        h.distance_sq(st, d_m.ptr, 4, 8, 12, 0, d_o.ptr.value + 2)
    with pytest.raises(_lib.TomoError, match="r2 must be"):
        h.open(st, d_m.ptr, 4, 8, 12, -1, 0, d_b.ptr)
    with pytest.raises(_lib.TomoError, match="border_value must be"):
        h.close_ball(st, d_m.ptr, 4, 8, 12, 1, 2, d_b.ptr)
    with pytest.raises(_lib.TomoError, match="NULL pointer"):
        h.distance(st, d_m.ptr, 4, 8, 12, 0, 0)
    with pytest.raises(_lib.TomoError, match="limit is"):
        h.set_line_limit(_morph_lib.LINE_LIMIT + 1)
    assert h.device_bytes() == idle == 0 and np.array_equal(d_b.download(), m)      # nothing was allocated, so nothing ran
    with pytest.raises(ValueError):
        morphology.Morphology(ctx).distance_sq(d_o)                                  # a device array of the wrong dtype
    with pytest.raises(ValueError):
        morphology.Morphology(ctx).erode(d_m, 1, shape=(4, 8, 11))                   # ... and of the wrong size
    h.distance_sq(st, d_m.ptr, 4, 8, 12, 0, d_o.ptr)
    in_output = h.device_bytes()
    h.erode(st, d_m.ptr, 4, 8, 12, 2, 0, d_b.ptr)
    small = h.device_bytes()
    assert np.array_equal(d_o.download(), mm.distance_sq(m)) and np.array_equal(d_b.download(), mm.erode(m, 2))
    assert in_output == 0 and small == 4 * m.size <= _morph_lib.KEEP_BYTES           # one int32 volume, kept
    shape = (64, 64, 1100)                                                           # one int32 volume of it is more than the handle keeps
    big = np.ones(shape, np.uint8)
    big[10, 20, 30] = 0
    d_big = ctx.to_device(big, np.uint8)
    h.dilate(st, d_big.ptr, 64, 64, 1100, 1, d_big.ptr)
    after = h.device_bytes()
    print("idle %d bytes, after distance_sq %d, after a small erosion %d, after a dilation of %s (%d bytes of scratch) %d"
          % (idle, in_output, small, shape, 4 * big.size, after))
    assert 4 * big.size > _morph_lib.KEEP_BYTES and after == idle and int(d_big.download().sum()) == big.size
    h.close()
    h.close()
    with pytest.raises(_lib.TomoError, match="^morph handle closed$"):
        h.distance_sq(st, d_m.ptr, 4, 8, 12, 0, d_o.ptr)
    with pytest.raises(_lib.TomoError, match="^morph handle closed$"):
        h.device_bytes()
    with pytest.raises(_lib.TomoError, match="device out of range"):
        _morph_lib.MorphHandle(10 ** 6)
    live = len(_lib.LIVE_CONTEXTS)
    s = morphology.Morphology()
    assert np.array_equal(s.fill_holes(m), mm.fill_holes(m)[0]) and isinstance(s.handle, _morph_lib.MorphHandle)
    assert len(_lib.LIVE_CONTEXTS) == live + 1
    s.close()
    assert s.ctx is None and s.handle is None and s._seg is None and len(_lib.LIVE_CONTEXTS) == live
    for a in (d_m, d_o, d_b, d_big):
        a.free()


# ----------------------------------------------------------------------------------------------------------------------- end to end

def _model_mask(rec):
    nx, ny, nz = rec.shape
    r4 = vm.r4_of(1.0, nx, ny)
    s = vm.statistics(rec, r4)
    counts = vm.histogram(rec, s["min"], s["max"], 4096, r4)[0]
    edges = float(s["min"]) + (float(s["max"]) - float(s["min"])) * np.arange(4097, dtype=np.float64) / 4096
    t, = sm.otsu(counts, edges)
    return sm.threshold(rec, t, None, r4)


def test_align_rigid_measures_the_mask_it_segmented(tmp_path):
    data = generate_data.make(32, 24, seed=1)
    kw = dict(n_outer=1, sirt_iters=5, verbose=False, segment=True)
    plain = align_rigid.run(dict(data), export=str(tmp_path / "plain"), **kw)
    out = align_rigid.run(dict(data), export=str(tmp_path / "morph"), morphology=True, **kw)
    for a, b in zip(plain[:4], out[:4]):
        assert np.array_equal(a, b)
    assert sorted(os.listdir(str(tmp_path / "morph"))) == sorted(os.listdir(str(tmp_path / "plain")))
    got, before = dict(out[4][-1]["segmentation"]), plain[4][-1]["segmentation"]
    mask = _model_mask(out[0])
    fg, filled = int(mask.sum()), mm.fill_holes(mask)[1]
    ref = {"max_inscribed_radius": float(mm.distance(mask, "background").max()), "closed_porosity": filled / float(fg + filled) if fg else 0.0}
    print("morphology %s; model %s (%d voxels of foreground, %d filled)" % ({k: got[k] for k in ref}, ref, fg, filled))
    assert {k: got.pop(k) for k in sorted(ref)} == ref and got == before and fg > 0 and ref["max_inscribed_radius"] >= 1.0
    with open(str(tmp_path / "morph" / "labels_meta.json")) as f:
        meta = json.load(f)
    with open(str(tmp_path / "plain" / "labels_meta.json")) as f:
        meta_plain = json.load(f)
    assert {k: meta.pop(k) for k in sorted(ref)} == ref and meta == meta_plain
    with pytest.raises(ValueError, match="goes with segment"):
        align_rigid.run(dict(data), n_outer=1, sirt_iters=1, verbose=False, morphology=True)
