"""morphology without a GPU: the model of tests/morph_model.py against the brute force over all background voxels and against
scipy.ndimage (distance_transform_edt, binary_erosion for both border values, binary_dilation, binary_opening, binary_closing,
binary_fill_holes), the argument checks of every public function, check_shape and ball_r2.  Every test prints what it measured."""
import numpy as np
import pytest

import morph_model as mm

from tomography_alignment_amd import _morph_lib, morphology

BORDERS = ("ignore", "background")


def _cases():
    out = []
    for shape in ((1, 1, 1), (1, 1, 7), (5, 1, 1), (4, 1, 6), (5, 6, 7), (7, 9, 11)):
        for p in (0.5, 0.8, 0.95):
            for seed in range(2):
                out.append(("bernoulli %g seed %d %s" % (p, seed, shape), mm.bernoulli(shape, p, seed)))
        out += [("%s %s" % (name, shape), m) for name, m in mm.masks(shape).items()]
    return out


CASES = _cases()


# -------------------------------------------------------------------------------------------------------------------- the yardstick

def test_the_model_is_the_brute_force():
    n = 0
    for shape in ((1, 1, 1), (1, 1, 7), (5, 1, 1), (3, 4, 5), (5, 6, 7)):
        for name, m in list(mm.masks(shape).items()) + [("bernoulli 0.7", mm.bernoulli(shape, 0.7, 3))]:
            for border in BORDERS:
                assert np.array_equal(mm.distance_sq(m, border), mm.brute_distance_sq(m, border)), (shape, name, border)
                n += 1
            for r2 in (0, 1, 3, 5, 9):
                for bv in (0, 1):
                    assert np.array_equal(mm.erode(m, r2, bv), mm.brute_erode(m, r2, bv)), (shape, name, r2, bv)
    ones = np.ones((3, 4, 5), np.uint8)
    assert (mm.distance_sq(ones) == mm.INF).all() and np.isposinf(mm.distance(ones)).all()
    assert mm.distance_sq(ones, "background").max() == 4 and mm.distance_sq(ones, "background")[0, 0, 0] == 1
    print("%d transforms equal the brute force over all background voxels; erosion equals the ball's integer test" % n)


def test_the_models_distances_are_scipys():
    ndimage = pytest.importorskip("scipy.ndimage")
    worst = 0
    for name, m in CASES:
        if not (m == 0).any():
            continue                                                       # scipy has no answer without background
        edt = ndimage.distance_transform_edt(m)
        d2 = mm.distance_sq(m, "ignore")
        assert np.array_equal(np.rint(edt * edt).astype(np.int64), d2), name
        assert np.array_equal(edt.astype(np.float32).view(np.uint32), mm.distance(m, "ignore").view(np.uint32)), name
        worst = max(worst, int(d2.max()))
    print("%d masks: rint(edt^2) and float32(edt) equal the model's, largest squared distance %d" % (len(CASES), worst))


def test_the_models_morphology_is_scipys():
    ndimage = pytest.importorskip("scipy.ndimage")
    n = 0
    for name, m in CASES:
        b = m != 0
        for r2 in mm.R2:
            s = mm.ball(r2)
            for bv in (0, 1):
                assert np.array_equal(mm.erode(m, r2, bv), ndimage.binary_erosion(b, s, border_value=bv)), (name, r2, bv)
            assert np.array_equal(mm.dilate(m, r2), ndimage.binary_dilation(b, s)), (name, r2)
            assert np.array_equal(mm.open_(m, r2), ndimage.binary_opening(b, s)), (name, r2)
            assert np.array_equal(mm.close_(m, r2), ndimage.binary_closing(b, s)), (name, r2)
            n += 5
    print("%d comparisons with binary_erosion / dilation / opening / closing over r2 in %s: equal" % (n, mm.R2))


def test_the_models_fill_is_scipys():
    ndimage = pytest.importorskip("scipy.ndimage")
    cases = CASES + [("nested shells", mm.nested_shells((9, 10, 11))), ("corner hole", mm.corner_hole((5, 6, 7))),
                     ("shells in a thin volume", mm.nested_shells((3, 9, 9)))]
    filled = 0
    for name, m in cases:
        got, count = mm.fill_holes(m)
        ref = ndimage.binary_fill_holes(m)
        assert np.array_equal(got, ref) and count == int(ref.sum()) - int((m != 0).sum()), name
        filled += count
    corner, count = mm.fill_holes(mm.corner_hole((5, 6, 7)))
    assert corner[1, 1, 1] == 1 and corner[0, 0, 0] == 0 and corner[1, 3, 3] == 0 and count == 1 + 6
    print("%d masks, %d voxels filled in all: equal binary_fill_holes" % (len(cases), filled))


# ----------------------------------------------------------------------------------------------------------------- argument checks

def test_ball_r2():
    assert [morphology.ball_r2(r) for r in (0, 1, 1.5, 2, np.sqrt(2), np.sqrt(3), 2.9999, 16383)] == [0, 1, 2, 4, 2, 2, 8, 16383 ** 2]
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            morphology.ball_r2(bad)


def test_arguments_are_checked_before_a_device_is_needed():
    m = np.zeros((3, 4, 5), np.uint8)
    bad = [
        ("distance_sq: dtype", lambda: morphology.distance_sq(m.astype(np.int32))),
        ("distance_sq: rank", lambda: morphology.distance_sq(m.ravel())),
        ("distance_sq: shape", lambda: morphology.distance_sq(m, shape=(3, 4, 6))),
        ("distance_sq: border", lambda: morphology.distance_sq(m, "reflect")),
        ("distance_sq: out dtype", lambda: morphology.distance_sq(m, out=np.zeros(m.shape, np.float32))),
        ("distance_sq: out size", lambda: morphology.distance_sq(m, out=np.zeros((3, 4, 4), np.int32))),
        ("distance: dtype", lambda: morphology.distance(m.astype(np.float32))),
        ("distance: border", lambda: morphology.distance(m, None)),
        ("distance: out dtype", lambda: morphology.distance(m, out=np.zeros(m.shape, np.int32))),
        ("erode: dtype", lambda: morphology.erode(m.astype(np.int8), 1)),
        ("erode: r2 negative", lambda: morphology.erode(m, -1)),
        ("erode: r2 fraction", lambda: morphology.erode(m, 1.5)),
        ("erode: r2 bool", lambda: morphology.erode(m, True)),
        ("erode: border_value", lambda: morphology.erode(m, 1, 2)),
        ("erode: out dtype", lambda: morphology.erode(m, 1, out=np.zeros(m.shape, np.int32))),
        ("dilate: rank", lambda: morphology.dilate(m[0], 1)),
        ("dilate: r2", lambda: morphology.dilate(m, -4)),
        ("dilate: out size", lambda: morphology.dilate(m, 1, out=np.zeros((3, 4), np.uint8))),
        ("open: r2", lambda: morphology.open(m, 2.5)),
        ("open: border_value", lambda: morphology.open(m, 1, -1)),
        ("close: dtype", lambda: morphology.close(m.astype(np.float64), 1)),
        ("close: border_value", lambda: morphology.close(m, 1, 0.5)),
        ("fill_holes: dtype", lambda: morphology.fill_holes(m.astype(np.int32))),
        ("fill_holes: rank", lambda: morphology.fill_holes(m.ravel())),
        ("fill_holes: out", lambda: morphology.fill_holes(m, out=np.zeros(m.shape, np.int32))),
        ("root: dtype", lambda: morphology.Morphology().root(np.zeros(4, np.float32))),
        ("line_limit", lambda: morphology.Morphology(line_limit=-1)),
    ]
    for name, call in bad:
        with pytest.raises(ValueError):
            call()
        print("%s: ValueError" % name)


def test_check_shape_needs_no_device():
    for shape in ((1, 1, 1), (16384, 16384, 7), (2047, 1024, 1024), (1, 8191, 16384), (16384, 1, 1), (1, 1, 16384)):
        morphology.check_shape(*shape)
    for shape in ((16385, 1, 1), (1, 16385, 1), (1, 1, 16385), (2048, 1024, 1024), (16384, 16384, 8), (0, 4, 4), (4, 4, 0)):
        with pytest.raises(morphology.MorphUnsupported, match="nothing was launched"):
            morphology.check_shape(*shape)
    assert 2048 * 1024 * 1024 == 2 ** 31
    assert issubclass(morphology.MorphUnsupported, _morph_lib.TomoError) and _morph_lib.ERR_UNSUPPORTED == 4
    with pytest.raises(morphology.MorphUnsupported):
        morphology.distance_sq(np.zeros((16385, 1, 1), np.uint8))           # before a device is asked for
    print("16385 on each axis and 2^31 voxels refused, 2^31 - 2^20 accepted")


def test_no_squared_distance_reaches_the_value_of_no_background():
    assert 3 * (_morph_lib.MAX_DIM - 1) ** 2 < _morph_lib.INF == morphology.INF == 2 ** 31 - 1
