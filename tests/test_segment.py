"""segment without a GPU: the model of tests/seg_model.py against scipy.ndimage.label (the yardstick's own check), otsu_threshold against
the brute force, the argument checks of every public function and check_shape.  Every test prints what it measured."""
import numpy as np
import pytest

import seg_model as sm

from tomography_alignment_amd import _seg_lib, postprocess, segment


# -------------------------------------------------------------------------------------------------------------------- the yardstick

@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_the_models_labels_are_scipys(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(3, connectivity)
    masks = []
    for shape in ((7, 9, 11), (1, 1, 13), (4, 1, 6), (9, 10, 12)):
        for p in (0.05, 0.3116, 0.6):
            for seed in range(3):
                masks.append(("bernoulli %g seed %d %s" % (p, seed, shape), sm.bernoulli(shape, p, seed)))
        masks += [("%s %s" % (name, shape), m) for name, m in sm.structured(shape).items()]
    masks += [("%s pair %d" % (kind, i), m) for i, (kind, m) in enumerate(sm.pairs_at_corner((5, 5, 5), (2, 2, 2)))]
    total = 0
    for name, m in masks:
        ref, n_ref = ndimage.label(m, structure)
        got, n = sm.label(m, connectivity)
        assert n == n_ref and got.dtype == np.int32 and np.array_equal(got, ref), name
        total += n
    print("connectivity %d: %d masks, %d components in all, labels and counts equal scipy's" % (connectivity, len(masks), total))


def test_the_patterns_separate_the_connectivities():
    shape = (9, 10, 13)
    n = {name: [sm.label(m, c)[1] for c in (1, 2, 3)] for name, m in sm.structured(shape).items()}
    print(n)
    ones = int(sm.checkerboard(shape).sum())
    assert n["checkerboard"] == [ones, 1, 1]                         # same-coloured cells share edges: one component from 18 neighbours on
    lattice = int(sm.even_lattice(shape).sum())
    assert n["even lattice"] == [lattice, lattice, lattice]
    assert n["serpentine"] == [1, 1, 1] and n["serpentine cut"] == [2, 2, 2]
    assert abs(sm.serpentine(shape).mean() - 0.25) < 0.08
    rods_apart = n["rods x apart"][0]
    assert rods_apart == 5 * 7 and n["rods x apart"] == [rods_apart] * 3 and n["rods x"] == [1, 1, 1] and n["rods z"] == [1, 1, 1]
    assert n["nested u"][0] > 1 and len(set(n["nested u"])) == 1
    for kind, m in sm.pairs_at_corner((5, 5, 5), (2, 2, 2)):
        assert [sm.label(m, c)[1] for c in (1, 2, 3)] == ([2, 1, 1] if kind == "edge" else [2, 2, 1])


# ----------------------------------------------------------------------------------------------------------------------------- otsu

def _hist(counts, lo=0.0, hi=1.0):
    return postprocess.Histogram(np.asarray(counts, np.uint64), 0, 0, 0, lo, hi)


def test_otsu_threshold_is_the_brute_force():
    rng = np.random.default_rng(0)
    x = np.arange(64)
    two = (1000 * np.exp(-0.5 * ((x - 14) / 4.0) ** 2) + 600 * np.exp(-0.5 * ((x - 45) / 6.0) ** 2)).astype(np.int64) + rng.integers(0, 5, 64)
    three = two + (800 * np.exp(-0.5 * ((x - 30) / 2.0) ** 2)).astype(np.int64)
    for name, c in (("two peaks", two), ("three peaks", three), ("random", rng.integers(0, 1000, 64)), ("sparse", rng.integers(0, 2, 64) * 7)):
        h = _hist(c, -2.0, 5.0)
        for classes in (2, 3):
            got, ref = segment.otsu_threshold(h, classes), sm.otsu(c, h.edges, classes)
            print("%s, %d classes: thresholds %s, brute force %s" % (name, classes, got, ref))
            assert got == ref and len(got) == classes - 1 and all(t.dtype == np.float32 for t in got)
    t, = segment.otsu_threshold(_hist(two, -2.0, 5.0))
    assert h.edges[14] < t < h.edges[46]
    a, b = segment.otsu_threshold(_hist(three, -2.0, 5.0), 3)
    assert h.edges[14] < a < h.edges[31] and h.edges[30] < b < h.edges[46]
    big = _hist(rng.integers(0, 2 ** 31, 4096))                      # more than any volume holds: still exact integers behind the floats
    assert segment.otsu_threshold(big) == sm.otsu(big.counts, big.edges)
    assert len(segment.otsu_threshold(big, 3)) == 3 - 1


def test_otsu_ties_go_to_the_first_maximum_and_under_over_are_ignored():
    flat = _hist(np.full(8, 5))
    assert segment.otsu_threshold(flat) == sm.otsu(flat.counts, flat.edges) == (np.float32(flat.edges[4]),)
    sym = _hist([3, 0, 0, 3])                                         # the cuts after bins 0, 1 and 2 are equally good: the first
    assert segment.otsu_threshold(sym) == (np.float32(sym.edges[1]),)
    assert segment.otsu_threshold(_hist([3, 0, 0, 3, 0, 0, 3]), 3) == sm.otsu([3, 0, 0, 3, 0, 0, 3], _hist([0] * 7).edges, 3)
    h = postprocess.Histogram(np.array([1, 5, 0, 0, 9, 2], np.uint64), 10 ** 6, 10 ** 7, 5, 0.0, 6.0)
    assert segment.otsu_threshold(h) == segment.otsu_threshold(_hist([1, 5, 0, 0, 9, 2], 0.0, 6.0))
    print("flat: %s; symmetric: %s" % (segment.otsu_threshold(flat), segment.otsu_threshold(sym)))


def test_otsu_refusals():
    with pytest.raises(ValueError, match="classes must be 2 or 3"):
        segment.otsu_threshold(_hist([1, 2, 3, 4]), 4)
    with pytest.raises(ValueError, match="classes must be 2 or 3"):
        segment.otsu_threshold(_hist([1, 2, 3, 4]), 1)
    with pytest.raises(ValueError, match="empty"):
        segment.otsu_threshold(_hist(np.zeros(16)))
    with pytest.raises(ValueError, match="at least 3 bins"):
        segment.otsu_threshold(_hist([4, 4]), 3)
    with pytest.raises(ValueError, match="classes must be 2 or 3"):
        segment.Segmenter().otsu(np.zeros((2, 2, 2), np.float32), classes=4)


# ----------------------------------------------------------------------------------------------------------------- argument checks

def test_arguments_are_checked_before_a_device_is_needed():
    v = np.zeros((3, 4, 5), np.float32)
    m = np.zeros((3, 4, 5), np.uint8)
    lab = np.zeros((3, 4, 5), np.int32)
    bad = [
        ("threshold: no bound", lambda: segment.threshold(v)),
        ("threshold: dtype", lambda: segment.threshold(v.astype(np.float64), lo=0.0)),
        ("threshold: rank", lambda: segment.threshold(v[0], lo=0.0)),
        ("threshold: NaN bound", lambda: segment.threshold(v, lo=float("nan"))),
        ("threshold: infinite bound", lambda: segment.threshold(v, hi=float("inf"))),
        ("threshold: region", lambda: segment.threshold(v, lo=0.0, region="sphere")),
        ("threshold: out dtype", lambda: segment.threshold(v, lo=0.0, out=np.zeros(v.shape, np.int32))),
        ("threshold: out size", lambda: segment.threshold(v, lo=0.0, out=np.zeros((3, 4, 4), np.uint8))),
        ("label: dtype", lambda: segment.label(lab)),
        ("label: rank", lambda: segment.label(m.ravel())),
        ("label: connectivity 0", lambda: segment.label(m, 0)),
        ("label: connectivity 4", lambda: segment.label(m, 4)),
        ("label: connectivity True", lambda: segment.label(m, True)),
        ("label: out dtype", lambda: segment.label(m, out=np.zeros(m.shape, np.int64))),
        ("measure: dtype", lambda: segment.measure(m, 1)),
        ("measure: rank", lambda: segment.measure(lab[0], 1)),
        ("measure: n", lambda: segment.measure(lab, -1)),
        ("measure: vol shape", lambda: segment.measure(lab, 1, np.zeros((3, 5, 4), np.float32))),
        ("measure: vol dtype", lambda: segment.measure(lab, 1, np.zeros((3, 4, 5), np.float64))),
        ("remove_small: dtype", lambda: segment.remove_small(m, 1, 2)),
        ("remove_small: min_size", lambda: segment.remove_small(lab, 1, -2)),
        ("remove_small: n", lambda: segment.remove_small(lab, 1.5, 2)),
        ("remove_small: out", lambda: segment.remove_small(lab, 1, 2, out=np.zeros((3, 4, 5), np.uint8))),
        ("largest: dtype", lambda: segment.largest(v, 1)),
        ("largest: rank", lambda: segment.largest(lab.ravel(), 1)),
        ("otsu: dtype", lambda: segment.Segmenter().otsu(lab)),
    ]
    for name, call in bad:
        with pytest.raises(ValueError):
            call()
        print("%s: ValueError" % name)
    c = segment.measure(lab, 0, v)                                   # no component: empty tables, no device needed
    assert c.n == 0 and c.count.shape == (0,) and c.bbox.shape == (0, 6) and c.coord_sum.shape == (0, 3) and c.centroid.shape == (0, 3)
    assert c.min.shape == c.max.shape == c.sum.shape == (0,) and c.sum.dtype == np.float64 and c.table() == []
    assert segment.measure(lab, 0).min is None


def test_check_shape_needs_no_device():
    for shape in ((1, 1, 2 ** 31 - 1), (16384, 16384, 7), (2047, 1024, 1024), (1, 1, 1)):
        segment.check_shape(*shape)
    for shape in ((2048, 1024, 1024), (1, 1, 2 ** 31), (16385, 1, 1), (1, 16385, 1), (0, 4, 4), (16384, 16384, 8)):
        with pytest.raises(segment.SegUnsupported, match="nothing was launched"):
            segment.check_shape(*shape)
    assert issubclass(segment.SegUnsupported, _seg_lib.TomoError) and _seg_lib.ERR_UNSUPPORTED == 4
    print("2^31 voxels refused, 2^31 - 1 accepted")
    assert _seg_lib.measure_passes(0, True) == 0 and _seg_lib.measure_passes(1000, True) == 1
    assert _seg_lib.measure_passes(1000, False, 56 * 100) == 10 and _seg_lib.measure_passes(1000, True, 72 * 100) == 10
    assert _seg_lib.measure_passes(7, True, 1) == 7                  # never less than one component a pass


def test_the_front_ends_tile_is_the_bindings():
    assert (_seg_lib.TILE_X, _seg_lib.TILE_Y, _seg_lib.TILE_Z) == segment.TILE
