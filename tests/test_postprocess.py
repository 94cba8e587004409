"""postprocess without a GPU: the numpy model (tests/vol_model.py) against independent numpy, Histogram.window on hand-made counts, the
shape check of libtomo_vol.so and the argument errors that Python raises before any device use.  Needs the built library, no GPU.  Every
test prints the figures it measured."""
import ctypes

import numpy as np
import pytest

import vol_model as vm

from tomography_alignment_amd import _vol_lib, postprocess


# ------------------------------------------------------------------------------------------------------ the model against independent numpy

@pytest.mark.parametrize("nbins", [7, 100, 4096, 16384])
def test_model_histogram_is_numpys_on_integers_over_a_power_of_two(nbins):
    rng = np.random.default_rng(nbins)
    v = rng.integers(-40, 1100, (6, 7, 50)).astype(np.float32)
    lo, hi = 0.0, 1024.0
    counts, under, over, nonfinite = vm.histogram(v, lo, hi, nbins)
    ref, _ = np.histogram(v.astype(np.float64), bins=nbins, range=(lo, hi))
    diff = int(np.count_nonzero(counts != ref.astype(np.uint64)))
    print("%d bins: %d differ from np.histogram; under %d over %d" % (nbins, diff, under, over))
    assert diff == 0 and counts.dtype == np.uint64
    assert under == np.count_nonzero(v < lo) and over == np.count_nonzero(v > hi) and nonfinite == 0
    assert int(counts.sum()) + under + over + nonfinite == v.size


def test_model_histogram_counts_the_edges_and_the_non_finite():
    lo, hi = np.float32(1.0), np.float32(3.0)
    v = np.array([lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(9)), np.nan, np.inf, -np.inf, 2.0], np.float32).reshape(1, 1, 8)
    counts, under, over, nonfinite = vm.histogram(v, lo, hi, 4)
    print(counts, under, over, nonfinite)
    assert counts.tolist() == [1, 0, 1, 1] and (under, over, nonfinite) == (1, 1, 3)


def test_model_zyx_is_the_transpose():
    v = np.random.default_rng(0).uniform(-1, 2, (5, 3, 9)).astype(np.float32)
    for dt in (np.uint8, np.uint16):
        c = vm.quantize(v, 0.0, 1.0, dt, "xyz", R4=vm.r4_of(1.0, 5, 3), fill=7)
        t = vm.quantize(v, 0.0, 1.0, dt, "zyx", R4=vm.r4_of(1.0, 5, 3), fill=7)
        assert t.shape == (9, 3, 5) and t.dtype == dt and np.array_equal(t, np.transpose(c, (2, 1, 0)))


def test_model_cylinder_is_the_disc():
    n_checked = 0
    for nx, ny, ratio in [(31, 31, 1.0), (32, 32, 1.0), (20, 33, 0.9), (33, 20, 0.77), (7, 7, 0.5), (64, 64, 0.613)]:
        R4 = vm.r4_of(ratio, nx, ny)
        x = np.arange(nx, dtype=np.float64)[:, None] - (nx - 1) / 2.0
        y = np.arange(ny, dtype=np.float64)[None, :] - (ny - 1) / 2.0
        d = np.sqrt(x * x + y * y) - ratio * min(nx, ny) / 2.0
        if np.min(np.abs(d)) <= 1e-9:        # a voxel centre on the rim: the float64 disc is not defined there
            continue
        n_checked += 1
        assert np.array_equal(vm.region(nx, ny, R4), d <= 0), (nx, ny, ratio)
    print("%d shapes checked against the float64 disc" % n_checked)
    assert n_checked >= 4
    # by hand.  N = 3: centres at -1, 0, 1, radius 1.5: the corners (distance 1.414) are inside.  N = 4, ratio 1: centres at +-0.5 and
    # +-1.5, radius 2: (1.5, 1.5) is at 2.12, outside; (1.5, 0.5) at 1.58, inside.
    assert vm.r4_of(1.0, 3, 3) == 9 and vm.region(3, 3, 9).all()
    m = vm.region(4, 4, vm.r4_of(1.0, 4, 4))
    assert vm.r4_of(1.0, 4, 4) == 16 and m.sum() == 12 and not m[0, 0] and not m[3, 3] and not m[0, 3] and not m[3, 0] and m[0, 1]
    assert vm.region(4, 4, -1).all() and vm.region(3, 3, 0).sum() == 1 and vm.region(3, 3, 0)[1, 1]         # R4 = 0 on an odd width: the centre voxel alone


def test_model_rounds_half_to_even_and_maps_the_non_finite():
    v = np.array([0.5, 1.5, 2.5, 3.5, 254.5, 255.5, -0.5, np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32).reshape(1, 1, 12)
    c8 = vm.codes(v, 0.0, 255.0, np.uint8).ravel().tolist()
    c16 = vm.codes(v, 0.0, 65535.0, np.uint16).ravel().tolist()
    print(c8, c16)
    assert c8 == [0, 2, 2, 4, 254, 255, 0, 0, 255, 0, 255, 0]
    assert c16 == [0, 2, 2, 4, 254, 256, 0, 0, 65535, 0, 65535, 0]


def test_model_statistics_and_projections():
    v = np.array([[[1, np.nan, 3, -np.inf]], [[np.inf, np.nan, -2, 5]]], np.float32)
    s = vm.statistics(v)
    assert (s["n_finite"], s["n_nonfinite"], s["min"], s["max"], s["sum"], s["sumsq"]) == (4, 4, -2, 5, 7.0, 39.0)
    e = vm.statistics(np.full((1, 1, 3), np.nan, np.float32))
    assert e["n_finite"] == 0 and np.isnan(e["min"]) and np.isnan(e["max"]) and e["sum"] == 0.0 and e["sumsq"] == 0.0
    assert np.array_equal(vm.project(v, 0, "max"), np.array([[1, np.nan, 3, 5]], np.float32), equal_nan=True)
    assert np.array_equal(vm.project(v, 2, "min"), np.array([[1], [-2]], np.float32))
    assert vm.plane(v, 2, 3).shape == (2, 1)


# --------------------------------------------------------------------------------------------------------------------- Histogram.window

def _hist(counts, lo=0.0, hi=10.0):
    return postprocess.Histogram(np.array(counts, np.uint64), 0, 0, 0, lo, hi)


def test_window_on_hand_made_counts():
    h = _hist([0, 10, 80, 10, 0])                                # edges 0 2 4 6 8 10; cumulative 0 10 90 100 100
    assert np.allclose(h.edges, [0, 2, 4, 6, 8, 10]) and h.edges.dtype == np.float64
    assert h.window(0, 100) == (2.0, 8.0)                        # the first and the last bin that hold anything
    assert h.window(10, 90) == (4.0, 6.0)                        # exceeds 10: bin 2; reaches 90: bin 2
    assert h.window(5, 95) == (2.0, 8.0)
    assert h.window(9.999, 90.001) == (2.0, 8.0)
    assert h.window(50, 50) == (4.0, 6.0)
    one = _hist([0, 0, 0, 7, 0, 0, 0, 0, 0, 0])                  # all mass in one bin
    for p in [(0, 100), (0.1, 99.9), (50, 50), (0, 0), (100, 100)]:
        assert one.window(*p) == (3.0, 4.0), p
    assert _hist([0, 0]).window(1, 99) == (0.0, 10.0)            # nothing counted: the range itself
    big = _hist([2 ** 40, 1, 2 ** 40], -1.0, 2.0)
    assert big.window(0, 100) == (-1.0, 2.0) and big.window(0, 50) == (-1.0, 1.0)
    for bad in [(-1, 50), (60, 40), (0, 101)]:
        with pytest.raises(ValueError):
            h.window(*bad)


# ------------------------------------------------------------------------------------------------------------------------------ the binding

def test_the_error_class_and_the_shape_check_without_a_device():
    assert postprocess.VolUnsupported is _vol_lib.VolUnsupported and ctypes.sizeof(_vol_lib.StatsStruct) == 40
    _vol_lib.check_shape(1, 1, 1)
    _vol_lib.check_shape(_vol_lib.MAX_DIM, _vol_lib.MAX_DIM, 8)
    _vol_lib.check_shape(2, 1, 2 ** 30 + 192)
    for s in [(0, 4, 4), (4, 0, 4), (4, 4, 0), (_vol_lib.MAX_DIM + 1, 4, 4), (4, _vol_lib.MAX_DIM + 1, 4), (4, 4, _vol_lib.MAX_NZ + 1), (-3, 4, 4)]:
        with pytest.raises(_vol_lib.VolUnsupported, match=r"^libtomo_vol error 4: tomo_vol: a volume of "):
            _vol_lib.check_shape(*s)


# ------------------------------------------------------------------------------------------- argument errors, before any device use

class _NoDevice(postprocess.PostProcessor):
    def _ready(self, like):
        raise AssertionError("the device was asked for")


def test_argument_errors_come_from_python_before_any_device_use():
    p = _NoDevice()
    v = np.zeros((4, 5, 6), np.float32)
    bad = [
        lambda: p.histogram(v, range=(1.0, 1.0)),
        lambda: p.histogram(v, range=(2.0, 1.0)),
        lambda: p.histogram(v, range=(0.0, np.inf)),
        lambda: p.histogram(v, bins=0, range=(0.0, 1.0)),
        lambda: p.histogram(v, bins=postprocess.MAX_BINS + 1, range=(0.0, 1.0)),
        lambda: p.histogram(v, bins=2.5, range=(0.0, 1.0)),
        lambda: p.quantize(v, (1.0, 1.0)),
        lambda: p.quantize(v, (0.0, 1.0), dtype=np.int16),
        lambda: p.quantize(v, (0.0, 1.0), dtype=np.float32),
        lambda: p.quantize(v, (0.0, 1.0), order="yxz"),
        lambda: p.quantize(v, (0.0, 1.0), fill=256),
        lambda: p.quantize(v, (0.0, 1.0), out=np.zeros((6, 5, 4), np.uint16)),
        lambda: p.project(v, 3),
        lambda: p.project(v, 0, op="mean"),
        lambda: p.slice(v, -1, 0),
        lambda: p.slice(v, 0, 4),
        lambda: p.slice(v, 2, -1),
        lambda: p.slice(v, 1, 5),
        lambda: p.statistics(v[0]),
        lambda: p.statistics(v.astype(np.float64)),
        lambda: p.statistics(v, region="sphere"),
        lambda: p.statistics(v, region=("cylinder", -1.0)),
        lambda: p.circular_mask(v[0]),
        lambda: p.export_stack(v, "nowhere", dtype=np.int8),
        lambda: p.statistics(v.ravel(), shape=(4, 5, 7)),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
    print("%d argument errors raised without a device" % len(bad))
    with pytest.raises(_vol_lib.VolUnsupported):                 # the library's own limit, still without a device
        p.statistics(np.zeros((_vol_lib.MAX_DIM + 1, 1, 1), np.float32))
    assert postprocess.region_r4(None, 5, 7) == -1 and postprocess.region_r4("cylinder", 5, 7) == 25
    assert postprocess.region_r4(("cylinder", 0.5), 8, 9) == 16 == vm.r4_of(0.5, 8, 9)
