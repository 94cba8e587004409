"""postprocess on the GPU (libtomo_vol.so) against the model of tests/vol_model.py: statistics (the model's bits on exactly summable
data, within (N - 1) 2^-53 sum |v| of its correctly rounded sums on data spanning 18 decades, identical bits across repeats, handles,
host and device input and the 16-byte and 4-byte load paths), the histogram, the 8- and 16-bit codes in both orders, the mask, the
projections and the planes, all bit for bit; one volume of more than 2^31 elements; the handle's lifetime and its refusals; and, end
to end, export_stack and align_rigid.run(export=).  Every test prints the figures it measured.

The shapes are vol_model.GPU_SHAPES.  The library's transpose tile is 64 x 64 and a work-group of the elementwise kernels owns 4096
groups of four z, so (17, 1, 964) = 4097 groups crosses that by one group."""
import json
import os

import numpy as np
import pytest

import vol_model as vm

from tomography_alignment_amd import _lib, _vol_lib, postprocess
from tomography_alignment_amd.examples import align_rigid, generate_data

pytestmark = pytest.mark.gpu

SHAPES = vm.GPU_SHAPES
IDS = ["%dx%dx%d" % s for s in SHAPES]
REGIONS = [None, "cylinder", ("cylinder", 0.8)]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def pp(ctx):
    p = postprocess.PostProcessor(ctx)
    yield p
    p.close()


def _r4(region, shape):
    return postprocess.region_r4(region, shape[0], shape[1])


def _bits64(x):
    return np.float64(x).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stat_bits(s):
    return (s.n_finite, s.n_nonfinite, int(_bits32(s.min)[0]), int(_bits32(s.max)[0]), int(_bits64(s.sum)), int(_bits64(s.sumsq)))


def _integers(shape, seed, lo=-512, hi=1024):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.float32)


def _decades(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-9, 9, shape)).astype(np.float32)


def _plant(v, seed, n=5):
    """NaN, +inf and -inf at n places each."""
    v = v.copy()
    flat = v.reshape(-1)
    idx = np.random.default_rng(seed).choice(flat.size, 3 * n, replace=False)
    flat[idx[:n]], flat[idx[n:2 * n]], flat[idx[2 * n:]] = np.nan, np.inf, -np.inf
    return v


def _offset_view(ctx, p):
    """p on the device at a pointer one element past a 16-byte boundary: the 4-byte load path whatever nz is."""
    big = ctx.empty(p.size + 4, np.float32)
    v = big.view(1, p.size)
    v.upload(p)
    return big, v


# ----------------------------------------------------------------------------------------------------------------------- statistics

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_statistics_of_exactly_summable_data_are_the_models_bits(pp, shape):
    v = _integers(shape, 1)
    for region in REGIONS:
        s, m = pp.statistics(v, region), vm.statistics(v, _r4(region, shape))
        print("%s %s: n %d sum %r sumsq %r min %r max %r" % (shape, region, s.n_finite, s.sum, s.sumsq, s.min, s.max))
        assert (s.n_finite, s.n_nonfinite, s.min, s.max) == (m["n_finite"], 0, m["min"], m["max"])
        assert _bits64(s.sum) == _bits64(m["sum"]) and _bits64(s.sumsq) == _bits64(m["sumsq"])
        assert s.mean == m["sum"] / m["n_finite"] and s.min.dtype == np.float32


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_statistics_over_18_decades_with_non_finite_values(pp, shape):
    v = _plant(_decades(shape, 2), 3)
    for region in REGIONS:
        s, m = pp.statistics(v, region), vm.statistics(v, _r4(region, shape))
        n = m["n_finite"]
        bound = (n - 1) * 2.0 ** -53 * m["sumabs"]
        bound2 = (n - 1) * 2.0 ** -53 * m["sumsq"]
        e1, e2 = abs(s.sum - m["sum"]), abs(s.sumsq - m["sumsq"])
        print("%s %s: n_finite %d n_nonfinite %d; |sum - model| %.3e (bound %.3e), |sumsq - model| %.3e (bound %.3e)"
              % (shape, region, s.n_finite, s.n_nonfinite, e1, bound, e2, bound2))
        n_region = int(vm.region(shape[0], shape[1], _r4(region, shape)).sum()) * shape[2]
        assert (s.n_finite, s.n_nonfinite) == (n, m["n_nonfinite"]) and s.n_finite + s.n_nonfinite == n_region
        assert s.min == m["min"] and s.max == m["max"]
        assert e1 <= bound and e2 <= bound2
    assert pp.statistics(v).n_nonfinite == 15


def test_statistics_of_a_region_without_finite_values(pp):
    v = _integers((9, 9, 6), 4)
    inside = vm.region(9, 9, _r4(("cylinder", 0.5), (9, 9, 6)))
    v[inside] = np.nan
    v[4, 4, 0], v[4, 4, 1] = np.inf, -np.inf
    s = pp.statistics(v, ("cylinder", 0.5))
    print(s)
    assert s.n_finite == 0 and s.n_nonfinite == int(inside.sum()) * 6 and np.isnan(s.min) and np.isnan(s.max)
    assert s.sum == 0.0 and s.sumsq == 0.0 and np.isnan(s.mean) and np.isnan(s.std)
    assert pp.statistics(v).n_finite == v.size - s.n_nonfinite


@pytest.mark.parametrize("shape", [(70, 5, 130), (64, 4, 256), (17, 1, 964)], ids=["4-byte loads", "16-byte loads", "two work-groups"])
def test_statistics_bits_do_not_depend_on_the_call_the_handle_or_the_load_path(ctx, pp, shape):
    v = _plant(_decades(shape, 5), 6)
    d = ctx.to_device(v)
    big, off = _offset_view(ctx, v)
    for region in (None, "cylinder"):
        ref = _stat_bits(pp.statistics(v, region))
        with postprocess.PostProcessor(ctx) as fresh:
            others = {"repeat": pp.statistics(v, region), "fresh handle": fresh.statistics(v, region), "device input": pp.statistics(d, region),
                      "offset pointer": pp.statistics(off, region, shape=shape), "module function": postprocess.statistics(d, region)}
        for name, s in others.items():
            print("%s %s %s: %s" % (shape, region, name, "same bits" if _stat_bits(s) == ref else "DIFFERENT"))
            assert _stat_bits(s) == ref, name
    assert off.ptr.value % 16 == 4 and d.ptr.value % 16 == 0
    d.free()
    big.free()


# ------------------------------------------------------------------------------------------------------------------------ histogram

def _hist_data(shape, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.float32(-1.5), np.float32(2.25)
    levels = np.array([0.0, 0.25, 1.0], np.float32)[rng.integers(0, 3, (shape[0], shape[1], 1))] * np.ones(shape, np.float32)
    edges = np.array([lo, hi, np.nextafter(lo, np.float32(-9)), np.nextafter(hi, np.float32(9)), np.nextafter(lo, np.float32(9)),
                      np.nextafter(hi, np.float32(-9)), 0.0, 0.375], np.float32)[rng.integers(0, 8, shape)]
    return lo, hi, {"random": _plant(rng.standard_normal(shape).astype(np.float32), seed + 1, 2), "three levels": levels.astype(np.float32),
                    "at and next to the edges": edges}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_histogram_is_the_models(ctx, pp, shape):
    lo, hi, data = _hist_data(shape, 7)
    for name, v in data.items():
        d = ctx.to_device(v)
        for region in (None, "cylinder"):
            r4 = _r4(region, shape)
            n_region = int(vm.region(shape[0], shape[1], r4).sum()) * shape[2]
            for nbins in (1, 7, 256, 4096, 16384):
                h = pp.histogram(d, nbins, (lo, hi), region)
                counts, under, over, nonfinite = vm.histogram(v, lo, hi, nbins, r4)
                diff = int(np.count_nonzero(h.counts != counts))
                print("%s %s %s %d bins: %d bins differ; under %d over %d nonfinite %d of %d" % (shape, name, region, nbins, diff, h.under, h.over,
                                                                                                   h.nonfinite, n_region))
                assert h.counts.dtype == np.uint64 and h.counts.shape == (nbins,) and diff == 0
                assert (h.under, h.over, h.nonfinite) == (under, over, nonfinite)
                assert int(h.counts.sum()) + h.under + h.over + h.nonfinite == n_region
        d.free()


def test_histogram_without_a_range_takes_it_from_the_statistics(pp):
    shape = (70, 5, 130)
    v = _plant(np.random.default_rng(8).standard_normal(shape).astype(np.float32), 9)
    for region in (None, ("cylinder", 0.8)):
        r4 = _r4(region, shape)
        m = vm.statistics(v, r4)
        h = pp.histogram(v, 100, None, region)
        counts, under, over, nonfinite = vm.histogram(v, m["min"], m["max"], 100, r4)
        print("%s: range (%r, %r), %d counted, nonfinite %d" % (region, h.lo, h.hi, int(h.counts.sum()), h.nonfinite))
        assert (h.lo, h.hi) == (m["min"], m["max"]) and np.array_equal(h.counts, counts) and (h.under, h.over, h.nonfinite) == (0, 0, nonfinite)
        assert int(h.counts.sum()) == m["n_finite"] and h.edges[0] == float(h.lo) and h.edges[-1] == float(h.hi)
    flat = np.full((4, 4, 8), 3.0, np.float32)
    h = pp.histogram(flat, 16)
    assert h.lo == np.nextafter(np.float32(3), np.float32(0)) and h.hi == np.nextafter(np.float32(3), np.float32(9)) and int(h.counts.sum()) == 128
    assert np.array_equal(h.counts, vm.histogram(flat, h.lo, h.hi, 16)[0])
    with pytest.raises(ValueError):
        pp.histogram(np.full((2, 2, 2), np.nan, np.float32))


# ------------------------------------------------------------------------------------------------------------------------- quantize

def _half_data(shape, qmax, seed):
    """k + 0.5 and its float32 neighbours for k in -2 ... qmax + 2, with NaN and +-inf planted: lo = 0, hi = qmax gives s = 1."""
    rng = np.random.default_rng(seed)
    base = (rng.integers(-2, qmax + 3, shape) + 0.5).astype(np.float32)
    which = rng.integers(0, 3, shape)
    v = np.where(which == 0, base, np.where(which == 1, np.nextafter(base, np.float32(-np.inf)), np.nextafter(base, np.float32(np.inf))))
    return _plant(v.astype(np.float32), seed + 1, 2)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_quantize_is_the_models_codes(ctx, pp, shape, dtype):
    qmax = vm.QMAX[np.dtype(dtype)]
    cases = [(_half_data(shape, qmax, 10), 0.0, float(qmax)),
             (_plant(np.random.default_rng(11).uniform(-0.5, 2.0, shape).astype(np.float32), 12, 2), -0.3, 1.7)]
    for v, lo, hi in cases:
        d = ctx.to_device(v)
        for order in ("xyz", "zyx"):
            for region, fill in ((None, 0), ("cylinder", 0), (("cylinder", 0.8), 201)):
                ref = vm.quantize(v, lo, hi, dtype, order, _r4(region, shape), fill)
                d_c = pp.quantize(d, (lo, hi), dtype, order, region, fill)
                got = d_c.download()
                d_c.free()
                diff = int(np.count_nonzero(got != ref))
                print("%s %s %s window (%g, %g) region %s fill %d: %d of %d codes differ" % (shape, np.dtype(dtype).name, order, lo, hi, region, fill,
                                                                                            diff, ref.size))
                assert isinstance(d_c, _lib.DeviceArray) and got.shape == ref.shape and got.dtype == ref.dtype and diff == 0
        d.free()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
def test_quantize_into_a_given_output_aligned_or_not(ctx, pp, dtype):
    shape = (64, 4, 256)
    v = _half_data(shape, vm.QMAX[np.dtype(dtype)], 13)
    lo, hi = 0.0, float(vm.QMAX[np.dtype(dtype)])
    d = ctx.to_device(v)
    big, off = _offset_view(ctx, v)
    for order in ("xyz", "zyx"):
        ref = vm.quantize(v, lo, hi, dtype, order, _r4("cylinder", shape), 9)
        host = np.full(ref.shape, 77, dtype)
        assert pp.quantize(v, (lo, hi), dtype, order, "cylinder", 9, out=host) is host and np.array_equal(host, ref)
        d_out = ctx.empty(v.size + 16, dtype)
        for k, name in ((0, "aligned"), (1, "one code past a 16-byte boundary")):
            o = d_out.view(k, v.size)
            for src_name, src in (("aligned input", d), ("offset input", off)):
                d_out.upload(np.full(v.size + 16, 77, dtype))
                assert pp.quantize(src, (lo, hi), dtype, order, "cylinder", 9, out=o, shape=shape) is o
                got = o.download().reshape(ref.shape)
                rest = d_out.download()
                diff = int(np.count_nonzero(got != ref))
                print("%s %s output %s, %s: %d codes differ" % (np.dtype(dtype).name, order, name, src_name, diff))
                assert diff == 0 and (rest[:k] == 77).all() and (rest[k + v.size:] == 77).all()        # and nothing outside it was written
        d_out.free()
    with pytest.raises(ValueError):
        pp.quantize(d, (lo, hi), dtype, out=np.zeros(shape[::-1], dtype))          # a host output for a device volume
    d.free()
    big.free()


# ---------------------------------------------------------------------------------------------------------- mask, projections, planes

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_mask_in_place_and_out_of_place(ctx, pp, shape):
    v = _plant(_decades(shape, 14), 15, 2)
    for ratio, value in ((1.0, 0.0), (0.8, -7.5), (0.0, np.nan)):
        ref = vm.circular_mask(v, vm.r4_of(ratio, shape[0], shape[1]), value)
        host = pp.circular_mask(v, ratio, value)
        d = ctx.to_device(v)
        d_new = pp.circular_mask(d, ratio, value)
        kept = np.array_equal(_bits32(d.download()), _bits32(v))
        assert pp.circular_mask(d, ratio, value, out=d) is d
        big, off = _offset_view(ctx, v)
        pp.circular_mask(off, ratio, value, out=off, shape=shape)
        results = {"host": host, "device, new": d_new.download(), "device, in place": d.download(), "offset pointer, in place": off.download().reshape(shape)}
        for name, got in results.items():
            diff = int(np.count_nonzero(_bits32(got) != _bits32(ref)))
            print("%s ratio %g value %g %s: %d of %d voxels differ" % (shape, ratio, value, name, diff, ref.size))
            assert got.shape == ref.shape and diff == 0
        assert kept
        for a in (d, d_new, big):
            a.free()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_projections_and_planes(ctx, pp, shape):
    v = _plant(np.random.default_rng(16).standard_normal(shape).astype(np.float32), 17, 4)
    v[0, :, 0] = np.nan                                  # lines without a finite value along each axis
    v[:, 0, shape[2] - 1] = np.inf
    v[shape[0] - 1, shape[1] - 1, :] = -np.inf
    d = ctx.to_device(v)
    big, off = _offset_view(ctx, v)
    for axis in range(3):
        for op in ("max", "min"):
            ref = vm.project(v, axis, op)
            got = {"host": pp.project(v, axis, op), "device": pp.project(d, axis, op).download(),
                   "offset pointer": pp.project(off, axis, op, shape=shape).download()}
            for name, g in got.items():
                ok = g.shape == ref.shape and g.dtype == np.float32 and np.array_equal(g, ref, equal_nan=True)
                print("%s project axis %d %s %s: %s, %d NaN" % (shape, axis, op, name, "equal" if ok else "DIFFERENT", int(np.isnan(ref).sum())))
                assert ok
            assert np.isnan(ref).any()
        for index in sorted({0, shape[axis] // 2, shape[axis] - 1}):
            ref = vm.plane(v, axis, index)
            g = pp.slice(d, axis, index).download()
            assert g.shape == ref.shape and np.array_equal(_bits32(g), _bits32(ref)), (axis, index)
            assert np.array_equal(_bits32(pp.slice(v, axis, index)), _bits32(ref))
        print("%s slice axis %d: 3 planes with numpy's bits" % (shape, axis))
    d.free()
    big.free()


# ------------------------------------------------------------------------------------------------------------------- past 2^31 elements

def test_a_volume_of_more_than_2_to_the_31_elements(ctx, pp):
    nz = 2 ** 30 + 192
    shape = (2, 1, nz)
    n = 2 * nz
    planted = (np.arange(64, dtype=np.float32) * 3.0 + 1.5)                    # 1.5, 4.5, ... 190.5
    d = ctx.zeros(shape, np.float32)
    d.view(n - 64, 64).upload(planted)
    s = pp.statistics(d)
    print("n_finite %d max %r sum %r" % (s.n_finite, s.max, s.sum))
    assert s.n_finite == 2 ** 31 + 384 and s.n_nonfinite == 0 and s.max == planted.max() and s.min == 0.0
    assert s.sum == float(planted.astype(np.float64).sum()) and s.sumsq == float((planted.astype(np.float64) ** 2).sum())
    h = pp.histogram(d, 256, (0.0, 128.0))
    counts, under, over, nonfinite = vm.histogram(planted.reshape(1, 1, 64), 0.0, 128.0, 256)
    counts[0] += np.uint64(n - 64)
    print("histogram: %d counted, over %d" % (int(h.counts.sum()), h.over))
    assert int(h.counts.sum()) + h.under + h.over + h.nonfinite == n and np.array_equal(h.counts, counts) and (h.under, h.over, h.nonfinite) == (0, over, 0)
    tail = np.zeros((2, 1, 64), np.float32)                                     # the last 64 z of both rows
    tail[1, 0] = planted
    for order in ("xyz", "zyx"):
        d_c = pp.quantize(d, (0.0, 255.0), np.uint8, order)
        ref = vm.quantize(tail, 0.0, 255.0, np.uint8, order)
        if order == "xyz":
            got = d_c.view(n - 64, 64).download()
            want = ref[1, 0]
        else:
            got = d_c.view(n - 128, 128).download()                            # out[z][0][x]: the last 64 z, both x
            want = ref.reshape(-1)
        head = d_c.view(0, 4096).download()
        mid = d_c.view(nz - 64, 128).download()                                 # xyz: the end of row 0 and the start of row 1; zyx: z around nz / 2
        print("%s: %d of %d planted codes differ; %d non-zero codes in the first 4096" % (order, int(np.count_nonzero(got != want)), want.size,
                                                                                           int(np.count_nonzero(head))))
        assert d_c.shape == (shape if order == "xyz" else shape[::-1]) and d_c.dtype == np.uint8
        assert np.array_equal(got, want) and want.max() > 100 and not head.any() and not mid.any()
        d_c.free()
    d.free()


# ------------------------------------------------------------------------------------------------------------- refusals and lifetime

def test_refusals_come_before_any_launch(ctx, pp):
    v = _integers((4, 8, 12), 18)
    d = ctx.to_device(v)
    h = _vol_lib.VolHandle(ctx.device)
    st = ctx.stream()
    with pytest.raises(_vol_lib.VolUnsupported, match="nothing was launched"):
        h.stats(st, d.ptr, _vol_lib.MAX_DIM + 1, 8, 12)
    with pytest.raises(_vol_lib.VolUnsupported):
        h.quantize(st, d.ptr, 4, 0, 12, -1, 0.0, 1.0, 8, 0, 0, d.ptr)
    with pytest.raises(_lib.TomoError, match="bins are outside") as e:
        h.histogram(st, d.ptr, 4, 8, 12, -1, 0.0, 1.0, _vol_lib.MAX_BINS + 1)
    assert type(e.value) is _lib.TomoError
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(_lib.TomoError, match="finite lo < hi"):
            h.histogram(st, d.ptr, 4, 8, 12, -1, lo, hi, 16)
        with pytest.raises(_lib.TomoError, match="finite lo < hi"):
            h.quantize(st, d.ptr, 4, 8, 12, -1, lo, hi, 8, 0, 0, d.ptr)
    with pytest.raises(_lib.TomoError, match="misaligned"):
        h.stats(st, d.ptr.value + 2, 4, 8, 12)
    with pytest.raises(_lib.TomoError, match="bits must be"):
        h.quantize(st, d.ptr, 4, 8, 12, -1, 0.0, 1.0, 12, 0, 0, d.ptr)
    with pytest.raises(_lib.TomoError, match="index 12 is outside"):
        h.slice(st, d.ptr, 4, 8, 12, 2, 12, d.ptr)
    with pytest.raises(_lib.TomoError, match="no statistics were computed"):
        h.fetch_stats(st)
    with pytest.raises(_lib.TomoError, match="no histogram was computed"):
        h.fetch_histogram(st)
    assert h.device_bytes() == 0                                                    # nothing was allocated, so nothing ran
    assert h.stats(st, d.ptr, 4, 8, 12, fetch=False) is None and h.histogram(st, d.ptr, 4, 8, 12, -1, 0.0, 1024.0, 64, fetch=False) is None
    s, (counts, extra) = h.fetch_stats(st), h.fetch_histogram(st)
    m = vm.statistics(v)
    assert (s.n_finite, s.sum, s.sumsq) == (m["n_finite"], m["sum"], m["sumsq"]) and h.device_bytes() > 0
    assert np.array_equal(counts, vm.histogram(v, 0.0, 1024.0, 64)[0]) and extra == vm.histogram(v, 0.0, 1024.0, 64)[1:]
    h.close()
    assert np.array_equal(d.download(), v)
    d.free()


def test_handle_lifetime(ctx):
    h = _vol_lib.VolHandle(0)
    assert h.handle and h.device == 0
    h.close()
    h.close()
    with pytest.raises(_lib.TomoError, match="^vol handle closed$"):
        h.handle
    with pytest.raises(_lib.TomoError, match="^vol handle closed$"):
        h.stats(0, 0, 1, 1, 1)
    with _vol_lib.VolHandle(0) as h2:
        assert h2.handle
    with pytest.raises(_lib.TomoError, match="^vol handle closed$"):
        h2.handle
    with pytest.raises(_lib.TomoError, match="device out of range"):
        _vol_lib.VolHandle(10 ** 6)
    live = len(_lib.LIVE_CONTEXTS)
    p = postprocess.PostProcessor()
    v = _integers((5, 6, 7), 19)
    assert p.statistics(v).n_finite == v.size
    c, hh = p.ctx, p.handle
    assert isinstance(hh, _vol_lib.VolHandle) and c.handle and len(_lib.LIVE_CONTEXTS) == live + 1
    p.close()
    assert p.ctx is None and p.handle is None and len(_lib.LIVE_CONTEXTS) == live
    with pytest.raises(_lib.TomoError, match="handle closed"):
        hh.handle
    p.close()
    with postprocess.PostProcessor(ctx) as q:
        d = ctx.to_device(v)
        sizes = []
        for _ in range(4):
            q.statistics(d), q.histogram(d, 4096), q.quantize(d, (0.0, 1.0)).free(), q.project(d, 2).free(), q.circular_mask(d, out=d)
            sizes.append(q.device_bytes())
        print("device bytes of the handle over four rounds: %s" % sizes)
        assert sizes[0] > 0 and len(set(sizes)) == 1
        d.free()
    assert q.handle is None and q.ctx is ctx and ctx.handle


# ---------------------------------------------------------------------------------------------------------------------- end to end

FILES = sorted(["meta.json"] + ["preview_%s_axis%d.npy" % (k, a) for k in ("slice", "max") for a in range(3)])


def _check_export(directory, rec, dtype, pp):
    """The files of export_stack(rec) in `directory` against the model and against slice / project."""
    nx, ny, nz = rec.shape
    names = sorted(os.listdir(directory))
    assert names == sorted(FILES + ["slice_%05d.npy" % z for z in range(nz)])
    with open(os.path.join(directory, "meta.json")) as f:
        meta = json.load(f)
    stack = np.stack([np.load(os.path.join(directory, "slice_%05d.npy" % z)) for z in range(nz)])
    lo, hi = meta["window"]
    ref = vm.quantize(rec, lo, hi, dtype, "zyx", vm.r4_of(1.0, nx, ny), 0)
    diff = int(np.count_nonzero(stack != ref))
    s = vm.statistics(rec, vm.r4_of(1.0, nx, ny))
    print("export: window (%g, %g), %d of %d codes differ from the model, codes %d ... %d, mean %g" % (lo, hi, diff, ref.size, stack.min(), stack.max(),
                                                                                                  meta["statistics"]["mean"]))
    assert stack.shape == (nz, ny, nx) and stack.dtype == np.dtype(dtype) and diff == 0 and stack.max() > stack.min()
    assert meta["dtype"] == np.dtype(dtype).name and meta["shape"] == [nx, ny, nz] and meta["region"] == ["cylinder", 1.0]
    assert np.float32(lo) == lo and np.float32(hi) == hi and lo < hi                     # the stored window is the float32 one that was used
    assert meta["statistics"]["n_finite"] == s["n_finite"] and meta["statistics"]["min"] == float(s["min"]) and meta["statistics"]["max"] == float(s["max"])
    hm = meta["histogram"]
    assert hm["counted"] + hm["under"] + hm["over"] + hm["nonfinite"] == s["n_finite"] + s["n_nonfinite"]
    assert json.loads(json.dumps(meta)) == meta
    for a in range(3):
        assert np.array_equal(_bits32(np.load(os.path.join(directory, "preview_slice_axis%d.npy" % a))), _bits32(vm.plane(rec, a, rec.shape[a] // 2)))
        assert np.array_equal(np.load(os.path.join(directory, "preview_max_axis%d.npy" % a)), pp.project(rec, a, "max"), equal_nan=True)
        assert np.array_equal(pp.project(rec, a, "max"), vm.project(rec, a, "max"), equal_nan=True)
    return meta


def test_export_stack_of_a_reconstruction(pp, tmp_path):
    data = generate_data.make(48, 60, seed=1)
    loop = align_rigid.OuterLoop(dict(data))
    loop.reconstruct(sirt_iters=10)
    rec = loop.download()
    assert rec.shape == (48, 48, 48)
    with postprocess.PostProcessor(loop.ctx) as p:
        meta = p.export_stack(loop.d_rec, str(tmp_path / "u8"), shape=loop.vox_shape)
        meta16 = p.export_stack(rec, str(tmp_path / "u16"), dtype=np.uint16, percentiles=(1.0, 99.0), bins=1024)
    assert _check_export(str(tmp_path / "u8"), rec, np.uint8, pp) == meta
    assert _check_export(str(tmp_path / "u16"), rec, np.uint16, pp) == meta16


def test_align_rigid_exports_what_it_reconstructed(pp, tmp_path):
    data = generate_data.make(32, 24, seed=1)
    kw = dict(n_outer=1, sirt_iters=5, verbose=False)
    plain = align_rigid.run(dict(data), **kw)
    out = align_rigid.run(dict(data), export=str(tmp_path / "stack"), **kw)
    for a, b in zip(plain[:4], out[:4]):
        assert np.array_equal(a, b)
    assert len(plain) == len(out) == 5 and len(out[4]) == 1
    _check_export(str(tmp_path / "stack"), out[0], np.uint8, pp)
