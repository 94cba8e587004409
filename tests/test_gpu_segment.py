"""segment on the GPU (libtomo_seg.so) against the model of tests/seg_model.py, bit for bit: the threshold (both load paths, every
region, non-finite values and values on the bounds), the labels for the three connectivities on every shape of seg_model.GPU_SHAPES
(trivial, random, the patterns that separate the connectivities, the ones that force long chains and late merges, pairs of voxels at
every position around a brick corner), their determinism, one larger run against scipy, the measures (the float64 sum within
(count - 1) 2^-53 sum |v| of the correctly rounded one, everything else exact, also under a budget that forces several passes),
remove_small and largest, the handle's lifetime, and align_rigid.run(segment=True) end to end.  Every test prints what it measured.

The shapes sit one below, at and one above every edge of the library's brick (seg_model.GPU_SHAPES)."""
import json
import os

import numpy as np
import pytest

import seg_model as sm
import vol_model as vm

from tomography_alignment_amd import _lib, _seg_lib, postprocess, segment
from tomography_alignment_amd.examples import align_rigid, generate_data

pytestmark = pytest.mark.gpu

SHAPES = sm.GPU_SHAPES
IDS = ["%dx%dx%d" % s for s in SHAPES]
REGIONS = [None, "cylinder", ("cylinder", 0.8)]
CONN = [1, 2, 3]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def seg(ctx):
    s = segment.Segmenter(ctx)
    yield s
    s.close()


_REFS = {}


def _ref(name, mask, connectivity):
    """The model's labels, computed once per mask and connectivity and handed out read-only."""
    key = (name, mask.shape, connectivity)
    if key not in _REFS:
        lab, n = sm.label(mask, connectivity)
        lab.setflags(write=False)
        _REFS[key] = (lab, n)
    return _REFS[key]


def _r4(region, shape):
    return postprocess.region_r4(region, shape[0], shape[1])


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _plant(v, seed, n=5):
    """NaN, +inf and -inf at up to n places each."""
    v = v.copy()
    flat = v.reshape(-1)
    n = min(n, flat.size // 3)
    idx = np.random.default_rng(seed).choice(flat.size, 3 * n, replace=False)
    flat[idx[:n]], flat[idx[n:2 * n]], flat[idx[2 * n:]] = np.nan, np.inf, -np.inf
    return v


def _offset(ctx, a):
    """a on the device one element past a 16-byte boundary (one byte for uint8): the guarded single accesses whatever nz is."""
    big = ctx.empty(a.size + 16, a.dtype)
    v = big.view(1, a.size)
    v.upload(a)
    return big, v


def _masks(shape):
    out = dict(sm.structured(shape))
    for p in (0.05, 0.3116, 0.6):
        out["bernoulli %g" % p] = sm.bernoulli(shape, p, 11)
    return out


# ------------------------------------------------------------------------------------------------------------------------ threshold

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_threshold_is_the_models_mask(ctx, seg, shape):
    rng = np.random.default_rng(1)
    lo, hi = np.float32(-3.0), np.float32(40.0)
    ints = rng.integers(-8, 48, shape).astype(np.float32)
    ints.reshape(-1)[::5] = lo
    ints.reshape(-1)[2::7] = hi
    decades = (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-9, 9, shape)).astype(np.float32)
    decades.reshape(-1)[::3] = np.nextafter(lo, np.float32(-np.inf))
    decades.reshape(-1)[1::4] = np.nextafter(hi, np.float32(np.inf))
    for name, v in (("integers", _plant(ints, 2)), ("18 decades", _plant(decades, 3))):
        d = ctx.to_device(v)
        big, off = _offset(ctx, v)
        for region in REGIONS:
            for a, b in ((lo, hi), (lo, None), (None, hi)):
                ref = sm.threshold(v, a, b, _r4(region, shape))
                host = seg.threshold(v, a, b, region)
                d_m = seg.threshold(d, a, b, region)
                d_o = seg.threshold(off, a, b, region, shape=shape)
                got = {"host": host, "device": d_m.download(), "offset pointer": d_o.download().reshape(shape)}
                for how, g in got.items():
                    diff = int(np.count_nonzero(g != ref))
                    print("%s %s region %s bounds (%s, %s) %s: %d of %d differ, %d set" % (shape, name, region, a, b, how, diff, ref.size, int(ref.sum())))
                    assert g.dtype == np.uint8 and g.shape == ref.shape and diff == 0
                assert isinstance(d_m, _lib.DeviceArray) and d_m.shape == shape
                d_m.free(), d_o.free()
        d.free(), big.free()


def test_threshold_into_a_given_output(ctx, seg):
    shape = (sm.TX + 1, 5, 64)
    v = _plant(np.random.default_rng(4).standard_normal(shape).astype(np.float32), 5)
    ref = sm.threshold(v, -0.5, 0.75, _r4("cylinder", shape))
    host = np.full(shape, 77, np.uint8)
    assert seg.threshold(v, -0.5, 0.75, "cylinder", out=host) is host and np.array_equal(host, ref)
    d = ctx.to_device(v)
    d_out = ctx.empty(v.size + 16, np.uint8)
    for k, name in ((0, "aligned"), (1, "one byte past a 16-byte boundary")):
        d_out.upload(np.full(v.size + 16, 77, np.uint8))
        o = d_out.view(k, v.size)
        assert seg.threshold(d, -0.5, 0.75, "cylinder", out=o, shape=shape) is o
        rest = d_out.download()
        diff = int(np.count_nonzero(rest[k:k + v.size].reshape(shape) != ref))
        print("output %s: %d bytes differ" % (name, diff))
        assert diff == 0 and (rest[:k] == 77).all() and (rest[k + v.size:] == 77).all()
    assert np.array_equal(segment.threshold(d, lo=0.0).download(), sm.threshold(v, 0.0))          # the module function, a handle of its own
    with pytest.raises(ValueError):
        seg.threshold(d, lo=0.0, out=np.zeros(shape, np.uint8))          # a host output for a device volume
    d.free(), d_out.free()


# --------------------------------------------------------------------------------------------------------------------------- labels

@pytest.mark.parametrize("connectivity", CONN)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_labels_are_the_models(ctx, seg, shape, connectivity):
    for name, m in _masks(shape).items():
        ref, n_ref = _ref(name, m, connectivity)
        lab, n = seg.label(m, connectivity)
        diff = int(np.count_nonzero(lab != ref))
        print("%s connectivity %d %s: n %d (model %d), %d of %d labels differ, %d foreground" % (shape, connectivity, name, n, n_ref, diff, ref.size,
                                                                                           int(m.sum())))
        assert lab.dtype == np.int32 and lab.shape == shape and n == n_ref and diff == 0
    assert _ref("zeros", np.zeros(shape, np.uint8), connectivity)[1] == 0 and _ref("ones", np.ones(shape, np.uint8), connectivity)[1] == 1


@pytest.mark.parametrize("connectivity", CONN)
def test_labels_of_a_bool_mask_an_offset_pointer_and_a_given_output(ctx, seg, connectivity):
    shape = sm.CROSSING[:2] + (sm.TZ + 4,)                               # nz % 4 == 0: the 16-byte path unless the pointers say otherwise
    m = sm.bernoulli(shape, 0.3116, 12)
    ref, n_ref = _ref("bernoulli 12", m, connectivity)
    d = ctx.to_device(m, np.uint8)
    big, off = _offset(ctx, m)
    d_b = ctx.to_device(m.astype(bool), np.bool_)
    out = ctx.empty(m.size + 16, np.int32)
    host_out = np.full(shape, -5, np.int32)
    res = {"host bool": seg.label(m.astype(bool), connectivity), "host into out": seg.label(m, connectivity, out=host_out),
           "module function": segment.label(m, connectivity)}
    for name, (src, o) in {"device": (d, None), "device bool": (d_b, None), "offset mask": (off, None), "aligned out": (d, out.view(0, m.size)),
                           "offset out": (d, out.view(1, m.size)), "offset both": (off, out.view(1, m.size))}.items():
        lab, n = seg.label(src, connectivity, out=o, shape=shape)
        assert isinstance(lab, _lib.DeviceArray) and (o is None or lab is o)
        res[name] = (lab.download().reshape(shape), n)
        if o is None:
            lab.free()
    assert res["host into out"][0] is host_out
    for name, (lab, n) in res.items():
        diff = int(np.count_nonzero(lab != ref))
        print("connectivity %d %s: n %d (model %d), %d labels differ" % (connectivity, name, n, n_ref, diff))
        assert n == n_ref and diff == 0, name
    assert off.ptr.value % 16 == 1 and np.array_equal(d.download(), m)   # the mask is not written
    for a in (d, big, d_b, out):
        a.free()


@pytest.mark.parametrize("connectivity", CONN)
def test_pairs_of_voxels_around_a_brick_corner(seg, connectivity):
    shape = (sm.TX + 2, sm.TY + 2, sm.TZ + 2)
    pairs = sm.pairs_at_corner(shape, (sm.TX, sm.TY, sm.TZ))
    counts = {"edge": [], "corner": []}
    for kind, m in pairs:
        ref, n_ref = sm.label(m, connectivity)
        lab, n = seg.label(m, connectivity)
        assert n == n_ref and np.array_equal(lab, ref), (kind, np.argwhere(m).tolist())
        counts[kind].append(n)
    print("connectivity %d: %d edge pairs with n in %s, %d corner pairs with n in %s" % (connectivity, len(counts["edge"]), sorted(set(counts["edge"])),
                                                                                       len(counts["corner"]), sorted(set(counts["corner"]))))
    assert len(counts["edge"]) == 8 * 6 and len(counts["corner"]) == 8 * 4
    assert set(counts["edge"]) == {2 if connectivity == 1 else 1} and set(counts["corner"]) == {2 if connectivity < 3 else 1}


def test_labels_do_not_depend_on_the_run_or_the_handle(ctx, seg):
    m = sm.bernoulli(sm.LARGEST, 0.3116, 13)
    d = ctx.to_device(m, np.uint8)
    for connectivity in CONN:
        ref, n_ref = _ref("bernoulli 13", m, connectivity)
        runs = []
        d_l = ctx.empty(m.shape, np.int32)
        for _ in range(10):
            _, n = seg.label(d, connectivity, out=d_l)
            runs.append((n, d_l.download().tobytes()))
        with segment.Segmenter(ctx) as fresh:
            lab, n = fresh.label(m, connectivity)
            runs.append((n, lab.tobytes()))
        same = sum(1 for r in runs if r == (n_ref, ref.tobytes()))
        print("%s connectivity %d: n %d, %d of %d runs give the model's bytes" % (sm.LARGEST, connectivity, n_ref, same, len(runs)))
        assert same == len(runs)
        d_l.free()
    d.free()


@pytest.mark.parametrize("connectivity", CONN)
def test_a_larger_volume_against_scipy(ctx, seg, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    shape = (160, 160, 192)
    m = sm.bernoulli(shape, 0.3116, 14)
    ref, n_ref = ndimage.label(m, ndimage.generate_binary_structure(3, connectivity))
    lab, n = seg.label(m, connectivity)
    diff = int(np.count_nonzero(lab != ref))
    print("%s connectivity %d: n %d (scipy %d), %d of %d labels differ, largest component %d voxels" % (shape, connectivity, n, n_ref, diff, ref.size,
                                                                                                     int(np.bincount(ref.ravel())[1:].max())))
    assert n == n_ref and diff == 0


# ------------------------------------------------------------------------------------------------------------------------- measures

def _check_measure(c, ref, n, with_vol, exact_sum, what):
    assert c.n == n and c.count.dtype == np.int64 and c.bbox.dtype == np.int32 and c.coord_sum.dtype == np.int64
    assert np.array_equal(c.count, ref["count"]) and np.array_equal(c.bbox, ref["bbox"]) and np.array_equal(c.coord_sum, ref["coord_sum"]), what
    assert np.array_equal(c.centroid, ref["centroid"])
    if not with_vol:
        assert c.min is None and c.max is None and c.sum is None
        return 0.0
    assert c.min.dtype == np.float32 and c.sum.dtype == np.float64
    assert np.array_equal(_bits32(c.min), _bits32(ref["min"])) and np.array_equal(_bits32(c.max), _bits32(ref["max"])), what
    err = np.abs(c.sum - ref["sum"])
    bound = np.maximum(ref["n_finite"] - 1, 0) * 2.0 ** -53 * ref["sumabs"]
    if exact_sum:
        assert np.array_equal(c.sum.view(np.uint64), ref["sum"].view(np.uint64)), what
    assert (err <= bound).all(), what
    return float((err / np.where(bound > 0, bound, 1.0)).max()) if n else 0.0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_measures_are_the_models(ctx, seg, shape):
    rng = np.random.default_rng(15)
    ints = rng.integers(-512, 1024, shape).astype(np.float32)
    decades = _plant((rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-9, 9, shape)).astype(np.float32), 16)
    for name, m in (("bernoulli 0.3116", sm.bernoulli(shape, 0.3116, 17)), ("bernoulli 0.6", sm.bernoulli(shape, 0.6, 18)),
                    ("ones", np.ones(shape, np.uint8)), ("even lattice", sm.even_lattice(shape))):
        lab, n = sm.label(m, 1)
        assert np.array_equal(sm.measure(lab, n)["count"], np.bincount(lab.ravel(), minlength=n + 1)[1:])
        d_l = ctx.to_device(lab, np.int32)
        big, off = _offset(ctx, lab)
        for vname, v, exact in (("integers", ints, True), ("18 decades", decades, False)):
            ref = sm.measure(lab, n, v)
            d_v = ctx.to_device(v)
            worst = max(_check_measure(seg.measure(lab, n, v), ref, n, True, exact, "host"),
                        _check_measure(seg.measure(d_l, n, d_v), ref, n, True, exact, "device"),
                        _check_measure(seg.measure(off, n, d_v, shape=shape), ref, n, True, exact, "offset pointer"))
            print("%s %s n %d, vol %s: integer tables, min and max equal; |sum - fsum| at most %.3f of its bound" % (shape, name, n, vname, worst))
            d_v.free()
        _check_measure(seg.measure(d_l, n), sm.measure(lab, n), n, False, False, "no volume")
        d_l.free(), big.free()


def test_measures_skip_non_finite_values_and_take_no_components(ctx, seg):
    shape = (5, 6, 8)
    lab = np.zeros(shape, np.int32)
    lab[:1], lab[3:] = 1, 2
    v = np.arange(lab.size, dtype=np.float32).reshape(shape)
    v[:2] = np.nan                                                       # component 1 has no finite value at all
    v[3, 0, 0], v[3, 0, 1], v[4, 5, 7] = np.inf, -np.inf, np.nan
    c, ref = seg.measure(lab, 2, v), sm.measure(lab, 2, v)
    print("min %s max %s sum %s" % (c.min, c.max, c.sum))
    _check_measure(c, ref, 2, True, True, "non-finite")
    assert np.isnan(c.min[0]) and np.isnan(c.max[0]) and c.sum[0] == 0.0 and c.min[1] == v[3, 0, 2] and c.max[1] == v[4, 5, 6]
    d_l = ctx.to_device(lab, np.int32)
    e = seg.measure(d_l, 0, ctx.to_device(v))
    assert e.n == 0 and e.count.shape == (0,) and e.bbox.shape == (0, 6) and e.sum.shape == (0,)
    with pytest.raises(ValueError, match="both"):
        seg.measure(d_l, 2, v)
    assert [t["label"] for t in c.table()] == [2, 1] and c.table(1)[0]["count"] == int(ref["count"][1])


def test_measures_in_several_passes_are_the_same_integers(ctx, seg):
    shape = sm.CROSSING
    m = sm.bernoulli(shape, 0.3116, 19)
    lab, n = sm.label(m, 1)
    v = np.random.default_rng(20).integers(-512, 1024, shape).astype(np.float32)
    ref = sm.measure(lab, n, v)
    budget = 72 * 37                                                     # 37 components a pass with a volume, 47 without
    passes = _seg_lib.measure_passes(n, True, budget)
    with segment.Segmenter(ctx, max_scratch=budget) as small:
        c = small.measure(lab, n, v)
        c0 = small.measure(lab, n)
        held = small.device_bytes()
    one = seg.measure(lab, n, v)
    print("n %d: %d passes under %d bytes (the handle held %d), 1 pass by default" % (n, passes, budget, held))
    assert passes == -(-n // 37) and passes > 5 and _seg_lib.measure_passes(n, True) == 1 and held <= budget + 72
    _check_measure(c, ref, n, True, True, "several passes")
    _check_measure(c0, sm.measure(lab, n), n, False, False, "several passes, no volume")
    for a, b in ((c.count, one.count), (c.bbox, one.bbox), (c.coord_sum, one.coord_sum), (_bits32(c.min), _bits32(one.min)), (_bits32(c.max), _bits32(one.max))):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------------------------------------- remove_small and largest

@pytest.mark.parametrize("shape", [(3, 4, 5), sm.CROSSING, (5, 6, 8), sm.LARGEST], ids=["3x4x5", "crossing", "5x6x8", "largest"])
def test_remove_small_and_largest_are_the_models(ctx, seg, shape):
    for name, m in (("bernoulli 0.3116", sm.bernoulli(shape, 0.3116, 21)), ("bernoulli 0.05", sm.bernoulli(shape, 0.05, 22)),
                    ("even lattice", sm.even_lattice(shape)), ("zeros", np.zeros(shape, np.uint8))):
        lab, n = sm.label(m, 1)
        top = int(np.bincount(lab.ravel(), minlength=2)[1:].max()) if n else 0
        d_l = ctx.to_device(lab, np.int32)
        for min_size in sorted({0, 1, 2, 3, max(top, 1), top + 1}):
            ref, kept_ref = sm.remove_small(lab, n, min_size)
            host, kept = seg.remove_small(lab, n, min_size)
            d_o, kept_d = seg.remove_small(d_l, n, min_size)
            dev = d_o.download()
            d_o.free()
            print("%s %s n %d min_size %d: kept %d (model %d), %d labels differ" % (shape, name, n, min_size, kept, kept_ref,
                                                                                  int(np.count_nonzero(host != ref))))
            assert kept == kept_d == kept_ref and np.array_equal(host, ref) and np.array_equal(dev, ref) and host.dtype == np.int32
            if min_size <= 1:
                assert kept == n and np.array_equal(host, lab)
            if min_size == top + 1:
                assert kept == 0 and not host.any()
        work = lab.copy()                                                # in place, on the host and on the device
        out, kept = seg.remove_small(work, n, 2, out=work)
        assert out is work and np.array_equal(work, sm.remove_small(lab, n, 2)[0])
        d_same, kept_d = seg.remove_small(d_l, n, 2, out=d_l)
        assert d_same is d_l and kept_d == kept and np.array_equal(d_l.download(), work)
        big_m = seg.largest(lab, n)
        d_l.upload(lab)
        d_m = seg.largest(d_l, n)
        ref_m = sm.largest(lab, n)
        print("%s %s: the largest of %d components has %d voxels" % (shape, name, n, int(ref_m.sum())))
        assert big_m.dtype == np.uint8 and np.array_equal(big_m, ref_m) and np.array_equal(d_m.download(), ref_m)
        d_m.free(), d_l.free()
    tie = np.zeros((2, 3, 8), np.int32)                                  # 2 and 3 have four voxels each, 1 has three: the tie goes to 2
    tie[0, 0, :3], tie[0, 2, :4], tie[1, 1, 4:] = 1, 2, 3
    assert np.array_equal(seg.largest(tie, 3), (tie == 2).astype(np.uint8)) and np.array_equal(sm.largest(tie, 3), (tie == 2).astype(np.uint8))
    assert not seg.largest(tie, 0).any()


# ------------------------------------------------------------------------------------------------------------------ handle lifetime

def test_handle_lifetime_and_refusals(ctx):
    h = _seg_lib.SegHandle(ctx.device)
    st = ctx.stream()
    m = sm.bernoulli((4, 8, 12), 0.5, 23)
    d_m, d_l, d_v = ctx.to_device(m, np.uint8), ctx.empty(m.shape, np.int32), ctx.to_device(m.astype(np.float32))
    idle = h.device_bytes()
    with pytest.raises(_seg_lib.SegUnsupported, match="nothing was launched"):
        h.label(st, d_m.ptr, _seg_lib.MAX_DIM + 1, 8, 12, 1, d_l.ptr)
    with pytest.raises(_seg_lib.SegUnsupported, match="2\\^31 - 1 voxels"):
        h.label(st, d_m.ptr, 2048, 1024, 1024, 1, d_l.ptr)
    with pytest.raises(_lib.TomoError, match="connectivity must be"):
        h.label(st, d_m.ptr, 4, 8, 12, 4, d_l.ptr)
    with pytest.raises(_lib.TomoError, match="misaligned"):
        h.label(st, d_m.ptr, 4, 8, 12, 1, d_l.ptr.value + 2)
    with pytest.raises(_lib.TomoError, match="at least one bound"):
        h.threshold(st, d_v.ptr, 4, 8, 12, -1, None, None, d_m.ptr)
    with pytest.raises(_lib.TomoError, match="must be finite"):
        h.threshold(st, d_v.ptr, 4, 8, 12, -1, float("inf"), None, d_m.ptr)
    with pytest.raises(_lib.TomoError, match="NULL pointer"):
        h.label(st, d_m.ptr, 4, 8, 12, 1, 0)
    assert h.device_bytes() == idle == 0 and np.array_equal(d_m.download(), m)      # nothing was allocated, so nothing ran
    with pytest.raises(ValueError):
        segment.Segmenter(ctx).label(ctx.empty((4, 8, 12), np.int32))               # a device array of the wrong dtype
    with pytest.raises(ValueError):
        segment.Segmenter(ctx).label(d_m, shape=(4, 8, 11))                         # ... and of the wrong size
    with pytest.raises(ValueError):
        segment.Segmenter(ctx).measure(d_l, 1, ctx.empty((4, 8, 11), np.float32))
    n = h.label(st, d_m.ptr, 4, 8, 12, 1, d_l.ptr)
    small = h.device_bytes()
    assert n == sm.label(m, 1)[1] and 0 < small <= _seg_lib.KEEP_BYTES
    # a large call: more components than the handle keeps tables for between calls
    shape = (64, 64, 1024)
    lattice = sm.even_lattice(shape)
    d_big, d_bl = ctx.to_device(lattice, np.uint8), ctx.empty(shape, np.int32)
    nb = h.label(st, d_big.ptr, 64, 64, 1024, 3, d_bl.ptr)
    warm = h.device_bytes()                                              # the root counts of this volume: 4 bytes per 4096 voxels
    count, bbox, csum, _, _, _ = h.measure(st, d_bl.ptr, None, 64, 64, 1024, nb)
    after = h.device_bytes()
    print("idle %d bytes, after a small label %d, after a label of %s %d, after measuring %d components (%d bytes of tables) %d"
          % (idle, small, shape, warm, nb, 56 * nb, after))
    assert nb == int(lattice.sum()) == 32 * 32 * 512 and 56 * nb > _seg_lib.KEEP_BYTES and after == warm <= 8 + 4 * (lattice.size // 4096 + 1)
    assert (count == 1).all() and np.array_equal(bbox[:, 0], bbox[:, 1]) and np.array_equal(csum, np.argwhere(lattice))
    h.close()
    h.close()
    with pytest.raises(_lib.TomoError, match="^seg handle closed$"):
        h.label(st, d_m.ptr, 4, 8, 12, 1, d_l.ptr)
    with pytest.raises(_lib.TomoError, match="^seg handle closed$"):
        h.device_bytes()
    with pytest.raises(_lib.TomoError, match="device out of range"):
        _seg_lib.SegHandle(10 ** 6)
    live = len(_lib.LIVE_CONTEXTS)
    s = segment.Segmenter()
    assert s.label(m)[1] == n and s.otsu(m.astype(np.float32), bins=16) == (np.float32(1.0 / 16),)
    assert isinstance(s.handle, _seg_lib.SegHandle) and len(_lib.LIVE_CONTEXTS) == live + 1
    s.close()
    assert s.ctx is None and s.handle is None and len(_lib.LIVE_CONTEXTS) == live
    for a in (d_m, d_l, d_v, d_big, d_bl):
        a.free()


# ----------------------------------------------------------------------------------------------------------------------- end to end

def _model_segmentation(rec):
    nx, ny, nz = rec.shape
    r4 = vm.r4_of(1.0, nx, ny)
    s = vm.statistics(rec, r4)
    counts = vm.histogram(rec, s["min"], s["max"], 4096, r4)[0]
    edges = float(s["min"]) + (float(s["max"]) - float(s["min"])) * np.arange(4097, dtype=np.float64) / 4096
    t, = sm.otsu(counts, edges)
    mask = sm.threshold(rec, t, None, r4)
    lab, n = sm.label(mask, 1)
    m = sm.measure(lab, n)
    fg = int(mask.sum())
    return {"threshold": float(t), "n_components": n, "foreground_fraction": fg / float(int(vm.region(nx, ny, r4).sum()) * nz),
            "largest_fraction": float(m["count"].max()) / fg if n else 0.0}, m


def test_align_rigid_segments_what_it_reconstructed(tmp_path):
    data = generate_data.make(32, 24, seed=1)
    kw = dict(n_outer=1, sirt_iters=5, verbose=False)
    plain = align_rigid.run(dict(data), export=str(tmp_path / "plain"), **kw)
    out = align_rigid.run(dict(data), export=str(tmp_path / "seg"), segment=True, **kw)
    for a, b in zip(plain[:4], out[:4]):
        assert np.array_equal(a, b)
    assert "segmentation" not in plain[4][-1] and not os.path.exists(str(tmp_path / "plain" / "labels_meta.json"))
    assert sorted(os.listdir(str(tmp_path / "seg"))) == sorted(os.listdir(str(tmp_path / "plain")) + ["labels_meta.json"])
    got = out[4][-1]["segmentation"]
    ref, m = _model_segmentation(out[0])
    print("segmentation %s; model %s" % (got, ref))
    assert got == ref and sorted(got) == ["foreground_fraction", "largest_fraction", "n_components", "threshold"]
    with open(str(tmp_path / "seg" / "labels_meta.json")) as f:
        meta = json.load(f)
    assert {k: meta[k] for k in ref} == ref
    order = np.argsort(-m["count"], kind="stable")[:1000]
    assert [c["label"] for c in meta["components"]] == [int(k) + 1 for k in order]
    assert [c["count"] for c in meta["components"]] == [int(m["count"][k]) for k in order]
    assert [c["bbox"] for c in meta["components"]] == [[int(b) for b in m["bbox"][k]] for k in order]
    assert [c["centroid"] for c in meta["components"]] == [[float(x) for x in m["centroid"][k]] for k in order]
    no_export = align_rigid.run(dict(data), segment=True, **kw)
    assert no_export[4][-1]["segmentation"] == ref
