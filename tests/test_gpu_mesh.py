"""mesh on the GPU (libtomo_mesh.so) against the model of tests/mesh_model.py: the canonical form of the triangles bit for bit, their
number, area and volume within 1e-12 of the model's float64 sums, measure against isosurface, on every shape of mesh_model.GPU_SHAPES
under both borders and on every input (Bernoulli masks, empty and full, one voxel in each corner, a ball, the checkerboard, float noise
at a level, integer-valued floats at a level that is one of the values, voxels that are not finite); closedness of the GPU's own output;
unaligned pointers and a given out; a capacity one too small; repeats and a second handle; the scratch the handle keeps; the handle's
lifetime and the refusals; host arrays and the one-shots; and align_rigid.run(segment=True, surface=True) end to end.  Every test
prints what it measured."""
import json
import os

import numpy as np
import pytest

import mesh_model as mm

from tomography_alignment_amd import _lib, _mesh_lib, mesh
from tomography_alignment_amd.examples import align_rigid, generate_data

pytestmark = pytest.mark.gpu

SHAPES = mm.GPU_SHAPES
IDS = ["%dx%dx%d" % s for s in SHAPES]
REL = 1e-12


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def mx(ctx):
    m = mesh.MeshExtractor(ctx)
    yield m
    m.close()


def _ball_mask(shape):
    g = np.meshgrid(*[np.arange(n) - (n - 1) / 2.0 for n in shape], indexing="ij")
    r = max(1.0, 0.45 * min(max(shape), 12))
    return (sum(x * x for x in g) <= r * r).astype(np.uint8)


def inputs(shape):
    """name -> (volume, level)"""
    return {
        "bernoulli 0.1": (mm.bernoulli(shape, 0.1, 1), None), "bernoulli 0.5": (mm.bernoulli(shape, 0.5, 2), None),
        "bernoulli 0.9": (mm.bernoulli(shape, 0.9, 3), None), "zeros": (np.zeros(shape, np.uint8), None),
        "ones": (np.full(shape, 255, np.uint8), None), "corners": (mm.corners_mask(shape), None), "ball": (_ball_mask(shape), None),
        "checkerboard": (mm.checkerboard(shape), None), "noise": (mm.noise(shape, 4), 0.3), "integers": (mm.integers(shape, 5), 2.0),
        "non-finite": (mm.nonfinite(shape, 6), -0.2),
    }


_REF = {}


def _ref(shape, name, border, vol, level):
    """The model's surface in canonical form with its measures, computed once per input and handed out read-only."""
    key = (shape, name, border)
    if key not in _REF:
        t = mm.isosurface(vol, level, border)
        c = mm.canonical(t)
        c.setflags(write=False)
        _REF[key] = (c,) + mm.measures(t)
    return _REF[key]


def _close(a, b):
    return abs(a - b) <= REL * abs(b)


def _tri(s):
    """The triangles of a device Surface on the host; its array freed."""
    if s.n == 0:
        assert tuple(s.triangles.shape) == (0, 3, 3)
        s.triangles.free()
        return np.zeros((0, 3, 3), np.float32)
    t = s.triangles.download().reshape(s.n, 3, 3)
    s.triangles.free()
    return t


def _offset(ctx, a):
    """a on the device one element past a 16-byte boundary (one byte for uint8): the guarded single accesses whatever nz is."""
    big = ctx.empty(a.size + 16, a.dtype)
    v = big.view(1, a.size)
    v.upload(a)
    return big, v


# -------------------------------------------------------------------------------------------------------------------- the surface

@pytest.mark.parametrize("border", mm.BORDERS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_surface_is_the_models(ctx, mx, shape, border):
    worst_a = worst_v = 0.0
    total = 0
    for name, (vol, level) in inputs(shape).items():
        ref, area, volume = _ref(shape, name, border, vol, level)
        d = ctx.to_device(vol, vol.dtype)
        s = mx.isosurface(d, level, border)
        m = mx.measure(d, level, border)
        d.free()
        assert (s.n, s.border, s.shape) == (len(ref), border, shape) and s.level == (0.5 if level is None else float(np.float32(level)))
        assert tuple(m) == (s.n, s.area, s.volume), (name, m, s[1:])
        t = _tri(s)
        print("%s: %d triangles, area %r (model %r), volume %r (model %r)" % (name, s.n, s.area, area, s.volume, volume))
        assert np.array_equal(mm.canonical(t).view(np.uint32), ref.view(np.uint32)), name
        if border == "closed":
            assert mm.closed(t), name
        assert _close(s.area, area) and _close(s.volume, volume), (name, s.area, area, s.volume, volume)
        worst_a = max(worst_a, abs(s.area - area) / area if area else 0.0)
        worst_v = max(worst_v, abs(s.volume - volume) / abs(volume) if volume else 0.0)
        total += s.n
    print("%s %s: %d triangles in all; largest relative difference of the area %.1e, of the volume %.1e" % (shape, border, total, worst_a, worst_v))
    if border == "closed":
        assert total > 0


def test_the_checkerboard_fills_every_cell(ctx, mx):
    shape = (9, 9, 34)
    m = mm.checkerboard(shape)
    d = ctx.to_device(m, np.uint8)
    s = mx.isosurface(d, border="open")
    d.free()
    t = _tri(s)
    cells = 8 * 8 * 33
    print("checkerboard %s, open: %d triangles in %d cells" % (shape, s.n, cells))
    assert s.n == 12 * cells                                 # two triangles in each of the six tetrahedra of every cell: the most a cell has
    assert np.array_equal(mm.canonical(t), mm.canonical(mm.isosurface(m, None, "open")))


def test_unaligned_pointers_and_a_given_out(ctx, mx):
    shape = (9, 6, 36)                                       # nz a multiple of four: aligned pointers take the 16-byte path
    for vol, level in ((mm.noise(shape, 8), 0.1), (mm.bernoulli(shape, 0.5, 9), None)):
        ref, area, volume = _ref(shape, "unaligned %s" % vol.dtype, "closed", vol, level)
        d = ctx.to_device(vol, vol.dtype)
        big, v = _offset(ctx, vol.ravel())
        assert d.ptr.value % 16 == 0 and v.ptr.value % 16 == vol.dtype.itemsize
        a = mx.isosurface(d, level)
        b = mx.isosurface(v, level, shape=shape)
        ta, tb = _tri(a), _tri(b)
        assert ta.tobytes() == tb.tobytes() and (a.n, a.area, a.volume) == (b.n, b.area, b.volume)      # the same order too
        assert np.array_equal(mm.canonical(ta), ref) and _close(a.area, area) and _close(a.volume, volume)
        # a given out, itself one float past a 16-byte boundary, with room to spare behind the triangles
        room = ctx.empty(9 * (a.n + 5) + 16, np.float32)
        room.upload(np.full(room.size, -7.0, np.float32))
        out = room.view(1, 9 * (a.n + 5))
        c = mx.isosurface(d, level, out=out)
        assert c.n == a.n and tuple(c.triangles.shape) == (a.n, 3, 3) and c.triangles.ptr.value == out.ptr.value
        h = room.download()
        assert h[1:1 + 9 * a.n].tobytes() == ta.tobytes() and (h[0] == -7.0) and (h[1 + 9 * a.n:] == -7.0).all()
        with pytest.raises(mesh.MeshCapacity, match="nothing was written") as e:
            mx.isosurface(d, level, out=room.view(0, 9 * (a.n - 1)))
        assert e.value.needed == a.n and room.download().tobytes() == h.tobytes()
        for x in (d, big, room):
            x.free()
    print("aligned and unaligned volumes: equal bytes; a given out filled from its front, the rest untouched")


def test_a_capacity_one_too_small(ctx):
    shape = (9, 9, 33)
    vol = mm.bernoulli(shape, 0.5, 11)
    n = len(mm.isosurface(vol))
    d = ctx.to_device(vol, np.uint8)
    guard = 64
    buf = ctx.empty(9 * n + guard, np.float32)
    fill = np.full(buf.size, -3.0, np.float32)
    buf.upload(fill)
    st = ctx.stream()
    with _mesh_lib.MeshHandle(ctx.device) as h:
        with pytest.raises(_mesh_lib.MeshCapacity, match="the buffer holds %d; nothing was written" % (n - 1)) as e:
            h.extract(st, d.ptr, _mesh_lib.U8, shape[0], shape[1], shape[2], 0.5, 1, buf.ptr, n - 1)
        assert e.value.needed == n and isinstance(e.value, _mesh_lib.MeshUnsupported)
        assert buf.download().tobytes() == fill.tobytes()                       # nothing at all was written
        with pytest.raises(_mesh_lib.MeshCapacity):
            h.extract(st, d.ptr, _mesh_lib.U8, shape[0], shape[1], shape[2], 0.5, 1, 0, 0)
        assert h.extract(st, d.ptr, _mesh_lib.U8, shape[0], shape[1], shape[2], 0.5, 1, buf.ptr, n) == n
        got = buf.download()
        assert (got[9 * n:] == -3.0).all() and not (got[:9 * n] == -3.0).any()   # exactly n triangles, the guard behind them untouched
        assert np.array_equal(mm.canonical(got[:9 * n].reshape(n, 3, 3)), mm.canonical(mm.isosurface(vol)))
    d.free()
    buf.free()
    print("%d triangles: capacity %d refused with nothing written; capacity %d fills the buffer and leaves the %d floats behind it" % (n, n - 1, n, guard))


def test_repeats_and_a_second_handle_give_the_same_bytes(ctx, mx):
    shape = (11, 10, 37)
    other = mesh.MeshExtractor(ctx)
    for vol, level in ((mm.noise(shape, 12), 0.0), (mm.bernoulli(shape, 0.5, 13), None), (mm.integers(shape, 14), 1.0)):
        d = ctx.to_device(vol, vol.dtype)
        first = None
        for who in [mx] * 10 + [other]:
            for border in mm.BORDERS:
                s = who.isosurface(d, level, border)
                got = (border, s.n, s.area, s.volume, _tri(s).tobytes(), tuple(who.measure(d, level, border)))
                first = first or {}
                assert first.setdefault(border, got) == got
        d.free()
    other.close()
    print("ten runs on one handle and one on a second: equal numbers, equal bytes in equal order")


def test_host_arrays_and_the_one_shots(ctx):
    shape = (5, 6, 7)
    for vol, level in ((mm.noise(shape, 15), 0.2), (mm.bernoulli(shape, 0.5, 16), None), (mm.bernoulli(shape, 0.5, 16).astype(bool), None)):
        ref = mm.isosurface(vol, level)
        area, volume = mm.measures(ref)
        s = mesh.isosurface(vol, level, ctx=ctx)
        assert isinstance(s.triangles, np.ndarray) and s.triangles.shape == (s.n, 3, 3) and s.triangles.dtype == np.float32
        assert np.array_equal(mm.canonical(s.triangles), mm.canonical(ref)) and _close(s.area, area) and _close(s.volume, volume)
        assert tuple(mesh.measure(vol, level, ctx=ctx)) == (s.n, s.area, s.volume)
        out = np.full((s.n + 2, 3, 3), -1.0, np.float32)
        t = mesh.isosurface(vol, level, out=out, ctx=ctx)
        assert np.shares_memory(t.triangles, out) and t.triangles.tobytes() == s.triangles.tobytes() and (out[s.n:] == -1.0).all()
        with pytest.raises(mesh.MeshCapacity):
            mesh.isosurface(vol, level, out=np.zeros((s.n - 1, 3, 3), np.float32), ctx=ctx)
    e = mesh.isosurface(np.zeros(shape, np.uint8), ctx=ctx)
    assert e.triangles.shape == (0, 3, 3) and (e.n, e.area, e.volume) == (0, 0.0, 0.0)
    assert tuple(mesh.measure(np.ones((1, 4, 5), np.float32), 0.5, "open", ctx=ctx)) == (0, 0.0, 0.0)       # no cells at all
    d = ctx.to_device(mm.bernoulli(shape, 0.5, 17), np.uint8)
    live = len(_lib.LIVE_CONTEXTS)
    s = mesh.isosurface(d)                                                    # the device array's context
    assert len(_lib.LIVE_CONTEXTS) == live and s.triangles.ctx is ctx
    s.triangles.free()
    d.free()


# ------------------------------------------------------------------------------------------------------------------ the handle

def test_handle_lifetime_scratch_and_refusals(ctx):
    h = _mesh_lib.MeshHandle(ctx.device)
    st = ctx.stream()
    m = mm.bernoulli((4, 8, 12), 0.5, 23)
    n = len(mm.isosurface(m))
    d_m, d_t = ctx.to_device(m, np.uint8), ctx.empty((n, 3, 3), np.float32)
    d_f = ctx.to_device(m.astype(np.float32), np.float32)
    idle = h.device_bytes()
    U8, F32 = _mesh_lib.U8, _mesh_lib.F32
    with pytest.raises(_mesh_lib.MeshUnsupported, match="nothing was launched"):
        h.measure(st, d_m.ptr, U8, _mesh_lib.MAX_DIM + 1, 8, 12, 0.5, 1)
    with pytest.raises(_mesh_lib.MeshUnsupported, match="nothing was launched"):
        h.extract(st, d_m.ptr, U8, 4, 8, _mesh_lib.MAX_DIM + 1, 0.5, 1, d_t.ptr, n)
    with pytest.raises(_mesh_lib.MeshUnsupported, match="2\\^31 - 1 voxels"):
        h.measure(st, d_m.ptr, U8, 2048, 1024, 1024, 0.5, 1)
    with pytest.raises(_lib.TomoError, match="border must be"):
        h.measure(st, d_m.ptr, U8, 4, 8, 12, 0.5, 2)
    with pytest.raises(_lib.TomoError, match="dtype must be"):
        h.measure(st, d_m.ptr, 2, 4, 8, 12, 0.5, 1)
    with pytest.raises(_lib.TomoError, match="level must be finite"):
        h.measure(st, d_f.ptr, F32, 4, 8, 12, float("nan"), 1)
    with pytest.raises(_lib.TomoError, match="misaligned"):
        h.measure(st, d_f.ptr.value + 2, F32, 4, 8, 12, 0.5, 1)
    with pytest.raises(_lib.TomoError, match="misaligned"):
        h.extract(st, d_m.ptr, U8, 4, 8, 12, 0.5, 1, d_t.ptr.value + 2, n - 1)
    with pytest.raises(_lib.TomoError, match="NULL pointer"):
        h.measure(st, 0, U8, 4, 8, 12, 0.5, 1)
    with pytest.raises(_lib.TomoError, match="capacity must be"):
        h.extract(st, d_m.ptr, U8, 4, 8, 12, 0.5, 1, d_t.ptr, -1)
    assert h.device_bytes() == idle == 0                                         # nothing was allocated, so nothing ran
    d_i = ctx.empty((4, 8, 12), np.int32)
    with pytest.raises(ValueError):
        mesh.MeshExtractor(ctx).measure(d_i)                                     # a device array of the wrong dtype
    with pytest.raises(ValueError):
        mesh.MeshExtractor(ctx).measure(d_m, shape=(4, 8, 11))                   # ... and of the wrong size
    with pytest.raises(ValueError):
        mesh.MeshExtractor(ctx).isosurface(d_m, out=np.zeros((n, 3, 3), np.float32))     # a host out for a device volume
    got = h.measure(st, d_m.ptr, U8, 4, 8, 12, 0.5, 1)
    small = h.device_bytes()
    assert h.extract(st, d_m.ptr, U8, 4, 8, 12, 0.5, 1, d_t.ptr, n) == n == got[0]
    kept = h.device_bytes()
    assert 0 < small < kept <= _mesh_lib.KEEP_BYTES and h.measure(st, d_m.ptr, U8, 4, 8, 12, 0.5, 1) == got and h.device_bytes() == kept
    assert h.measure(st, d_f.ptr, F32, 4, 8, 12, 0.5, 1) == got                   # the mask as float32 at a half
    shape = (8200, 8192, 1)                      # 2 x 8193 x 8201 cells in bricks of 8 x 8 x 32: over a million bricks, 20 bytes each
    d_big = ctx.zeros(shape, np.uint8)
    bricks = -(-(shape[0] + 1) // 8) * -(-(shape[1] + 1) // 8)
    assert h.measure(st, d_big.ptr, U8, shape[0], shape[1], shape[2], 0.5, 1) == (0, 0.0, 0.0)
    after = h.device_bytes()
    print("idle %d bytes, after a small measure %d, after a small extract %d, after a measure of %s (%d bricks, %d bytes of scratch) %d"
          % (idle, small, kept, shape, bricks, 20 * bricks, after))
    assert 20 * bricks > _mesh_lib.KEEP_BYTES and after == idle
    h.close()
    h.close()
    with pytest.raises(_lib.TomoError, match="^mesh handle closed$"):
        h.measure(st, d_m.ptr, U8, 4, 8, 12, 0.5, 1)
    with pytest.raises(_lib.TomoError, match="^mesh handle closed$"):
        h.device_bytes()
    with pytest.raises(_lib.TomoError, match="device out of range"):
        _mesh_lib.MeshHandle(10 ** 6)
    live = len(_lib.LIVE_CONTEXTS)
    s = mesh.MeshExtractor()
    assert s.measure(m).n_triangles == n and isinstance(s.handle, _mesh_lib.MeshHandle)
    assert len(_lib.LIVE_CONTEXTS) == live + 1
    s.close()
    assert s.ctx is None and s.handle is None and len(_lib.LIVE_CONTEXTS) == live
    for a in (d_m, d_t, d_f, d_i, d_big):
        a.free()


# ----------------------------------------------------------------------------------------------------------------------- end to end

def test_align_rigid_measures_and_writes_the_surface(tmp_path):
    data = generate_data.make(32, 24, seed=1)
    kw = dict(n_outer=1, sirt_iters=5, verbose=False, segment=True)
    plain = align_rigid.run(dict(data), export=str(tmp_path / "plain"), **kw)
    out = align_rigid.run(dict(data), export=str(tmp_path / "surface"), surface=True, **kw)
    bare = align_rigid.run(dict(data), surface=True, **kw)                    # without export: the numbers alone
    for a, b in zip(plain[:4], out[:4]):
        assert np.array_equal(a, b)
    assert sorted(os.listdir(str(tmp_path / "surface"))) == sorted(os.listdir(str(tmp_path / "plain")) + ["surface.stl"])
    got, before = dict(out[4][-1]["segmentation"]), plain[4][-1]["segmentation"]
    assert bare[4][-1]["segmentation"] == got
    rec = np.ascontiguousarray(out[0], np.float32)
    tri = mm.isosurface(rec, np.float32(got["threshold"]), "closed")
    area, volume = mm.measures(tri)
    keys = ("enclosed_volume", "specific_surface", "surface_area")
    print("surface %s; model: %d triangles, area %r, volume %r" % ({k: got[k] for k in keys}, len(tri), area, volume))
    assert len(tri) > 0 and volume > 0 and mm.closed(tri)
    assert _close(got["surface_area"], area) and _close(got["enclosed_volume"], volume)
    assert got["specific_surface"] == got["surface_area"] / got["enclosed_volume"]
    surf = {k: got.pop(k) for k in keys}
    assert got == before
    normals, back = mesh.read_stl(str(tmp_path / "surface" / "surface.stl"))
    assert len(back) == len(tri) and np.array_equal(mm.canonical(back), mm.canonical(tri))
    assert os.path.getsize(str(tmp_path / "surface" / "surface.stl")) == 84 + 50 * len(tri)
    with open(str(tmp_path / "surface" / "labels_meta.json")) as f:
        meta = json.load(f)
    with open(str(tmp_path / "plain" / "labels_meta.json")) as f:
        meta_plain = json.load(f)
    assert {k: meta.pop(k) for k in keys} == surf and meta == meta_plain
    with pytest.raises(ValueError, match="goes with segment"):
        align_rigid.run(dict(data), n_outer=1, sirt_iters=1, verbose=False, surface=True)
