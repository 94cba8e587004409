"""mesh without a GPU: the model of tests/mesh_model.py on its own (closed surfaces on random volumes, masks, voxels equal to the level
and voxels that are not finite; the sign of the volume; masks against their float32 form; the two borders; the ball of the issue
against the sphere), the tables of csrc/tomo_side_tets.h against tools/tets_table.py, the STL writer byte for byte, the argument
checks of every public function, check_shape, and what the binding mirrors of the header under names of its own.  Every test prints
what it measured."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import abi
import mesh_model as mm

from tomography_alignment_amd import _lib, _mesh_lib, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1, 1), (1, 4, 5), (4, 1, 5), (2, 2, 2), (5, 6, 7), (9, 4, 11))


# -------------------------------------------------------------------------------------------------------------------- the model

def _inputs(shape, seed):
    return [("noise", mm.noise(shape, seed), 0.1), ("mask 0.5", mm.bernoulli(shape, 0.5, seed), None),
            ("mask 0.1", mm.bernoulli(shape, 0.1, seed + 1), None), ("mask 0.9", mm.bernoulli(shape, 0.9, seed + 2), None),
            ("integers at 1", mm.integers(shape, seed), 1.0), ("integers at 2", mm.integers(shape, seed + 1), 2.0),
            ("non-finite", mm.nonfinite(shape, seed), 0.25), ("checkerboard", mm.checkerboard(shape), None),
            ("corners", mm.corners_mask(shape), None)]


def test_the_model_is_closed_under_the_closed_border():
    n = total = 0
    for shape in SHAPES:
        for seed in range(2):
            for name, vol, level in _inputs(shape, 10 * seed):
                t = mm.isosurface(vol, level, "closed")
                assert t.dtype == np.float32 and t.shape[1:] == (3, 3)
                assert mm.closed(t), (shape, name)
                area, volume = mm.measures(t)
                if vol.dtype == np.uint8 and vol.any():
                    assert volume > 0 and area > 0, (shape, name)           # a solid
                n += 1
                total += len(t)
    print("%d surfaces, %d triangles: every directed edge has its reverse, bit for bit" % (n, total))


def test_closed_is_a_real_check():
    t = mm.isosurface(mm.bernoulli((5, 6, 7), 0.5, 3))
    assert mm.closed(t) and not mm.closed(t[1:])
    flipped = t.copy()
    flipped[0] = flipped[0, [0, 2, 1]]
    assert not mm.closed(flipped)
    c = mm.canonical(t)
    assert np.array_equal(mm.canonical(t[::-1]), c) and np.array_equal(mm.canonical(t[:, [1, 2, 0]]), c)
    assert not np.array_equal(mm.canonical(flipped), c) and sorted(map(bytes, c)) == sorted(map(bytes, mm.canonical(c)))


def test_ties_give_zero_area_triangles_that_are_kept():
    v = mm.integers((6, 6, 6), 4)
    t = mm.isosurface(v, 2.0)
    e = np.cross(t[:, 1].astype(np.float64) - t[:, 0], t[:, 2].astype(np.float64) - t[:, 0])
    flat = int((np.abs(e).sum(1) == 0).sum())
    print("%d triangles, %d without area" % (len(t), flat))
    assert flat > 0 and mm.closed(t)


def test_a_mask_is_its_float_form_at_a_half():
    for shape in SHAPES:
        m = mm.bernoulli(shape, 0.5, 7)
        for border in mm.BORDERS:
            a = mm.isosurface(m, None, border)
            assert np.array_equal(a, mm.isosurface(m.astype(np.float32), 0.5, border))
            assert np.array_equal(a, mm.isosurface(m.astype(bool), None, border))
            assert np.array_equal(a, mm.isosurface((m * 200).astype(np.uint8), None, border))


def test_open_equals_closed_away_from_the_faces():
    m = np.zeros((9, 10, 11), np.uint8)
    m[2:-2, 2:-2, 2:-2] = mm.bernoulli((5, 6, 7), 0.6, 5)
    f = np.full(m.shape, -1.0, np.float32)
    f[2:-2, 2:-2, 2:-2] = mm.noise((5, 6, 7), 6)
    for vol, level in ((m, None), (f, 0.0)):
        a, b = mm.isosurface(vol, level, "open"), mm.isosurface(vol, level, "closed")
        assert len(a) > 0 and np.array_equal(mm.canonical(a), mm.canonical(b)) and mm.closed(a)


def test_a_full_box():
    box = np.ones((3, 4, 5), np.uint8)
    t = mm.isosurface(box, None, "closed")
    area, volume = mm.measures(t)
    print("full 3 x 4 x 5 box, closed: %d triangles, area %g, volume %g" % (len(t), area, volume))
    assert mm.closed(t) and len(t) > 0 and t.min() == -0.5 and t.max() == 4.5
    assert volume > 2 * 3 * 4 and volume < 3 * 4 * 5                       # the box of the voxel centres, grown by half a voxel, corners cut
    assert mm.isosurface(box, None, "open").shape == (0, 3, 3)
    assert mm.isosurface(np.zeros((3, 4, 5), np.uint8)).shape == (0, 3, 3)
    assert mm.isosurface(np.ones((1, 4, 5), np.uint8), None, "open").shape == (0, 3, 3)        # an axis of length 1 has no cells
    assert len(mm.isosurface(np.ones((1, 1, 1), np.uint8))) > 0


def test_the_ball():
    """The issue's ball: 24^3, centre (N - 1) / 2 - (0.3, 0.1, -0.2), R = 8.5, field R - r, level 0.  Area within 1 % and volume within
    1.5 % of the sphere's; the definition gives 8120 triangles, 0.9964 of the area and 0.9931 of the volume."""
    R = 8.5
    t = mm.isosurface(mm.ball_field(24, R), 0.0)
    area, volume = mm.measures(t)
    ra, rv = area / (4 * np.pi * R * R), volume / (4 * np.pi * R ** 3 / 3)
    print("%d triangles, area %.4f and volume %.4f of the sphere's" % (len(t), ra, rv))
    assert mm.closed(t)
    assert abs(ra - 1) < 0.01 and abs(rv - 1) < 0.015
    assert len(t) == 8120 and round(ra, 4) == 0.9964 and round(rv, 4) == 0.9931


def test_the_headers_tables_are_the_generators():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tets_table.py")], stdout=subprocess.PIPE, universal_newlines=True,
                         check=True).stdout
    with open(os.path.join(ROOT, "tomography_alignment_amd", "csrc", "tomo_side_tets.h")) as f:
        text = f.read()
    block = re.search(r"// ---- generated by tools/tets_table\.py: begin\n(.*)// ---- generated by tools/tets_table\.py: end", text, re.S).group(1)
    assert block == out and "TETS_CASES[16]" in out
    # ... and the model's own rule gives the same words
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-f]{7})u", out)]
    for case in range(16):
        tris = mm.oriented_case(mm.PERMS[0], [(case >> i) & 1 for i in range(4)])
        w = len(tris)
        for k, (i, j) in enumerate(v for tri in tris for v in tri):
            w |= ((i << 2) | j) << (2 + 4 * k)
        assert w == words[case], case
    consts = dict(re.findall(r"TETS_(B[XYZ]) = (\d+)", text))
    assert tuple(int(consts[k]) for k in ("BX", "BY", "BZ")) == mm.BRICK == _mesh_lib.BRICK


# ------------------------------------------------------------------------------------------------------------------------ the STL

def test_write_stl_byte_for_byte(tmp_path):
    t = mm.isosurface(mm.integers((4, 5, 6), 1), 2.0)                      # some triangles without area
    path = str(tmp_path / "s.stl")
    scale = 0.25
    assert mesh.write_stl(path, t, scale) == len(t)
    with open(path, "rb") as f:
        data = f.read()
    assert len(data) == 84 + 50 * len(t) and data[:80] == mesh.STL_HEADER and len(mesh.STL_HEADER) == 80
    assert not data.startswith(b"solid") and struct.unpack("<I", data[80:84])[0] == len(t)
    zero = 0
    for k in range(len(t)):
        v = (t[k] * np.float32(scale)).astype(np.float32)
        e = np.cross(v[1].astype(np.float64) - v[0], v[2].astype(np.float64) - v[0])
        length = np.sqrt((e * e).sum())
        normal = (e / length if length > 0 else np.zeros(3)).astype(np.float32)
        zero += length == 0
        assert data[84 + 50 * k:84 + 50 * (k + 1)] == normal.astype("<f4").tobytes() + v.astype("<f4").tobytes() + b"\0\0", k
    normals, back = mesh.read_stl(path)
    assert np.array_equal(back, (t * np.float32(scale))) and zero > 0 and (normals[np.abs(normals).sum(1) > 0] ** 2).sum(1).round(5).tolist().count(1.0) == len(t) - zero
    s = mesh.Surface(t, len(t), 0.0, 0.0, 2.0, "closed", (4, 5, 6))
    other = str(tmp_path / "t.stl")
    mesh.write_stl(other, s, scale)
    with open(other, "rb") as f:
        assert f.read() == data
    assert mesh.write_stl(other, np.zeros((0, 3, 3), np.float32)) == 0 and os.path.getsize(other) == 84
    print("%d triangles, %d of them without area and with a zero normal: %d bytes, as specified" % (len(t), zero, len(data)))


# ----------------------------------------------------------------------------------------------------------------- argument checks

def test_arguments_are_checked_before_a_device_is_needed(tmp_path):
    f = np.zeros((3, 4, 5), np.float32)
    m = np.zeros((3, 4, 5), np.uint8)
    tri = np.zeros((2, 3, 3), np.float32)
    p = str(tmp_path / "x.stl")
    bad = [
        ("measure: dtype", lambda: mesh.measure(f.astype(np.float64), 0.0)),
        ("measure: int dtype", lambda: mesh.measure(m.astype(np.int32))),
        ("measure: rank", lambda: mesh.measure(f.ravel(), 0.0)),
        ("measure: shape", lambda: mesh.measure(f, 0.0, shape=(3, 4, 6))),
        ("measure: no level", lambda: mesh.measure(f)),
        ("measure: level nan", lambda: mesh.measure(f, float("nan"))),
        ("measure: level inf", lambda: mesh.measure(f, float("inf"))),
        ("measure: level beyond float32", lambda: mesh.measure(f, 1e39)),
        ("measure: level text", lambda: mesh.measure(f, "otsu")),
        ("measure: level bool", lambda: mesh.measure(f, True)),
        ("measure: mask level", lambda: mesh.measure(m, 0.3)),
        ("measure: bool mask level", lambda: mesh.measure(m.astype(bool), 1)),
        ("measure: border", lambda: mesh.measure(m, None, "reflect")),
        ("measure: border None", lambda: mesh.measure(f, 0.0, None)),
        ("isosurface: dtype", lambda: mesh.isosurface(m.astype(np.int8))),
        ("isosurface: no level", lambda: mesh.isosurface(f)),
        ("isosurface: mask level", lambda: mesh.isosurface(m, 1.0)),
        ("isosurface: border", lambda: mesh.isosurface(m, None, "ignore")),
        ("isosurface: rank", lambda: mesh.isosurface(m[0])),
        ("isosurface: out dtype", lambda: mesh.isosurface(m, out=np.zeros((4, 3, 3), np.float64))),
        ("isosurface: out size", lambda: mesh.isosurface(m, out=np.zeros(10, np.float32))),
        ("isosurface: out not contiguous", lambda: mesh.isosurface(m, out=np.zeros((4, 3, 6), np.float32)[:, :, ::2])),
        ("write_stl: shape", lambda: mesh.write_stl(p, np.zeros((2, 3, 2), np.float32))),
        ("write_stl: dtype", lambda: mesh.write_stl(p, np.zeros((2, 3, 3), np.int32))),
        ("write_stl: scale 0", lambda: mesh.write_stl(p, tri, 0)),
        ("write_stl: scale nan", lambda: mesh.write_stl(p, tri, float("nan"))),
        ("write_stl: scale negative", lambda: mesh.write_stl(p, tri, -1.0)),
    ]
    for name, call in bad:
        with pytest.raises(ValueError):
            call()
        print("%s: ValueError" % name)
    assert not os.path.exists(p)
    for ok in (None, 0.5, np.float32(0.5)):
        assert mesh._level(m, ok, "x") == (_mesh_lib.U8, 0.5)
    assert mesh._level(f, 1, "x") == (_mesh_lib.F32, 1.0) and mesh.BORDERS == mm.BORDERS


def test_check_shape_needs_no_device():
    for shape in ((1, 1, 1), (16384, 16384, 7), (2047, 1024, 1024), (1, 8191, 16384), (16384, 1, 1), (1, 1, 16384)):
        mesh.check_shape(*shape)
    for shape in ((16385, 1, 1), (1, 16385, 1), (1, 1, 16385), (2048, 1024, 1024), (16384, 16384, 8), (0, 4, 4), (4, 4, 0)):
        with pytest.raises(mesh.MeshUnsupported, match="nothing was launched"):
            mesh.check_shape(*shape)
    assert issubclass(mesh.MeshUnsupported, _mesh_lib.TomoError) and issubclass(mesh.MeshCapacity, mesh.MeshUnsupported)
    assert _mesh_lib.ERR_UNSUPPORTED == 4 and _mesh_lib.ERR_CAPACITY == 5
    with pytest.raises(mesh.MeshUnsupported):
        mesh.measure(np.zeros((16385, 1, 1), np.uint8))                    # before a device is asked for
    print("16385 on each axis and 2^31 voxels refused, 2^31 - 2^20 accepted")


# ------------------------------------------------------------------------------------------------------------------- the binding

def test_the_binding_covers_the_header():
    """What _mesh_lib mirrors under a name of its own; tests/test_binding.py holds everything else against the header."""
    c = abi.parse_header(abi.header_path("mesh")).constants
    assert (c["TOMO_MESH_BRICK_X"], c["TOMO_MESH_BRICK_Y"], c["TOMO_MESH_BRICK_Z"]) == _mesh_lib.BRICK
    assert c["TOMO_MESH_GROUP"] == _mesh_lib.GROUP == _mesh_lib.BRICK[1] * _mesh_lib.BRICK[2]
    assert {"open": c["TOMO_MESH_OPEN"], "closed": c["TOMO_MESH_CLOSED"]} == _mesh_lib.BORDERS


def test_errors_are_one_family_and_in_the_common_format():
    assert issubclass(_mesh_lib.MeshUnsupported, _lib.TomoError)
    with pytest.raises(_mesh_lib.MeshUnsupported, match=r"^libtomo_mesh error 4: tomo_mesh"):
        _mesh_lib.check_shape(0, 1, 1)
