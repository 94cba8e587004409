"""
The isosurface of a volume on the GPU (libtomo_mesh.so, include/tomo_mesh.h): the surface of a segmented object as triangles, its area
and the volume it encloses -- what specific surface is computed from, and what a viewer or a mesh tool takes -- from the float32
reconstruction at a level (the Otsu threshold, say; the surface then sits at sub-voxel positions) or from a uint8 / bool mask, where it
lies in HBM.

    measure(vol, level, border)              -> SurfaceMeasures(n_triangles, area, volume): one pass, no triangle written
    isosurface(vol, level, border, out)      -> Surface(triangles (n, 3, 3) float32, n, area, volume, level, border, shape)
    write_stl(path, surface_or_triangles, scale)    binary STL on the host

Marching tetrahedra, six per cell around the cell's main diagonal: no ambiguous case, and a surface that is closed bit for bit -- every
directed edge has its reverse -- also where voxels equal the level or are not finite (tests/mesh_model.py is the same in numpy).
Volumes are [nx][ny][nz], z fastest; voxel (i, j, k) is the lattice point (i, j, k) and vertices are in that frame (isotropic voxels).
A corner is inside when v >= level; a mask counts non-zero as 1 and is taken at 0.5.  border "closed" (default): the volume stands in
one layer of -inf, so an object that touches a face is closed there (vertices down to -1 + t); "open": only the cells inside the volume.
The triangles' normals point away from the inside; their order is fixed by shape, border and input.  area and volume are float64 sums
over the float32 vertices in a fixed order.  An array is a numpy array or a _lib.DeviceArray (a flat one with shape=); device in gives
device out.

Not here: welded / indexed vertices, per-label areas, smoothing or decimation, anisotropic voxels, marching cubes, more than one GPU.
The module-level functions make a temporary MeshExtractor; keep one to reuse its handle.  No CPU fallback.
"""
import collections
import math
import struct

import numpy as np

from . import _mesh_lib, _ops
from ._mesh_lib import MeshCapacity, MeshUnsupported  # noqa: F401  (part of this module's interface)

BORDERS = tuple(_mesh_lib.BORDERS)
_DTYPES = [np.float32, np.uint8, np.bool_]

SurfaceMeasures = collections.namedtuple("SurfaceMeasures", "n_triangles area volume")
Surface = collections.namedtuple("Surface", "triangles n area volume level border shape")


def _border(border, what):
    if border not in _mesh_lib.BORDERS:
        raise ValueError("%s: border must be 'open' or 'closed', not %r" % (what, border))
    return _mesh_lib.BORDERS[border]


def _level(vol, level, what):
    """(the library's dtype, the level as a float32 value) of a float32 volume at `level` or of a mask at 0.5."""
    if np.dtype(vol.dtype) == np.float32:
        if level is None or isinstance(level, bool):
            raise ValueError("%s: a float32 volume needs a level" % what)
        try:
            with np.errstate(over="ignore"):
                lv = float(np.float32(level))
        except (TypeError, ValueError):
            raise ValueError("%s: level must be a number, not %r" % (what, level))
        if not math.isfinite(lv):
            raise ValueError("%s: level must be finite as float32, not %r" % (what, level))
        return _mesh_lib.F32, lv
    if level is not None and (isinstance(level, bool) or level != 0.5):
        raise ValueError("%s: a mask is taken at 0.5; level must be None or 0.5, not %r" % (what, level))
    return _mesh_lib.U8, 0.5


def _check_out(out, vol, what):
    if out is None:
        return
    if _ops._is_dev(out) != _ops._is_dev(vol) or np.dtype(out.dtype) != np.float32 or out.size % 9 != 0:
        raise ValueError("%s: out must be a float32 array of the input's kind that holds whole triangles (9 values each)" % what)
    if not _ops._is_dev(out) and not (out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]):
        raise ValueError("%s: out must be C-contiguous and writeable" % what)


class MeshExtractor(_ops.HandleOwner):
    """The operations of this module on one libtomo_mesh handle (made on first use; see _ops.HandleOwner for ctx)."""

    def _new_handle(self):
        return _mesh_lib.MeshHandle(self.ctx.device)

    def device_bytes(self):
        return 0 if self.handle is None else self.handle.device_bytes()

    def _args(self, what, vol, level, border, shape):
        s = _ops.volume_shape(vol, shape, _DTYPES, what, "volume")
        dtype, lv = _level(vol, level, what)
        b = _border(border, what)
        return s, dtype, lv, b

    def measure(self, vol, level=None, border="closed", shape=None):
        """SurfaceMeasures(n_triangles, area, volume) of the isosurface; no triangle is written.  volume is the signed volume the
        surface encloses: positive for a solid, and meaningful under "open" only where the object stays inside the volume."""
        s, dtype, lv, b = self._args("measure", vol, level, border, shape)
        _mesh_lib.check_shape(*s)
        self._ready(vol)
        with self._staging(vol) as st:
            d = st.source(vol, np.float32 if dtype == _mesh_lib.F32 else np.uint8)
            return SurfaceMeasures(*self.handle.measure(self.ctx.stream(), d.ptr, dtype, s[0], s[1], s[2], lv, b))

    def isosurface(self, vol, level=None, border="closed", out=None, shape=None):
        """Surface: `triangles` (n, 3, 3) float32, vertex by vertex, of the input's kind ((0, 3, 3) without a surface), and n, area,
        volume, level, border, shape.  out: a float32 buffer of the input's kind for the triangles, of which `triangles` is then the
        front; MeshCapacity, and nothing written, where it is too small."""
        s, dtype, lv, b = self._args("isosurface", vol, level, border, shape)
        _check_out(out, vol, "isosurface")
        _mesh_lib.check_shape(*s)
        self._ready(vol)
        with self._staging(vol) as st:
            d = st.source(vol, np.float32 if dtype == _mesh_lib.F32 else np.uint8)
            stream = self.ctx.stream()
            n, area, volume = self.handle.measure(stream, d.ptr, dtype, s[0], s[1], s[2], lv, b)
            if n > _mesh_lib.MAX_TRIANGLES:
                raise MeshUnsupported("isosurface: the surface has %d triangles, more than 2^31 - 1; nothing was written" % n)
            if out is not None and n > out.size // 9:
                e = MeshCapacity("isosurface: the surface has %d triangles, out holds %d; nothing was written" % (n, out.size // 9))
                e.needed = n
                raise e
            if st.dev:
                d_tri = out if out is not None else st.dest((n, 3, 3), np.float32)
                self.handle.extract(stream, d.ptr, dtype, s[0], s[1], s[2], lv, b, d_tri.ptr, d_tri.size // 9)
                tri = st.result(d_tri)
                if out is not None:
                    tri = out.view(0, 9 * n)
                    tri.shape = (n, 3, 3)
            elif n == 0:
                tri = np.zeros((0, 3, 3), np.float32) if out is None else out.reshape(-1)[:0].reshape(0, 3, 3)
            else:
                d_tri = st.dest((n, 3, 3), np.float32)
                self.handle.extract(stream, d.ptr, dtype, s[0], s[1], s[2], lv, b, d_tri.ptr, n)
                if out is None:
                    tri = st.result(d_tri)
                else:
                    tri = out.reshape(-1)[:9 * n].reshape(n, 3, 3)
                    d_tri.download(tri)
        return Surface(tri, int(n), area, volume, lv, border, s)


def check_shape(nx, ny, nz):
    """MeshUnsupported for a volume of more than 2^31 - 1 voxels or an axis above 16384.  Needs no device."""
    _mesh_lib.check_shape(nx, ny, nz)


def measure(vol, level=None, border="closed", ctx=None, shape=None):
    with MeshExtractor(ctx) as m:                            # without a ctx: a device array's (_ops.HandleOwner)
        return m.measure(vol, level, border, shape=shape)


def isosurface(vol, level=None, border="closed", out=None, ctx=None, shape=None):
    with MeshExtractor(ctx) as m:
        return m.isosurface(vol, level, border, out, shape=shape)


STL_HEADER = b"tomography_alignment_amd isosurface, binary STL, index frame times scale".ljust(80, b"\0")
_STL_RECORD = np.dtype([("normal", "<f4", 3), ("v", "<f4", (3, 3)), ("attr", "<u2")])


def write_stl(path, surface, scale=1.0):
    """Binary STL of a Surface or of an (n, 3, 3) array on the host: the 80-byte STL_HEADER, the uint32 count, then 50 bytes a triangle
    -- the float32 unit normal of the written vertices (zero for a triangle without area), the three vertices times `scale` (the voxel
    size) as float32, two zero bytes.  -> the number of triangles."""
    tri = surface.triangles if isinstance(surface, Surface) else surface
    if _ops._is_dev(tri):
        raise ValueError("write_stl: the triangles are on the device; download them first (triangles.download())")
    tri = np.asarray(tri)
    if tri.ndim != 3 or tri.shape[1:] != (3, 3) or tri.dtype.kind != "f":
        raise ValueError("write_stl: need a Surface or a float array of shape (n, 3, 3), not %s %r" % (tri.dtype, tri.shape))
    if isinstance(scale, bool) or not (math.isfinite(float(scale)) and float(scale) > 0):
        raise ValueError("write_stl: scale must be finite and > 0, not %r" % (scale,))
    if len(tri) > 2 ** 32 - 1:
        raise ValueError("write_stl: binary STL holds at most 2^32 - 1 triangles")
    rec = np.zeros(len(tri), _STL_RECORD)
    rec["v"] = tri.astype(np.float32) * np.float32(scale)
    v = rec["v"].astype(np.float64)
    e = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    length = np.sqrt((e * e).sum(1))
    rec["normal"] = np.where(length[:, None] > 0, e / np.where(length > 0, length, 1.0)[:, None], 0.0)
    with open(path, "wb") as f:
        f.write(STL_HEADER)
        f.write(struct.pack("<I", len(tri)))
        f.write(rec.tobytes())
    return len(tri)


def read_stl(path):
    """(normals (n, 3), triangles (n, 3, 3)) float32 of a binary STL as write_stl writes it."""
    with open(path, "rb") as f:
        data = f.read()
    n, = struct.unpack("<I", data[80:84])
    if len(data) != 84 + 50 * n:
        raise ValueError("read_stl: %s holds %d bytes, not the %d of %d triangles" % (path, len(data), 84 + 50 * n, n))
    rec = np.frombuffer(data, _STL_RECORD, n, 84)
    return np.array(rec["normal"], np.float32), np.array(rec["v"], np.float32)
