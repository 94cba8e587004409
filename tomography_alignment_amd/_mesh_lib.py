"""
ctypes binding of libtomo_mesh.so (include/tomo_mesh.h): the isosurface of a device volume by marching tetrahedra -- the number of its
triangles, its area and enclosed volume in one pass, and the triangles themselves: the device operations of mesh.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_MESH_LIB") or os.path.join(_HERE, "libtomo_mesh.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_i64 = ctypes.c_int64
_i64_p = ctypes.POINTER(ctypes.c_int64)
_f64_p = ctypes.POINTER(ctypes.c_double)

ERR_UNSUPPORTED = 4                 # TOMO_MESH_ERR_UNSUPPORTED
ERR_CAPACITY = 5                    # TOMO_MESH_ERR_CAPACITY
MAX_DIM = 16384                     # TOMO_MESH_MAX_DIM: nx, ny, nz
MAX_VOXELS = 2 ** 31 - 1            # TOMO_MESH_MAX_VOXELS
MAX_TRIANGLES = 2 ** 31 - 1         # TOMO_MESH_MAX_TRIANGLES
BRICK = (8, 8, 32)                  # TOMO_MESH_BRICK_X / _Y / _Z: the cells of a work-group's brick
GROUP = 256                         # TOMO_MESH_GROUP: lanes of a work-group
KEEP_BYTES = 16 << 20               # TOMO_MESH_KEEP_BYTES

F32, U8 = 0, 1                      # TOMO_MESH_F32, TOMO_MESH_U8
BORDERS = {"open": 0, "closed": 1}  # TOMO_MESH_OPEN, TOMO_MESH_CLOSED

# handle, stream, volume, dtype, nx, ny, nz, level, border
_CALL = [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, ctypes.c_float, _c_int]

# every symbol include/tomo_mesh.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_mesh_abi_version": (_c_int, []),
    "tomo_mesh_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_mesh_destroy": (_c_int, [_c_vp]),
    "tomo_mesh_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_mesh_device_bytes": (_c_int, [_c_vp, _i64_p]),
    "tomo_mesh_check_shape": (_c_int, [_c_i64, _c_i64, _c_i64]),
    "tomo_mesh_measure": (_c_int, _CALL + [_i64_p, _f64_p, _f64_p]),
    "tomo_mesh_extract": (_c_int, _CALL + [_c_vp, _c_i64, _i64_p]),
}


class MeshUnsupported(TomoError):
    """A refusal of the library: a shape beyond its limits (1 <= nx, ny, nz <= MAX_DIM, at most MAX_VOXELS voxels), raised before
    anything is launched, or a surface of more than MAX_TRIANGLES triangles."""


class MeshCapacity(MeshUnsupported):
    """extract: the surface has more triangles than the buffer holds; nothing was written.  `needed`: how many it has."""
    needed = None


def load():
    """Load libtomo_mesh.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("mesh", LIB_PATH, SIGNATURES)


ERRORS = {ERR_UNSUPPORTED: MeshUnsupported, ERR_CAPACITY: MeshCapacity}


def check_shape(nx, ny, nz):
    """MeshUnsupported for a volume the library does not take.  Needs no device."""
    lib = load()
    _binding.check(lib, "mesh", lib.tomo_mesh_check_shape(int(nx), int(ny), int(nz)), None, ERRORS)


class MeshHandle(Handle):
    """One tomo_mesh handle: a device, its scratch (at most KEEP_BYTES between calls) and the last error.  A context manager; close()
    frees everything.  device: the tomo context's (ctx.device).  Both calls are enqueued on the stream they are given and wait for it:
    they hand numbers back."""

    NAME = "mesh"
    load = staticmethod(load)
    ERRORS = ERRORS

    def _call(self, stream, d_vol, dtype, nx, ny, nz, level, border):
        return self.handle, _ptr(stream), _ptr(d_vol), int(dtype), int(nx), int(ny), int(nz), float(level), int(border)

    def measure(self, stream, d_vol, dtype, nx, ny, nz, level, border):
        """-> (n_triangles, area, volume)"""
        n, a, v = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._check(self.lib.tomo_mesh_measure(*self._call(stream, d_vol, dtype, nx, ny, nz, level, border),
                                               ctypes.byref(n), ctypes.byref(a), ctypes.byref(v)))
        return n.value, a.value, v.value

    def extract(self, stream, d_vol, dtype, nx, ny, nz, level, border, d_triangles, capacity):
        """-> n_triangles, written to d_triangles as float32 [n][3][3]; MeshCapacity (with .needed) if capacity is too small."""
        n = ctypes.c_int64(0)
        rc = self.lib.tomo_mesh_extract(*self._call(stream, d_vol, dtype, nx, ny, nz, level, border), _ptr(d_triangles), int(capacity),
                                        ctypes.byref(n))
        try:
            self._check(rc)
        except MeshCapacity as e:
            e.needed = n.value
            raise
        return n.value
