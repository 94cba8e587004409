"""
ctypes binding of libtomo_morph.so (include/tomo_morph.h): the exact squared Euclidean distance transform of a device mask, its root,
erosion, dilation, opening and closing by a ball, and the invert and select kernels of hole filling: the device operations of
morphology.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_MORPH_LIB") or os.path.join(_HERE, "libtomo_morph.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_i32 = ctypes.c_int32
_c_i64 = ctypes.c_int64
_i64_p = ctypes.POINTER(ctypes.c_int64)

ERR_UNSUPPORTED = 4                 # TOMO_MORPH_ERR_UNSUPPORTED
MAX_DIM = 16384                     # TOMO_MORPH_MAX_DIM: nx, ny, nz
MAX_VOXELS = 2 ** 31 - 1            # TOMO_MORPH_MAX_VOXELS
INF = 2 ** 31 - 1                   # TOMO_MORPH_INF: no background anywhere
W = 4                               # TOMO_MORPH_W: adjacent z a lane of the x and y passes owns
MAX_WQ = 16                         # TOMO_MORPH_MAX_WQ: groups of W a work-group owns at most
GROUP = 512                         # TOMO_MORPH_GROUP: lanes of a work-group of the staged passes
LINE_LIMIT = 4096                   # TOMO_MORPH_LINE_LIMIT: the longest line the LDS path takes by default
KEEP_BYTES = 16 << 20               # TOMO_MORPH_KEEP_BYTES

BORDERS = {"ignore": 0, "background": 1}

_DIMS = [_c_int, _c_int, _c_int]
_CALL = [_c_vp, _c_vp, _c_vp] + _DIMS          # handle, stream, mask, nx, ny, nz

# every symbol include/tomo_morph.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_morph_abi_version": (_c_int, []),
    "tomo_morph_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_morph_destroy": (_c_int, [_c_vp]),
    "tomo_morph_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_morph_device_bytes": (_c_int, [_c_vp, _i64_p]),
    "tomo_morph_check_shape": (_c_int, [_c_i64, _c_i64, _c_i64]),
    "tomo_morph_set_line_limit": (_c_int, [_c_vp, _c_int]),
    "tomo_morph_distance_sq": (_c_int, _CALL + [_c_int, _c_vp]),
    "tomo_morph_distance": (_c_int, _CALL + [_c_int, _c_vp]),
    "tomo_morph_line_pass": (_c_int, _CALL + [_c_int, _c_int, _c_vp]),
    "tomo_morph_root": (_c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp]),
    "tomo_morph_erode": (_c_int, _CALL + [_c_i64, _c_int, _c_vp]),
    "tomo_morph_dilate": (_c_int, _CALL + [_c_i64, _c_vp]),
    "tomo_morph_open": (_c_int, _CALL + [_c_i64, _c_int, _c_vp]),
    "tomo_morph_close": (_c_int, _CALL + [_c_i64, _c_int, _c_vp]),
    "tomo_morph_invert": (_c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_vp]),
    "tomo_morph_select": (_c_int, [_c_vp, _c_vp, _c_vp, _c_i64, _c_i32, _c_vp, _c_vp]),
}


class MorphUnsupported(TomoError):
    """A shape beyond the library's limits (1 <= nx, ny, nz <= MAX_DIM, at most MAX_VOXELS voxels); raised before anything is launched."""


def load():
    """Load libtomo_morph.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("morph", LIB_PATH, SIGNATURES)


ERRORS = {ERR_UNSUPPORTED: MorphUnsupported}


def check_shape(nx, ny, nz):
    """MorphUnsupported for a volume the library does not take.  Needs no device."""
    lib = load()
    _binding.check(lib, "morph", lib.tomo_morph_check_shape(int(nx), int(ny), int(nz)), None, ERRORS)


class MorphHandle(Handle):
    """One tomo_morph handle: a device, its scratch (at most KEEP_BYTES between calls) and the last error.  A context manager; close()
    frees everything.  device: the tomo context's (ctx.device) -- every call is enqueued on the stream it is given; a call waits for it
    only when it gives scratch above KEEP_BYTES back."""

    NAME = "morph"
    load = staticmethod(load)
    ERRORS = ERRORS

    def set_line_limit(self, n):
        """The longest line the LDS path takes (0: LINE_LIMIT).  No bit of any result depends on it."""
        self._check(self.lib.tomo_morph_set_line_limit(self.handle, int(n)))

    def _dims(self, stream, d_mask, nx, ny, nz):
        return self.handle, _ptr(stream), _ptr(d_mask), int(nx), int(ny), int(nz)

    def distance_sq(self, stream, d_mask, nx, ny, nz, border, d_out):
        self._check(self.lib.tomo_morph_distance_sq(*self._dims(stream, d_mask, nx, ny, nz), int(border), _ptr(d_out)))

    def distance(self, stream, d_mask, nx, ny, nz, border, d_out):
        self._check(self.lib.tomo_morph_distance(*self._dims(stream, d_mask, nx, ny, nz), int(border), _ptr(d_out)))

    def line_pass(self, stream, d_src, nx, ny, nz, axis, border, d_dst):
        """One pass alone: axis 2 from the mask, 1 and 0 from int32."""
        self._check(self.lib.tomo_morph_line_pass(*self._dims(stream, d_src, nx, ny, nz), int(axis), int(border), _ptr(d_dst)))

    def root(self, stream, d_d2, n, d_out):
        self._check(self.lib.tomo_morph_root(self.handle, _ptr(stream), _ptr(d_d2), int(n), _ptr(d_out)))

    def erode(self, stream, d_mask, nx, ny, nz, r2, border_value, d_out):
        self._check(self.lib.tomo_morph_erode(*self._dims(stream, d_mask, nx, ny, nz), int(r2), int(border_value), _ptr(d_out)))

    def dilate(self, stream, d_mask, nx, ny, nz, r2, d_out):
        self._check(self.lib.tomo_morph_dilate(*self._dims(stream, d_mask, nx, ny, nz), int(r2), _ptr(d_out)))

    def open(self, stream, d_mask, nx, ny, nz, r2, border_value, d_out):
        self._check(self.lib.tomo_morph_open(*self._dims(stream, d_mask, nx, ny, nz), int(r2), int(border_value), _ptr(d_out)))

    def close_ball(self, stream, d_mask, nx, ny, nz, r2, border_value, d_out):
        """tomo_morph_close (close() is the handle's own)."""
        self._check(self.lib.tomo_morph_close(*self._dims(stream, d_mask, nx, ny, nz), int(r2), int(border_value), _ptr(d_out)))

    def invert(self, stream, d_mask, n, d_out):
        self._check(self.lib.tomo_morph_invert(self.handle, _ptr(stream), _ptr(d_mask), int(n), _ptr(d_out)))

    def select(self, stream, d_labels, voxels, n, d_table, d_mask):
        self._check(self.lib.tomo_morph_select(self.handle, _ptr(stream), _ptr(d_labels), int(voxels), int(n), _ptr(d_table), _ptr(d_mask)))
