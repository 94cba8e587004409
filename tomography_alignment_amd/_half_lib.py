"""
ctypes binding of libtomo_half.so (include/tomo_half.h): half-acquisition scans over 2 pi -- the gather of detector rows out of a device
sinogram, both overlap-search curves of every gathered row (float64, deterministic sums), and the stitch of the 2 pi series to the pi
series of double width: the device operations of half_acquisition.find_center_360 and half_acquisition.sino_360_to_180.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

import numpy as np

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_HALF_LIB") or os.path.join(_HERE, "libtomo_half.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_double = ctypes.c_double
_c_float = ctypes.c_float
_c_size = ctypes.c_size_t
_int_p = ctypes.POINTER(_c_int)
_double_p = ctypes.POINTER(_c_double)
_float_p = ctypes.POINTER(_c_float)

ERR_UNSUPPORTED = 4       # TOMO_HALF_ERR_UNSUPPORTED
MAX_N = 65536             # TOMO_HALF_MAX_N
MIN_NX, MAX_NX = 8, 16384  # TOMO_HALF_MIN_NX, TOMO_HALF_MAX_NX
MAX_NZ = 16384            # TOMO_HALF_MAX_NZ
MAX_ROWS = 4096           # TOMO_HALF_MAX_ROWS
MIN_W = 4                 # TOMO_HALF_MIN_W
TILE_J, TILE_P, TILE_C = 8, 1024, 32      # TOMO_HALF_TILE_J, TOMO_HALF_TILE_P, TOMO_HALF_TILE_C
A_VALID, B_VALID = 1, 2   # TOMO_HALF_A_VALID, TOMO_HALF_B_VALID


class Column(ctypes.Structure):
    """tomo_half_column: one output column of the stitch."""
    _fields_ = [("flags", _c_int), ("ja", _c_int), ("i0", _c_int), ("i1", _c_int), ("f0", _c_float), ("f1", _c_float), ("wa", _c_float),
                ("wb", _c_float)]


_column_p = ctypes.POINTER(Column)

# every symbol include/tomo_half.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_half_abi_version": (_c_int, []),
    "tomo_half_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_half_destroy": (_c_int, [_c_vp]),
    "tomo_half_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_half_check_shape": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "tomo_half_stitched_shape": (_c_int, [_c_int, _c_int, _c_double, _int_p, _int_p, _int_p, _double_p]),
    "tomo_half_table": (_c_int, [_c_int, _c_double, _c_int, _column_p, _double_p, _double_p]),
    "tomo_half_scratch_bytes": (_c_int, [_c_int, _c_int, ctypes.POINTER(_c_size)]),
    "tomo_half_batch": (_c_int, [_c_int, _c_int, _c_int, _c_size, _int_p]),
    "tomo_half_set_max_scratch": (_c_int, [_c_vp, _c_size]),
    "tomo_half_device_bytes": (_c_int, [_c_vp, ctypes.POINTER(ctypes.c_int64)]),
    "tomo_half_load": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _int_p, _c_int]),
    "tomo_half_search": (_c_int, [_c_vp, _c_vp, _c_int, _double_p]),
    "tomo_half_fetch": (_c_int, [_c_vp, _c_vp, _double_p]),
    "tomo_half_debug_sinogram": (_c_int, [_c_vp, _c_vp, _c_int, _float_p]),
    "tomo_half_stitch": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_double, _c_vp]),
}


class HalfUnsupported(TomoError):
    """A shape, a window or an axis beyond the library's limits (even 2 <= n <= MAX_N, MIN_NX <= nx <= MAX_NX, 1 <= nz <= MAX_NZ, at most
    MAX_ROWS detector rows, MIN_W <= w <= nx / 2, 0 <= c <= nx - 1); raised before anything is launched."""


def load():
    """Load libtomo_half.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("half", LIB_PATH, SIGNATURES)


ERRORS = {ERR_UNSUPPORTED: HalfUnsupported}


def _check(lib, rc):
    _binding.check(lib, "half", rc, None, ERRORS)


def check_shape(n, nx, nz=1, nrows=0, w=0):
    """HalfUnsupported for a series, a number of detector rows (if > 0) or a window (if > 0) the library does not take.  Needs no device."""
    lib = load()
    _check(lib, lib.tomo_half_check_shape(int(n), int(nx), int(nz), int(nrows), int(w)))


def stitched_shape(n, nx, c):
    """(h, W, j0, c_out) as the library computes them.  Needs no device."""
    lib = load()
    h, W, j0, c_out = _c_int(0), _c_int(0), _c_int(0), _c_double(0.0)
    _check(lib, lib.tomo_half_stitched_shape(int(n), int(nx), float(c), ctypes.byref(h), ctypes.byref(W), ctypes.byref(j0), ctypes.byref(c_out)))
    return h.value, W.value, j0.value, c_out.value


def table(nx, c):
    """The column table of the stitch as the library uploads it: dict of flags, ja, i0, i1 (int32), f0, f1, wa, wb (float32, the rounded
    weights) and f, wA (float64, before rounding), W entries each.  Needs no device."""
    lib = load()
    _, W, _, _ = stitched_shape(2, nx, c)
    cols = (Column * W)()
    f, wa = np.zeros(W, np.float64), np.zeros(W, np.float64)
    _check(lib, lib.tomo_half_table(int(nx), float(c), W, cols, f.ctypes.data_as(_double_p), wa.ctypes.data_as(_double_p)))
    raw = np.frombuffer(cols, dtype=np.dtype([("flags", "i4"), ("ja", "i4"), ("i0", "i4"), ("i1", "i4"), ("f0", "f4"), ("f1", "f4"), ("wa", "f4"),
                                              ("wb", "f4")])).copy()
    out = {k: raw[k] for k in raw.dtype.names}
    out.update(f=f, wA=wa)
    return out


def scratch_bytes(nx, w):
    """Bytes of partial sums one detector row of the search needs.  Needs no device."""
    lib = load()
    b = _c_size(0)
    _check(lib, lib.tomo_half_scratch_bytes(int(nx), int(w), ctypes.byref(b)))
    return b.value


def batch(nrows, nx, w, max_scratch_bytes=0):
    """The detector rows per batch of the search for this shape and scratch budget (0: no limit; never fewer than one).  Needs no device."""
    lib = load()
    b = _c_int(0)
    _check(lib, lib.tomo_half_batch(int(nrows), int(nx), int(w), int(max_scratch_bytes), ctypes.byref(b)))
    return b.value


class HalfHandle(Handle):
    """One tomo_half handle: a device, the gathered sinograms, the sums and curves of the search, the column table of the stitch, and the
    last error.  A context manager; close() frees everything.  device: the tomo context's (ctx.device) -- every call is enqueued on the
    stream it is given, in practice that context's; only a call that hands values to the host waits."""

    NAME = "half"
    load = staticmethod(load)
    ERRORS = ERRORS

    def __init__(self, device=0):
        super(HalfHandle, self).__init__(device)
        self.shape = None           # (nrows, n, nx) of the last load
        self.window = None          # w of the last search

    def set_max_scratch(self, max_scratch_bytes):
        """The budget of the search's partial sums for the calls that follow (0 / None: no limit)."""
        self._check(self.lib.tomo_half_set_max_scratch(self.handle, int(max_scratch_bytes or 0)))

    def load_rows(self, stream, d_p, n_p, nx, nz, n, rows):
        """Gather the detector rows `rows` of the device sinogram p[n_p][nx][nz], projections 0 .. n - 1.  Enqueues."""
        rows = np.ascontiguousarray(rows, np.int32).ravel()
        self.shape = self.window = None
        self._check(self.lib.tomo_half_load(self.handle, _ptr(stream), _ptr(d_p), int(n_p), int(nx), int(nz), int(n), rows.ctypes.data_as(_int_p),
                                            int(rows.size)))
        self.shape = (int(rows.size), int(n), int(nx))

    def _loaded_shape(self):
        if self.shape is None:
            raise TomoError("half handle: no sinogram is loaded")
        return self.shape

    def search(self, stream, w, fetch=True):
        """Both curves of every loaded row for the window w.  fetch=True waits and returns m (nrows, 2, nx - w + 1) float64, side right
        first; fetch=False only enqueues (fetch() hands the table over later)."""
        nr, _, nx = self._loaded_shape()
        self.window = None
        m = np.zeros((nr, 2, max(nx - int(w) + 1, 1)), np.float64) if fetch else None
        self._check(self.lib.tomo_half_search(self.handle, _ptr(stream), int(w), m.ctypes.data_as(_double_p) if fetch else None))
        self.window = int(w)
        return m

    def fetch(self, stream):
        """The curves of the last search(); waits for the stream."""
        nr, _, nx = self._loaded_shape()
        if self.window is None:
            raise TomoError("half handle: no curves were computed")
        m = np.zeros((nr, 2, nx - self.window + 1), np.float64)
        self._check(self.lib.tomo_half_fetch(self.handle, _ptr(stream), m.ctypes.data_as(_double_p)))
        return m

    def debug_sinogram(self, stream, row):
        _, n, nx = self._loaded_shape()
        out = np.zeros((n, nx), np.float32)
        self._check(self.lib.tomo_half_debug_sinogram(self.handle, _ptr(stream), int(row), out.ctypes.data_as(_float_p)))
        return out

    def stitch(self, stream, d_p, n, nx, nz, c, d_out):
        """d_out[n / 2][W][nz] = the stitch of d_p[n][nx][nz] about the axis c.  Enqueues."""
        self._check(self.lib.tomo_half_stitch(self.handle, _ptr(stream), _ptr(d_p), int(n), int(nx), int(nz), float(c), _ptr(d_out)))
