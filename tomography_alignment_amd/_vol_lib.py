"""
ctypes binding of libtomo_vol.so (include/tomo_vol.h): what a device volume v[nx][ny][nz] goes through before it leaves the device --
statistics, the grey-value histogram, the conversion to 8 or 16 bit (in the volume's layout or as the stack of z slices), the cylinder
mask, minimum / maximum projections and single planes: the device operations of postprocess.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

import numpy as np

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_VOL_LIB") or os.path.join(_HERE, "libtomo_vol.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_i64 = ctypes.c_int64
_c_float = ctypes.c_float
_u64_p = ctypes.POINTER(ctypes.c_uint64)

ERR_UNSUPPORTED = 4       # TOMO_VOL_ERR_UNSUPPORTED
MAX_DIM = 16384           # TOMO_VOL_MAX_DIM: nx, ny
MAX_NZ = 2147418112       # TOMO_VOL_MAX_NZ
MAX_BINS = 16384          # TOMO_VOL_MAX_BINS
SPAN_GROUPS = 4096        # TOMO_VOL_SPAN_GROUPS
TILE = 64                 # TOMO_VOL_TILE


class StatsStruct(ctypes.Structure):
    """tomo_vol_stats_t"""
    _fields_ = [("n_finite", _c_i64), ("n_nonfinite", _c_i64), ("sum", ctypes.c_double), ("sumsq", ctypes.c_double),
                ("min", _c_float), ("max", _c_float)]


_stats_p = ctypes.POINTER(StatsStruct)
_VOL = [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_i64]      # h, stream, d_v, nx, ny, nz, R4

# every symbol include/tomo_vol.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_vol_abi_version": (_c_int, []),
    "tomo_vol_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_vol_destroy": (_c_int, [_c_vp]),
    "tomo_vol_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_vol_device_bytes": (_c_int, [_c_vp, ctypes.POINTER(_c_i64)]),
    "tomo_vol_check_shape": (_c_int, [_c_i64, _c_i64, _c_i64]),
    "tomo_vol_stats": (_c_int, _VOL + [_stats_p]),
    "tomo_vol_fetch_stats": (_c_int, [_c_vp, _c_vp, _stats_p]),
    "tomo_vol_histogram": (_c_int, _VOL + [_c_float, _c_float, _c_int, _u64_p, _u64_p]),
    "tomo_vol_fetch_histogram": (_c_int, [_c_vp, _c_vp, _u64_p, _u64_p]),
    "tomo_vol_quantize": (_c_int, _VOL + [_c_float, _c_float, _c_int, _c_int, _c_int, _c_vp]),
    "tomo_vol_mask": (_c_int, _VOL + [_c_float, _c_vp]),
    "tomo_vol_project": (_c_int, _VOL + [_c_int, _c_int, _c_vp]),
    "tomo_vol_slice": (_c_int, _VOL + [_c_int, _c_int, _c_vp]),
}


class VolUnsupported(TomoError):
    """A shape beyond the library's limits (1 <= nx, ny <= MAX_DIM, 1 <= nz <= MAX_NZ); raised before anything is launched."""


def load():
    """Load libtomo_vol.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("vol", LIB_PATH, SIGNATURES)


ERRORS = {ERR_UNSUPPORTED: VolUnsupported}


def check_shape(nx, ny, nz):
    """VolUnsupported for a volume the library does not take.  Needs no device."""
    lib = load()
    _binding.check(lib, "vol", lib.tomo_vol_check_shape(int(nx), int(ny), int(nz)), None, ERRORS)


class VolHandle(Handle):
    """One tomo_vol handle: a device, the partial sums and the small result tables, and the last error.  A context manager; close()
    frees everything.  device: the tomo context's (ctx.device) -- every call is enqueued on the stream it is given, in practice that
    context's; only a call that hands a table to the host waits.  R4 < 0: no region (include/tomo_vol.h)."""

    NAME = "vol"
    load = staticmethod(load)
    ERRORS = ERRORS

    def __init__(self, device=0):
        super(VolHandle, self).__init__(device)
        self.nbins = None           # of the last histogram()

    def _vol(self, stream, d_v, nx, ny, nz, R4):
        return (self.handle, _ptr(stream), _ptr(d_v), int(nx), int(ny), int(nz), int(R4))

    def stats(self, stream, d_v, nx, ny, nz, R4=-1, fetch=True):
        """The statistics of the region.  fetch=True waits and returns a StatsStruct; fetch=False only enqueues."""
        out = StatsStruct() if fetch else None
        self._check(self.lib.tomo_vol_stats(*self._vol(stream, d_v, nx, ny, nz, R4), ctypes.byref(out) if fetch else None))
        return out

    def fetch_stats(self, stream):
        out = StatsStruct()
        self._check(self.lib.tomo_vol_fetch_stats(self.handle, _ptr(stream), ctypes.byref(out)))
        return out

    def histogram(self, stream, d_v, nx, ny, nz, R4, lo, hi, nbins, fetch=True):
        """fetch=True waits and returns (counts (nbins,) uint64, (under, over, nonfinite)); fetch=False only enqueues."""
        nbins = int(nbins)
        self.nbins = None
        if fetch:
            counts, extra = np.zeros(max(nbins, 0), np.uint64), np.zeros(3, np.uint64)
            args = (counts.ctypes.data_as(_u64_p), extra.ctypes.data_as(_u64_p))
        else:
            args = (None, None)
        self._check(self.lib.tomo_vol_histogram(*self._vol(stream, d_v, nx, ny, nz, R4), float(lo), float(hi), nbins, *args))
        self.nbins = nbins
        return (counts, tuple(int(e) for e in extra)) if fetch else None

    def fetch_histogram(self, stream):
        if self.nbins is None:
            raise TomoError("vol handle: no histogram was computed")
        counts, extra = np.zeros(self.nbins, np.uint64), np.zeros(3, np.uint64)
        self._check(self.lib.tomo_vol_fetch_histogram(self.handle, _ptr(stream), counts.ctypes.data_as(_u64_p), extra.ctypes.data_as(_u64_p)))
        return counts, tuple(int(e) for e in extra)

    def quantize(self, stream, d_v, nx, ny, nz, R4, lo, hi, bits, order, fill, d_out):
        """bits 8 or 16; order 0 (out[x][y][z]) or 1 (out[z][y][x])."""
        self._check(self.lib.tomo_vol_quantize(*self._vol(stream, d_v, nx, ny, nz, R4), float(lo), float(hi), int(bits), int(order), int(fill),
                                               _ptr(d_out)))

    def mask(self, stream, d_v, nx, ny, nz, R4, value, d_out):
        self._check(self.lib.tomo_vol_mask(*self._vol(stream, d_v, nx, ny, nz, R4), float(value), _ptr(d_out)))

    def project(self, stream, d_v, nx, ny, nz, axis, op, d_out):
        """op 0 (max) or 1 (min)."""
        self._check(self.lib.tomo_vol_project(*self._vol(stream, d_v, nx, ny, nz, -1), int(axis), int(op), _ptr(d_out)))

    def slice(self, stream, d_v, nx, ny, nz, axis, index, d_out):
        self._check(self.lib.tomo_vol_slice(*self._vol(stream, d_v, nx, ny, nz, -1), int(axis), int(index), _ptr(d_out)))
