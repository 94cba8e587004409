"""
ctypes binding of libtomo_seg.so (include/tomo_seg.h): the threshold of a device volume to a mask, 3-D connected-component labels,
per-component measures, the removal of small components and the largest component: the device operations of segment.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

import numpy as np

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_SEG_LIB") or os.path.join(_HERE, "libtomo_seg.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_i32 = ctypes.c_int32
_c_i64 = ctypes.c_int64
_c_float = ctypes.c_float
_c_size = ctypes.c_size_t
_i32_p = ctypes.POINTER(ctypes.c_int32)
_i64_p = ctypes.POINTER(ctypes.c_int64)

ERR_UNSUPPORTED = 4                 # TOMO_SEG_ERR_UNSUPPORTED
MAX_DIM = 16384                     # TOMO_SEG_MAX_DIM: nx, ny
MAX_VOXELS = 2 ** 31 - 1            # TOMO_SEG_MAX_VOXELS
TILE_X, TILE_Y, TILE_Z = 8, 8, 64   # TOMO_SEG_TILE_X / _Y / _Z: the brick of the labelling's tile pass
SPAN_GROUPS = 1024                  # TOMO_SEG_SPAN_GROUPS
KEEP_BYTES = 16 << 20               # TOMO_SEG_KEEP_BYTES
DEFAULT_SCRATCH = 256 << 20         # TOMO_SEG_DEFAULT_SCRATCH

_DIMS = [_c_int, _c_int, _c_int]

# every symbol include/tomo_seg.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_seg_abi_version": (_c_int, []),
    "tomo_seg_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_seg_destroy": (_c_int, [_c_vp]),
    "tomo_seg_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_seg_device_bytes": (_c_int, [_c_vp, _i64_p]),
    "tomo_seg_check_shape": (_c_int, [_c_i64, _c_i64, _c_i64]),
    "tomo_seg_set_max_scratch": (_c_int, [_c_vp, _c_size]),
    "tomo_seg_measure_passes": (_c_int, [_c_i64, _c_int, _c_size, ctypes.POINTER(_c_int)]),
    "tomo_seg_threshold": (_c_int, [_c_vp, _c_vp, _c_vp] + _DIMS + [_c_i64, _c_float, _c_float, _c_int, _c_int, _c_vp]),
    "tomo_seg_label": (_c_int, [_c_vp, _c_vp, _c_vp] + _DIMS + [_c_int, _c_vp, _i32_p]),
    "tomo_seg_measure": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp] + _DIMS + [_c_i32, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "tomo_seg_remove_small": (_c_int, [_c_vp, _c_vp, _c_vp] + _DIMS + [_c_i32, _c_i64, _c_vp, _i32_p]),
    "tomo_seg_largest": (_c_int, [_c_vp, _c_vp, _c_vp] + _DIMS + [_c_i32, _c_vp, _i32_p, _i64_p]),
}


class SegUnsupported(TomoError):
    """A shape beyond the library's limits (1 <= nx, ny <= MAX_DIM, at most MAX_VOXELS voxels); raised before anything is launched."""


def load():
    """Load libtomo_seg.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("seg", LIB_PATH, SIGNATURES)


ERRORS = {ERR_UNSUPPORTED: SegUnsupported}


def check_shape(nx, ny, nz):
    """SegUnsupported for a volume the library does not take.  Needs no device."""
    lib = load()
    _binding.check(lib, "seg", lib.tomo_seg_check_shape(int(nx), int(ny), int(nz)), None, ERRORS)


def measure_passes(n, with_vol, max_scratch=0):
    """The passes over the volume measure makes for n components under a budget (0: the default).  Needs no device."""
    lib = load()
    p = _c_int(0)
    _binding.check(lib, "seg", lib.tomo_seg_measure_passes(int(n), int(bool(with_vol)), int(max_scratch), ctypes.byref(p)), None, ERRORS)
    return p.value


def _host(a):
    return a.ctypes.data_as(_c_vp)


class SegHandle(Handle):
    """One tomo_seg handle: a device, its scratch (at most KEEP_BYTES between calls) and the last error.  A context manager; close()
    frees everything.  device: the tomo context's (ctx.device) -- every call is enqueued on the stream it is given; a call that hands a
    number or a table to the host waits."""

    NAME = "seg"
    load = staticmethod(load)
    ERRORS = ERRORS

    def set_max_scratch(self, nbytes):
        """The budget of measure's tables (0: DEFAULT_SCRATCH)."""
        self._check(self.lib.tomo_seg_set_max_scratch(self.handle, int(nbytes)))

    def threshold(self, stream, d_v, nx, ny, nz, R4, lo, hi, d_mask):
        """lo, hi: None for a bound that is not tested."""
        self._check(self.lib.tomo_seg_threshold(self.handle, _ptr(stream), _ptr(d_v), int(nx), int(ny), int(nz), int(R4),
                                                0.0 if lo is None else float(lo), 0.0 if hi is None else float(hi), int(lo is not None),
                                                int(hi is not None), _ptr(d_mask)))

    def label(self, stream, d_mask, nx, ny, nz, connectivity, d_labels):
        """-> n, the number of components (waits)."""
        n = _c_i32(0)
        self._check(self.lib.tomo_seg_label(self.handle, _ptr(stream), _ptr(d_mask), int(nx), int(ny), int(nz), int(connectivity),
                                            _ptr(d_labels), ctypes.byref(n)))
        return n.value

    def measure(self, stream, d_labels, d_v, nx, ny, nz, n):
        """-> (count int64 (n,), bbox int32 (n, 6), coord_sum int64 (n, 3), vmin, vmax float32 (n,), vsum float64 (n,)); the last three
        None without d_v.  Waits."""
        n = int(n)
        count, bbox, csum = np.zeros(n, np.int64), np.zeros((n, 6), np.int32), np.zeros((n, 3), np.int64)
        vmin = vmax = vsum = None
        if d_v is not None:
            vmin, vmax, vsum = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float64)
        self._check(self.lib.tomo_seg_measure(self.handle, _ptr(stream), _ptr(d_labels), _ptr(d_v), int(nx), int(ny), int(nz), n, _host(count),
                                              _host(bbox), _host(csum), *(None if a is None else _host(a) for a in (vmin, vmax, vsum))))
        return count, bbox, csum, vmin, vmax, vsum

    def remove_small(self, stream, d_labels, nx, ny, nz, n, min_size, d_out):
        """-> n_kept (waits)."""
        k = _c_i32(0)
        self._check(self.lib.tomo_seg_remove_small(self.handle, _ptr(stream), _ptr(d_labels), int(nx), int(ny), int(nz), int(n), int(min_size),
                                                   _ptr(d_out), ctypes.byref(k)))
        return k.value

    def largest(self, stream, d_labels, nx, ny, nz, n, d_mask):
        """-> (label, count) of the component taken, (0, 0) when n = 0 (waits)."""
        label, count = _c_i32(0), _c_i64(0)
        self._check(self.lib.tomo_seg_largest(self.handle, _ptr(stream), _ptr(d_labels), int(nx), int(ny), int(nz), int(n), _ptr(d_mask),
                                              ctypes.byref(label), ctypes.byref(count)))
        return label.value, count.value
