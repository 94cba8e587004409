"""
ctypes binding of libtomo_cor.so (include/tomo_cor.h): the Fourier-space sinogram metric for the position of the rotation axis --
gather of detector rows out of a device sinogram, the float64 spline prefilter, the stacked 360-degree sinograms built into the hipFFT
buffer, and the masked magnitude reduction: the device operations of rotation_axis.find_center.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

import numpy as np

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_COR_LIB") or os.path.join(_HERE, "libtomo_cor.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_double = ctypes.c_double
_c_float = ctypes.c_float
_c_size = ctypes.c_size_t
_int_p = ctypes.POINTER(_c_int)
_double_p = ctypes.POINTER(_c_double)
_float_p = ctypes.POINTER(_c_float)

ERR_UNSUPPORTED = 4       # TOMO_COR_ERR_UNSUPPORTED
MIN_N, MIN_NX = 8, 16     # TOMO_COR_MIN_N, TOMO_COR_MIN_NX
MAX_NX = 8192             # TOMO_COR_MAX_NX
MAX_R = 16384             # TOMO_COR_MAX_R
MAX_SLICES = 4096         # TOMO_COR_MAX_SLICES
LOAD_PASSES = ("gather", "prefilter")            # TOMO_COR_MS_* of tomo_cor_load
METRIC_PASSES = ("build", "r2c", "reduce")       # TOMO_COR_MS_* of tomo_cor_metric

# every symbol include/tomo_cor.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_cor_abi_version": (_c_int, []),
    "tomo_cor_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_cor_destroy": (_c_int, [_c_vp]),
    "tomo_cor_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_cor_check_shape": (_c_int, [_c_int, _c_int, _c_int]),
    "tomo_cor_wedge": (_c_int, [_c_int, _c_int, _c_double, _c_int, _int_p]),
    "tomo_cor_batch": (_c_int, [_c_int, _c_int, _c_int, _c_size, _int_p]),
    "tomo_cor_device_bytes": (_c_int, [_c_vp, ctypes.POINTER(ctypes.c_int64)]),
    "tomo_cor_plan_seconds": (_c_int, [_c_vp, _double_p]),
    "tomo_cor_load": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _int_p, _c_int, _float_p]),
    "tomo_cor_metric": (_c_int, [_c_vp, _c_vp, _int_p, _double_p, _c_int, _c_double, _c_int, _c_size, _double_p, _float_p]),
    "tomo_cor_debug_build": (_c_int, [_c_vp, _c_vp, _c_int, _c_double, _float_p]),
    "tomo_cor_debug_sinogram": (_c_int, [_c_vp, _c_vp, _c_int, _float_p]),
    "tomo_cor_debug_coefficients": (_c_int, [_c_vp, _c_vp, _c_int, _double_p]),
}


class CorUnsupported(TomoError):
    """A sinogram shape beyond the library's limits (MIN_N, MIN_NX, MAX_NX, MAX_R, MAX_SLICES); raised before anything is launched."""


def load():
    """Load libtomo_cor.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("cor", LIB_PATH, SIGNATURES)


ERRORS = {ERR_UNSUPPORTED: CorUnsupported}


def check_shape(n, nx, nslices=1):
    """CorUnsupported for sinograms the library does not take.  Needs no device."""
    lib = load()
    _binding.check(lib, "cor", lib.tomo_cor_check_shape(int(n), int(nx), int(nslices)), None, ERRORS)


def wedge(n, nx, ratio=0.5, drop=20):
    """The mask as the reduction uses it: for each of the 2 n rows of the transform the last column 2 <= ku <= hi of the half-spectrum
    that counts (0: the row is cut).  Needs no device."""
    lib = load()
    hi = np.zeros(2 * int(n), np.int32)
    _binding.check(lib, "cor", lib.tomo_cor_wedge(int(n), int(nx), float(ratio), int(drop), hi.ctypes.data_as(_int_p)), None, ERRORS)
    return hi


def batch(npairs, n, nx, max_scratch_bytes=0):
    """The (slice, t) pairs per batch tomo_cor_metric starts from for this shape and scratch budget (0: no limit).  Needs no device."""
    lib = load()
    b = _c_int(0)
    _binding.check(lib, "cor", lib.tomo_cor_batch(int(npairs), int(n), int(nx), int(max_scratch_bytes), ctypes.byref(b)), None, ERRORS)
    return b.value


class CorHandle(Handle):
    """One tomo_cor handle: a device, the loaded sinograms with their spline coefficients, the batch buffer, the hipFFT plans with
    their shared work area, and the last error.  A context manager; close() frees everything.  device: the tomo context's
    (ctx.device) -- every call is enqueued on the stream it is given, in practice that context's; metric() and the debug calls wait."""

    NAME = "cor"
    load = staticmethod(load)
    ERRORS = ERRORS

    def __init__(self, device=0):
        super(CorHandle, self).__init__(device)
        self.shape = None           # (nslices, n, nx) of the last load

    def load_rows(self, stream, d_p, n_p, nx, nz, first, n, rows, timed=False):
        """Gather the detector rows `rows` of the device sinogram p[n_p][nx][nz], angles first .. first + n - 1, and prefilter them.
        timed=True waits and returns the device ms of the two passes."""
        rows = np.ascontiguousarray(rows, np.int32).ravel()
        ms = (_c_float * len(LOAD_PASSES))() if timed else None
        self.shape = None
        self._check(self.lib.tomo_cor_load(self.handle, _ptr(stream), _ptr(d_p), int(n_p), int(nx), int(nz), int(first), int(n),
                                           rows.ctypes.data_as(_int_p), int(rows.size), ms))
        self.shape = (int(rows.size), int(n), int(nx))
        return tuple(ms) if timed else None

    def metric(self, stream, slices, ts, ratio=0.5, drop=20, max_scratch_bytes=0, timed=False):
        """m of every pair (slices[k], ts[k]) as float64; waits.  timed=True: (m, device ms of build, R2C, reduce)."""
        slices = np.ascontiguousarray(slices, np.int32).ravel()
        ts = np.ascontiguousarray(ts, np.float64).ravel()
        if slices.size != ts.size:
            raise ValueError("metric: %d slices for %d shifts" % (slices.size, ts.size))
        m = np.zeros(ts.size, np.float64)
        ms = (_c_float * len(METRIC_PASSES))() if timed else None
        self._check(self.lib.tomo_cor_metric(self.handle, _ptr(stream), slices.ctypes.data_as(_int_p), ts.ctypes.data_as(_double_p),
                                             int(ts.size), float(ratio), int(drop), int(max_scratch_bytes), m.ctypes.data_as(_double_p), ms))
        return (m, tuple(ms)) if timed else m

    def _loaded_shape(self):
        if self.shape is None:
            raise TomoError("cor handle: no sinogram is loaded")
        return self.shape

    def debug_build(self, stream, slice_, t):
        """M_t of one pair as the build kernel wrote it, float32 (2 n, nx)."""
        _, n, nx = self._loaded_shape()
        out = np.zeros((2 * n, nx), np.float32)
        self._check(self.lib.tomo_cor_debug_build(self.handle, _ptr(stream), int(slice_), float(t), out.ctypes.data_as(_float_p)))
        return out

    def debug_sinogram(self, stream, slice_):
        _, n, nx = self._loaded_shape()
        out = np.zeros((n, nx), np.float32)
        self._check(self.lib.tomo_cor_debug_sinogram(self.handle, _ptr(stream), int(slice_), out.ctypes.data_as(_float_p)))
        return out

    def debug_coefficients(self, stream, slice_):
        _, n, nx = self._loaded_shape()
        out = np.zeros((n, nx), np.float64)
        self._check(self.lib.tomo_cor_debug_coefficients(self.handle, _ptr(stream), int(slice_), out.ctypes.data_as(_double_p)))
        return out
