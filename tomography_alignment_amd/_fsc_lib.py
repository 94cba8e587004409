"""
ctypes binding of libtomo_fsc.so (include/tomo_fsc.h): the masked, mean-free FFT input of a device volume or stack, its in-place hipFFT
R2C transform, and the deterministic float64 shell / ring sums of two spectra -- the device operations of resolution.py.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

import numpy as np

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_FSC_LIB") or os.path.join(_HERE, "libtomo_fsc.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_double = ctypes.c_double
_c_size = ctypes.c_size_t

ERR_UNSUPPORTED = 4       # TOMO_FSC_ERR_UNSUPPORTED
MAX_N = 2048              # TOMO_FSC_MAX_N
MAX_PLANES = 65535        # TOMO_FSC_MAX_PLANES
MASK_NONE, MASK_ARRAY, MASK_SPHERE = 0, 1, 2

# every symbol include/tomo_fsc.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_fsc_abi_version": (_c_int, []),
    "tomo_fsc_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_fsc_destroy": (_c_int, [_c_vp]),
    "tomo_fsc_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_fsc_n_shells": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, ctypes.POINTER(_c_int)]),
    "tomo_fsc_set_shape": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_int, _c_int]),
    "tomo_fsc_device_bytes": (_c_int, [_c_vp, ctypes.POINTER(ctypes.c_int64)]),
    "tomo_fsc_plan_seconds": (_c_int, [_c_vp, ctypes.POINTER(_c_double)]),
    "tomo_fsc_prepare": (_c_int, [_c_vp, _c_vp, _c_int, _c_vp, _c_int, _c_vp, _c_double, _c_double, _c_int]),
    "tomo_fsc_fft": (_c_int, [_c_vp, _c_vp, _c_int]),
    "tomo_fsc_reduce": (_c_int, [_c_vp, _c_vp]),
    "tomo_fsc_fetch": (_c_int, [_c_vp, _c_vp, _c_vp]),
    "tomo_fsc_take_rows": (_c_int, [_c_vp, _c_vp, _c_vp, _c_size, _c_size, _c_size, _c_size, _c_vp]),
}


class FscUnsupported(TomoError):
    """A shape the library does not handle: an axis shorter than 2 or longer than MAX_N, more than MAX_PLANES planes."""


def load():
    """Load libtomo_fsc.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("fsc", LIB_PATH, SIGNATURES)


ERRORS = {ERR_UNSUPPORTED: FscUnsupported}


def n_shells(ndim, nb, nx, ny, nz):
    """min(n) / 2 + 1 of a shape the library handles; FscUnsupported otherwise.  Needs no device."""
    lib = load()
    n = _c_int(0)
    _binding.check(lib, "fsc", lib.tomo_fsc_n_shells(int(ndim), int(nb), int(nx), int(ny), int(nz), ctypes.byref(n)), None, ERRORS)
    return n.value


class FscHandle(Handle):
    """One tomo_fsc handle: a device, the hipFFT plans and spectrum buffers of the shapes it has seen, and the last error.  A context
    manager.  device: the tomo context's (ctx.device) -- every call is enqueued on the stream it is given, in practice that context's,
    and only fetch() synchronises."""

    NAME = "fsc"
    load = staticmethod(load)
    ERRORS = ERRORS
    shape = None              # (ndim, nb, nx, ny, nz) of the last set_shape

    def set_shape(self, ndim, nb, nx, ny, nz):
        """The shape of the calls that follow; returns the number of shells.  Raises FscUnsupported before anything is launched."""
        shape = (int(ndim), int(nb), int(nx), int(ny), int(nz))
        self._check(self.lib.tomo_fsc_set_shape(self.handle, *shape))
        self.shape = shape
        self.n_shells = n_shells(*shape)
        return self.n_shells

    def prepare(self, stream, slot, d_vol, mask=MASK_NONE, d_mask=None, radius=0.0, edge=0.0, subtract_mean=True):
        self._check(self.lib.tomo_fsc_prepare(self.handle, _ptr(stream), int(slot), _ptr(d_vol), int(mask), _ptr(d_mask), float(radius),
                                              float(edge), 1 if subtract_mean else 0))

    def fft(self, stream, slot):
        self._check(self.lib.tomo_fsc_fft(self.handle, _ptr(stream), int(slot)))

    def reduce(self, stream):
        self._check(self.lib.tomo_fsc_reduce(self.handle, _ptr(stream)))

    def fetch(self, stream):
        """The table of the last reduce(): float64 (nb, 4, n_shells) in the order C, PA, PB, n.  Waits for the stream."""
        out = np.empty((self.shape[1], 4, self.n_shells), np.float64)
        self._check(self.lib.tomo_fsc_fetch(self.handle, _ptr(stream), out.ctypes.data_as(_c_vp)))
        return out

    def take_rows(self, stream, d_src, row_elems, first, step, count, d_dst):
        self._check(self.lib.tomo_fsc_take_rows(self.handle, _ptr(stream), _ptr(d_src), int(row_elems), int(first), int(step), int(count),
                                                _ptr(d_dst)))
