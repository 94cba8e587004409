"""
ctypes binding of libtomo_vreg.so (include/tomo_vreg.h): the masked, mean-free FFT input of two device volumes, their cross-power
spectrum and its coarse peak, the upsampled-DFT refinement of the peak, the Fourier shift and the deterministic argmax -- the device
operations of registration.py.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

import numpy as np

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_VREG_LIB") or os.path.join(_HERE, "libtomo_vreg.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_double = ctypes.c_double

ERR_UNSUPPORTED = 4       # TOMO_VREG_ERR_UNSUPPORTED
MAX_N = 2048              # TOMO_VREG_MAX_N
MAX_UPSAMPLE = 100        # TOMO_VREG_MAX_UPSAMPLE
MASK_NONE, MASK_ARRAY, MASK_SPHERE = 0, 1, 2
NORM_NONE, NORM_PHASE = 0, 1

# every symbol include/tomo_vreg.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_vreg_abi_version": (_c_int, []),
    "tomo_vreg_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_vreg_destroy": (_c_int, [_c_vp]),
    "tomo_vreg_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_vreg_check": (_c_int, [_c_int, _c_int, _c_int, _c_int]),
    "tomo_vreg_set_shape": (_c_int, [_c_vp, _c_int, _c_int, _c_int]),
    "tomo_vreg_device_bytes": (_c_int, [_c_vp, ctypes.POINTER(ctypes.c_int64)]),
    "tomo_vreg_plan_seconds": (_c_int, [_c_vp, ctypes.POINTER(_c_double)]),
    "tomo_vreg_set_scratch_bytes": (_c_int, [_c_vp, ctypes.c_size_t]),
    "tomo_vreg_prepare": (_c_int, [_c_vp, _c_vp, _c_int, _c_vp, _c_int, _c_vp, _c_double, _c_double, _c_int]),
    "tomo_vreg_correlate": (_c_int, [_c_vp, _c_vp, _c_int]),
    "tomo_vreg_refine": (_c_int, [_c_vp, _c_vp, _c_int]),
    "tomo_vreg_fetch": (_c_int, [_c_vp, _c_vp, _c_vp]),
    "tomo_vreg_shift": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_vp]),
    "tomo_vreg_argmax": (_c_int, [_c_vp, _c_vp, _c_vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_float)]),
}


class VregUnsupported(TomoError):
    """A shape or an upsampling the library does not handle: an axis shorter than 2 or longer than MAX_N, more than 2^31 - 1 values,
    upsample outside 1 ... MAX_UPSAMPLE."""


def load():
    """Load libtomo_vreg.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("vreg", LIB_PATH, SIGNATURES)


ERRORS = {ERR_UNSUPPORTED: VregUnsupported}


def check(nx, ny, nz, upsample=0):
    """VregUnsupported for a shape (and, unless 0, an upsampling) the library refuses.  Needs no device."""
    lib = load()
    _binding.check(lib, "vreg", lib.tomo_vreg_check(int(nx), int(ny), int(nz), int(upsample)), None, ERRORS)


class VregHandle(Handle):
    """One tomo_vreg handle: a device, the hipFFT plans, padded buffers and scratch of the shapes it has seen, and the last error.  A
    context manager.  device: the tomo context's (ctx.device) -- every call is enqueued on the stream it is given, in practice that
    context's, and only fetch() and argmax() synchronise."""

    NAME = "vreg"
    load = staticmethod(load)
    ERRORS = ERRORS
    shape = None              # (nx, ny, nz) of the last set_shape

    def set_shape(self, nx, ny, nz):
        """The shape of the calls that follow.  Raises VregUnsupported before anything is allocated or launched."""
        shape = (int(nx), int(ny), int(nz))
        self._check(self.lib.tomo_vreg_set_shape(self.handle, *shape))
        self.shape = shape

    def set_scratch_bytes(self, nbytes):
        """The budget of refine's z-contraction scratch (0: the default, 1 GiB); it changes no bit of a result."""
        self._check(self.lib.tomo_vreg_set_scratch_bytes(self.handle, int(nbytes)))

    def prepare(self, stream, slot, d_vol, mask=MASK_NONE, d_mask=None, radius=0.0, edge=0.0, subtract_mean=True):
        self._check(self.lib.tomo_vreg_prepare(self.handle, _ptr(stream), int(slot), _ptr(d_vol), int(mask), _ptr(d_mask), float(radius),
                                               float(edge), 1 if subtract_mean else 0))

    def correlate(self, stream, normalization=NORM_NONE):
        self._check(self.lib.tomo_vreg_correlate(self.handle, _ptr(stream), int(normalization)))

    def refine(self, stream, upsample):
        self._check(self.lib.tomo_vreg_refine(self.handle, _ptr(stream), int(upsample)))

    def fetch(self, stream):
        """float64 (8,): shift[3], peak, E[0], E[1], the coarse flat index, upsample.  Waits for the stream."""
        out = np.empty(8, np.float64)
        self._check(self.lib.tomo_vreg_fetch(self.handle, _ptr(stream), out.ctypes.data_as(_c_vp)))
        return out

    def shift(self, stream, d_src, shift, d_dst):
        s = np.ascontiguousarray(shift, np.float64)
        if s.shape != (3,):
            raise ValueError("shift must have three values, got shape %s" % (s.shape,))
        self._check(self.lib.tomo_vreg_shift(self.handle, _ptr(stream), _ptr(d_src), s.ctypes.data_as(_c_vp), _ptr(d_dst)))

    def argmax(self, stream, d_vol):
        """(flat index, value) of the largest element of a float32 device volume of the shape set.  Waits for the stream."""
        i, v = ctypes.c_int64(0), ctypes.c_float(0)
        self._check(self.lib.tomo_vreg_argmax(self.handle, _ptr(stream), _ptr(d_vol), ctypes.byref(i), ctypes.byref(v)))
        return i.value, np.float32(v.value)
