"""
ctypes binding of libtomo_pyr.so (include/tomo_pyr.h): binning of device sinograms and volumes and the prolongation of a coarse
reconstruction, the device operations of multires.py.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_PYR_LIB") or os.path.join(_HERE, "libtomo_pyr.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_float = ctypes.c_float

ERR_UNSUPPORTED = 4       # TOMO_PYR_ERR_UNSUPPORTED
MAX_FACTOR = 8            # TOMO_PYR_MAX_FACTOR
FACTORS = (2, 4, 8)

# every symbol include/tomo_pyr.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_pyr_abi_version": (_c_int, []),
    "tomo_pyr_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_pyr_destroy": (_c_int, [_c_vp]),
    "tomo_pyr_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_pyr_bin_sino": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_float, _c_vp]),
    "tomo_pyr_bin_vol": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_float, _c_vp]),
    "tomo_pyr_prolong_vol": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_float, _c_vp]),
}


class PyrUnsupported(TomoError):
    """A binning the kernels do not support: a factor other than 2, 4 or 8, or an extent the factor does not divide."""


def load():
    """Load libtomo_pyr.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("pyr", LIB_PATH, SIGNATURES)


class PyrHandle(Handle):
    """One tomo_pyr handle: a device and the last error.  A context manager.  device: the tomo context's (ctx.device) -- every call is
    enqueued on the stream it is given, in practice that context's, and none synchronises."""

    NAME = "pyr"
    load = staticmethod(load)
    ERRORS = {ERR_UNSUPPORTED: PyrUnsupported}

    def bin_sino(self, stream, d_src, n, nx, nz, f, scale, d_dst):
        self._check(self.lib.tomo_pyr_bin_sino(self.handle, _ptr(stream), _ptr(d_src), int(n), int(nx), int(nz), int(f), float(scale),
                                               _ptr(d_dst)))

    def bin_vol(self, stream, d_src, nx, ny, nz, f, scale, d_dst):
        self._check(self.lib.tomo_pyr_bin_vol(self.handle, _ptr(stream), _ptr(d_src), int(nx), int(ny), int(nz), int(f), float(scale),
                                              _ptr(d_dst)))

    def prolong_vol(self, stream, d_src, nx, ny, nz, scale, d_dst):
        self._check(self.lib.tomo_pyr_prolong_vol(self.handle, _ptr(stream), _ptr(d_src), int(nx), int(ny), int(nz), float(scale),
                                                  _ptr(d_dst)))
