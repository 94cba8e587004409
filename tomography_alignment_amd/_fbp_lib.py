"""
ctypes binding of libtomo_fbp.so (include/tomo_fbp.h): the ramp filter of recon/fbp.py.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

import numpy as np

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_FBP_LIB") or os.path.join(_HERE, "libtomo_fbp.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_dp = ctypes.POINTER(ctypes.c_double)
_c_int = ctypes.c_int

ERR_UNSUPPORTED = 4       # TOMO_FBP_ERR_UNSUPPORTED

# every symbol include/tomo_fbp.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_fbp_abi_version": (_c_int, []),
    "tomo_fbp_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_fbp_destroy": (_c_int, [_c_vp]),
    "tomo_fbp_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_fbp_set_response": (_c_int, [_c_vp, _c_int, _c_dp]),
    "tomo_fbp_filter": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_dp]),
}


class FbpUnsupported(TomoError):
    """The detector is wider than the kernel supports (ndx > 4096)."""


def response_length(ndx):
    """Npad/2 + 1, the number of doubles tomo_fbp_set_response reads for detector width ndx (Npad: recon/fbp.py::padded_length)."""
    from .recon.fbp import padded_length
    return padded_length(ndx) // 2 + 1


def load():
    """Load libtomo_fbp.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("fbp", LIB_PATH, SIGNATURES)


class FbpHandle(Handle):
    """One tomo_fbp handle: a device, the twiddle and response tables and the device copy of the scales.  A context manager; close()
    frees everything.  device: the tomo context's (ctx.device) -- the filter runs on that context's stream."""

    NAME = "fbp"
    load = staticmethod(load)
    ERRORS = {ERR_UNSUPPORTED: FbpUnsupported}

    def set_response(self, ndx, table):
        """The response H[0 .. Npad/2] (recon/fbp.py::filter_response) for detector width ndx.  The C call takes the table without a
        length and reads response_length(ndx) doubles from it, so any other length is a ValueError here, before the call."""
        t = np.ascontiguousarray(table, np.float64)
        # ndx < 1 has no length to check: it goes to the library, which refuses it (TOMO_FBP_ERR_ARG) before it reads the table
        if int(ndx) >= 1 and t.size != response_length(ndx):
            raise ValueError("set_response: the table for ndx %d must hold Npad/2 + 1 = %d values, not %d"
                             % (int(ndx), response_length(ndx), t.size))
        self._check(self.lib.tomo_fbp_set_response(self.handle, int(ndx), t.ctypes.data_as(_c_dp)))

    def filter(self, stream, d_in, d_out, n_proj, ndx, ndz, scales):
        """Enqueue q = scales * filter(p) on `stream`; d_in / d_out device pointers (may be equal)."""
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(scales, np.float64), (int(n_proj),)))
        self._check(self.lib.tomo_fbp_filter(self.handle, _ptr(stream), _ptr(d_in), _ptr(d_out), int(n_proj), int(ndx),
                                             int(ndz), s.ctypes.data_as(_c_dp)))
