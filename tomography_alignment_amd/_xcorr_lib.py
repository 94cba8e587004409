"""
ctypes binding of libtomo_xcorr.so (include/tomo_xcorr.h): the cross-correlation pre-alignment of align/align_cc.py.

As with _lib, there is NO CPU fallback: if the library, hipFFT or a device is missing, every entry point raises.
"""
import ctypes
import os

import numpy as np

from . import _binding
from ._binding import Handle, TomoError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_XCORR_LIB") or os.path.join(_HERE, "libtomo_xcorr.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_dp = ctypes.POINTER(ctypes.c_double)
_c_int = ctypes.c_int

# every symbol include/tomo_xcorr.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_xcorr_abi_version": (_c_int, []),
    "tomo_xcorr_device_count": (_c_int, [ctypes.POINTER(_c_int)]),
    "tomo_xcorr_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_xcorr_destroy": (_c_int, [_c_vp]),
    "tomo_xcorr_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_xcorr_device_bytes": (ctypes.c_int64, []),
    "tomo_xcorr_last_timing": (_c_int, [_c_vp, _c_dp]),
    "tomo_xcorr_chain_numpy": (_c_int, [_c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_dp, _c_dp, _c_dp, _c_vp]),
    "tomo_xcorr_chain_skimage": (_c_int, [_c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_dp, _c_vp]),
    "tomo_xcorr_pcc_batch": (_c_int, [_c_vp, _c_dp, _c_dp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_dp, _c_dp, _c_dp]),
    "tomo_xcorr_spline_shift": (_c_int, [_c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_dp, _c_vp]),
}
DTYPES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1}


def load():
    """Load libtomo_xcorr.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("xcorr", LIB_PATH, SIGNATURES)


def device_bytes():
    """Device bytes the library holds now, over every live handle of this process."""
    return int(load().tomo_xcorr_device_bytes())


def _dp(a):
    return a.ctypes.data_as(_c_dp)


class XcorrHandle(Handle):
    """One tomo_xcorr handle: a device, a stream, the hipFFT plans and the work buffers, all kept between calls on it.  A context
    manager; close() frees everything.  The device is chosen as _lib.Context chooses it: LOCAL_RANK modulo the device count."""

    NAME = "xcorr"
    load = staticmethod(load)

    def __init__(self, device=None):
        self._h = None
        lib = load()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        n = ctypes.c_int(0)
        rc = lib.tomo_xcorr_device_count(ctypes.byref(n))
        if rc != 0 or n.value < 1:
            raise TomoError("no HIP device visible (rc=%d: %s); this package has no CPU path"
                            % (rc, (lib.tomo_xcorr_last_error(None) or b"").decode()))
        Handle.__init__(self, int(device) % n.value)

    def last_timing(self):
        """{'plan_s', 'upload_ms', 'steps_ms', 'download_ms'} of the last chain / batch call on this handle (device events; plan
        creation on the host clock, 0 when every plan was cached)."""
        t = np.zeros(4)
        self._check(self.lib.tomo_xcorr_last_timing(self.handle, _dp(t)))
        return dict(plan_s=t[0], upload_ms=t[1], steps_ms=t[2], download_ms=t[3])

    # ---- entry points (arrays are validated by the callers in align/align_cc.py)
    def chain_numpy(self, proj, rfilt, kfilt):
        n, nx, nz = proj.shape
        off = np.zeros((n, 2))
        out = np.empty_like(proj)
        self._check(self.lib.tomo_xcorr_chain_numpy(self.handle, proj.ctypes.data, DTYPES[proj.dtype], n, nx, nz, _dp(rfilt), _dp(kfilt),
                                                    _dp(off), out.ctypes.data))
        return off, out

    def chain_skimage(self, proj, upsample_factor):
        n, nx, nz = proj.shape
        off = np.zeros((n, 2))
        out = np.empty_like(proj)
        self._check(self.lib.tomo_xcorr_chain_skimage(self.handle, proj.ctypes.data, DTYPES[proj.dtype], n, nx, nz, int(upsample_factor),
                                                      _dp(off), out.ctypes.data))
        return off, out

    def pcc_batch(self, refs, movs, upsample_factor, phase):
        B, nx, nz = refs.shape
        shifts = np.zeros((B, 2))
        err = np.zeros(B)
        ph = np.zeros(B)
        self._check(self.lib.tomo_xcorr_pcc_batch(self.handle, _dp(refs), _dp(movs), B, nx, nz, int(upsample_factor), int(bool(phase)),
                                                  _dp(shifts), _dp(err), _dp(ph)))
        return shifts, err, ph

    def spline_shift(self, imgs, shifts):
        B, nx, nz = imgs.shape
        out = np.empty_like(imgs)
        self._check(self.lib.tomo_xcorr_spline_shift(self.handle, imgs.ctypes.data, DTYPES[imgs.dtype], B, nx, nz, _dp(shifts),
                                                     out.ctypes.data))
        return out
