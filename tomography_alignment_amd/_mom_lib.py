"""
ctypes binding of libtomo_mom.so (include/tomo_mom.h): both marginals of every projection of a device sinogram p[n][nx][nz] in one
read of p -- Q[n][nx] (summed over a window of z), Z[n][nz] (summed over x) and the count of non-finite values, in float64 and with
deterministic sums: the device operation of align.consistency.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

import numpy as np

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_MOM_LIB") or os.path.join(_HERE, "libtomo_mom.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_double = ctypes.c_double
_c_size = ctypes.c_size_t
_int_p = ctypes.POINTER(_c_int)
_double_p = ctypes.POINTER(_c_double)

ERR_UNSUPPORTED = 4       # TOMO_MOM_ERR_UNSUPPORTED
MAX_NZ = 16384            # TOMO_MOM_MAX_NZ
TILE_X = 128              # TOMO_MOM_TILE_X
CHUNK_Z = 1024            # TOMO_MOM_CHUNK_Z

# every symbol include/tomo_mom.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_mom_abi_version": (_c_int, []),
    "tomo_mom_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_mom_destroy": (_c_int, [_c_vp]),
    "tomo_mom_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_mom_check_shape": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "tomo_mom_scratch_bytes": (_c_int, [_c_int, _c_int, ctypes.POINTER(_c_size)]),
    "tomo_mom_batch": (_c_int, [_c_int, _c_int, _c_int, _c_size, _int_p]),
    "tomo_mom_set_max_scratch": (_c_int, [_c_vp, _c_size]),
    "tomo_mom_device_bytes": (_c_int, [_c_vp, ctypes.POINTER(ctypes.c_int64)]),
    "tomo_mom_marginals": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_double, _c_int, _c_int, _double_p, _double_p, _int_p]),
    "tomo_mom_fetch": (_c_int, [_c_vp, _c_vp, _double_p, _double_p, _int_p]),
}


class MomUnsupported(TomoError):
    """A shape or a z window beyond the library's limits (1 <= n, 1 <= nx, 1 <= nz <= MAX_NZ, 0 <= z0 < z1 <= nz); raised before
    anything is launched."""


def load():
    """Load libtomo_mom.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("mom", LIB_PATH, SIGNATURES)


ERRORS = {ERR_UNSUPPORTED: MomUnsupported}


def check_shape(n, nx, nz, z0=0, z1=None):
    """MomUnsupported for a stack or a window the library does not take.  Needs no device."""
    lib = load()
    _binding.check(lib, "mom", lib.tomo_mom_check_shape(int(n), int(nx), int(nz), int(z0), int(nz if z1 is None else z1)), None, ERRORS)


def scratch_bytes(nx, nz):
    """Bytes of partial sums one projection needs.  Needs no device."""
    lib = load()
    b = _c_size(0)
    _binding.check(lib, "mom", lib.tomo_mom_scratch_bytes(int(nx), int(nz), ctypes.byref(b)), None, ERRORS)
    return b.value


def batch(n, nx, nz, max_scratch_bytes=0):
    """The projections per batch for this shape and scratch budget (0: no limit; never fewer than one).  Needs no device."""
    lib = load()
    b = _c_int(0)
    _binding.check(lib, "mom", lib.tomo_mom_batch(int(n), int(nx), int(nz), int(max_scratch_bytes), ctypes.byref(b)), None, ERRORS)
    return b.value


class MomHandle(Handle):
    """One tomo_mom handle: a device, the partial sums, the device tables Q, Z and bad, and the last error.  A context manager; close()
    frees everything.  device: the tomo context's (ctx.device) -- every call is enqueued on the stream it is given, in practice that
    context's; only a call that hands the tables to the host waits."""

    NAME = "mom"
    load = staticmethod(load)
    ERRORS = ERRORS

    def __init__(self, device=0):
        super(MomHandle, self).__init__(device)
        self.shape = None           # (n, nx, nz) of the last marginals()

    def set_max_scratch(self, max_scratch_bytes):
        """The budget of the partial sums for the calls that follow (0 / None: no limit)."""
        self._check(self.lib.tomo_mom_set_max_scratch(self.handle, int(max_scratch_bytes or 0)))

    def marginals(self, stream, d_p, n, nx, nz, floor=-np.inf, z0=0, z1=None, fetch=True):
        """The marginals of the device sinogram p[n][nx][nz].  fetch=True waits and returns (Q (n, nx), Z (n, nz) float64, bad (n,)
        int32); fetch=False only enqueues (fetch() hands the tables over later)."""
        n, nx, nz = int(n), int(nx), int(nz)
        z1 = nz if z1 is None else int(z1)
        self.shape = None
        if fetch:
            Q, Z, bad = np.zeros((n, nx), np.float64), np.zeros((n, nz), np.float64), np.zeros(n, np.int32)
            args = (Q.ctypes.data_as(_double_p), Z.ctypes.data_as(_double_p), bad.ctypes.data_as(_int_p))
        else:
            args = (None, None, None)
        self._check(self.lib.tomo_mom_marginals(self.handle, _ptr(stream), _ptr(d_p), n, nx, nz, float(floor), int(z0), z1, *args))
        self.shape = (n, nx, nz)
        return (Q, Z, bad) if fetch else None

    def fetch(self, stream):
        """(Q, Z, bad) of the last marginals(); waits for the stream."""
        if self.shape is None:
            raise TomoError("mom handle: no marginals were computed")
        n, nx, nz = self.shape
        Q, Z, bad = np.zeros((n, nx), np.float64), np.zeros((n, nz), np.float64), np.zeros(n, np.int32)
        self._check(self.lib.tomo_mom_fetch(self.handle, _ptr(stream), Q.ctypes.data_as(_double_p), Z.ctypes.data_as(_double_p),
                                            bad.ctypes.data_as(_int_p)))
        return Q, Z, bad
