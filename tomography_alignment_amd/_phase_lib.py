"""
ctypes binding of libtomo_phase.so (include/tomo_phase.h): Paganin phase retrieval of a device-resident stack of transmission frames
(edge-replicating pad, hipFFT R2C, the filter, C2R, crop + clamp + -log) and the -log alone -- the device operations of
preprocess.retrieve_phase and preprocess.minus_log.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

from . import _binding
from ._binding import Handle, _ptr
from ._prep_lib import PrepUnsupported      # preprocess has one Unsupported class, whichever of its two libraries refuses

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_PHASE_LIB") or os.path.join(_HERE, "libtomo_phase.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_double = ctypes.c_double
_c_float = ctypes.c_float
_c_size = ctypes.c_size_t

ERR_UNSUPPORTED = 4       # TOMO_PHASE_ERR_UNSUPPORTED
MAX_P = 8192              # TOMO_PHASE_MAX_P
MAX_STRENGTH = 1e12       # TOMO_PHASE_MAX_STRENGTH
PASSES = ("pad", "r2c", "filter", "c2r", "crop")     # TOMO_PHASE_MS_*

# every symbol include/tomo_phase.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_phase_abi_version": (_c_int, []),
    "tomo_phase_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_phase_destroy": (_c_int, [_c_vp]),
    "tomo_phase_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_phase_padded_length": (_c_int, [_c_int, _c_int, ctypes.POINTER(_c_int)]),
    "tomo_phase_batch": (_c_int, [_c_int, _c_int, _c_int, _c_size, ctypes.POINTER(_c_int)]),
    "tomo_phase_device_bytes": (_c_int, [_c_vp, ctypes.POINTER(ctypes.c_int64)]),
    "tomo_phase_mem_info": (_c_int, [_c_vp, ctypes.POINTER(_c_size), ctypes.POINTER(_c_size)]),
    "tomo_phase_plan_seconds": (_c_int, [_c_vp, ctypes.POINTER(_c_double)]),
    "tomo_phase_retrieve": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_double, _c_int, _c_int, _c_int, _c_float,
                                     _c_size, ctypes.POINTER(_c_float)]),
    "tomo_phase_minus_log": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_size, _c_float]),
}


def load():
    """Load libtomo_phase.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("phase", LIB_PATH, SIGNATURES)


ERRORS = {ERR_UNSUPPORTED: PrepUnsupported}


def padded_length(n, m):
    """The library's padded length of an axis of n values with m values of padding on each side; PrepUnsupported beyond MAX_P.  Needs
    no device."""
    lib = load()
    p = _c_int(0)
    _binding.check(lib, "phase", lib.tomo_phase_padded_length(int(n), int(m), ctypes.byref(p)), None, ERRORS)
    return p.value


def batch(n, px, pz, max_scratch_bytes=0):
    """The frames per batch tomo_phase_retrieve starts from for this padded shape and scratch budget (0: no limit).  Needs no device."""
    lib = load()
    b = _c_int(0)
    _binding.check(lib, "phase", lib.tomo_phase_batch(int(n), int(px), int(pz), int(max_scratch_bytes), ctypes.byref(b)), None, ERRORS)
    return b.value


class PhaseHandle(Handle):
    """One tomo_phase handle: a device, the hipFFT plans of the padded shapes it has seen with their shared work area, and the last
    error.  A context manager; close() frees everything.  device: the tomo context's (ctx.device) -- every call is enqueued on the
    stream it is given, in practice that context's; retrieve() waits for it."""

    NAME = "phase"
    load = staticmethod(load)
    ERRORS = ERRORS

    def mem_info(self):
        """(free, total) bytes of the device's memory, as hipMemGetInfo reports them."""
        f, t = _c_size(0), _c_size(0)
        self._check(self.lib.tomo_phase_mem_info(self.handle, ctypes.byref(f), ctypes.byref(t)))
        return f.value, t.value

    def retrieve(self, stream, d_in, d_out, n, nx, nz, strength, pad_x, pad_z, minus_log=True, min_ratio=1e-6, max_scratch_bytes=0,
                 timed=False):
        """Run the retrieval and wait for it; timed=True returns the device ms of the pad, R2C, filter, C2R and crop passes."""
        ms = (_c_float * len(PASSES))() if timed else None
        self._check(self.lib.tomo_phase_retrieve(self.handle, _ptr(stream), _ptr(d_in), _ptr(d_out), int(n), int(nx), int(nz),
                                                 float(strength), int(pad_x), int(pad_z), 1 if minus_log else 0, float(min_ratio),
                                                 int(max_scratch_bytes), ms))
        return tuple(ms) if timed else None

    def minus_log(self, stream, d_in, d_out, count, min_ratio=1e-6):
        self._check(self.lib.tomo_phase_minus_log(self.handle, _ptr(stream), _ptr(d_in), _ptr(d_out), int(count), float(min_ratio)))
