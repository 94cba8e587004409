"""
ctypes binding of libtomo_phase.so (include/tomo_phase.h): Paganin phase retrieval of a device-resident stack of transmission frames
(edge-replicating pad, hipFFT R2C, the filter, C2R, crop + clamp + -log) and the -log alone -- the device operations of
preprocess.retrieve_phase and preprocess.minus_log.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os
import threading

from ._lib import TomoError
from ._prep_lib import PrepUnsupported

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

_lib = None
_lock = threading.Lock()


def load():
    """Load libtomo_phase.so and bind every symbol; raises TomoError (never falls back) on failure."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise TomoError("libtomo_phase.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` or "
                                "`make -C tomography_alignment_amd/csrc/phase`; there is no CPU fallback" % LIB_PATH)
            try:
                lib = ctypes.CDLL(LIB_PATH)
            except OSError as e:
                raise TomoError("cannot load %s: %s" % (LIB_PATH, e))
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)          # AttributeError if include/tomo_phase.h and the .so disagree
                fn.restype = res
                fn.argtypes = args
            if lib.tomo_phase_abi_version() != 1:
                raise TomoError("libtomo_phase.so ABI version mismatch")
            _lib = lib
    return _lib


def _raise(lib, rc, h):
    msg = (lib.tomo_phase_last_error(h) or b"").decode(errors="replace")
    raise (PrepUnsupported if rc == ERR_UNSUPPORTED else TomoError)("libtomo_phase error %d: %s" % (rc, msg))


def padded_length(n, m):
    """The library's padded length of an axis of n values with m values of padding on each side; PrepUnsupported beyond MAX_P.  Needs
    no device."""
    lib = load()
    p = _c_int(0)
    rc = lib.tomo_phase_padded_length(int(n), int(m), ctypes.byref(p))
    if rc != 0:
        _raise(lib, rc, None)
    return p.value


def batch(n, px, pz, max_scratch_bytes=0):
    """The frames per batch tomo_phase_retrieve starts from for this padded shape and scratch budget (0: no limit).  Needs no device."""
    lib = load()
    b = _c_int(0)
    rc = lib.tomo_phase_batch(int(n), int(px), int(pz), int(max_scratch_bytes), ctypes.byref(b))
    if rc != 0:
        _raise(lib, rc, None)
    return b.value


class PhaseHandle(object):
    """One tomo_phase handle: a device, the hipFFT plans of the padded shapes it has seen with their shared work area, and the last
    error.  A context manager; close() frees everything.  device: the tomo context's (ctx.device) -- every call is enqueued on the
    stream it is given, in practice that context's; retrieve() waits for it."""

    def __init__(self, device=0):
        self._h = None
        self.lib = load()
        h = _c_vp()
        self._check(self.lib.tomo_phase_create(int(device), ctypes.byref(h)), None)
        self._h = h
        self.device = int(device)

    def _check(self, rc, h="self"):
        if rc != 0:
            _raise(self.lib, rc, self._h if h == "self" else h)

    @property
    def handle(self):
        if self._h is None:
            raise TomoError("phase handle closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.lib.tomo_phase_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass

    def device_bytes(self):
        n = ctypes.c_int64(0)
        self._check(self.lib.tomo_phase_device_bytes(self.handle, ctypes.byref(n)))
        return n.value

    def mem_info(self):
        """(free, total) bytes of the device's memory, as hipMemGetInfo reports them."""
        f, t = _c_size(0), _c_size(0)
        self._check(self.lib.tomo_phase_mem_info(self.handle, ctypes.byref(f), ctypes.byref(t)))
        return f.value, t.value

    def plan_seconds(self):
        s = _c_double(0.0)
        self._check(self.lib.tomo_phase_plan_seconds(self.handle, ctypes.byref(s)))
        return s.value

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


def _ptr(p):
    if isinstance(p, ctypes.c_void_p):
        return p
    return _c_vp(int(p)) if p else None
