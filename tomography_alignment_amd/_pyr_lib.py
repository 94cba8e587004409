"""
ctypes binding of libtomo_pyr.so (include/tomo_pyr.h): binning of device sinograms and volumes and the prolongation of a coarse
reconstruction, the device operations of multires.py.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os
import threading

from ._lib import TomoError

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

_lib = None
_lock = threading.Lock()


class PyrUnsupported(TomoError):
    """A binning the kernels do not support: a factor other than 2, 4 or 8, or an extent the factor does not divide."""


def load():
    """Load libtomo_pyr.so and bind every symbol; raises TomoError (never falls back) on failure."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise TomoError("libtomo_pyr.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` or "
                                "`make -C tomography_alignment_amd/csrc/pyr`; there is no CPU fallback" % LIB_PATH)
            try:
                lib = ctypes.CDLL(LIB_PATH)
            except OSError as e:
                raise TomoError("cannot load %s: %s" % (LIB_PATH, e))
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)          # AttributeError if include/tomo_pyr.h and the .so disagree
                fn.restype = res
                fn.argtypes = args
            if lib.tomo_pyr_abi_version() != 1:
                raise TomoError("libtomo_pyr.so ABI version mismatch")
            _lib = lib
    return _lib


class PyrHandle(object):
    """One tomo_pyr handle: a device and the last error.  A context manager.  device: the tomo context's (ctx.device) -- every call is
    enqueued on the stream it is given, in practice that context's, and none synchronises."""

    def __init__(self, device=0):
        self._h = None
        self.lib = load()
        h = _c_vp()
        self._check(self.lib.tomo_pyr_create(int(device), ctypes.byref(h)), None)
        self._h = h
        self.device = int(device)

    def _check(self, rc, h="self"):
        if rc != 0:
            msg = (self.lib.tomo_pyr_last_error(self._h if h == "self" else h) or b"").decode(errors="replace")
            raise (PyrUnsupported if rc == ERR_UNSUPPORTED else TomoError)("libtomo_pyr error %d: %s" % (rc, msg))

    @property
    def handle(self):
        if self._h is None:
            raise TomoError("pyr handle closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None:
            self.lib.tomo_pyr_destroy(self._h)
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

    def bin_sino(self, stream, d_src, n, nx, nz, f, scale, d_dst):
        self._check(self.lib.tomo_pyr_bin_sino(self.handle, _ptr(stream), _ptr(d_src), int(n), int(nx), int(nz), int(f), float(scale),
                                               _ptr(d_dst)))

    def bin_vol(self, stream, d_src, nx, ny, nz, f, scale, d_dst):
        self._check(self.lib.tomo_pyr_bin_vol(self.handle, _ptr(stream), _ptr(d_src), int(nx), int(ny), int(nz), int(f), float(scale),
                                              _ptr(d_dst)))

    def prolong_vol(self, stream, d_src, nx, ny, nz, scale, d_dst):
        self._check(self.lib.tomo_pyr_prolong_vol(self.handle, _ptr(stream), _ptr(d_src), int(nx), int(ny), int(nz), float(scale),
                                                  _ptr(d_dst)))


def _ptr(p):
    if isinstance(p, ctypes.c_void_p):
        return p
    return _c_vp(int(p)) if p else None
