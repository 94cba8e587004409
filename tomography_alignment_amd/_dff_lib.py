"""
ctypes binding of libtomo_dff.so (include/tomo_dff.h): dynamic flat-field correction -- the Gram matrix of the flats, the eigen flat
fields, the binning, the total-variation cost and gradient of any subset of the projections in one launch, and the normalisation with a
flat per projection: the device operations of preprocess.eigen_flats and preprocess.normalize_dynamic.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

import numpy as np

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_DFF_LIB") or os.path.join(_HERE, "libtomo_dff.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_float = ctypes.c_float
_c_size = ctypes.c_size_t
_int_p = ctypes.POINTER(_c_int)
_float_p = ctypes.POINTER(_c_float)
_double_p = ctypes.POINTER(ctypes.c_double)

ERR_UNSUPPORTED = 4       # TOMO_DFF_ERR_UNSUPPORTED
MAX_FLATS = 128           # TOMO_DFF_MAX_FLATS
MAX_EFF = 8               # TOMO_DFF_MAX_EFF
MAX_BIN = 8               # TOMO_DFF_MAX_BIN
TILE_Z, TILE_X = 16, 64   # TOMO_DFF_TILE_Z, TOMO_DFF_TILE_X
MAX_IDS = 65535           # TOMO_DFF_MAX_IDS
U16, F32 = 0, 1           # tomo_dff_dtype

# every symbol include/tomo_dff.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_dff_abi_version": (_c_int, []),
    "tomo_dff_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_dff_destroy": (_c_int, [_c_vp]),
    "tomo_dff_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_dff_check": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int]),
    "tomo_dff_gram_chunk": (_c_int, [_c_int, _int_p]),
    "tomo_dff_scratch_bytes": (_c_int, [_c_int, _c_int, _c_int, ctypes.POINTER(_c_size)]),
    "tomo_dff_batch": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_size, _int_p]),
    "tomo_dff_set_max_scratch": (_c_int, [_c_vp, _c_size]),
    "tomo_dff_device_bytes": (_c_int, [_c_vp, ctypes.POINTER(ctypes.c_int64)]),
    "tomo_dff_gram": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp, _double_p]),
    "tomo_dff_eff": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp, _double_p, _c_int, _c_vp]),
    "tomo_dff_bin": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_vp, _c_vp]),
    "tomo_dff_load": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "tomo_dff_cost": (_c_int, [_c_vp, _c_vp, _c_int, _int_p, _float_p, _float_p, _float_p, _c_int, _c_float, _c_vp, _c_vp, _double_p]),
    "tomo_dff_apply": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_vp, _c_int, _float_p, _c_int, _c_int, _c_int,
                                _c_int, _c_int, _c_float, _c_int, _c_float, _c_vp]),
}


class DffUnsupported(TomoError):
    """Flats, eigen flat fields, a frame or a bin factor beyond the library's limits (2 <= K <= MAX_FLATS, 0 <= m <= MAX_EFF and
    m <= K - 1, 1 <= bin <= MAX_BIN with rows // bin >= 2 and cols // bin >= 2); raised before anything is launched."""


def load():
    """Load libtomo_dff.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("dff", LIB_PATH, SIGNATURES)


ERRORS = {ERR_UNSUPPORTED: DffUnsupported}


def check(K, m, rows, cols, bin=1):
    """DffUnsupported for what the library does not take.  Needs no device."""
    lib = load()
    _binding.check(lib, "dff", lib.tomo_dff_check(int(K), int(m), int(rows), int(cols), int(bin)), None, ERRORS)


def gram_chunk(K):
    """The pixels of a chunk of the Gram kernel for K flats.  Needs no device."""
    lib = load()
    c = _c_int(0)
    _binding.check(lib, "dff", lib.tomo_dff_gram_chunk(int(K), ctypes.byref(c)), None, ERRORS)
    return c.value


def scratch_bytes(rows, cols, bin):
    """Bytes of binned counts one projection needs.  Needs no device."""
    lib = load()
    b = _c_size(0)
    _binding.check(lib, "dff", lib.tomo_dff_scratch_bytes(int(rows), int(cols), int(bin), ctypes.byref(b)), None, ERRORS)
    return b.value


def batch(n, rows, cols, bin, max_scratch_bytes=0):
    """The projections per batch for this shape and scratch budget (0: no limit; never fewer than one).  Needs no device."""
    lib = load()
    b = _c_int(0)
    _binding.check(lib, "dff", lib.tomo_dff_batch(int(n), int(rows), int(cols), int(bin), int(max_scratch_bytes), ctypes.byref(b)), None, ERRORS)
    return b.value


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


class DffHandle(Handle):
    """One tomo_dff handle: a device, the binned counts of the loaded projections, the partial sums and the last error.  A context
    manager; close() frees everything.  device: the tomo context's (ctx.device) -- every call is enqueued on the stream it is given, in
    practice that context's; gram() and cost() hand results to the host and wait."""

    NAME = "dff"
    load = staticmethod(load)
    ERRORS = ERRORS

    def set_max_scratch(self, max_scratch_bytes):
        """The budget of the binned counts for the calls that follow (0 / None: no limit)."""
        self._check(self.lib.tomo_dff_set_max_scratch(self.handle, int(max_scratch_bytes or 0)))

    def gram(self, stream, d_flats, dtype, K, rows, cols, d_fbar):
        """The (K, K) float64 Gram matrix of the flats' deviations from the float32 frame d_fbar; waits."""
        G = np.zeros((int(K), int(K)), np.float64)
        self._check(self.lib.tomo_dff_gram(self.handle, _ptr(stream), _ptr(d_flats), int(dtype), int(K), int(rows), int(cols), _ptr(d_fbar),
                                           G.ctypes.data_as(_double_p)))
        return G

    def eff(self, stream, d_flats, dtype, K, rows, cols, d_fbar, V, d_eff):
        """d_eff[m][rows][cols] from the (K, m) float64 table V."""
        V = np.ascontiguousarray(V, np.float64)
        V = V.reshape(int(K), V.size // int(K))
        self._check(self.lib.tomo_dff_eff(self.handle, _ptr(stream), _ptr(d_flats), int(dtype), int(K), int(rows), int(cols), _ptr(d_fbar),
                                          V.ctypes.data_as(_double_p), V.shape[1], _ptr(d_eff)))

    def bin(self, stream, d_src, dtype, n, rows, cols, bin, d_dark, d_out):
        """d_out[n][rows // bin][cols // bin] of the n frames d_src, the frame d_dark (None: nothing) subtracted."""
        self._check(self.lib.tomo_dff_bin(self.handle, _ptr(stream), _ptr(d_src), int(dtype), int(n), int(rows), int(cols), int(bin), _ptr(d_dark),
                                          _ptr(d_out)))

    def load_projections(self, stream, d_raw, dtype, i0, nb, rows, cols, bin, d_dark):
        """The binned counts of the projections i0 ... i0 + nb - 1 of the stack d_raw into the scratch."""
        self._check(self.lib.tomo_dff_load(self.handle, _ptr(stream), _ptr(d_raw), int(dtype), int(i0), int(nb), int(rows), int(cols), int(bin),
                                           _ptr(d_dark)))

    def cost(self, stream, ids, w, s, a, eps, d_Fb, d_Eb):
        """(f (len(ids),), g (len(ids), m)) float64 of the loaded projections ids at the weights w (len(ids), m); waits."""
        ids = np.ascontiguousarray(ids, np.int32).ravel()
        a = _f32(a).ravel()
        m = a.size - 1
        w, s = _f32(w).reshape(ids.size, m), _f32(s).reshape(ids.size)
        fg = np.zeros((ids.size, 1 + m), np.float64)
        self._check(self.lib.tomo_dff_cost(self.handle, _ptr(stream), ids.size, ids.ctypes.data_as(_int_p), w.ctypes.data_as(_float_p),
                                           s.ctypes.data_as(_float_p), a.ctypes.data_as(_float_p), m, float(eps), _ptr(d_Fb), _ptr(d_Eb),
                                           fg.ctypes.data_as(_double_p)))
        return fg[:, 0].copy(), fg[:, 1:].copy()

    def apply(self, stream, d_raw, dtype, n, rows, cols, d_fbar, d_dark, d_eff, w, crop, cutoff, minus_log, min_ratio, d_out):
        """The sinogram d_out (n, x1 - x0, z1 - z0) with the flat fbar + sum_j w[i][j] e_j for projection i; w (n, m)."""
        w = _f32(w)
        w = w.reshape(int(n), w.size // max(int(n), 1))
        (z0, z1), (x0, x1) = crop
        self._check(self.lib.tomo_dff_apply(self.handle, _ptr(stream), _ptr(d_raw), int(dtype), int(n), int(rows), int(cols), _ptr(d_fbar),
                                            _ptr(d_dark), _ptr(d_eff), w.shape[1], w.ctypes.data_as(_float_p), int(z0), int(z1), int(x0), int(x1),
                                            int(cutoff is not None), float(cutoff if cutoff is not None else 0.0), int(bool(minus_log)),
                                            float(min_ratio), _ptr(d_out)))
