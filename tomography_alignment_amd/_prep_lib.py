"""
ctypes binding of libtomo_prep.so (include/tomo_prep.h): flat-field normalisation and stripe removal of preprocess.py.

As with _lib, there is NO CPU fallback: if the library or a device is missing, every entry point raises.
"""
import ctypes
import os

from . import _binding
from ._binding import Handle, TomoError, _ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TOMO_PREP_LIB") or os.path.join(_HERE, "libtomo_prep.so")   # override: development builds only

_c_vp = ctypes.c_void_p
_c_int = ctypes.c_int
_c_float = ctypes.c_float
_c_fp = ctypes.POINTER(ctypes.c_float)

ERR_UNSUPPORTED = 4       # TOMO_PREP_ERR_UNSUPPORTED
U16, F32 = 0, 1           # TOMO_PREP_U16, TOMO_PREP_F32
MEAN, MEDIAN = 0, 1       # TOMO_PREP_MEAN, TOMO_PREP_MEDIAN
MAX_NPROJ = 8192          # TOMO_PREP_MAX_NPROJ
MAX_MEDIAN_FRAMES = 64
MAX_STRIPE_SIZE = 63
MIN_STRIPE_NDX, MAX_STRIPE_NDX = 8, 8192      # TOMO_PREP_MIN_STRIPE_NDX, TOMO_PREP_MAX_STRIPE_NDX (large / dead / all)
MIN_DEAD_NPROJ = 10       # TOMO_PREP_MIN_DEAD_NPROJ
OUTLIER, MEDIAN2D = 0, 1  # TOMO_PREP_OUTLIER, TOMO_PREP_MEDIAN2D
MAX_OUTLIER_SIZE = 7      # TOMO_PREP_MAX_OUTLIER_SIZE
OUTLIER_SIZES = (3, 5, 7)

# every symbol include/tomo_prep.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tomo_prep_abi_version": (_c_int, []),
    "tomo_prep_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "tomo_prep_destroy": (_c_int, [_c_vp]),
    "tomo_prep_last_error": (ctypes.c_char_p, [_c_vp]),
    "tomo_prep_reference": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_vp]),
    "tomo_prep_normalize": (_c_int, [_c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int,
                                     _c_int, _c_float, _c_int, _c_float, _c_vp]),
    "tomo_prep_stripe_chunk": (_c_int, [_c_int, _c_int, _c_int, ctypes.c_size_t, ctypes.POINTER(_c_int)]),
    "tomo_prep_stripe_sorting": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, ctypes.c_size_t, _c_fp]),
    "tomo_prep_stripe_all_chunk": (_c_int, [_c_int, _c_int, _c_int, ctypes.c_size_t, ctypes.POINTER(_c_int)]),
    "tomo_prep_stripe_large": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_float, _c_int, _c_float, _c_int,
                                        ctypes.c_size_t, _c_vp]),
    "tomo_prep_stripe_dead": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_float, _c_int, _c_int, ctypes.c_size_t,
                                       _c_vp, _c_vp]),
    "tomo_prep_stripe_all": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_float, _c_int, _c_int, ctypes.c_size_t,
                                      _c_vp, _c_vp]),
    "tomo_prep_outlier_batch": (_c_int, [_c_int, _c_int, _c_int, _c_int, ctypes.c_size_t, ctypes.POINTER(_c_int)]),
    "tomo_prep_outlier": (_c_int, [_c_vp, _c_vp, _c_vp, _c_vp, _c_int, _c_int, _c_int, _c_int, _c_int, _c_int, _c_float, _c_int,
                                   ctypes.c_size_t, _c_vp]),
}


class PrepUnsupported(TomoError):
    """A shape the kernels do not support: more than 8192 angles for the stripe removal (or, for the large- and dead-stripe passes, more
    than 8192 columns), or a median over more than 64 frames."""


def load():
    """Load libtomo_prep.so and bind every symbol; raises TomoError (never falls back) on failure."""
    return _binding.load("prep", LIB_PATH, SIGNATURES)


def stripe_chunk(n_proj, ndx, ndz, max_scratch_bytes=0):
    """The z rows per chunk tomo_prep_stripe_sorting uses for this shape and scratch budget (0: no limit)."""
    lib = load()
    zc = _c_int(0)
    _binding.check(lib, "prep", lib.tomo_prep_stripe_chunk(int(n_proj), int(ndx), int(ndz), int(max_scratch_bytes), ctypes.byref(zc)))
    return zc.value


def stripe_all_chunk(n_proj, ndx, ndz, max_scratch_bytes=0):
    """The z rows per chunk tomo_prep_stripe_large / _dead / _all use for this shape and scratch budget (0: no limit)."""
    lib = load()
    zc = _c_int(0)
    _binding.check(lib, "prep", lib.tomo_prep_stripe_all_chunk(int(n_proj), int(ndx), int(ndz), int(max_scratch_bytes), ctypes.byref(zc)))
    return zc.value


def outlier_batch(rows, cols, dtype, n, max_scratch_bytes=0):
    """The frames per batch the in-place tomo_prep_outlier uses for this shape, dtype (U16 / F32) and scratch budget (0: no limit)."""
    lib = load()
    nb = _c_int(0)
    _binding.check(lib, "prep", lib.tomo_prep_outlier_batch(int(rows), int(cols), int(dtype), int(n), int(max_scratch_bytes),
                                                            ctypes.byref(nb)))
    return nb.value


class PrepHandle(Handle):
    """One tomo_prep handle: a device, the stripe scratch and the last error.  A context manager; close() frees everything.  device: the
    tomo context's (ctx.device) -- every call is enqueued on the stream it is given, in practice that context's."""

    NAME = "prep"
    load = staticmethod(load)
    ERRORS = {ERR_UNSUPPORTED: PrepUnsupported}

    def reference(self, stream, d_frames, dtype, n, rows, cols, method, d_out):
        self._check(self.lib.tomo_prep_reference(self.handle, _ptr(stream), _ptr(d_frames), int(dtype), int(n), int(rows), int(cols),
                                                 int(method), _ptr(d_out)))

    def normalize(self, stream, d_raw, dtype, n, rows, cols, d_flat, d_dark, crop, cutoff, minus_log, min_ratio, d_out):
        (z0, z1), (x0, x1) = crop
        self._check(self.lib.tomo_prep_normalize(self.handle, _ptr(stream), _ptr(d_raw), int(dtype), int(n), int(rows), int(cols),
                                                 _ptr(d_flat), _ptr(d_dark), int(z0), int(z1), int(x0), int(x1), 0 if cutoff is None else 1,
                                                 0.0 if cutoff is None else float(cutoff), 1 if minus_log else 0, float(min_ratio),
                                                 _ptr(d_out)))

    def stripe_sorting(self, stream, d_in, d_out, n_proj, ndx, ndz, size, max_scratch_bytes=0, timed=False):
        """Enqueue the stripe removal; timed=True synchronises and returns the device ms of the sort, median and scatter passes."""
        ms = (ctypes.c_float * 3)() if timed else None
        self._check(self.lib.tomo_prep_stripe_sorting(self.handle, _ptr(stream), _ptr(d_in), _ptr(d_out), int(n_proj), int(ndx), int(ndz),
                                                      int(size), int(max_scratch_bytes), ms))
        return tuple(ms) if timed else None

    def stripe_large(self, stream, d_in, d_out, n_proj, ndx, ndz, snr, size, drop_ratio, norm, max_scratch_bytes=0, d_mask=None):
        """Enqueue the large-stripe removal; d_mask: None or ndx * ndz bytes for the detector's mask."""
        self._check(self.lib.tomo_prep_stripe_large(self.handle, _ptr(stream), _ptr(d_in), _ptr(d_out), int(n_proj), int(ndx), int(ndz),
                                                    float(snr), int(size), float(drop_ratio), 1 if norm else 0, int(max_scratch_bytes),
                                                    _ptr(d_mask)))

    def stripe_dead(self, stream, d_in, d_out, n_proj, ndx, ndz, snr, size, norm, max_scratch_bytes=0, d_mask=None, d_mask_large=None):
        """Enqueue the dead-stripe removal (with norm: followed by the large-stripe pass, whose mask goes to d_mask_large)."""
        self._check(self.lib.tomo_prep_stripe_dead(self.handle, _ptr(stream), _ptr(d_in), _ptr(d_out), int(n_proj), int(ndx), int(ndz),
                                                   float(snr), int(size), 1 if norm else 0, int(max_scratch_bytes), _ptr(d_mask),
                                                   _ptr(d_mask_large)))

    def stripe_all(self, stream, d_in, d_out, n_proj, ndx, ndz, snr, la_size, sm_size, max_scratch_bytes=0, d_mask_dead=None,
                   d_mask_large=None):
        """Enqueue dead (la_size, norm) then sorting (sm_size)."""
        self._check(self.lib.tomo_prep_stripe_all(self.handle, _ptr(stream), _ptr(d_in), _ptr(d_out), int(n_proj), int(ndx), int(ndz),
                                                  float(snr), int(la_size), int(sm_size), int(max_scratch_bytes), _ptr(d_mask_dead),
                                                  _ptr(d_mask_large)))

    def outlier(self, stream, d_in, d_out, dtype, n, rows, cols, size, mode, dif=0.0, two_sided=False, max_scratch_bytes=0, d_count=None):
        """Enqueue the zinger removal (mode OUTLIER) or the 2-D median filter (MEDIAN2D); d_out may be d_in; d_count: None or n uint32."""
        self._check(self.lib.tomo_prep_outlier(self.handle, _ptr(stream), _ptr(d_in), _ptr(d_out), int(dtype), int(n), int(rows), int(cols),
                                               int(size), int(mode), float(dif), 1 if two_sided else 0, int(max_scratch_bytes),
                                               _ptr(d_count)))
