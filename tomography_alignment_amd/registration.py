"""
Registration of two volumes by a translation: the 3-D sibling of align.align_cc.phase_cross_correlation.  Two reconstructions of one
object that were aligned independently (the two halves of a half-set FSC, two runs, two energies) differ by the alignment's gauge, a
global translation of the object that the data cannot see (align.consistency.gauge_fix); resolution.fsc of two unregistered volumes
falls at once, and an RMSE against a phantom punishes a correct alignment that moved the object by half a voxel like a wrong one.
`register` finds the translation on the device, `shift_volume` applies it.

Definition (include/tomo_vreg.h, tests/vreg_model.py).  With A, B the real-to-complex transforms of the masked, mean-free reference and
moving volume (the mask and the mean are resolution.py's), P = A conj(B) -- or P / |P| with normalization="phase" -- and c = C2R(P) / N:
the coarse shift is the position of the largest c, index i on an axis of n read as i for i <= n // 2 and i - n beyond.  With
upsample = u > 1 the peak is refined on a grid of U = ceil(1.5 u) candidates an axis, 1 / u apart, about the coarse shift: the
upsampled DFT of P there (Guizar-Sicairos, Thurman & Fienup 2008, Opt. Lett. 33, 156, as scikit-image does it in 2-D), written for
the Hermitian half-spectrum, with exact integer phases and float64 sums.  The model defines it; no equality with another package is
claimed.

Sign: `shift` moves the MOVING volume onto the reference, shift_volume(mov, shift) ~ ref.

The default normalization is None, not "phase": on smooth volumes the weak high shells are float32 rounding noise, and phase
normalisation gives them full weight; it misses planted shifts that the plain correlation finds.

shift_volume(v, s) is the Fourier shift C2R(R2C(v) prod_i exp(-2 pi i k_i s_i / n_i)) / N with the real cos(pi s_i) at the Nyquist
frequency of an even axis, periodic; an integer s is the circular roll np.roll(v, s, (0, 1, 2)), bit for bit, without a transform.

All results are deterministic: the same input gives the same bits, whatever the scratch budget.  Host arrays in are uploaded;
_lib.DeviceArrays in stay where they are (a flat device buffer, such as a solver's d_rec, needs `shape`).

Limits: a translation only.  A rotation between the volumes is out of scope: the gauge of two alignments that start from the same
poses is a translation to first order.  One GPU; axes of 2 ... 2048; float32 transforms; no windowed (local) registration; no trilinear
or spline resampling.
"""
import numpy as np

from . import _vreg_lib
from ._ops import HandleOwner, Staging, _is_dev, shape_of
from ._vreg_lib import VregUnsupported  # noqa: F401  (re-exported)

NORMALIZATIONS = {None: _vreg_lib.NORM_NONE, "phase": _vreg_lib.NORM_PHASE}


def coefficient_of(peak, E0, E1, normalization=None):
    """The normalised correlation at the peak: peak / sqrt(E0 E1), 0 where that is 0; with "phase" the peak itself."""
    if normalization == "phase":
        return float(peak)
    den = np.sqrt(float(E0) * float(E1))
    return float(peak) / den if den > 0 else 0.0


class Registration(object):
    """What register() found.
    shift         float64 (3,): moves the moving volume onto the reference, in voxels (the sum over the passes)
    peak          the winning value of c (upsample 1) or of the upsampled c_u, of the last pass
    coefficient   peak / sqrt(E0 E1), E the energies of the two prepared volumes (0 where that is 0); with "phase" the peak
    error         sqrt(max(0, 1 - coefficient^2)): 0 for volumes that are translates of each other
    coarse        the integer shift of the first pass's coarse peak, three ints
    upsample, passes, normalization, E0, E1"""

    def __init__(self, shift, peak, E0, E1, coarse, upsample, passes, normalization=None):
        self.shift = np.asarray(shift, np.float64).reshape(3)
        self.peak, self.E0, self.E1 = float(peak), float(E0), float(E1)
        self.coarse = tuple(int(v) for v in coarse)
        self.upsample, self.passes, self.normalization = int(upsample), int(passes), normalization
        self.coefficient = coefficient_of(self.peak, self.E0, self.E1, normalization)
        self.error = float(np.sqrt(max(0.0, 1.0 - self.coefficient * self.coefficient)))

    def __repr__(self):
        return "Registration(shift (%.4g, %.4g, %.4g), coefficient %.4f, upsample %d, passes %d)" % (
            self.shift[0], self.shift[1], self.shift[2], self.coefficient, self.upsample, self.passes)


def _shape_of(a, shape, what):
    return shape_of(a, shape, 3, what)


def _mask_args(mask, edge, radius, shape):
    """(mode, radius, edge) of the library for resolution.py's mask arguments; an array mask is checked and handled by the caller."""
    edge = float(edge)
    if isinstance(mask, str):
        if mask != "sphere":
            raise ValueError("mask must be 'sphere', None or an array of shape %s, got %r" % (shape, mask))
        if not (edge >= 0 and np.isfinite(edge)):
            raise ValueError("edge must be >= 0, got %r" % (edge,))
        radius = max(0.0, min(shape) / 2.0 - edge) if radius is None else float(radius)
        if not (radius >= 0 and np.isfinite(radius)):
            raise ValueError("radius must be >= 0, got %r" % (radius,))
        return _vreg_lib.MASK_SPHERE, radius, edge
    if mask is None:
        return _vreg_lib.MASK_NONE, 0.0, 0.0
    if _shape_of(mask, shape if _is_dev(mask) else None, "mask") != shape:
        raise ValueError("mask must have the shape %s" % (shape,))
    return _vreg_lib.MASK_ARRAY, 0.0, 0.0


def _shift3(shift):
    s = np.asarray(shift, np.float64)
    if s.shape != (3,) or not np.all(np.isfinite(s)):
        raise ValueError("shift must be three finite numbers, got %r" % (shift,))
    return s


class Registrar(HandleOwner):
    """One libtomo_vreg handle and its hipFFT plans and buffers reused across calls.  ctx: the _lib.Context whose device and stream the
    work uses (default: that of the first DeviceArray passed in, or a context of the handle's own)."""

    def _new_handle(self):
        return _vreg_lib.VregHandle(self.ctx.device)

    def device_bytes(self):
        return 0 if self.handle is None else self.handle.device_bytes()

    def register(self, ref, mov, upsample=10, normalization=None, mask="sphere", edge=6, radius=None, subtract_mean=True, passes=1,
                 shape=None):
        """The translation that moves `mov` onto `ref` (module docstring) -> Registration.
        upsample        1 ... 100: the shift is found to 1 / upsample voxel
        normalization   None (default) or "phase".  On smooth volumes the weak high shells are float32 rounding noise, and phase
                        normalisation gives them full weight; it misses planted shifts that the plain correlation finds.
        mask, edge, radius, subtract_mean   as resolution.fsc: the soft sphere by default
        passes          p > 1: after each estimate the moving volume is Fourier-shifted by the total so far into a scratch volume and
                        registered again; the shifts add.  This removes the bias a fixed mask leaves when the object sits differently
                        under it in the two volumes.
        A non-finite peak (NaN or inf in a volume) raises ValueError."""
        sa, sb = _shape_of(ref, shape, "ref"), _shape_of(mov, shape, "mov")
        if sa != sb:
            raise ValueError("the two volumes must have one shape, got %s and %s" % (sa, sb))
        if normalization not in NORMALIZATIONS:
            raise ValueError("normalization must be None or 'phase', got %r" % (normalization,))
        passes, upsample = int(passes), int(upsample)
        if passes < 1:
            raise ValueError("passes must be >= 1, got %d" % passes)
        _vreg_lib.check(sa[0], sa[1], sa[2], upsample if upsample != 0 else -1)     # VregUnsupported before a context, a handle or a launch
        mode, radius, edge = _mask_args(mask, edge, radius, sa)
        self._ready(ref if _is_dev(ref) else mov)
        ctx, h = self.ctx, self.handle
        with self._staging(ref) as staging:
            m_ptr = staging.source(mask).ptr if mode == _vreg_lib.MASK_ARRAY else None
            d_ref, d_mov = staging.source(ref), staging.source(mov)
            h.set_shape(*sa)
            st = ctx.stream()
            total, first, d_cur = np.zeros(3), None, d_mov
            for p in range(passes):
                if p > 0:
                    if d_cur is d_mov:
                        d_cur = staging.scratch((int(np.prod(sa)),))
                    h.shift(st, d_mov.ptr, total, d_cur.ptr)
                h.prepare(st, 0, d_ref.ptr, mode, m_ptr, radius, edge, subtract_mean)
                h.prepare(st, 1, d_cur.ptr, mode, m_ptr, radius, edge, subtract_mean)
                h.correlate(st, NORMALIZATIONS[normalization])
                h.refine(st, upsample)
                out = h.fetch(st)
                if not np.isfinite(out[3]):
                    raise ValueError("register: the correlation peak is not finite (%r): a volume holds NaN or inf" % (out[3],))
                total = total + out[:3]
                if first is None:
                    first = np.unravel_index(int(out[6]), sa)
            coarse = [int(i) if i <= n // 2 else int(i) - n for i, n in zip(first, sa)]
            return Registration(total, out[3], out[4], out[5], coarse, upsample, passes, normalization)

    def shift_volume(self, vol, shift, out=None, shape=None):
        """`vol` moved by `shift` voxels (module docstring), periodic -> a device array of the volume's shape, `out` if given (a float32
        device array of as many values; it may be `vol` itself)."""
        sv = _shape_of(vol, shape, "vol")
        s = _shift3(shift)
        _vreg_lib.check(*sv)
        if out is not None and not (_is_dev(out) and np.dtype(out.dtype) == np.float32 and out.size == int(np.prod(sv))):
            raise ValueError("out must be a float32 device array of %d values" % int(np.prod(sv)))
        self._ready(vol if _is_dev(vol) else out)
        with Staging(self.ctx, True) as st:                      # the result stays on the device whatever `vol` is
            d_v = st.source(vol)
            d_out = st.dest(sv, np.float32, out)
            self.handle.set_shape(*sv)
            self.handle.shift(self.ctx.stream(), d_v.ptr, s, d_out.ptr)
            return st.result(d_out)

    def argmax(self, vol, shape=None):
        """(index, value) of the largest element of a volume, index a tuple of three ints: NaN never wins, a tie goes to the smallest
        flat index, a volume of NaN only gives (0, 0, 0) and NaN.  The reduction behind the coarse peak; deterministic."""
        sv = _shape_of(vol, shape, "vol")
        _vreg_lib.check(*sv)
        self._ready(vol)
        with self._staging(vol) as st:
            d_v = st.source(vol)
            self.handle.set_shape(*sv)
            i, v = self.handle.argmax(self.ctx.stream(), d_v.ptr)
            return tuple(int(j) for j in np.unravel_index(i, sv)), v


def register(ref, mov, upsample=10, normalization=None, mask="sphere", edge=6, radius=None, subtract_mean=True, passes=1, ctx=None,
             shape=None):
    """Registrar.register on a handle of its own."""
    with Registrar(ctx) as r:
        return r.register(ref, mov, upsample=upsample, normalization=normalization, mask=mask, edge=edge, radius=radius,
                          subtract_mean=subtract_mean, passes=passes, shape=shape)


def shift_volume(vol, shift, out=None, ctx=None, shape=None):
    """Registrar.shift_volume on a handle of its own; with a context of its own too (host input, no ctx) the result comes back as a host
    array, because a device array does not outlive its context."""
    with Registrar(ctx) as r:
        d = r.shift_volume(vol, shift, out=out, shape=shape)
        return d if r._own_ctx is None else d.download()         # the context closes on the way out and frees d


def argmax(vol, ctx=None, shape=None):
    """Registrar.argmax on a handle of its own."""
    with Registrar(ctx) as r:
        return r.argmax(vol, shape=shape)
