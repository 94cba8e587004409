"""
The position of the rotation axis on the detector, found from the sinogram alone.

Every operator of the package honours `Geometry(cor_shift=)`; this module produces the value.  Scans over [0, pi) hold no 0 / 180 degree
pair of projections (what align_cc.cor_flipping needs), and the rigid alignment searches a few pixels only, so an axis that is tens of
pixels off the detector's centre column has to be found first.

The method is the Fourier-space sinogram metric of Vo et al., Opt. Express 22 (2014) 19078: a sinogram S[n][nx] over [0, pi) is stacked
on its mirrored copy, shifted by t columns, to a 360-degree sinogram M_t.  The 2-D spectrum of a consistent 360-degree sinogram is
confined to a double wedge; energy outside it appears when t is not twice the axis offset.  The metric m(t) is the mean magnitude of
the spectrum over a mask outside the wedge, and the offset is t / 2 at its minimum.

This is Vo's method with two choices of this package's own, so no equality with any other package's numbers is claimed:
  * the mask is made symmetric about DC -- W(kv, ku) = 1 iff |ku| <= ceil(|kv| dv / (radius du)), |kv| > min(drop, ceil(0.05 R)) and
    |ku| >= 2, with R = 2 n, dv = (R - 1) / (2 pi R), du = 1 / nx, radius = 0.5 ratio nx -- so the real-to-complex half-spectrum with
    Hermitian weights suffices;
  * integer shifts are exact copies, B_t[i][j] = S[i][nx - 1 - (j - t)]; other shifts are the cubic B-spline interpolant of the
    mirrored row (mirror boundary, float64, rounded to float32 once).  The columns that wrap are taken from the complementary row
    S[n - 1 - i][j].
include/tomo_cor.h states it in full and tests/cor_model.py is the same in numpy.

Search: coarse over the integer shifts t = 2 smin ... 2 smax (half-pixel offsets), first minimum t0; then fine over
t0 + 2 step k, k = -K ... K, K = round(srad / step).  offset = t_best / 2 detector pixels from the detector centre (nx - 1) / 2.

Sign: `offset` is positive when the axis projects to a larger column index than the detector centre.  The operators' `cor_shift`
moves the source and the detector by +d along x, so the axis then projects to the column (nx - 1) / 2 - d: data projected with
`Geometry(cor_shift=[d, 0, 0])` give offset = -d, and to_cor_shift(offset, n) is [-offset, 0, 0] per projection
(tests/test_gpu_rotation_axis.py::test_sign_against_the_projector).

Limits: one sinogram needs 8 <= n <= 8192 angles that cover [0, pi) uniformly and 16 <= nx <= 8192 columns (CorUnsupported before any
launch otherwise); 360-degree scans with an off-centre axis, an axis tilt, and Vo's optional pre-smoothing and down-sampling are not
covered.  The sums are float64 and deterministic: the same input gives the same bits whatever the scratch budget or the number of rows
searched in one call.
"""
import numpy as np

from . import _cor_lib
from ._cor_lib import CorUnsupported  # noqa: F401  (re-exported)
from ._ops import HandleOwner, _is_dev, stack_shape

DEFAULT_SCRATCH = 2 << 30


class CenterResult(object):
    """offset    the median of `offsets`: detector pixels from the detector centre (nx - 1) / 2
    offsets   one per detector row searched
    center    (nx - 1) / 2 + offset, the column the axis projects to
    rows      the detector rows searched
    coarse, fine   with return_curves: per row a pair (t, m) of float64 arrays"""

    def __init__(self, offsets, rows, nx, coarse=None, fine=None):
        self.offsets = np.asarray(offsets, np.float64)
        self.rows = np.asarray(rows, np.int64)
        self.offset = float(np.median(self.offsets))
        self.center = 0.5 * (int(nx) - 1) + self.offset
        self.coarse, self.fine = coarse, fine

    def __repr__(self):
        return "CenterResult(offset %+.3f px over %d rows, center column %.3f)" % (self.offset, self.offsets.size, self.center)


def check_arguments(n, nx, smin, smax, srad, step):
    """ValueError for a search that the detector cannot hold; needs no device."""
    if n < _cor_lib.MIN_N or nx < _cor_lib.MIN_NX:
        raise ValueError("find_center: a sinogram needs n >= %d angles and nx >= %d columns, got %d x %d" % (_cor_lib.MIN_N, _cor_lib.MIN_NX, n, nx))
    if smin > smax:
        raise ValueError("find_center: smin = %r > smax = %r" % (smin, smax))
    if not step > 0:
        raise ValueError("find_center: step must be > 0, got %r" % (step,))
    if not srad >= 0:
        raise ValueError("find_center: srad must be >= 0, got %r" % (srad,))
    if max(abs(smin), abs(smax)) > nx / 2.0 - srad - 1:
        raise ValueError("find_center: |smin|, |smax| must not exceed nx / 2 - srad - 1 = %g on a detector of %d columns, got %r, %r"
                         % (nx / 2.0 - srad - 1, nx, smin, smax))


def angle_span(angles, n):
    """How many rows of a sinogram of n rows cover [0, pi): n when the n uniformly spaced `angles` span pi (n d = pi), n - 1 when they
    include the endpoint ((n - 1) d = pi, what examples/generate_data.make writes; the last row repeats the first, mirrored, and is
    dropped).  ValueError for anything else.  None: n."""
    if angles is None:
        return int(n)
    a = np.asarray(angles, np.float64).ravel()
    if a.size != n:
        raise ValueError("find_center: %d angles for %d projections" % (a.size, n))
    if n < 2:
        raise ValueError("find_center: needs at least two angles")
    d = (a[-1] - a[0]) / (n - 1)
    if not (np.isfinite(d) and d != 0.0) or np.max(np.abs(np.diff(a) - d)) > 1e-6 * abs(d):
        raise ValueError("find_center: the angles must be uniformly spaced")
    tol = 1e-6 * abs(d)
    if abs(n * abs(d) - np.pi) <= tol:
        return int(n)
    if abs((n - 1) * abs(d) - np.pi) <= tol:
        return int(n) - 1
    raise ValueError("find_center: the angles must span pi (n d = pi, or (n - 1) d = pi with the endpoint), got a spacing of %g rad over %d angles"
                     % (d, n))


def coarse_list(smin, smax):
    return np.arange(2 * int(smin), 2 * int(smax) + 1).astype(np.float64)


def fine_list(t0, srad, step):
    K = int(round(srad / step))
    return np.array([t0 + 2.0 * step * k for k in range(-K, K + 1)], np.float64)


def widest_range(nx, srad=6, limit=50):
    """(smin, smax): the symmetric search range of +-limit pixels, cut to what check_arguments admits on a detector of nx columns."""
    s = int(min(int(limit), np.floor(nx / 2.0 - srad - 1)))
    return -s, s


def spread_rows(nz, k):
    """k detector rows spread evenly over the central half of the nz rows (fewer where they coincide): what the drivers search, the
    median over them being robust against a row whose sinogram is poor in structure."""
    k = int(k)
    if k < 1:
        raise ValueError("spread_rows: needs k >= 1, got %d" % k)
    if k == 1:
        return np.array([nz // 2], np.int64)
    return np.unique(np.rint(np.linspace(nz / 4.0, 3.0 * nz / 4.0, k)).astype(np.int64).clip(0, nz - 1))


def to_cor_shift(offset, n_proj):
    """The (n_proj, 3) array for Geometry(cor_shift=) with which the operators put the axis `offset` pixels from the detector centre:
    [-offset, 0, 0] per projection (module docstring, Sign)."""
    out = np.zeros((int(n_proj), 3))
    out[:, 0] = -float(offset)
    return out


class RotationAxis(HandleOwner):
    """One libtomo_cor handle -- its buffers and hipFFT plans -- reused across calls.  ctx: the _lib.Context whose device and stream
    the work uses (default: that of the DeviceArray passed in, or a context of the handle's own)."""

    def _new_handle(self):
        return _cor_lib.CorHandle(self.ctx.device)

    def device_bytes(self):
        return 0 if self.handle is None else self.handle.device_bytes()

    def load(self, proj, angles=None, rows=None, shape=None, timed=False):
        """Gather and prefilter the detector rows `rows` (default the middle one) of proj (n, nx, nz); returns (rows, n used, nx)
        (and the pass times with `timed`)."""
        n_p, nx, nz = stack_shape(proj, shape, "find_center")
        n = angle_span(angles, n_p)
        rows = np.array([nz // 2] if rows is None else rows, np.int64).ravel()
        if rows.size < 1 or rows.min() < 0 or rows.max() >= nz:
            raise ValueError("find_center: rows must be in 0 ... %d" % (nz - 1))
        if n < _cor_lib.MIN_N or nx < _cor_lib.MIN_NX:
            raise ValueError("find_center: a sinogram needs n >= %d angles and nx >= %d columns, got %d x %d" % (_cor_lib.MIN_N, _cor_lib.MIN_NX, n, nx))
        _cor_lib.check_shape(n, nx, rows.size)                      # CorUnsupported before a context, a handle or a launch
        self._ready(proj)
        ctx, h = self.ctx, self.handle
        with self._staging(proj) as st:
            src, nz_d, rows_d = proj, nz, rows
            if not st.dev:                                           # only the rows searched are uploaded
                src, nz_d, rows_d, n_p = np.asarray(proj, np.float32)[:n, :, rows], rows.size, np.arange(rows.size), n
            d_p = st.source(src)
            ms = h.load_rows(ctx.stream(), d_p.ptr, n_p, nx, nz_d, 0, n, rows_d, timed=timed)      # the gather reads the upload: its free waits
        return (rows, n, nx, ms) if timed else (rows, n, nx)

    def metric(self, slices, ts, ratio=0.5, drop=20, max_scratch_bytes=DEFAULT_SCRATCH, timed=False):
        """m of the (slice, t) pairs of the loaded sinograms (float64)."""
        budget = 0 if max_scratch_bytes is None else int(max_scratch_bytes)
        return self.handle.metric(self.ctx.stream(), slices, ts, ratio, drop, budget, timed=timed)

    def stack(self, slice_, t):
        """M_t of a loaded sinogram as the library builds it (float32 (2 n, nx)): for the tests."""
        return self.handle.debug_build(self.ctx.stream(), slice_, t)

    def find_center(self, proj, angles=None, rows=None, smin=-50, smax=50, srad=6, step=0.25, ratio=0.5, drop=20, return_curves=False,
                    shape=None, max_scratch_bytes=DEFAULT_SCRATCH):
        """The axis offset of proj (n, nx, nz): numpy, or a _lib.DeviceArray (a flat one needs `shape`) -> CenterResult.
        angles    None (the rows cover [0, pi) uniformly), or the n angles: uniformly spaced and spanning pi with or without the endpoint
        rows      the detector rows (z) to search, default the middle one; the result's offset is the median over them
        smin, smax, srad, step, ratio, drop   the search and the mask (module docstring)
        max_scratch_bytes   the budget of the batch buffer and hipFFT's work area (None or 0: no limit); the bits do not depend on it"""
        own = tuple(proj.shape) if _is_dev(proj) else np.shape(proj)
        shp = tuple(int(v) for v in (own if shape is None else shape))
        if len(shp) == 3:
            check_arguments(angle_span(angles, shp[0]), shp[1], smin, smax, srad, step)
        if not (ratio > 0 and np.isfinite(ratio)) or int(drop) < 0:
            raise ValueError("find_center: ratio must be > 0 and drop >= 0")
        rows, n, nx = self.load(proj, angles, rows, shape)
        ns = rows.size
        tc = coarse_list(smin, smax)
        mc = self.metric(np.repeat(np.arange(ns), tc.size), np.tile(tc, ns), ratio, drop, max_scratch_bytes).reshape(ns, tc.size)
        t0 = tc[np.argmin(mc, axis=1)]                               # the first minimum
        tf = np.stack([fine_list(t, srad, step) for t in t0])
        mf = self.metric(np.repeat(np.arange(ns), tf.shape[1]), tf.ravel(), ratio, drop, max_scratch_bytes).reshape(tf.shape)
        best = tf[np.arange(ns), np.argmin(mf, axis=1)]
        curves = ([(tc.copy(), mc[s]) for s in range(ns)], [(tf[s], mf[s]) for s in range(ns)]) if return_curves else (None, None)
        return CenterResult(best / 2.0, rows, nx, *curves)


def find_center(proj, angles=None, rows=None, smin=-50, smax=50, srad=6, step=0.25, ratio=0.5, drop=20, return_curves=False, ctx=None,
                shape=None, max_scratch_bytes=DEFAULT_SCRATCH):
    """RotationAxis.find_center on a handle of its own."""
    with RotationAxis(ctx) as r:
        return r.find_center(proj, angles=angles, rows=rows, smin=smin, smax=smax, srad=srad, step=step, ratio=ratio, drop=drop,
                             return_curves=return_curves, shape=shape, max_scratch_bytes=max_scratch_bytes)
