"""
Half-acquisition (offset-axis) scans over 2 pi: find the rotation axis and stitch the series to the pi series of double width.

A sample wider than the detector is measured with the rotation axis near one edge of the detector: the sample turns through 2 pi, and
the projection at phi + pi shows, mirrored, the half of the object that the projection at phi missed.  rotation_axis.find_center does not
take such data (its angles span pi and it searches +-50 columns about the detector centre; the axis here is hundreds of columns from
it), and every other stage -- recon.fbp, the solvers, the alignment -- expects a pi series that holds the whole object.  This module
produces the axis (find_center_360) and that series (sino_360_to_180).

Definition (include/tomo_half.h states it in full, tests/half_model.py is the same in numpy; no equality with any other package's
numbers is claimed).  proj is (n, nx, nz), float32, z fastest, n even, projection i taken at phi0 + i 2 pi / n; S is one detector row of
it, h = n / 2, A[i][x] = S[i][x], M[i][x] = S[h + i][nx - 1 - x].  With the axis at column c (centre convention (nx - 1) / 2),
A[i][x] = M[i][x + t], t = nx - 1 - 2 c.

Search -- the fixed-window overlap search of Vo et al.: a window of w columns at the detector edge next to the axis (side 'right':
ref = A[:, nx - w:]; side 'left': ref = A[:, :w]) is compared with M[:, p : p + w] for every p = 0 ... nx - w by m(p) = 1 - Pearson
correlation, float64 sums of the float32 values.  The library returns both curves of every detector row searched; the first minimum, a
parabola through its neighbours (clipped to +-1/2 px) and the median over the rows are taken here.  With side=None the side with the
lower minimum wins per row ('right' wins a tie).  The sums are deterministic: the same input gives the same bits in any call.

Stitch: h rows of W = floor(2 max(c, nx - 1 - c)) + 1 columns.  The first half keeps its integer columns (from output column j0 on);
the second half is mirrored about c, linearly interpolated where 2 c is not an integer, and the two are blended linearly across the
overlap of 2 g + 1 columns (g = min(c, nx - 1 - c)).  The axis lies at column c + j0 of the output, cor_offset = c + j0 - (W - 1) / 2 from
its centre; with the sign of rotation_axis (to_cor_shift), data stitched this way are reconstructed with Geometry(cor_shift=
[-cor_offset, 0, 0]).  The stitch pairs the projections i and i + h, so it assumes that they share a pose: it suits data whose jitter is
below a pixel, or data aligned beforehand.

Limits: an even 2 <= n <= 65536, 8 <= nx <= 16384, nz <= 16384, at most 4096 detector rows per search, 4 <= win_width <= nx / 2
(HalfUnsupported before any launch otherwise).  Not covered: intensity matching of the two halves, sharded search, per-projection poses,
360 -> 360 padding.
"""
import numpy as np

from . import _half_lib
from ._half_lib import HalfUnsupported  # noqa: F401  (re-exported)
from ._ops import HandleOwner, _is_dev, stack_shape as _shape3

SIDES = ("right", "left")          # the order of the curves of one row
DEFAULT_SCRATCH = 1 << 30


class Center360Result(object):
    """center    the median of `centers`: the column the axis projects to (centre convention (nx - 1) / 2)
    offset    center - (nx - 1) / 2
    side      'right' or 'left': the side asked for, else that of `center`
    overlap   2 g + 1, the columns both halves see, g = min(center, nx - 1 - center)
    centers   one per detector row searched;  sides: the side that won in each
    rows      the detector rows searched
    curves    with return_curves: float64 (rows, 2, nx - w + 1), side right first"""

    def __init__(self, centers, sides, rows, nx, side=None, curves=None):
        self.centers = np.asarray(centers, np.float64)
        self.sides = list(sides)
        self.rows = np.asarray(rows, np.int64)
        self.center = float(np.median(self.centers))
        self.offset = self.center - 0.5 * (int(nx) - 1)
        self.side = side if side is not None else ("right" if self.center >= int(nx) - 1 - self.center else "left")
        self.overlap = 2.0 * min(self.center, int(nx) - 1 - self.center) + 1.0
        self.curves = curves

    def __repr__(self):
        return "Center360Result(center column %.3f over %d rows, side %s, overlap %.1f columns)" % (self.center, self.centers.size, self.side,
                                                                                                    self.overlap)


class StitchResult(object):
    """projections   (h, W, nz) float32: a DeviceArray for device input, numpy for numpy input
    center        the column of the axis in the stitched series, c + j0
    cor_offset    center - (W - 1) / 2
    angles        the first h of the angles given (None if none were)"""

    def __init__(self, projections, center, W, angles):
        self.projections = projections
        self.center = float(center)
        self.cor_offset = self.center - 0.5 * (int(W) - 1)
        self.angles = angles

    def __repr__(self):
        return "StitchResult(projections %s, axis at column %.3f, cor_offset %+.3f)" % (tuple(self.projections.shape), self.center, self.cor_offset)


def angle_span(angles, n):
    """How many projections of a series of n cover [0, 2 pi): n for None or n d = 2 pi, n - 1 for (n - 1) d = 2 pi (the endpoint repeats
    the first projection and is dropped).  ValueError for anything else, and for an odd count after the drop."""
    n = int(n)
    if angles is None:
        used = n
    else:
        a = np.asarray(angles, np.float64).ravel()
        if a.size != n:
            raise ValueError("half acquisition: %d angles for %d projections" % (a.size, n))
        if n < 2:
            raise ValueError("half acquisition: needs at least two angles")
        d = (a[-1] - a[0]) / (n - 1)
        if not (np.isfinite(d) and d != 0.0) or np.max(np.abs(np.diff(a) - d)) > 1e-6 * abs(d):
            raise ValueError("half acquisition: the angles must be uniformly spaced")
        tol = 1e-6 * abs(d)
        if abs(n * abs(d) - 2.0 * np.pi) <= tol:
            used = n
        elif abs((n - 1) * abs(d) - 2.0 * np.pi) <= tol:
            used = n - 1
        else:
            raise ValueError("half acquisition: the angles must span 2 pi (n d = 2 pi, or (n - 1) d = 2 pi with the endpoint), got a spacing of "
                             "%g rad over %d angles" % (d, n))
    if used < 2 or used % 2:
        raise ValueError("half acquisition: needs an even number of projections over 2 pi, got %d" % used)
    return used


def default_window(nx):
    return max(8, int(nx) // 8)


def check_window(nx, win_width):
    """The window as an int; ValueError unless it is an integer in 4 ... nx / 2."""
    w = default_window(nx) if win_width is None else win_width
    if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, np.integer)) or not _half_lib.MIN_W <= w <= nx // 2:
        raise ValueError("half acquisition: win_width must be an integer in %d ... nx / 2 = %d, got %r" % (_half_lib.MIN_W, nx // 2, win_width))
    return int(w)


def check_side(side):
    if side not in (None,) + SIDES:
        raise ValueError("half acquisition: side must be None, 'left' or 'right', got %r" % (side,))
    return side


def check_center(nx, center):
    try:
        c = float(center)
    except (TypeError, ValueError):
        raise ValueError("half acquisition: center must be a number, got %r" % (center,))
    if not 0.0 <= c <= nx - 1:                                       # NaN too
        raise ValueError("half acquisition: the axis must lie on the detector, 0 <= center <= %d, got %r" % (nx - 1, center))
    return c


def stitched_shape(n, nx, center):
    """(h, W, j0): the rows and columns of the series sino_360_to_180 gives for n projections of nx columns and the axis at `center`, and
    the output column of the first half's column 0.  The axis lies at center + j0 there.  Needs no device."""
    c = check_center(nx, center)
    W = int(np.floor(2.0 * max(c, nx - 1 - c))) + 1
    return int(n) // 2, W, (0 if c >= nx - 1 - c else W - int(nx))


def refine(m):
    """(k, delta) of one curve: the first index of its minimum, and the step to the vertex of the parabola through the minimum and its
    neighbours, clipped to +-1/2; 0 at an end of the curve or where the parabola does not open upwards."""
    k = int(np.argmin(m))
    delta = 0.0
    if 0 < k < m.size - 1:
        den = m[k - 1] - 2.0 * m[k] + m[k + 1]
        if den > 0:
            delta = float(np.clip(0.5 * (m[k - 1] - m[k + 1]) / den, -0.5, 0.5))
    return k, delta


def center_from_curves(m_right, m_left, nx, w, side=None):
    """(c, side, k, minimum) of one detector row from its two curves."""
    best = None
    for s, m in zip(SIDES, (m_right, m_left)):
        if side not in (None, s):
            continue
        k, delta = refine(m)
        if best is None or m[k] < best[3]:                           # right first: it wins a tie
            p = k + delta
            t = p - (nx - w) if s == "right" else p
            best = (0.5 * (nx - 1 - t), s, k, float(m[k]))
    return best


class HalfAcquisition(HandleOwner):
    """One libtomo_half handle -- the gathered sinograms, the search's sums and the stitch's table -- reused across calls.  ctx: the
    _lib.Context whose device and stream the work uses (default: that of the DeviceArray passed in, or a context of the handle's own)."""

    def _new_handle(self):
        return _half_lib.HalfHandle(self.ctx.device)

    def device_bytes(self):
        return 0 if self.handle is None else self.handle.device_bytes()

    def curves(self, proj, angles=None, rows=None, win_width=None, shape=None, max_scratch_bytes=DEFAULT_SCRATCH):
        """(m, rows, n used, nx, w): both curves of the detector rows `rows` (default the middle one) of proj (n, nx, nz), float64
        (rows, 2, nx - w + 1), side right first."""
        n_p, nx, nz = _shape3(proj, shape, "find_center_360")
        n = angle_span(angles, n_p)
        w = check_window(nx, win_width)
        rows = np.array([nz // 2] if rows is None else rows, np.int64).ravel()
        if rows.size < 1 or rows.min() < 0 or rows.max() >= nz:
            raise ValueError("find_center_360: rows must be in 0 ... %d" % (nz - 1))
        if max_scratch_bytes is not None and int(max_scratch_bytes) < 0:
            raise ValueError("find_center_360: max_scratch_bytes must be >= 0 or None")
        _half_lib.check_shape(n, nx, nz, rows.size, w)             # HalfUnsupported before a context, a handle or a launch
        self._ready(proj)
        ctx, h = self.ctx, self.handle
        with self._staging(proj) as st:
            src, nz_d, rows_d = proj, nz, rows
            if not st.dev:                                           # only the rows searched are uploaded
                src, nz_d, rows_d, n_p = np.asarray(proj, np.float32)[:n, :, rows], rows.size, np.arange(rows.size), n
            d_p = st.source(src)
            h.set_max_scratch(max_scratch_bytes)
            h.load_rows(ctx.stream(), d_p.ptr, n_p, nx, nz_d, n, rows_d)
            m = h.search(ctx.stream(), w)                            # waits; so does the free of the upload, which the gather reads
        return m, rows, n, nx, w

    def find_center_360(self, proj, angles=None, rows=None, win_width=None, side=None, return_curves=False, shape=None,
                        max_scratch_bytes=DEFAULT_SCRATCH):
        """The rotation axis of the half-acquisition series proj (n, nx, nz): numpy, or a _lib.DeviceArray (a flat one needs `shape`)
        -> Center360Result.
        angles      None (the projections cover [0, 2 pi) uniformly), or the n angles: uniformly spaced, spanning 2 pi with or without
                    the endpoint (with it, the last projection is dropped)
        rows        the detector rows (z) to search, default the middle one; the result's center is the median over them
        win_width   the columns of the window, default max(8, nx // 8); 4 <= win_width <= nx / 2
        side        None (both sides are searched and the lower minimum wins), 'left' or 'right': where the axis lies on the detector
        max_scratch_bytes   the budget of the search's partial sums (None or 0: no limit); the bits do not depend on it"""
        check_side(side)
        m, rows, n, nx, w = self.curves(proj, angles, rows, win_width, shape, max_scratch_bytes)
        found = [center_from_curves(m[r, 0], m[r, 1], nx, w, side) for r in range(rows.size)]
        return Center360Result([f[0] for f in found], [f[1] for f in found], rows, nx, side, m if return_curves else None)

    def sino_360_to_180(self, proj, center, angles=None, out=None, shape=None):
        """The pi series of double width of the half-acquisition series proj (n, nx, nz) with the axis at column `center`
        -> StitchResult.  proj: numpy (the result's projections are numpy) or a _lib.DeviceArray (a DeviceArray; a flat one needs
        `shape`).  out: None, or where the (h, W, nz) float32 result goes -- of the kind of proj, of stitched_shape's size, and not
        overlapping proj.  angles: as for find_center_360."""
        n_p, nx, nz = _shape3(proj, shape, "sino_360_to_180")
        n = angle_span(angles, n_p)
        h, W, j0 = stitched_shape(n, nx, center)
        c = float(center)
        dev = _is_dev(proj)
        if out is not None:
            if _is_dev(out) != dev:
                raise ValueError("sino_360_to_180: out must be a %s, like proj" % ("DeviceArray" if dev else "numpy array"))
            if np.dtype(out.dtype) != np.float32 or int(np.prod(out.shape)) != h * W * nz:
                raise ValueError("sino_360_to_180: out must hold the %d x %d x %d float32 values of the stitched series" % (h, W, nz))
            if not dev and (tuple(out.shape) != (h, W, nz) or not out.flags["C_CONTIGUOUS"]):
                raise ValueError("sino_360_to_180: out must be a C-contiguous array of shape %s" % ((h, W, nz),))
            if not dev and np.shares_memory(out, proj):              # on the device the library compares the two ranges
                raise ValueError("sino_360_to_180: out overlaps proj: the stitch does not work in place")
        _half_lib.check_shape(n, nx, nz)                            # HalfUnsupported before a context, a handle or a launch
        self._ready(proj)
        ctx, hd = self.ctx, self.handle
        half_angles = None if angles is None else np.asarray(angles, np.float64).ravel()[:h].copy()
        with self._staging(proj) as st:
            d_p = st.source(proj if dev else np.asarray(proj, np.float32)[:n])
            d_out = st.dest((h, W, nz), np.float32, out)
            hd.stitch(ctx.stream(), d_p.ptr, n, nx, nz, c, d_out.ptr)          # refuses a device out that overlaps proj
            return StitchResult(st.result(d_out, out), c + j0, W, half_angles)


def find_center_360(proj, angles=None, rows=None, win_width=None, side=None, return_curves=False, ctx=None, shape=None,
                    max_scratch_bytes=DEFAULT_SCRATCH):
    """HalfAcquisition.find_center_360 on a handle of its own."""
    check_side(side)
    with HalfAcquisition(ctx) as a:
        return a.find_center_360(proj, angles=angles, rows=rows, win_width=win_width, side=side, return_curves=return_curves, shape=shape,
                                 max_scratch_bytes=max_scratch_bytes)


def sino_360_to_180(proj, center, angles=None, out=None, ctx=None, shape=None):
    """HalfAcquisition.sino_360_to_180 on a handle of its own."""
    with HalfAcquisition(ctx) as a:
        res = a.sino_360_to_180(proj, center, angles=angles, out=out, shape=shape)
        if _is_dev(proj):
            a.ctx.sync()                                             # the handle's table is freed on the way out
        return res
