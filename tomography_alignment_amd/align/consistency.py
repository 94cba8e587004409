"""
Consistency pre-alignment: per-projection shifts from the moments of the projections themselves.

The rigid alignment (examples/align_rigid) searches +-3 px (+-12 px with three levels) around its start, and align_cc chains
neighbour-to-neighbour correlations, whose errors add up as a random walk and which cannot tell the object's own sinusoidal motion across
the detector from jitter.  Parallel-beam data carry a drift-free start themselves, through the Helgason-Ludwig conditions of order 0
and 1 -- for p[i][x][z], the projection at the angle phi[i]:
  * the mass  sum_xz p[i]  is the same for every i;
  * the vertical centroid  cz[i] = sum_xz z p[i] / mass[i]  is the same for every i;
  * the horizontal centroid  cx[i] = sum_xz x p[i] / mass[i]  follows  c0 + a cos(phi[i]) + b sin(phi[i]).
What a projection's centroid deviates by from those laws is how far its image was displaced.  One pass over the sinogram, no
reconstruction and no chain.

The pass is libtomo_mom.so (include/tomo_mom.h): Q[i][x] = sum_z v(p), Z[i][z] = sum_x v(p) in float64 with deterministic sums, where
v(p) = p for a finite p >= floor and 0 otherwise, z restricted to a window `zrange`; non-finite values inside the window are counted in
`bad`.  Everything after it is numpy in float64 on n (nx + nz) values (tests/mom_model.py is the same, written independently).

Sign: the operators' `xyz_shift` moves the source and the detector, so the image moves the other way: xyz0 = -(centroid - law) on both
axes, column 1 (along the beam) zero.  It is the value for `OuterLoop(base=(xyz0, 0, 0))` and for `xyz_shifts`.

Gauge: the law absorbs any part of the shifts that lies in span{1, cos phi, sin phi} horizontally, or is constant vertically.  That
part is a translation of the object and of the axis; no method can see it, and it is left to `cor` and to the volume.  gauge_fix removes
it; compare estimates with true shifts only after applying it to both.

vertical="moment" uses cz - mean(cz).  vertical="profile" is for samples that extend past the detector vertically (pillars), where a
centroid means nothing: the profiles Z[i] are registered against their mean instead (profile_shifts).

axis_offset = c0 - (nx - 1) / 2 has the sign of rotation_axis.find_center's `offset`; it is a by-product and a cross-check (it includes
the object's own centre of mass only through a and b, but any constant part of the jitter goes into it), not a replacement.
mass_spread = max / min - 1 of the masses is the order-0 condition: the diagnostic for a sample that leaves the detector or a wrong
normalisation.  On a Shepp-Logan of 48^3 ... 64^3 a jitter of +-2 px gives 0.25 % and errors of a few hundredths of a pixel; +-8 ...
+-10 px, where the phantom leaves the detector, gives 8 % and x errors up to 1.7 px.

Not covered: sharded estimation (a rank holds a block of the angles; the fit needs all), uint16 input (the marginals mean something
only after the -log), robust fitting.
"""
import collections

import numpy as np

from .. import _mom_lib
from .._mom_lib import MomUnsupported  # noqa: F401  (re-exported)
from .._ops import HandleOwner, stack_shape as _shape_of

DEFAULT_SCRATCH = 2 << 30
MIN_N = 4
MIN_SPAN = 0.5 * np.pi
PROFILE_PASSES = 3

Marginals = collections.namedtuple("Marginals", "Q Z mass cx cz bad")
Marginals.__doc__ = """Q (n, nx), Z (n, nz) float64; mass (n,) = sum of Q[i]; cx, cz (n,) the centroids in pixels (NaN where the mass is 0);
bad (n,) int32, the non-finite values inside the z window."""


class ShiftEstimate(object):
    """xyz0          (n, 3): the shifts as `xyz_shift` takes them (column 1 zero), gauge-fixed
    axis_offset   c0 - (nx - 1) / 2, in the sign convention of rotation_axis.find_center's offset
    fit           (c0, a, b) of cx = c0 + a cos phi + b sin phi
    mass_spread   max / min - 1 of the masses
    residual_rms  the rms of cx minus the fitted law, pixels
    vertical      "moment" or "profile"
    marginals     the Marginals, with return_marginals"""

    def __init__(self, xyz0, axis_offset, fit, mass_spread, residual_rms, vertical, marginals=None):
        self.xyz0, self.axis_offset, self.fit, self.mass_spread = xyz0, float(axis_offset), tuple(float(v) for v in fit), float(mass_spread)
        self.residual_rms, self.vertical, self.marginals = float(residual_rms), vertical, marginals

    def __repr__(self):
        return ("ShiftEstimate(%d projections, x within %+.2f ... %+.2f px, z within %+.2f ... %+.2f px, axis offset %+.3f px, mass spread %.2e)"
                % (self.xyz0.shape[0], self.xyz0[:, 0].min(), self.xyz0[:, 0].max(), self.xyz0[:, 2].min(), self.xyz0[:, 2].max(),
                   self.axis_offset, self.mass_spread))


# --------------------------------------------------------------------------------------------------------- numpy: needs no device

def check_angles(n, phi):
    """phi as a float64 array of length n; ValueError for n < 4, another length, or a span below pi / 2.  Needs no device."""
    n = int(n)
    if n < MIN_N:
        raise ValueError("estimate_shifts: needs n >= %d projections, got %d" % (MIN_N, n))
    phi = np.asarray(phi, np.float64).ravel()
    if phi.size != n:
        raise ValueError("estimate_shifts: %d angles for %d projections" % (phi.size, n))
    if not np.all(np.isfinite(phi)):
        raise ValueError("estimate_shifts: the angles must be finite")
    span = float(phi.max() - phi.min())
    if span < MIN_SPAN:
        raise ValueError("estimate_shifts: the angles span %.3f rad; below pi / 2 the fit of c0 + a cos(phi) + b sin(phi) is ill-conditioned"
                         % span)
    return phi


def design(phi):
    """The columns 1, cos phi, sin phi."""
    phi = np.asarray(phi, np.float64).ravel()
    return np.column_stack([np.ones(phi.size), np.cos(phi), np.sin(phi)])


def fit_law(cx, phi):
    """The ordinary least-squares fit of cx to c0 + a cos phi + b sin phi -> ((c0, a, b), residual cx - law)."""
    A = design(phi)
    cx = np.asarray(cx, np.float64)
    coef = np.linalg.lstsq(A, cx, rcond=None)[0]
    return coef, cx - A.dot(coef)


def gauge_fix(shifts, phi):
    """`shifts` without what the laws absorb: (n, 3) as xyz (columns 0 and 2 are fixed, column 1 is kept) or (n, 2) as (x, z).  The x
    column loses its component in span{1, cos phi, sin phi}, the z column its mean."""
    s = np.array(shifts, np.float64)
    if s.ndim != 2 or s.shape[1] not in (2, 3):
        raise ValueError("gauge_fix: shifts must be (n, 3) or (n, 2), got shape %s" % (s.shape,))
    jz = s.shape[1] - 1
    s[:, 0] = fit_law(s[:, 0], phi)[1]
    s[:, jz] -= s[:, jz].mean()
    return s


def moments(Q, Z, bad=None):
    """Marginals from the two tables."""
    Q, Z = np.asarray(Q, np.float64), np.asarray(Z, np.float64)
    mass = Q.sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cx = Q.dot(np.arange(Q.shape[1], dtype=np.float64)) / mass
        cz = Z.dot(np.arange(Z.shape[1], dtype=np.float64)) / mass
    bad = np.zeros(Q.shape[0], np.int32) if bad is None else np.asarray(bad, np.int32)
    return Marginals(Q, Z, mass, cx, cz, bad)


def _aligned(Z, d, pad):
    """Row i of Z moved by -d[i] pixels, A[i](z) = Z[i](z + d[i]): a Fourier shift of the row continued by its edge values to 2 nz."""
    n, nz = Z.shape
    P = np.pad(Z, ((0, 0), (pad, nz - pad)), mode="edge")
    L = P.shape[1]
    k = np.arange(L // 2 + 1, dtype=np.float64)
    F = np.fft.rfft(P, axis=1) * np.exp(2j * np.pi * k[None, :] * d[:, None] / L)
    return np.fft.irfft(F, L, axis=1)[:, pad:pad + nz]


def profile_shifts(Z, upsample=20, max_lag=None, passes=PROFILE_PASSES):
    """The displacement d[i] of every profile Z[i] (n, nz) along z against the mean profile, minus its mean, to 1 / upsample px.
    A pass: every profile is moved back by the current d (_aligned), mean-removed and Hann-windowed; the reference is the mean of those;
    each is cross-correlated with it by FFT (zero-padded to 2 nz); the peak within |lag| <= max_lag (default nz // 4) is refined by an
    upsampled DFT over peak +- 1 on a grid of 1 / upsample, and added to d (kept within +- max_lag).  Three passes, the reference
    recomputed in each: in the first the window, fixed to the detector, pulls a profile d pixels off centre by a fraction of a pixel;
    from the second on the profiles lie under the same part of the window."""
    Z = np.asarray(Z, np.float64)
    n, nz = Z.shape
    upsample = int(upsample)
    max_lag = nz // 4 if max_lag is None else int(max_lag)
    if upsample < 1:
        raise ValueError("estimate_shifts: upsample must be >= 1, got %d" % upsample)
    if max_lag < 1 or max_lag >= nz:
        raise ValueError("estimate_shifts: max_lag must be in 1 ... nz - 1 = %d, got %d" % (nz - 1, max_lag))
    L = 2 * nz
    K = L // 2 + 1
    window = np.hanning(nz)
    lags = np.arange(-max_lag, max_lag + 1)
    frac = np.arange(-upsample, upsample + 1, dtype=np.float64) / upsample
    k = np.arange(K, dtype=np.float64)
    herm = np.full(K, 2.0)
    herm[0] = herm[-1] = 1.0
    E = np.exp(2j * np.pi * frac[:, None] * k[None, :] / L) * herm[None, :]          # (2 upsample + 1, K)
    d = np.zeros(n)
    for _ in range(int(passes)):
        A = _aligned(Z, d, nz // 2)
        A = (A - A.mean(axis=1, keepdims=True)) * window[None, :]
        X = np.fft.rfft(A, L, axis=1) * np.conj(np.fft.rfft(A.mean(axis=0), L))[None, :]
        cc = np.fft.irfft(X, L, axis=1)
        t0 = lags[np.argmax(cc[:, lags % L], axis=1)].astype(np.float64)
        X = X * np.exp(2j * np.pi * t0[:, None] * k[None, :] / L)
        fine = np.real(X.dot(E.T))                                                   # cc at t0 + frac, times L
        d = np.clip(d + t0 + frac[np.argmax(fine, axis=1)], -max_lag, max_lag)
    return d - d.mean()


def shifts_from_marginals(m, phi, vertical="moment", upsample=20, max_lag=None, allow_bad=False, return_marginals=False):
    """estimate_shifts from the Marginals `m` (numpy only)."""
    if vertical not in ("moment", "profile"):
        raise ValueError("estimate_shifts: vertical must be 'moment' or 'profile', not %r" % (vertical,))
    n, nx = m.Q.shape
    phi = check_angles(n, phi)
    if np.any(m.bad) and not allow_bad:
        raise ValueError("estimate_shifts: %d non-finite values in %d projections (they count as 0; allow_bad=True accepts that)"
                         % (int(np.sum(m.bad)), int(np.count_nonzero(m.bad))))
    if not np.all(m.mass > 0):
        raise ValueError("estimate_shifts: %d projections have a mass <= 0; the centroid of nothing is undefined (is `floor` too high, "
                         "or the -log missing?)" % int(np.count_nonzero(~(m.mass > 0))))
    coef, dx = fit_law(m.cx, phi)
    if vertical == "moment":
        dz = m.cz - m.cz.mean()
    else:
        dz = profile_shifts(m.Z, upsample, max_lag)
    xyz0 = np.zeros((n, 3))
    xyz0[:, 0], xyz0[:, 2] = -dx, -dz
    return ShiftEstimate(xyz0, coef[0] - 0.5 * (nx - 1), coef, m.mass.max() / m.mass.min() - 1.0, np.sqrt(np.mean(dx * dx)), vertical,
                         m if return_marginals else None)


# ------------------------------------------------------------------------------------------------------------------- the device

def _window(zrange, nz, who):
    if zrange is None:
        return 0, nz
    try:
        z0, z1 = (int(v) for v in zrange)
    except (TypeError, ValueError):
        raise ValueError("%s: zrange must be None or (z0, z1), got %r" % (who, zrange))
    return z0, z1


class Consistency(HandleOwner):
    """One libtomo_mom handle -- its partial sums and tables -- reused across calls.  ctx: the _lib.Context whose device and stream the
    work uses (default: that of the DeviceArray passed in, or a context of the handle's own)."""

    def _new_handle(self):
        return _mom_lib.MomHandle(self.ctx.device)

    def device_bytes(self):
        return 0 if self.handle is None else self.handle.device_bytes()

    def marginals(self, proj, floor=None, zrange=None, shape=None, max_scratch_bytes=DEFAULT_SCRATCH):
        """Marginals of proj (n, nx, nz): numpy (uploaded whole), or a float32 _lib.DeviceArray (a flat one needs `shape`).
        floor     None (no threshold), or the value below which a pixel counts as 0: background that is not exactly zero pulls every
                  centroid towards the detector centre
        zrange    None, or (z0, z1): only the detector rows z0 <= z < z1 are read
        max_scratch_bytes   the budget of the partial sums (None or 0: no limit); the bits do not depend on it"""
        n, nx, nz = _shape_of(proj, shape, "marginals")
        z0, z1 = _window(zrange, nz, "marginals")
        floor = -np.inf if floor is None else float(floor)
        if np.isnan(floor):
            raise ValueError("marginals: floor is NaN (None switches the threshold off)")
        _mom_lib.check_shape(n, nx, nz, z0, z1)                     # MomUnsupported before a context, a handle or a launch
        self._ready(proj)
        ctx, h = self.ctx, self.handle
        with self._staging(proj) as st:
            d_p = st.source(proj)
            h.set_max_scratch(max_scratch_bytes)
            Q, Z, bad = h.marginals(ctx.stream(), d_p.ptr, n, nx, nz, floor, z0, z1)      # waits
        return moments(Q, Z, bad)

    def estimate_shifts(self, proj, phi, floor=None, zrange=None, vertical="moment", upsample=20, max_lag=None, allow_bad=False,
                        return_marginals=False, shape=None, max_scratch_bytes=DEFAULT_SCRATCH):
        """The shifts of proj (n, nx, nz) taken at the angles phi -> ShiftEstimate (module docstring).
        floor, zrange, shape, max_scratch_bytes   as in marginals
        vertical     "moment": cz - mean(cz); "profile": profile_shifts of the Z[i], with upsample and max_lag
        allow_bad    False: ValueError if any value inside the window is non-finite; True: they count as 0
        ValueError before any launch for n < 4, phi not of length n, a span of phi below pi / 2 and a bad `vertical`; after the pass for
        non-finite values (unless allow_bad) and for a mass <= 0."""
        if vertical not in ("moment", "profile"):
            raise ValueError("estimate_shifts: vertical must be 'moment' or 'profile', not %r" % (vertical,))
        n, _, nz = _shape_of(proj, shape, "estimate_shifts")
        phi = check_angles(n, phi)
        if vertical == "profile":
            profile_shifts(np.zeros((1, nz)), upsample, max_lag, passes=0)              # its argument checks
        m = self.marginals(proj, floor, zrange, shape, max_scratch_bytes)
        return shifts_from_marginals(m, phi, vertical, upsample, max_lag, allow_bad, return_marginals)


def marginals(proj, floor=None, zrange=None, ctx=None, shape=None, handle=None, max_scratch_bytes=DEFAULT_SCRATCH):
    """Consistency.marginals on `handle` (a Consistency), or on one of its own on ctx."""
    if handle is not None:
        return handle.marginals(proj, floor, zrange, shape, max_scratch_bytes)
    with Consistency(ctx) as c:
        return c.marginals(proj, floor, zrange, shape, max_scratch_bytes)


def estimate_shifts(proj, phi, floor=None, zrange=None, vertical="moment", upsample=20, max_lag=None, allow_bad=False, return_marginals=False,
                    ctx=None, shape=None, handle=None, max_scratch_bytes=DEFAULT_SCRATCH):
    """Consistency.estimate_shifts on `handle` (a Consistency), or on one of its own on ctx."""
    kw = dict(floor=floor, zrange=zrange, vertical=vertical, upsample=upsample, max_lag=max_lag, allow_bad=allow_bad,
              return_marginals=return_marginals, shape=shape, max_scratch_bytes=max_scratch_bytes)
    if handle is not None:
        return handle.estimate_shifts(proj, phi, **kw)
    with Consistency(ctx) as c:
        return c.estimate_shifts(proj, phi, **kw)
