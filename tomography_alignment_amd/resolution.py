"""
Fourier shell correlation (FSC): a resolution measure that needs no ground truth.  Two independent reconstructions -- of the even and of
the odd projections -- are correlated shell by shell in Fourier space; the spatial frequency at which the curve falls below a threshold
is the resolution.  Alignment errors blur the two halves differently, so better poses push the crossing outwards.  The batched 2-D
form, the Fourier ring correlation (FRC), does the same for pairs of planes (projections, slices).

Definition (include/tomo_fsc.h, tests/fsc_model.py).  With A, B the real-to-complex transforms of the two masked, mean-free inputs, a
coefficient at the integer frequencies (kx, ky, kz), x and y signed and 0 <= kz <= nz/2, lies in the shell

    s = floor(r + 1/2),   r = sqrt(sum_i (k_i nmax / n_i)^2),   nmax = max(nx, ny, nz)

and counts with the Hermitian weight w = 1 on the planes kz = 0 and (nz even) kz = nz/2, w = 2 elsewhere.  For s <= min(n)/2:

    C[s] = sum w Re(A conj B)    PA[s] = sum w |A|^2    PB[s] = sum w |B|^2    count[s] = sum w        fsc[s] = C / sqrt(PA PB)

Shell s stands for the spatial frequency s / (nmax voxel_size) cycles per unit length.  The mask matters: without one the cube's edges
and the reconstruction cylinder correlate the two halves at every frequency and the curve never falls.  The default is a soft sphere
centred on the volume, radius R = min(n)/2 - E with a raised-cosine edge of E = 6 voxels; with subtract_mean the mask-weighted mean is
removed first.

The sums are float64 and deterministic -- the same input gives the same bits, so every rank of a sharded run takes the same decision
from the curve -- and only the 4 (min(n)/2 + 1) shell sums cross to the host.  Host arrays in are uploaded; _lib.DeviceArrays in stay
where they are (a flat device buffer, such as a solver's d_rec, needs `shape`).

Thresholds: the fixed 0.143 and 0.5, and van Heel & Schatz (2005), J. Struct. Biol. 151, 250: with n = count[s],
    half-bit  (0.2071 + 1.9102 / sqrt(n)) / (1.2071 + 0.9102 / sqrt(n))        one-bit  (0.5 + 2.4142 / sqrt(n)) / (1.5 + 1.4142 / sqrt(n))

Limits: one isotropic voxel_size; float32 transforms; one GPU holds both inputs and both spectra (about 17 GB plus the hipFFT work area
at 1024^3); no local-resolution maps; the n of the bit thresholds is the full shell's count, NOT corrected for the fraction of the
volume the mask leaves (a mask that covers a fraction q of the volume leaves about q n independent coefficients, so the bit curves
here are lower -- more lenient -- than a corrected one would be).
"""
import numpy as np

from . import _fsc_lib
from ._fsc_lib import FscUnsupported  # noqa: F401  (re-exported)
from ._ops import HandleOwner, _is_dev, shape_of as _shape_of
from .recon import fbp, sirt, sirt_mpi

THRESHOLDS = ("half-bit", "one-bit", "0.143", "0.5")


def threshold_curve(kind, count):
    """The threshold `kind` at every shell: float64 of count's shape.  kind: 'half-bit', 'one-bit', '0.143', '0.5' (or the numbers)."""
    n = np.asarray(count, np.float64)
    if kind in ("0.143", 0.143):
        return np.full(n.shape, 0.143)
    if kind in ("0.5", 0.5):
        return np.full(n.shape, 0.5)
    q = 1.0 / np.sqrt(np.where(n > 0, n, 1.0))
    if kind == "half-bit":
        t = (0.2071 + 1.9102 * q) / (1.2071 + 0.9102 * q)
    elif kind == "one-bit":
        t = (0.5 + 2.4142 * q) / (1.5 + 1.4142 * q)
    else:
        raise ValueError("unknown FSC threshold %r; choose one of %s" % (kind, ", ".join(THRESHOLDS)))
    return np.where(n > 0, t, 1.0)          # an empty shell resolves nothing


class FSCCurve(object):
    """The shell sums of one comparison and what is read off them.
    C, PA, PB, count   float64 (S,), S = min(n)/2 + 1 (module docstring)
    fsc                C / sqrt(PA PB); 0 where the denominator is 0 (shell 0 of mean-free inputs)
    freq               s / (nmax voxel_size), cycles per unit length
    nmax, voxel_size
    shift              None, or with fsc(..., register=True) the translation that was applied to the second volume first"""

    shift = None

    def __init__(self, C, PA, PB, count, nmax, voxel_size=1.0):
        self.C, self.PA, self.PB, self.count = (np.asarray(v, np.float64) for v in (C, PA, PB, count))
        self.nmax = int(nmax)
        self.voxel_size = float(voxel_size)
        if not (self.voxel_size > 0 and np.isfinite(self.voxel_size)):
            raise ValueError("voxel_size must be positive and finite, got %r" % (voxel_size,))
        den = np.sqrt(self.PA * self.PB)
        self.fsc = np.divide(self.C, den, out=np.zeros_like(self.C), where=den > 0)
        self.freq = np.arange(self.C.size) / (self.nmax * self.voxel_size)

    def __repr__(self):
        shell, status = self.crossing("half-bit")
        return "FSCCurve(%d shells, half-bit %s%s)" % (self.C.size, status, "" if shell is None else " at shell %.2f" % shell)

    def threshold(self, kind="half-bit"):
        return threshold_curve(kind, self.count)

    def crossing(self, kind="half-bit"):
        """(shell, status) of the FIRST downward crossing of the threshold after shell 0.
        'crossed'   the curve is below the threshold at a shell before the last one: `shell` is where the line between that shell and the
                    one before it meets the threshold (1.0 if shell 1 is already below);
        'nyquist'   it is below only at the last shell: resolved up to the Nyquist shell, shell None;
        'none'      it never is: shell None.
        A dip that recovers counts: the first crossing is the answer."""
        d = self.fsc - self.threshold(kind)
        last = d.size - 1
        for s in range(1, d.size):
            if d[s] < 0:
                if s == last and last > 1:
                    return None, "nyquist"
                if s == 1:
                    return 1.0, "crossed"
                return s - 1 + d[s - 1] / (d[s - 1] - d[s]), "crossed"
        return None, "none"

    def resolution(self, kind="half-bit"):
        """The length 1 / f of the first crossing (crossing()), or None if the curve does not cross before the last shell -- then
        crossing() says whether it reached the threshold at Nyquist or never."""
        shell, status = self.crossing(kind)
        if status != "crossed":
            return None
        return self.nmax * self.voxel_size / shell

    @property
    def nyquist(self):
        """The length of the last shell, the finest this sampling can show."""
        return self.nmax * self.voxel_size / (self.C.size - 1)


def pool_curves(curves):
    """One curve from several of the same shape (the planes of an frc): the sums added shell by shell, which weights every plane's shell
    by its power."""
    curves = list(curves)
    if not curves:
        raise ValueError("pool_curves: no curve")
    c0 = curves[0]
    return FSCCurve(sum(c.C for c in curves), sum(c.PA for c in curves), sum(c.PB for c in curves), sum(c.count for c in curves), c0.nmax,
                    c0.voxel_size)


def split_rows(n_proj, held=None):
    """The even / odd split of the GLOBAL projection indices 0 .. n_proj - 1, restricted to the rows `held` (global indices, default
    all): ((even rows held, their positions within the even half), (odd rows held, their positions within the odd half)).  The halves
    are formed before any sharding, so every world size reconstructs the same two halves."""
    held = np.arange(int(n_proj)) if held is None else np.asarray(held, np.int64).ravel()
    out = []
    for p in (0, 1):
        rows = held[held % 2 == p]
        out.append((rows, (rows - p) // 2))
    return tuple(out)


def half_weights(phi, parity):
    """fbp.angle_weights of ALL the angles of one half (parity 0: even global indices), so that the sum over the ranks is the unsharded
    FBP of that half; they sum to pi."""
    return fbp.angle_weights(np.asarray(phi, np.float64).ravel()[parity::2])


class Resolution(HandleOwner):
    """One libtomo_fsc handle and its hipFFT plans reused across calls.  ctx: the _lib.Context whose device and stream the work uses
    (default: that of the first DeviceArray passed in, or a context of the handle's own)."""

    def _new_handle(self):
        return _fsc_lib.FscHandle(self.ctx.device)

    def device_bytes(self):
        return 0 if self.handle is None else self.handle.device_bytes()

    def shell_sums(self, a, b, ndim, shape=None, mask="sphere", edge=6, radius=None, subtract_mean=True):
        """The table (nb, 4, S) of C, PA, PB, count for the pair a, b: volumes (ndim 3) or stacks of planes (ndim 2, shape (nb, nx, nz))."""
        sa, sb = _shape_of(a, shape, 3, "vol_a" if ndim == 3 else "stack_a"), _shape_of(b, shape, 3, "vol_b" if ndim == 3 else "stack_b")
        if sa != sb:
            raise ValueError("the two inputs must have one shape, got %s and %s" % (sa, sb))
        if ndim == 3:
            nb, (nx, ny, nz) = 1, sa
        else:
            nb, nx, nz = sa
            ny = 1
        _fsc_lib.n_shells(ndim, nb, nx, ny, nz)                  # FscUnsupported before a context, a handle or a launch
        mshape = (nx, ny, nz) if ndim == 3 else (nx, nz)
        axes = mshape
        mode = _fsc_lib.MASK_NONE
        edge = float(edge)
        if isinstance(mask, str):
            if mask != "sphere":
                raise ValueError("mask must be 'sphere', None or an array of shape %s, got %r" % (mshape, mask))
            if not (edge >= 0 and np.isfinite(edge)):
                raise ValueError("edge must be >= 0, got %r" % (edge,))
            mode = _fsc_lib.MASK_SPHERE
            radius = max(0.0, min(axes) / 2.0 - edge) if radius is None else float(radius)
            if not (radius >= 0 and np.isfinite(radius)):
                raise ValueError("radius must be >= 0, got %r" % (radius,))
        elif mask is not None:
            mode = _fsc_lib.MASK_ARRAY
            if _shape_of(mask, mshape if _is_dev(mask) else None, len(mshape), "mask") != mshape:
                raise ValueError("mask must have the shape %s" % (mshape,))
        self._ready(a if _is_dev(a) else b)
        ctx, h = self.ctx, self.handle
        with self._staging(a) as staging:
            m_ptr = staging.source(mask).ptr if mode == _fsc_lib.MASK_ARRAY else None
            h.set_shape(ndim, nb, nx, ny, nz)
            st = ctx.stream()
            for slot, v in enumerate((a, b)):
                h.prepare(st, slot, staging.source(v).ptr, mode, m_ptr, radius or 0.0, edge, subtract_mean)
                h.fft(st, slot)
            h.reduce(st)
            return h.fetch(st)

    def fsc(self, vol_a, vol_b, voxel_size=1.0, mask="sphere", edge=6, radius=None, subtract_mean=True, shape=None, register=False,
            upsample=10):
        """The FSC of two volumes (nx, ny, nz) -> FSCCurve (module docstring).
        register   True: vol_b is first registered to vol_a (registration.Registrar.register with the same mask arguments, `upsample`
                   and passes=2) and Fourier-shifted into a scratch volume, and the curve is taken of that; the curve's `shift` is the
                   translation found.  For two reconstructions that were aligned independently and so differ by the alignment's gauge."""
        if not register:
            t = self.shell_sums(vol_a, vol_b, 3, shape=shape, mask=mask, edge=edge, radius=radius, subtract_mean=subtract_mean)[0]
            return FSCCurve(t[0], t[1], t[2], t[3], max(_shape_of(vol_a, shape, 3, "vol_a")), voxel_size)
        from . import registration
        sv = _shape_of(vol_a, shape, 3, "vol_a")
        if _shape_of(vol_b, shape, 3, "vol_b") != sv:
            raise ValueError("the two inputs must have one shape, got %s and %s" % (sv, _shape_of(vol_b, shape, 3, "vol_b")))
        _fsc_lib.n_shells(3, 1, *sv)
        self._ready_ctx(vol_a if _is_dev(vol_a) else vol_b)
        with self._staging(vol_b) as st:
            d_b = st.source(vol_b)
            with registration.Registrar(self.ctx) as rg:
                reg = rg.register(vol_a, d_b, upsample=upsample, mask=mask, edge=edge, radius=radius, subtract_mean=subtract_mean, passes=2,
                                  shape=sv)
                d_s = rg.shift_volume(d_b, reg.shift, out=st.scratch(sv), shape=sv)
            t = self.shell_sums(vol_a, d_s, 3, shape=sv, mask=mask, edge=edge, radius=radius, subtract_mean=subtract_mean)[0]
        curve = FSCCurve(t[0], t[1], t[2], t[3], max(sv), voxel_size)
        curve.shift = tuple(float(v) for v in reg.shift)
        return curve

    def frc(self, stack_a, stack_b, voxel_size=1.0, mask="sphere", edge=6, radius=None, subtract_mean=True, shape=None, pool=False):
        """The FRC of every pair of planes of two stacks (nb, nx, nz): a list of nb FSCCurves, or with `pool` their pool_curves.  The
        mask is a disc, or an (nx, nz) array applied to every plane; the mean is per plane."""
        t = self.shell_sums(stack_a, stack_b, 2, shape=shape, mask=mask, edge=edge, radius=radius, subtract_mean=subtract_mean)
        nmax = max(_shape_of(stack_a, shape, 3, "stack_a")[1:])
        curves = [FSCCurve(p[0], p[1], p[2], p[3], nmax, voxel_size) for p in t]
        return pool_curves(curves) if pool else curves

    def take_rows(self, d_src, row_elems, first, step, count):
        """A new device buffer with the rows first, first + step, ... (count of them, row_elems floats each) of d_src."""
        self._ready(d_src)
        count, row_elems = int(count), int(row_elems)
        if count and int(first) + (count - 1) * int(step) >= d_src.size // row_elems:
            raise ValueError("take_rows: the rows asked for are not in the buffer")
        with self._staging(d_src) as st:
            out = st.dest((count * row_elems,))
            self.handle.take_rows(self.ctx.stream(), d_src.ptr, row_elems, first, step, count, out.ptr)
            return st.result(out)


def fsc(vol_a, vol_b, voxel_size=1.0, mask="sphere", edge=6, radius=None, subtract_mean=True, ctx=None, shape=None, register=False,
        upsample=10):
    """Resolution.fsc on a handle of its own."""
    with Resolution(ctx) as r:
        return r.fsc(vol_a, vol_b, voxel_size=voxel_size, mask=mask, edge=edge, radius=radius, subtract_mean=subtract_mean, shape=shape,
                     register=register, upsample=upsample)


def frc(stack_a, stack_b, voxel_size=1.0, mask="sphere", edge=6, radius=None, subtract_mean=True, ctx=None, shape=None, pool=False):
    """Resolution.frc on a handle of its own."""
    with Resolution(ctx) as r:
        return r.frc(stack_a, stack_b, voxel_size=voxel_size, mask=mask, edge=edge, radius=radius, subtract_mean=subtract_mean, shape=shape,
                     pool=pool)


class _HeldFBP(fbp.FBP):
    """recon.fbp.FBP of the rows a rank holds, with weights given from outside; the volume is summed over the communicator's ranks."""

    def __init__(self, comm, geometry, projections, angles, xyz_shifts, options):
        self._comm = comm
        super(_HeldFBP, self).__init__(geometry, projections, angles, xyz_shifts, options)

    def _allreduce_vol(self, buf):
        return buf if self._comm is None else self._comm.allreduce_sum_(buf)


def half_set_fsc(geometry, projections, angles, xyz_shifts, method="fbp", niter=None, options=None, comm=None, rows=None, resolution=None,
                 **fsc_kwargs):
    """The FSC of the reconstructions of the even and of the odd projections (GLOBAL indices) at the poses given -> FSCCurve.
    geometry, angles (n_proj, 3: phi, alpha, beta), xyz_shifts (n_proj, 3)   of ALL the projections, as for recon.fbp.FBP
    projections   a host array of all n_proj projections, or a device buffer that holds the rows `rows` (global indices; default this
                  rank's np.array_split block, i.e. all of them without a communicator)
    method        'fbp' (recon.fbp.FBP; options may carry `filter`) or 'sirt' with niter (recon.sirt.SIRT, one GPU only)
    comm          a communicator: every rank back-projects the rows of each half IT holds and the two volumes are all-reduced, so every
                  rank computes the curve of the same two volumes.  (recon.fbp_mpi.FBP itself would re-split each half over the ranks, and
                  the rows that split gives a rank are not in general among those it holds in HBM.)  The weights of a half are
                  fbp.angle_weights of all its angles (half_weights), as fbp_mpi does for the full set.
    options       `_backend`: the HipBackend to use (default one on the communicator's context or on a new one)
    resolution    a Resolution to reuse (default one for this call)
    Both reconstructions stay in HBM and are freed before the curve is returned; nothing volume-sized crosses to the host."""
    if method not in ("fbp", "sirt"):
        raise ValueError("half_set_fsc: method must be 'fbp' or 'sirt', not %r" % (method,))
    options = dict(options or {})
    angles = np.asarray(angles, np.float64).reshape(-1, 3)
    xyz = np.asarray(xyz_shifts, np.float64).reshape(-1, 3)
    n_proj = angles.shape[0]
    if n_proj < 2:
        raise ValueError("half_set_fsc: needs at least two projections")
    size = 1 if comm is None else (comm.Get_size() if hasattr(comm, "Get_size") else comm.size)
    rank = 0 if comm is None else (comm.Get_rank() if hasattr(comm, "Get_rank") else comm.rank)
    if method == "sirt":
        if size > 1:
            raise ValueError("half_set_fsc: method='sirt' runs on one GPU; use method='fbp' with a communicator")
        if niter is None or int(niter) < 1:
            raise ValueError("half_set_fsc: method='sirt' needs niter >= 1")
    held = np.array_split(np.arange(n_proj), size)[rank] if rows is None else np.asarray(rows, np.int64).ravel()
    be = options.pop("_backend", None)
    if be is None:
        from .backend import HipBackend
        be = HipBackend(sirt_mpi.SIRT._shard_geometry(geometry, held), ctx=getattr(comm, "ctx", None))
    ndx, ndz = (int(v) for v in geometry.det_shape)
    row_elems = ndx * ndz
    on_dev = be.is_buffer(projections)
    if on_dev and projections.size != held.size * row_elems:
        raise ValueError("half_set_fsc: the device projections must hold the %d rows given" % held.size)
    own = resolution is None
    res = Resolution(be.ctx) if own else resolution
    vols = []
    try:
        for parity, (mine, pos) in enumerate(split_rows(n_proj, held)):
            if on_dev:
                # this rank's rows of the half are every second row of its block
                first = int(np.searchsorted(held, mine[0])) if mine.size else 0
                if mine.size and not np.array_equal(held[first::2][:mine.size], mine):
                    raise ValueError("half_set_fsc: device rows must be consecutive global indices")
                d_p = res.take_rows(projections, row_elems, first, 2, mine.size) if mine.size else be.empty(0)
            else:
                d_p = be.upload(np.asarray(projections, np.float32).reshape(n_proj, -1)[mine])
            geo = sirt_mpi.SIRT._shard_geometry(geometry, mine)
            if method == "fbp":
                opts = dict(options, _backend=be, angle_weights=half_weights(angles[:, 0], parity)[pos], overwrite_projections=True,
                            download=False)
                f = _HeldFBP(comm, geo, d_p, angles[mine], xyz[mine], opts)
                f.run()
                vols.append(f.d_rec)
                f = None
            else:
                s = sirt.SIRT(geo, d_p, angles[mine], xyz[mine], options=dict(options, _backend=be))
                s.iterate_device(niter=int(niter))
                vols.append(s.d_rec)
                s = None
            d_p.free()
        return res.fsc(vols[0], vols[1], shape=tuple(int(v) for v in geometry.vox_shape), **fsc_kwargs)
    finally:
        for v in vols:
            v.free()
        if own:
            res.close()
