#!/usr/bin/env python3
"""
Joint reconstruction + rigid-body alignment -- the loop of the reference's examples/align_rigid.py:27-59:
alternate (a) SIRT with the current pose estimates and (b) a per-projection L-BFGS-B on cost_xzab / gradient_xzab
(tx, tz, alpha, beta; bounds +-3 px / +-0.02 rad).  Here (a) is the device-resident solver and (b) aligns all
projections in lock step, one fused cost/gradient launch per round (tomography_alignment_amd.alignment).

With a communicator (`comm`: tomography_alignment_amd.comm.RcclComm, one process per GPU) the projection angles are
sharded the way the reference shards them (np.array_split blocks, examples/mpi_reconstruct.py:34-38,
recon/sirt_mpi.py:40): rank r keeps ITS rows of the measured projections in HBM -- uploaded once, used by both halves
of every outer iteration -- reconstructs with the angle-sharded SIRT (recon/sirt_mpi.py: one sum of the voxel update
per iteration over xGMI) and aligns its own projections against the replicated reconstruction with no collective
inside the optimiser; the recovered pose table is summed once per outer iteration.  The reconstruction is warm-started
from the previous outer iteration's (examples/align_rigid.py:42) where it lies, in HBM.

Without ground truth (fsc=True, --fsc): after every alignment pass the even and the odd projections are reconstructed separately by FBP
at the current poses and their Fourier shell correlation (resolution.half_set_fsc) gives the half-bit resolution, in full-size pixels --
the monitor that measured data, which have no phantom, allow.

Rotation axis (cor=, --cor): measured data never have the axis on the detector's centre column, and the alignment searches a few pixels
only.  cor is the x component of `Geometry(cor_shift=)` in full-size pixels -- a number, or "auto": rotation_axis.find_center on
AUTO_COR_ROWS detector rows of the measured projections, the median offset turned into a cor_shift by rotation_axis.to_cor_shift.  The
reconstruction, the alignment pass and the FSC's FBPs all use it; None (the default) leaves every call as it was.

Pre-alignment (prealign=, --prealign): stages of nano-tomography jitter by tens of pixels, and the passes above search +-3 px around
their start.  prealign is that start -- "moment" or "profile": align.consistency.estimate_shifts on the measured projections (shifts
from the projections' own moments, no reconstruction); or an (n_proj, 3) array, e.g. the `xyz0` examples/preprocess --prealign stored.
It becomes the loop's base pose (xyz0, 0, 0): every alignment pass searches an increment around it.  None (the default) leaves every
call as it was.  Such a start is determined only up to what the consistency conditions absorb (a translation of the object and of the
axis), so the history's `shift_err_gauge_px` compares estimate and truth after consistency.gauge_fix.

Coarse to fine (run_multires, --levels): the first outer iterations run on data binned by 2^(levels-1), ..., 2 (multires.py: the
binning and prolongation kernels of libtomo_pyr.so), each level a unit-pitch geometry of its own; the poses (translations times 2, tilts
as they are) and the prolonged reconstruction are handed up, and only the last iterations run at full size.  The bounds of the optimiser
are in pixels of the level, so the same +-3 px reach +-12 full-size pixels at a level binned by 4.

    python -m tomography_alignment_amd.examples.align_rigid data.npz --outer 5 --sirt-iters 50
    python -m tomography_alignment_amd.examples.align_rigid data.npz --levels 3 --outer 3 --sirt-iters 50
    python -m tomography_alignment_amd.examples.align_rigid measured.npz --fsc          # no phantom needed: a resolution per outer iteration
    python -m tomography_alignment_amd.examples.align_rigid measured.npz --cor auto     # find the rotation axis first (rotation_axis.py)
    python -m tomography_alignment_amd.examples.align_rigid measured.npz --prealign moment   # start from the moments' shifts
    python -m torch.distributed.run --nproc-per-node 8 -m tomography_alignment_amd.examples.align_rigid data.npz
"""
import argparse
import time

import numpy as np

from .. import alignment, multires, registration, resolution, rotation_axis
from ..align import consistency
from ..recon import fbp, fbp_mpi, sirt, sirt_mpi
from ..utilities import geometry

DEFAULT_BOUNDS = ((-3., 3.), (-3., 3.), (-0.02, 0.02), (-0.02, 0.02))        # examples/align_rigid.py:48


class OuterLoop(object):
    """The state of the alternation and its two halves as separate calls -- `run` below is `for it: reconstruct(); align()`.
    (Separate, so that a test can hand BOTH an unsharded and a sharded loop the same reconstruction / the same poses and compare
    each half at float32 accuracy: the composition itself is not comparable that tightly, see tests/test_dist_gloo.py.)

    data: dict with `projections` (n_proj, nx, nz) and `phi`; optional `phantom` (ground truth -> RMSE per outer iteration) and
    `xyz`, `alpha`, `beta` (true poses -> pose errors in the history).  `projections` may be a DEVICE buffer that already holds this
    rank's rows (then `projections_shape` = (n_proj, nx, nz) says what it is a block of), `phantom` a device buffer too.
    comm     None: one GPU.  A communicator: angle-sharded over its ranks (module docstring); every rank holds the same poses.
    base     None, or (xyz0 (n_proj, 3), alpha0, beta0): a fixed pose the estimates start from and every alignment pass searches an
             INCREMENT around (from a zero start, inside the bounds); the estimate is base + increment (run_multires: the coarser level's).
    d_rec    None, or a device buffer that is the warm start of the first SIRT (it is updated in place).
    factor   the binning factor of the level `data` belongs to: `xyz` of the true poses is in full-size pixels, and pose_errors reports
             in full-size pixels.
    cor      None, or the x component of the geometry's cor_shift in pixels of THIS level (resolve_cor; a level of factor f gets the
             full-size value / f): the SIRT, the FBPs and the alignment pass all project with it."""

    def __init__(self, data, backend=None, comm=None, kernel_names=None, base=None, d_rec=None, factor=1, cor=None):
        self.comm = comm
        self.size = 1 if comm is None else (comm.Get_size() if hasattr(comm, "Get_size") else comm.size)
        self.rank = 0 if comm is None else (comm.Get_rank() if hasattr(comm, "Get_rank") else comm.rank)
        self.data = data
        self.phi = np.asarray(data["phi"], np.float64)
        n_proj = self.n_proj = self.phi.size
        proj = data["projections"]
        on_device = backend is not None and backend.is_buffer(proj)
        if on_device:
            _, nx, nz = (int(v) for v in data["projections_shape"])
        else:
            proj = np.asarray(proj, np.float32)
            nx, nz = proj.shape[1], proj.shape[2]
        ground_truth = data["phantom"] if "phantom" in data else None
        ny = int(data["ny"]) if "ny" in data else (ground_truth.shape[1] if getattr(ground_truth, "ndim", 0) == 3 else nx)
        self.vox_shape = (nx, ny, nz)
        self.cor = None if cor is None else float(cor)
        if self.cor is None:
            self.geom = geometry.Geometry(n_proj, np.array([nx, ny, nz]), np.ones(3), np.array([nx, nz]), np.ones(2))
        else:
            self.geom = geometry.Geometry(n_proj, np.array([nx, ny, nz]), np.ones(3), np.array([nx, nz]), np.ones(2),
                                          cor_shift=np.array([self.cor, 0.0, 0.0]))
        self.mine = np.array_split(np.arange(n_proj), self.size)[self.rank]           # recon/sirt_mpi.py:40
        if backend is None:
            from ..backend import HipBackend
            backend = HipBackend(sirt_mpi.SIRT._shard_geometry(self.geom, self.mine), ctx=getattr(comm, "ctx", None))
        be = self.be = backend
        self.ctx = getattr(be, "ctx", None)
        self.kernel_names = kernel_names
        # this rank's measured rows and the ground truth go to HBM ONCE; every SIRT call and every alignment pass reads them there
        self.d_b = proj if on_device else be.upload(proj.reshape(n_proj, -1)[self.mine])
        if self.d_b.size != self.mine.size * nx * nz:
            raise ValueError("align_rigid: the device table of measured projections must hold this rank's %d rows" % self.mine.size)
        self.d_gt = None
        if ground_truth is not None:
            self.d_gt = ground_truth if be.is_buffer(ground_truth) else be.upload(np.asarray(ground_truth, np.float32).ravel())
        self.alpha_rec, self.beta_rec, self.xyz_rec = np.zeros(n_proj), np.zeros(n_proj), np.zeros((n_proj, 3))
        self.base = None
        if base is not None:
            xyz0, alpha0, beta0 = (np.array(v, np.float64) for v in base)
            if xyz0.shape != (n_proj, 3) or alpha0.shape != (n_proj,) or beta0.shape != (n_proj,):
                raise ValueError("align_rigid: base must be (xyz0 (n_proj, 3), alpha0 (n_proj,), beta0 (n_proj,))")
            self.base = (xyz0, alpha0, beta0)
            self.xyz_rec, self.alpha_rec, self.beta_rec = xyz0.copy(), alpha0.copy(), beta0.copy()
        self.factor = int(factor)
        if d_rec is not None and d_rec.size != nx * ny * nz:
            raise ValueError("align_rigid: the initial reconstruction must hold the %d voxels of the volume" % (nx * ny * nz))
        self.d_rec, self.solver = d_rec, None

    def reconstruct(self, sirt_iters=50, positivity=True, init="zero"):
        """SIRT at the current pose estimates, warm-started from the previous reconstruction where it lies (examples/align_rigid.py:37-39,42).
        init: the start of the FIRST reconstruction -- "zero" (the reference's) or "fbp" (the filtered back-projection at the current pose
        estimates, recon/fbp.py).  -> (iterations done, rms_error[:k]); the reconstruction is self.d_rec."""
        if init not in ("zero", "fbp"):
            raise ValueError("align_rigid: init must be 'zero' or 'fbp', not %r" % (init,))
        opts = {"_backend": self.be}
        if self.d_gt is not None:
            opts["ground_truth"] = self.d_gt
        angles = np.array([self.phi, self.alpha_rec, self.beta_rec]).T
        if self.d_rec is None and init == "fbp":
            f_opts = {"_backend": self.be}
            if self.comm is None:
                f = fbp.FBP(self.geom, self.d_b, angles, self.xyz_rec, options=f_opts)
            else:
                f = fbp_mpi.FBP(self.comm, self.geom, self.d_b, angles, self.xyz_rec, options=f_opts)
            f.run(positivity=positivity)
            self.d_rec = f.d_rec
            f = None
        if self.d_rec is not None:
            opts["rec"] = self.d_rec                                          # in place, in HBM
        self.solver = None              # drop the previous solver's buffers BEFORE the next one allocates its own (d_rec is held separately)
        if self.comm is None:
            self.solver = sirt.SIRT(self.geom, self.d_b, angles, self.xyz_rec, options=opts)
        else:
            self.solver = sirt_mpi.SIRT(self.comm, self.geom, self.d_b, angles, self.xyz_rec, options=opts)
        k_done, err = self.solver.iterate_device(niter=sirt_iters, positivity=positivity)
        self.d_rec = self.solver.d_rec
        return k_done, err

    def align(self, bounds=DEFAULT_BOUNDS, **align_kwargs):
        """One alignment pass: every projection's L-BFGS-B on cost_xzab / gradient_xzab from a zero start against self.d_rec
        (examples/align_rigid.py:40-52); sets the pose estimates, returns alignment.align_projections' result dict."""
        kw = dict(letters="xzab", bounds=bounds)
        if self.base is not None:
            kw.update(xyz0=self.base[0], angles0=np.column_stack([self.phi, self.base[1], self.base[2]]))
        if self.cor is not None:
            kw.update(cor_shift=np.asarray(self.geom.cor_shift, np.float64))
        kw.update(align_kwargs)
        if self.comm is None:
            res = alignment.align_projections(self.be, self.d_rec, self.d_b, self.phi, indices=self.mine, **kw)
        else:
            res = alignment.align_projections_sharded(self.comm, self.be, self.d_rec, self.d_b, self.phi, **kw)
        self.xyz_rec = np.zeros((self.n_proj, 3))
        self.xyz_rec[:, 0], self.xyz_rec[:, 2] = res["x"][:, 0], res["x"][:, 1]
        self.alpha_rec, self.beta_rec = res["x"][:, 2].copy(), res["x"][:, 3].copy()
        if self.base is not None:
            self.xyz_rec += self.base[0]
            self.alpha_rec += self.base[1]
            self.beta_rec += self.base[2]
        return res

    def pose_errors(self):
        d = self.data
        if "xyz" not in d:
            return {}
        shifts = self.xyz_rec[:, [0, 2]] if self.factor == 1 else self.factor * self.xyz_rec[:, [0, 2]]
        return {"shift_err_px": float(np.abs(shifts - np.asarray(d["xyz"])[:, [0, 2]]).mean()),
                "shift_err_gauge_px": gauge_shift_error(shifts, np.asarray(d["xyz"])[:, [0, 2]], self.phi),
                "tilt_err_deg": float(np.rad2deg(np.abs(np.column_stack([self.alpha_rec, self.beta_rec]) - np.column_stack([d["alpha"], d["beta"]])).mean()))}

    def half_set_fsc(self, res=None):
        """The FSC of the FBPs of the even and of the odd projections at the current pose estimates (resolution.half_set_fsc): the halves by
        the parity of the GLOBAL index, each rank back-projecting the rows it holds."""
        angles = np.array([self.phi, self.alpha_rec, self.beta_rec]).T
        return resolution.half_set_fsc(self.geom, self.d_b, angles, self.xyz_rec, method="fbp", comm=self.comm, rows=self.mine,
                                       options={"_backend": self.be}, resolution=res)

    def download(self):
        return self.be.download(self.d_rec).reshape(self.vox_shape)


def gauge_shift_error(shifts, truth, phi):
    """The mean |difference| of two (n, 2) or (n, 3) shift tables after consistency.gauge_fix on both: what is left once the part no
    method can see -- x in span{1, cos phi, sin phi}, a constant z -- is taken out of estimate and truth alike."""
    a, b = consistency.gauge_fix(shifts, phi), consistency.gauge_fix(truth, phi)
    return float(np.abs(a[:, [0, -1]] - b[:, [0, -1]]).mean())


def resolve_prealign(data, prealign, comm=None, ctx=None, verbose=False):
    """The (n_proj, 3) start of the shifts that `prealign` stands for, full-size pixels: None -> None, an array -> itself (checked),
    "moment" / "profile" -> consistency.estimate_shifts on the measured projections.  With a communicator only an array is taken: a
    rank holds a block of the angles and the fit needs all of them; a string raises ValueError there -- estimate beforehand."""
    if prealign is None:
        return None
    n = np.size(data["phi"])
    if not isinstance(prealign, str):
        xyz0 = np.array(prealign, np.float64)
        if xyz0.shape != (n, 3) or not np.all(np.isfinite(xyz0)):
            raise ValueError("align_rigid: prealign must be None, 'moment', 'profile' or a finite (n_proj, 3) = (%d, 3) array" % n)
        return xyz0
    if prealign not in ("moment", "profile"):
        raise ValueError("align_rigid: prealign must be None, 'moment', 'profile' or an (n_proj, 3) array, not %r" % (prealign,))
    if comm is not None:
        raise ValueError("align_rigid: prealign=%r needs all projections on one GPU; with a communicator pass the (n_proj, 3) array "
                         "(consistency.estimate_shifts beforehand)" % (prealign,))
    proj = data["projections"]
    shape = tuple(int(v) for v in (data["projections_shape"] if "projections_shape" in data else np.shape(proj)))
    est = consistency.estimate_shifts(proj, np.asarray(data["phi"], np.float64), vertical=prealign, ctx=ctx, shape=shape)
    if verbose:
        print({"prealign": prealign, "axis_offset": est.axis_offset, "mass_spread": est.mass_spread, "residual_rms": est.residual_rms})
    return est.xyz0


def _base_of(xyz0, factor=1):
    """OuterLoop's base for a start of the shifts alone, in pixels of a level binned by `factor`."""
    return (xyz0 / float(factor), np.zeros(xyz0.shape[0]), np.zeros(xyz0.shape[0]))


AUTO_COR_ROWS = 9      # cor="auto" searches this many detector rows, spread evenly over the central half of z, and takes the median


def resolve_cor(data, cor, comm=None, ctx=None, verbose=False):
    """The x component of cor_shift, full-size pixels, that `cor` stands for: None -> None, a number -> itself, "auto" ->
    rotation_axis.find_center on the measured projections (`phi` must cover pi uniformly, with or without the endpoint; the search
    range is the default +-50 half-pixel steps, cut to what the detector holds), its median offset as a cor_shift.
    With a communicator only a number is taken: a rank holds a block of the angles, the search needs all of them for a detector row,
    and every rank needs the same value; "auto" raises ValueError there -- find the offset beforehand and pass the number."""
    if cor is None:
        return None
    if not isinstance(cor, str):
        cor = float(cor)
        if not np.isfinite(cor):
            raise ValueError("align_rigid: cor must be finite, got %r" % (cor,))
        return cor
    if cor != "auto":
        raise ValueError("align_rigid: cor must be None, a number or 'auto', not %r" % (cor,))
    if comm is not None:
        raise ValueError("align_rigid: cor='auto' needs all angles of a detector row on one GPU; with a communicator pass the number "
                         "(rotation_axis.find_center beforehand)")
    proj = data["projections"]
    shape = tuple(int(v) for v in (data["projections_shape"] if "projections_shape" in data else np.shape(proj)))
    n, nx, nz = shape
    smin, smax = rotation_axis.widest_range(nx)
    rows = rotation_axis.spread_rows(nz, AUTO_COR_ROWS)
    found = rotation_axis.find_center(proj, angles=np.asarray(data["phi"], np.float64), rows=rows, smin=smin, smax=smax, ctx=ctx, shape=shape)
    value = float(rotation_axis.to_cor_shift(found.offset, 1)[0, 0])
    if verbose:
        print({"cor": value, "offsets": found.offsets.tolist(), "rows": rows.tolist()})
    return value


def run(data, n_outer=5, sirt_iters=50, bounds=DEFAULT_BOUNDS, verbose=True, backend=None, align_kwargs=None, comm=None,
        kernel_names=None, download=True, return_loop=False, init="zero", fsc=False, cor=None, prealign=None, export=None,
        export_dtype=np.uint8, register_truth=False, segment=False, morphology=False, surface=False):
    """The loop of examples/align_rigid.py:36-52 (see OuterLoop for `data` and `comm`).
    segment        True: after the last outer iteration the reconstruction is segmented where it lies in HBM (_segmentation: Otsu's
                   threshold over the cylinder, threshold, label with 6 neighbours, measure; rank 0 of a sharded run) and the last
                   history entry gains `segmentation` = {"threshold", "n_components", "foreground_fraction", "largest_fraction"};
                   with `export` as well, export/labels_meta.json holds the same figures and the table of at most the 1000 largest
                   components.  With False (the default) nothing of the run changes.
    morphology     True (with segment): `segmentation` gains "max_inscribed_radius", the largest distance of a mask voxel to the
                   background or the outside of the volume in voxels (morphology.distance, "background"), and "closed_porosity",
                   the voxels fill_holes adds over foreground plus those (0 without foreground); labels_meta.json holds them too.
                   Nothing else of the run changes.
    surface        True (with segment): `segmentation` gains "surface_area", "enclosed_volume" and "specific_surface" (area over
                   enclosed volume, 0 when the volume is not positive) of the isosurface of the reconstruction at the segmentation's
                   threshold (mesh, border "closed"; voxel units); labels_meta.json holds them too, and with `export` the surface is
                   written to export/surface.stl.  Nothing else of the run changes.
    register_truth True, and the data carry a phantom: every history entry gains `truth_shift` and `rmse_registered` (_truth_entry), the
                   RMSE after the gauge translation between reconstruction and phantom is taken out; `rmse` stays as it is.
    init           "zero" (default, the reference's) or "fbp": the first outer iteration's SIRT starts from the FBP at the current poses.
    fsc            True: every history entry gains `fsc_resolution` (pixels) and `fsc_curve` (_fsc_entry); needs no phantom.
    cor            None, a number or "auto" (resolve_cor; "auto" only without a communicator): the geometry's cor_shift x.  With a
                   value every history entry carries it as `cor`; with None nothing changes.
    prealign       None, "moment", "profile" (only without a communicator) or an (n_proj, 3) array (resolve_prealign): the loop's base
                   pose is (xyz0, 0, 0); with None the loop is built as before.
    export         None, or a directory: after the last outer iteration postprocess.export_stack writes the reconstruction there from
                   where it lies in HBM (8- or 16-bit z slices by export_dtype, meta.json, previews; rank 0 of a sharded run, whose
                   volume is whole on every rank).  With None nothing of the run changes.
    kernel_names   with a HIP context: the history carries the HIP-event kernel time of each half of each outer iteration for these names.
    Returns (rec or None when not `download`, alpha, beta, xyz, history) -- with `return_loop` a sixth element, the OuterLoop itself
    (`loop.d_rec`: the reconstruction where it lies in HBM, `loop.solver`, `loop.d_b`).  Nothing is kept alive behind the caller's back:
    until round 5 the loop was parked in `run.last_loop`, which pinned about six volume-sized buffers until the next call."""
    if morphology and not segment:
        raise ValueError("run: morphology=True goes with segment=True")
    if surface and not segment:
        raise ValueError("run: surface=True goes with segment=True")
    cor = resolve_cor(data, cor, comm, getattr(backend, "ctx", None), verbose)
    xyz0 = resolve_prealign(data, prealign, comm, getattr(backend, "ctx", None), verbose)
    start = {} if xyz0 is None else {"base": _base_of(xyz0)}
    loop = OuterLoop(data, backend=backend, comm=comm, kernel_names=kernel_names, cor=cor, **start)
    history = []
    res = resolution.Resolution(loop.ctx) if fsc else None
    reg = registration.Registrar(loop.ctx) if (register_truth and loop.d_gt is not None) else None
    try:
        for it in range(n_outer):
            history.append(_outer_iteration(loop, it, sirt_iters, bounds, init, align_kwargs, kernel_names, verbose, fsc_with=res,
                                            extra=None if cor is None else {"cor": cor}, truth_with=reg))
    finally:
        if res is not None:
            res.close()
        if reg is not None:
            reg.close()
    if export is not None and loop.d_rec is not None and loop.rank == 0:
        from .. import postprocess
        postprocess.export_stack(loop.d_rec, export, dtype=export_dtype, ctx=loop.ctx, shape=loop.vox_shape)
    if segment and loop.d_rec is not None and loop.rank == 0:
        if not history:
            history.append({})
        history[-1]["segmentation"] = _segmentation(loop, export, verbose, morphology=morphology, surface=surface)
    rec = loop.download() if (download and loop.d_rec is not None) else None
    out = (rec, loop.alpha_rec, loop.beta_rec, loop.xyz_rec, history)
    return out + (loop,) if return_loop else out


def _segmentation(loop, export=None, verbose=False, limit=1000, morphology=False, surface=False):
    """The reconstruction (loop.d_rec, not written) split into its connected objects on the device: Otsu's threshold of the 4096-bin
    histogram over the reconstruction cylinder, the mask v >= threshold inside the cylinder, its components with 6 neighbours and their
    measures; only the tables come to the host.  -> {"threshold", "n_components", "foreground_fraction" (of the cylinder's voxels),
    "largest_fraction" (of the foreground; 0 without one)}.  export: a directory; labels_meta.json there holds the same and
    "components", the `limit` largest as {"label", "count", "bbox", "centroid"}.  morphology: also "max_inscribed_radius" and
    "closed_porosity" (_mask_morphology), taken from the same mask before it is freed.  surface: also "surface_area", "enclosed_volume"
    and "specific_surface" (_surface), from the reconstruction itself at the threshold; with export, surface.stl there."""
    import json
    import os

    from .. import segment as seg_mod
    from ..postprocess import region_r4
    shape = tuple(int(s) for s in loop.vox_shape)
    with seg_mod.Segmenter(loop.ctx) as seg:
        t, = seg.otsu(loop.d_rec, 2, 4096, None, "cylinder", shape=shape)
        d_mask = seg.threshold(loop.d_rec, lo=t, region="cylinder", shape=shape)
        d_labels, n = seg.label(d_mask, 1, shape=shape)
        extra = _mask_morphology(loop, d_mask, shape) if morphology else None
        d_mask.free()
        comp = seg.measure(d_labels, n, shape=shape)
        d_labels.free()
    area = _surface(loop, float(t), shape, export) if surface else None
    fg = int(comp.count.sum())
    a, b = (2 * np.arange(k, dtype=np.int64) - k + 1 for k in shape[:2])          # the region's integer test (postprocess)
    inside = int(np.count_nonzero(a[:, None] ** 2 + b[None, :] ** 2 <= region_r4("cylinder", shape[0], shape[1]))) * shape[2]
    out = {"threshold": float(t), "n_components": int(n), "foreground_fraction": fg / float(inside),
           "largest_fraction": float(comp.count.max()) / fg if n else 0.0}
    if extra is not None:
        radius, filled = extra
        out.update(max_inscribed_radius=radius, closed_porosity=filled / float(fg + filled) if fg else 0.0)
    if area is not None:
        out.update(surface_area=area[0], enclosed_volume=area[1], specific_surface=area[0] / area[1] if area[1] > 0 else 0.0)
    if export is not None:
        os.makedirs(export, exist_ok=True)
        with open(os.path.join(export, "labels_meta.json"), "w") as f:
            json.dump(dict(out, components=comp.table(limit)), f, indent=1)
    if verbose:
        print({"segmentation": out})
    return out


def _mask_morphology(loop, d_mask, shape):
    """-> (the largest distance of a voxel of the device mask to its background or the outside of the volume, in voxels; the number of
    voxels fill_holes adds to it).  Only the two numbers come to the host."""
    from .. import morphology as morph_mod
    from .. import postprocess
    with morph_mod.Morphology(loop.ctx) as mo:
        d_dist = mo.distance(d_mask, "background", shape=shape)
        radius = float(postprocess.statistics(d_dist, ctx=loop.ctx, shape=shape).max)
        d_dist.free()
        d_filled, filled = mo.fill_holes(d_mask, return_count=True, shape=shape)
        d_filled.free()
    return radius, int(filled)


def _surface(loop, level, shape, export=None):
    """-> (area, enclosed volume) of the isosurface of the reconstruction (loop.d_rec, not written) at `level` with the closed border,
    in voxel units.  Without export only the numbers come to the host; with it the triangles do, once, for export/surface.stl."""
    import os

    from .. import mesh as mesh_mod
    with mesh_mod.MeshExtractor(loop.ctx) as mx:
        if export is None:
            m = mx.measure(loop.d_rec, level, "closed", shape=shape)
            return float(m.area), float(m.volume)
        s = mx.isosurface(loop.d_rec, level, "closed", shape=shape)
        tri = s.triangles.download() if s.n else np.zeros((0, 3, 3), np.float32)
        s.triangles.free()
    os.makedirs(export, exist_ok=True)
    mesh_mod.write_stl(os.path.join(export, "surface.stl"), tri)
    return float(s.area), float(s.volume)


def _fsc_entry(loop, res):
    """`fsc_resolution`: the half-bit resolution of the half-set FBPs at the current poses, in pixels of the level times the level's factor;
    where the curve stays above the threshold up to the last shell, that shell's length (the sampling limit, 2 pixels of the level).
    `fsc_curve`: the resolution.FSCCurve itself (its crossing() tells the two cases apart)."""
    curve = loop.half_set_fsc(res)
    r = curve.resolution("half-bit")
    return {"fsc_resolution": float(loop.factor * (curve.nyquist if r is None else r)), "fsc_curve": curve}


def _truth_entry(loop, reg, upsample=10):
    """`truth_shift`: the translation that moves the reconstruction onto the phantom (registration.Registrar.register, upsample 10, one
    pass).  No mask and no mean: the Fourier shift does not lengthen a volume, so the largest plain correlation IS the smallest
    ||phantom - shifted reconstruction|| over the candidates, the coarse peak is one of them and is no worse than a shift of zero;
    without a mask there is no mask bias for a second pass to remove.
    `rmse_registered`: ||phantom - shift_volume(rec, truth_shift)|| / ||phantom||, formed on the device from loop.d_rec, which is not
    written; `rmse` punishes a correct alignment that moved the object by half a voxel like a wrong one, this does not."""
    be, shape = loop.be, loop.vox_shape
    found = reg.register(loop.d_gt, loop.d_rec, upsample=upsample, mask=None, subtract_mean=False, passes=1, shape=shape)
    d_s = reg.shift_volume(loop.d_rec, found.shift, shape=shape)
    try:
        norm = np.sqrt(be.dot(loop.d_gt, loop.d_gt))
        rmse = float(np.sqrt(be.diff_sumsq(loop.d_gt, d_s)) / norm) if norm > 0 else float("nan")
    finally:
        d_s.free()
    return {"truth_shift": [float(v) for v in found.shift], "rmse_registered": rmse}


def _outer_iteration(loop, it, sirt_iters, bounds, init, align_kwargs, kernel_names, verbose, extra=None, fsc_with=None, truth_with=None):
    """One outer iteration of `loop` -- SIRT, then the alignment pass -- and its history entry (`extra`: more keys for it; `fsc_with`: a
    resolution.Resolution -> the entry of _fsc_entry; `truth_with`: a registration.Registrar -> the entry of _truth_entry)."""
    ctx = loop.ctx
    k0 = _kernel_ms(ctx, kernel_names)
    t0 = time.perf_counter()
    k_done, err = loop.reconstruct(sirt_iters, init=init)
    if ctx is not None:
        ctx.sync()
    t1 = time.perf_counter()
    truth = _truth_entry(loop, truth_with) if truth_with is not None else None      # of the reconstruction `rmse` is of; outside both walls
    t1a = time.perf_counter() if truth is not None else t1
    k1 = _kernel_ms(ctx, kernel_names)
    res = loop.align(bounds, **(align_kwargs or {}))
    t2 = time.perf_counter()
    k2 = _kernel_ms(ctx, kernel_names)
    entry = {"outer": it, "rmse": float(err[-1]), "sirt_iterations": int(k_done), "residual": float(res["fun"].sum()), "launches": res["n_launch"],
             "evals": res["n_eval"], "driver": res.get("driver"), "sirt_wall_s": round(t1 - t0, 3), "align_wall_s": round(t2 - t1a, 3),
             "ranks": loop.size}
    if kernel_names and ctx is not None:
        entry["sirt_kernel_ms"] = {k: round(k1[k] - k0[k], 1) for k in k1 if k1[k] - k0[k] > 0}
        entry["align_kernel_ms"] = {k: round(k2[k] - k1[k], 1) for k in k2 if k2[k] - k1[k] > 0}
    entry.update(loop.pose_errors())
    if extra:
        entry.update(extra)
    if fsc_with is not None:
        entry.update(_fsc_entry(loop, fsc_with))
    if truth is not None:
        entry.update(truth)
    if verbose and loop.rank == 0:
        print(entry)
    return entry


def _per_level(value, levels, name):
    """`value` as one entry per level, coarsest first: a number is repeated, a sequence must have `levels` entries."""
    if np.ndim(value) == 0:
        return [int(value)] * levels
    value = [int(v) for v in value]
    if len(value) != levels:
        raise ValueError("run_multires: %s needs one entry per level (%d), got %d" % (name, levels, len(value)))
    return value


def run_multires(data, levels=3, n_outer=(3, 3, 2), sirt_iters=50, bounds=DEFAULT_BOUNDS, verbose=True, align_kwargs=None, comm=None,
                 kernel_names=None, download=True, return_loop=False, init="zero", ctx=None, backend_factory=None, pyramid=None, fsc=False,
                 cor=None, prealign=None):
    """`run` coarse to fine (module docstring): levels binned by 2^(levels-1), ..., 2, 1, coarsest first.
    n_outer, sirt_iters   one number, or one per level, coarsest first.
    bounds                of the increment every pass searches around the pose carried up from the coarser level (zero at the coarsest),
                          in pixels of the level.
    init                  the start of the coarsest level's first SIRT; every finer level starts from the prolonged coarser reconstruction.
    fsc                   as in `run`; `fsc_resolution` is in full-size pixels at every level.
    cor                   as in `run`, in full-size pixels (found on the full-size data); a level binned by f projects with cor / f.
    prealign              as in `run`, in full-size pixels (estimated on the full-size data); the coarsest level's base pose is it divided
                          by that level's factor, and every finer level starts from the coarser level's estimate as before.
    ctx                   the _lib.Context all levels share (default: the communicator's, or a new one).
    backend_factory, pyramid   test seams: geometry -> backend (default a HipBackend on ctx per level), and the object with multires.Pyramid's
                          three methods (default a Pyramid on ctx).
    Per level: the data are bin_projections of this rank's FULL-SIZE rows and bin_volume of the full-size ground truth (never of the previous
    level's); the level's OuterLoop runs on the unit-pitch geometry of the binned sizes (multires.level_geometry); its base pose is the
    coarser level's estimate with the translations times 2 and the tilts as they are.  The centre-of-rotation offset `cor`, where one is
    given, is a length like the translations: the level's geometry gets cor / f.  A finished level's buffers are freed before the next
    level allocates its own.
    Returns what `run` returns; every history entry also carries `level` (0: the coarsest) and `factor`, and its shift error is in
    full-size pixels.  levels=1 IS `run`."""
    levels = int(levels)
    if levels < 1 or 2 ** (levels - 1) > multires.FACTORS[-1]:
        raise ValueError("run_multires: levels must be 1 ... %d, got %d" % (len(multires.FACTORS) + 1, levels))
    n_outer, sirt_iters = _per_level(n_outer, levels, "n_outer"), _per_level(sirt_iters, levels, "sirt_iters")
    if levels == 1:
        out = run(data, n_outer[0], sirt_iters[0], bounds=bounds, verbose=verbose, align_kwargs=align_kwargs, comm=comm,
                  kernel_names=kernel_names, download=download, return_loop=return_loop, init=init, fsc=fsc, cor=cor, prealign=prealign)
        for entry in out[4]:
            entry.update(level=0, factor=1)
        return out
    if init not in ("zero", "fbp"):
        raise ValueError("align_rigid: init must be 'zero' or 'fbp', not %r" % (init,))
    phi = np.asarray(data["phi"], np.float64)
    n_proj = phi.size
    proj = data["projections"]
    on_device = "projections_shape" in data
    _, nx, nz = (int(v) for v in (data["projections_shape"] if on_device else np.shape(proj)))
    ground_truth = data["phantom"] if "phantom" in data else None
    ny = int(data["ny"]) if "ny" in data else (ground_truth.shape[1] if getattr(ground_truth, "ndim", 0) == 3 else nx)
    f_max = 2 ** (levels - 1)
    for e in (nx, ny, nz):
        if e % f_max:
            raise ValueError("run_multires: %d levels need sizes divisible by %d, got %d x %d x %d" % (levels, f_max, nx, ny, nz))
    size = 1 if comm is None else (comm.Get_size() if hasattr(comm, "Get_size") else comm.size)
    rank = 0 if comm is None else (comm.Get_rank() if hasattr(comm, "Get_rank") else comm.rank)
    mine = np.array_split(np.arange(n_proj), size)[rank]
    if backend_factory is None:
        from .. import _lib
        from ..backend import HipBackend
        if ctx is None:
            ctx = getattr(comm, "ctx", None)
        if ctx is None:
            ctx = _lib.Context()
        backend_factory = lambda g: HipBackend(g, ctx=ctx)      # noqa: E731
    cor = resolve_cor(data, cor, comm, ctx, verbose)
    xyz0 = resolve_prealign(data, prealign, comm, ctx, verbose)
    own_pyramid = pyramid is None
    if own_pyramid:
        pyramid = multires.Pyramid(ctx)
    res = None
    try:
        poses = {k: data[k] for k in ("xyz", "alpha", "beta") if "xyz" in data}
        be = backend_factory(sirt_mpi.SIRT._shard_geometry(multires.level_geometry(n_proj, (nx, ny, nz)), mine))
        # this rank's full-size rows and the ground truth go to HBM once: every level's data are made from them there
        d_b = proj if on_device else be.upload(np.asarray(proj, np.float32).reshape(n_proj, -1)[mine])
        d_gt = None
        if ground_truth is not None:
            d_gt = ground_truth if be.is_buffer(ground_truth) else be.upload(np.asarray(ground_truth, np.float32).ravel())
        history, carried, d_rec, loop = [], None if xyz0 is None else _base_of(xyz0, f_max), None, None
        for level in range(levels):
            f = 2 ** (levels - 1 - level)
            shape = (nx // f, ny // f, nz // f)
            if f == 1:
                be_l, d_b_l, d_gt_l = be, d_b, d_gt
            else:
                be_l = backend_factory(sirt_mpi.SIRT._shard_geometry(multires.level_geometry(n_proj, (nx, ny, nz), f), mine))
                # (a rank that owns no angle keeps a zero-row table, as in `run`)
                d_b_l = pyramid.bin_projections(d_b, f, shape=(mine.size, nx, nz)) if mine.size else be_l.empty(0)
                d_gt_l = pyramid.bin_volume(d_gt, f, shape=(nx, ny, nz)) if d_gt is not None else None
            ldata = dict(poses, projections=d_b_l, projections_shape=(n_proj,) + shape[::2], phi=phi, ny=shape[1])
            if d_gt_l is not None:
                ldata["phantom"] = d_gt_l
            loop = OuterLoop(ldata, backend=be_l, comm=comm, kernel_names=kernel_names, base=carried, d_rec=d_rec, factor=f,
                             cor=None if cor is None else cor / f)
            if fsc and res is None:
                res = resolution.Resolution(loop.ctx)
            for _ in range(n_outer[level]):
                history.append(_outer_iteration(loop, len(history), sirt_iters[level], bounds, init if level == 0 else "zero", align_kwargs,
                                                kernel_names, verbose, fsc_with=res,
                                                extra={"level": level, "factor": f} if cor is None else {"level": level, "factor": f, "cor": cor}))
            if f == 1:
                break
            # hand up, and free what this level held before the finer one allocates: the solver's buffers, the binned data, then -- once it is
            # prolonged -- the coarse reconstruction
            carried = (2.0 * loop.xyz_rec, loop.alpha_rec.copy(), loop.beta_rec.copy())
            coarse, loop.solver, loop.d_rec, loop.d_b, loop.d_gt = loop.d_rec, None, None, None, None
            _free(d_b_l, d_gt_l)
            d_b_l = d_gt_l = ldata = None
            d_rec = None
            if coarse is not None:
                d_rec = pyramid.prolong_volume(coarse, shape=shape)
                _free(coarse)
    finally:
        if res is not None:
            res.close()
        if own_pyramid:
            pyramid.close()
    rec = loop.download() if (download and loop.d_rec is not None) else None
    out = (rec, loop.alpha_rec, loop.beta_rec, loop.xyz_rec, history)
    return out + (loop,) if return_loop else out


def _free(*bufs):
    for b in bufs:
        if b is not None and hasattr(b, "free"):
            b.free()


def _kernel_ms(ctx, names):
    if ctx is None or not names:
        return {}
    return {k: ctx.profile_get(k)[1] for k in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("data")
    ap.add_argument("--outer", type=int, default=5)
    ap.add_argument("--sirt-iters", type=int, default=50)
    ap.add_argument("--init", choices=("zero", "fbp"), default="zero", help="start of the first SIRT: zero or the FBP")
    ap.add_argument("--levels", type=int, default=1, help="resolution levels, coarse to fine (run_multires); --outer and --sirt-iters "
                    "then count per level.  1: the plain loop")
    ap.add_argument("--fsc", action="store_true", help="report the half-bit resolution of the half-set Fourier shell correlation per outer "
                    "iteration (needs no phantom)")
    ap.add_argument("--cor", default=None, metavar="D|auto", help="the rotation axis as Geometry's cor_shift x in pixels, or 'auto' to find it "
                    "from the sinograms first (rotation_axis.find_center; one GPU)")
    ap.add_argument("--prealign", default=None, metavar="moment|profile|file", help="start the shifts from the projections' moments "
                    "(align.consistency; one GPU), or from the key xyz0 of the data file itself with 'file' (preprocess --prealign)")
    ap.add_argument("--export", default=None, metavar="DIR", help="write the reconstruction as a stack of z slices (slice_%%05d.npy), "
                    "meta.json and previews into DIR, converted on the GPU (postprocess.export_stack; --levels 1)")
    ap.add_argument("--export-dtype", choices=("uint8", "uint16"), default="uint8")
    ap.add_argument("--segment", action="store_true", help="segment the reconstruction on the GPU after the last outer iteration: Otsu's "
                    "threshold over the cylinder, connected components with 6 neighbours and their measures (segment; --levels 1); with "
                    "--export, DIR/labels_meta.json holds the component table")
    ap.add_argument("--morphology", action="store_true", help="with --segment: also the largest inscribed radius of the mask (the exact "
                    "Euclidean distance transform) and its closed porosity (hole filling) on the GPU (morphology)")
    ap.add_argument("--surface", action="store_true", help="with --segment: also the area and the enclosed volume of the isosurface of "
                    "the reconstruction at the segmentation's threshold and their ratio, the specific surface, on the GPU (mesh); "
                    "with --export the surface is written to surface.stl")
    ap.add_argument("--register-truth", action="store_true", help="with a phantom in the data: also report the RMSE after the reconstruction "
                    "is registered to the phantom (truth_shift, rmse_registered); --levels 1 only")
    a = ap.parse_args()
    cor = a.cor if a.cor in (None, "auto") else float(a.cor)
    if a.export is not None and a.levels != 1:
        ap.error("--export goes with --levels 1")
    if a.segment and a.levels != 1:
        ap.error("--segment goes with --levels 1")
    if a.morphology and not a.segment:
        ap.error("--morphology goes with --segment")
    if a.surface and not a.segment:
        ap.error("--surface goes with --segment")
    if a.prealign not in (None, "moment", "profile", "file"):
        ap.error("--prealign must be moment, profile or file")
    import os
    comm = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:       # launched one process per GPU: python -m torch.distributed.run --nproc-per-node N -m ...
        from ..comm import RcclComm
        comm = RcclComm.from_env()
    data = dict(np.load(a.data))
    if a.prealign == "file" and "xyz0" not in data:
        ap.error("--prealign file: %s holds no xyz0 (write it with examples/preprocess --prealign)" % a.data)
    prealign = data["xyz0"] if a.prealign == "file" else a.prealign
    if a.levels == 1:
        run(data, a.outer, a.sirt_iters, comm=comm, init=a.init, fsc=a.fsc, cor=cor, prealign=prealign, export=a.export,
            export_dtype=np.dtype(a.export_dtype), register_truth=a.register_truth, segment=a.segment, morphology=a.morphology, surface=a.surface)
    else:
        run_multires(data, a.levels, a.outer, a.sirt_iters, comm=comm, init=a.init, fsc=a.fsc, cor=cor, prealign=prealign)
    if comm is not None:
        comm.close()


if __name__ == "__main__":
    main()
