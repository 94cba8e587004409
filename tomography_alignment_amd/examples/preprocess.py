#!/usr/bin/env python3
"""
Raw detector frames to the projections examples/align_rigid.py reads: flat-field normalisation, -log and sorting-based stripe removal
on the GPU (tomography_alignment_amd.preprocess).  The input is a file with `counts` ([n_proj][z][x], uint16 or float32), `flats` and
`darks` (stacks of frames in the same layout), such as `generate_data --raw` writes; an optional `mu` (the attenuation per unit of
projection) divides the line integrals back into the phantom's units.  Every other key (phi, alpha, beta, xyz, phantom, ...) is carried
through; counts, flats and darks are dropped.

For data recorded with a propagation distance, `phase` (--phase-strength A, or --pixel-size, --dist, --energy and --delta-beta) puts
Paganin's single-distance phase retrieval between the flat-field division and the -log: normalize(minus_log=False) -> retrieve_phase
-> stripe removal.  Without it the calls and the result are what they were before the option existed.

`--stripe all` replaces the sorting-based removal by preprocess.remove_all_stripe -- dead stripes, large stripes, then the sorting pass
with --stripe-size as its window -- for detectors with stuck or mis-gained columns (generate_data --dead-columns / --gain-columns);
`--stripe none` skips the removal.  The default, `--stripe sorting`, is the sorting pass alone.

`--zinger-dif D` (with `--zinger-size S`, default 3) first removes zingers (preprocess.remove_outlier, one-sided): from the uploaded
counts, in place on the device, and from the flats before normalize reduces them (generate_data --zingers).  Without it the calls and
the result are exactly what they were.

`--find-center` (with `--center-rows K`, default 9) finds the rotation axis on the finished sinogram, where it lies on the device
(rotation_axis.find_center on K detector rows spread over the central half of z, the median offset), and stores it as `cor_offset`: the
x component of Geometry's cor_shift, the number align_rigid's --cor takes.  The data need `phi`, covering pi uniformly.

`--prealign [moment|profile]` estimates the per-projection shifts from the moments of the finished sinogram, where it lies on the device
(align.consistency.estimate_shifts; `profile` for samples that extend past the detector vertically), and stores `xyz0` ((n, 3), the
number align_rigid's --prealign takes from the file), `axis_offset` and `mass_spread`.  The data need `phi`, spanning at least pi / 2.

`--dynamic-flat [M]` divides every projection by a flat of its own (preprocess.normalize_dynamic, for a beam that moves between the flats
and the projections: generate_data --beam-drift): the mean flat plus M eigen flat fields of the flats -- without a number, as many as
the flats' eigenvalues call for -- weighted per projection for the least total variation.  The weights are stored as `flat_weights`
((n, m)).  It takes the place of normalize, before the phase retrieval too, and needs --method mean.  Without it the calls and the
result are exactly what they were.

`--half-acquisition auto|C` is for half-acquisition (offset-axis) scans over 2 pi (generate_data --half-acquisition): after the stripe
removal the rotation axis is found on the finished sinogram, where it lies on the device (half_acquisition.find_center_360 on
--center-rows detector rows, the median), or taken to lie at the detector column C; the series is stitched to the pi series of double
width (half_acquisition.sino_360_to_180), and the file gets the stitched `projections`, the first half of `phi`, `alpha`, `beta` and
`xyz`, the axis on the unstitched detector as `half_axis`, and `cor_offset`: the x component of Geometry's cor_shift for the stitched
series, -(c_out - (W - 1) / 2), the number align_rigid's --cor takes.  The stitch pairs the projections i and i + n / 2, so it assumes
that they share a pose: it suits data whose jitter is below a pixel, or data aligned beforehand.  It excludes --find-center and
--prealign, which take pi series (run them on the stitched file).  Without it the calls and the result are exactly what they were.

The counts are uploaded once in their own dtype; the sinogram stays on the device from normalisation through stripe removal, which runs
on the full stack on one GPU (it needs every angle of a column).

    python -m tomography_alignment_amd.examples.generate_data --raw --out raw.npz
    python -m tomography_alignment_amd.examples.preprocess raw.npz --out data.npz
    python -m tomography_alignment_amd.examples.align_rigid data.npz --init fbp

    python -m tomography_alignment_amd.examples.generate_data --raw --propagate 25 --out fringed.npz
    python -m tomography_alignment_amd.examples.preprocess fringed.npz --phase-strength 25 --out data.npz
"""
import argparse

import numpy as np

from .. import _lib, half_acquisition as half_acq, preprocess, rotation_axis
from ..align import consistency

RAW_KEYS = ("counts", "flats", "darks", "mu", "dead_cols", "gain_cols", "zinger_mask")
STRIPE_MODES = ("sorting", "all", "none")
PREALIGN_MODES = ("moment", "profile")
LA_SIZE = 61              # the window of the dead- and large-stripe passes of --stripe all, where the detector is wide enough
PHASE_KEYS = ("strength", "pixel_size", "dist", "energy", "wavelength", "delta_beta", "pad", "min_ratio", "max_scratch_bytes")


def la_size_for(nx, la_size=None):
    """The window of the dead- and large-stripe passes: la_size if given, else 61 or the largest odd number the detector allows."""
    if la_size is not None:
        return int(la_size)
    return min(LA_SIZE, nx if nx % 2 else nx - 1)


def run(data, stripe_size=21, method="mean", cutoff=None, crop=None, ctx=None, verbose=False, phase=None, stripe="sorting", stripe_snr=3.0,
        la_size=None, zinger_dif=None, zinger_size=3, find_center=False, center_rows=9, prealign=None, dynamic_flat=None, half_acquisition=None):
    """The dict of `data` with `projections` ((n_proj, nx, nz) float32) in place of the raw keys.  stripe_size: the window of the stripe
    removal, or 0 / None to skip it.  phase: None, or a dict of preprocess.retrieve_phase's keywords (strength, or pixel_size, dist,
    energy / wavelength, delta_beta; pad, min_ratio, max_scratch_bytes): the phase retrieval before the -log.  stripe: 'sorting' (the
    sorting pass alone), 'all' (remove_all_stripe with snr stripe_snr, la_size -- default la_size_for(nx) -- and sm_size = stripe_size)
    or 'none'.  zinger_dif: None, or the threshold (counts) of preprocess.remove_outlier, window zinger_size, applied to the counts and to
    the flats before anything else.  find_center: True stores the rotation axis found on the finished sinogram as `cor_offset` (module
    docstring), searched on center_rows detector rows.  prealign: None, or 'moment' / 'profile': stores consistency.estimate_shifts'
    xyz0, axis_offset and mass_spread of the finished sinogram (module docstring).  dynamic_flat: None, or 'auto' / an integer >= 0:
    preprocess.normalize_dynamic with that many eigen flat fields ('auto': chosen from the flats' eigenvalues) in place of normalize;
    stores the weights as `flat_weights`.  half_acquisition: None, or 'auto' / the detector column of the rotation axis: the finished
    series over 2 pi is stitched to the pi series of double width about the axis found ('auto', on center_rows detector rows) or given;
    stores the stitched projections, the first half of phi, alpha, beta and xyz, `half_axis` and `cor_offset` (module docstring)."""
    if half_acquisition is not None:
        if half_acquisition != "auto":
            if isinstance(half_acquisition, (bool, np.bool_, str)) or not isinstance(half_acquisition, (int, float, np.integer, np.floating)) \
                    or not (np.isfinite(half_acquisition) and half_acquisition >= 0):
                raise ValueError("preprocess: half_acquisition must be None, 'auto' or the column of the axis, a number >= 0, got %r"
                                 % (half_acquisition,))
        if find_center or prealign is not None:
            raise ValueError("preprocess: half_acquisition excludes find_center and prealign, which take a series over pi: run them on "
                             "the stitched data")
        if "counts" in data:
            half_acq.angle_span(data.get("phi"), np.shape(data["counts"])[0])
    if dynamic_flat is not None:
        if dynamic_flat != "auto" and (isinstance(dynamic_flat, (bool, np.bool_)) or not isinstance(dynamic_flat, (int, np.integer))
                                       or dynamic_flat < 0):
            raise ValueError("preprocess: dynamic_flat must be None, 'auto' or an integer >= 0, got %r" % (dynamic_flat,))
        if method != "mean":
            raise ValueError("preprocess: dynamic_flat works on the mean flat: method must be 'mean', got %r" % (method,))
    if find_center and "phi" not in data:
        raise ValueError("preprocess: find_center needs the angles `phi`")
    if prealign is not None:
        if prealign not in PREALIGN_MODES:
            raise ValueError("preprocess: prealign must be None or one of %s, got %r" % (", ".join(PREALIGN_MODES), prealign))
        if "phi" not in data:
            raise ValueError("preprocess: prealign needs the angles `phi`")
        consistency.check_angles(np.shape(data["counts"])[0] if "counts" in data else np.size(data["phi"]), data["phi"])
    if stripe not in STRIPE_MODES:
        raise ValueError("preprocess: stripe must be one of %s, got %r" % (", ".join(STRIPE_MODES), stripe))
    if stripe == "all" and not stripe_size:
        raise ValueError("preprocess: stripe='all' needs a stripe_size (the window of its sorting pass)")
    if phase is not None:
        unknown = sorted(set(phase) - set(PHASE_KEYS))
        if unknown:
            raise ValueError("preprocess: phase has unknown keys %s (known: %s)" % (unknown, ", ".join(PHASE_KEYS)))
    for k in ("counts", "flats", "darks"):
        if k not in data:
            raise ValueError("preprocess: the data has no %r (write it with generate_data --raw)" % k)
    counts = np.asarray(data["counts"])
    own = ctx is None
    ctx = _lib.Context() if own else ctx
    p = preprocess.Preprocessor(ctx)
    d_frames = sino = None
    try:
        d_frames = ctx.to_device(counts, counts.dtype if counts.dtype in (np.uint16, np.float32) else np.float32)     # uploaded once
        flats = data["flats"]
        if zinger_dif is not None:
            p.remove_outlier(d_frames, zinger_dif, size=zinger_size, out=d_frames)                       # in place, on the device
            flats = np.asarray(flats)
            flats = p.remove_outlier(flats if flats.dtype in (np.uint16, np.float32) else flats.astype(np.float32), zinger_dif,
                                     size=zinger_size)
        flat_weights = None
        if dynamic_flat is not None:
            sino, flat_weights, _ = p.normalize_dynamic(d_frames, flats, data["darks"], n_eff=None if dynamic_flat == "auto" else int(dynamic_flat),
                                                        cutoff=cutoff, crop=crop, minus_log=phase is None, return_weights=True)
        elif phase is None:
            sino = p.normalize(d_frames, flats, data["darks"], cutoff=cutoff, method=method, crop=crop)
        else:
            sino = p.normalize(d_frames, flats, data["darks"], cutoff=cutoff, method=method, crop=crop, minus_log=False)
        d_frames.free()
        if phase is not None:
            p.retrieve_phase(sino, out=sino, **phase)                                                     # in place; applies the -log
        if stripe == "all":
            p.remove_all_stripe(sino, snr=stripe_snr, la_size=la_size_for(sino.shape[1], la_size), sm_size=stripe_size, out=sino)
        elif stripe == "sorting" and stripe_size:
            p.remove_stripe_sorting(sino, size=stripe_size, out=sino)                                    # in place, on the device
        cor = None
        if find_center:
            _, nx, nz = sino.shape
            smin, smax = rotation_axis.widest_range(nx)
            with rotation_axis.RotationAxis(ctx) as axis:
                found = axis.find_center(sino, angles=np.asarray(data["phi"], np.float64), rows=rotation_axis.spread_rows(nz, center_rows),
                                         smin=smin, smax=smax)
            cor = float(rotation_axis.to_cor_shift(found.offset, 1)[0, 0])
        est = None
        if prealign is not None:
            with consistency.Consistency(ctx) as c:
                est = c.estimate_shifts(sino, np.asarray(data["phi"], np.float64), vertical=prealign)
        half = None
        if half_acquisition is not None:
            phi = np.asarray(data["phi"], np.float64) if "phi" in data else None
            with half_acq.HalfAcquisition(ctx) as ha:
                if half_acquisition == "auto":
                    half_found = ha.find_center_360(sino, angles=phi, rows=rotation_axis.spread_rows(sino.shape[2], center_rows))
                    half_axis = half_found.center
                else:
                    half_found, half_axis = None, float(half_acquisition)
                half = ha.sino_360_to_180(sino, half_axis, angles=phi)
                stitched = half.projections
                ctx.sync()                                                                               # before the handle's table goes
            sino.free()
            sino = stitched
        proj = sino.download()
    finally:
        for d in (d_frames, sino):
            if d is not None:
                d.free()
        p.close()
        if own:
            ctx.close()
    if "mu" in data:
        proj = (proj / np.float32(data["mu"])).astype(np.float32)
    out = {k: v for k, v in data.items() if k not in RAW_KEYS}
    out["projections"] = proj
    if flat_weights is not None:
        out["flat_weights"] = flat_weights
    if cor is not None:
        out["cor_offset"] = np.float64(cor)
    if half is not None:
        nh = proj.shape[0]
        for k in ("phi", "alpha", "beta", "xyz"):
            if k in out:
                out[k] = np.asarray(out[k])[:nh]
        out.update(half_axis=np.float64(half_axis), cor_offset=np.float64(-half.cor_offset))
    if est is not None:
        out.update(xyz0=est.xyz0, axis_offset=np.float64(est.axis_offset), mass_spread=np.float64(est.mass_spread))
    if verbose:
        print("preprocess: %s counts -> projections %s (stripe removal %s, window %s, phase retrieval %s)"
              % (counts.shape, proj.shape, stripe, (stripe_size or "off") if stripe != "none" else "off",
                 phase if phase is not None else "off"))
        if flat_weights is not None:
            print("preprocess: dynamic flat field with %d eigen flat fields, largest |weight| %.2f"
                  % (flat_weights.shape[1], float(np.abs(flat_weights).max()) if flat_weights.size else 0.0))
        if cor is not None:
            print("preprocess: rotation axis at cor_offset %+.3f px (offsets per row %s)" % (cor, found.offsets.tolist()))
        if est is not None:
            print("preprocess: pre-alignment %r" % (est,))
        if half is not None:
            print("preprocess: half acquisition, axis at column %.3f (%s) -> %r" % (half_axis, half_found if half_found is not None else "given", half))
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="raw detector frames -> projections for align_rigid")
    ap.add_argument("data", help=".npz with counts, flats, darks (generate_data --raw)")
    ap.add_argument("--out", default="data.npz")
    ap.add_argument("--stripe-size", type=int, default=21, help="odd window of the stripe removal; 0 skips it")
    ap.add_argument("--stripe", choices=STRIPE_MODES, default="sorting",
                    help="sorting: the sorting pass alone; all: dead, large and sorting passes (remove_all_stripe); none: skip")
    ap.add_argument("--stripe-snr", type=float, default=3.0, help="with --stripe all: the detector's threshold")
    ap.add_argument("--stripe-la-size", type=int, default=None,
                    help="with --stripe all: odd window of the dead- and large-stripe passes (default 61, or what the detector allows)")
    ap.add_argument("--method", choices=("mean", "median"), default="mean", help="how flats and darks are reduced")
    ap.add_argument("--cutoff", type=float, default=None, help="upper bound of the flat-field ratio before the log")
    ap.add_argument("--crop", type=int, nargs=4, default=None, metavar=("Z0", "Z1", "X0", "X1"), help="detector window")
    ap.add_argument("--phase-strength", type=float, default=None, metavar="A",
                    help="Paganin phase retrieval with strength A = pi lambda z (delta/beta) / pixel_size^2 in pixels^2")
    ap.add_argument("--pixel-size", type=float, default=None, help="metres; with --dist and --energy, instead of --phase-strength")
    ap.add_argument("--dist", type=float, default=None, help="propagation distance, metres")
    ap.add_argument("--energy", type=float, default=None, help="keV")
    ap.add_argument("--delta-beta", type=float, default=None, help="delta / beta of the material (default 1000)")
    ap.add_argument("--zinger-dif", type=float, default=None, metavar="D",
                    help="remove zingers first: pixels of the counts and the flats D counts or more above their neighbourhood's median")
    ap.add_argument("--zinger-size", type=int, default=3, metavar="S", help="with --zinger-dif: the median window, 3, 5 or 7")
    ap.add_argument("--find-center", action="store_true", help="find the rotation axis on the finished sinogram and store it as cor_offset")
    ap.add_argument("--center-rows", type=int, default=9, metavar="K", help="with --find-center: the detector rows searched")
    ap.add_argument("--prealign", nargs="?", const="moment", default=None, choices=PREALIGN_MODES,
                    help="estimate the per-projection shifts from the sinogram's moments and store them as xyz0 (with axis_offset, mass_spread)")
    ap.add_argument("--dynamic-flat", nargs="?", const="auto", default=None, metavar="M",
                    help="a flat per projection from M eigen flat fields of the flats (no number: as many as their eigenvalues call for); "
                    "stores the weights as flat_weights")
    ap.add_argument("--half-acquisition", default=None, metavar="auto|C",
                    help="stitch a half-acquisition scan over 2 pi to the pi series of double width about the axis found (auto) or at the "
                    "detector column C; stores half_axis and cor_offset")
    a = ap.parse_args(argv)
    if a.half_acquisition is not None and a.half_acquisition != "auto":
        try:
            a.half_acquisition = float(a.half_acquisition)
        except ValueError:
            ap.error("--half-acquisition takes 'auto' or the detector column of the axis")
        if not 0 <= a.half_acquisition < float("inf"):
            ap.error("--half-acquisition must be a finite column >= 0")
    if a.half_acquisition is not None and (a.find_center or a.prealign is not None):
        ap.error("--half-acquisition excludes --find-center and --prealign: run them on the stitched file")
    if a.dynamic_flat is not None and a.dynamic_flat != "auto":
        try:
            a.dynamic_flat = int(a.dynamic_flat)
        except ValueError:
            ap.error("--dynamic-flat takes no value, 'auto' or an integer >= 0")
        if a.dynamic_flat < 0:
            ap.error("--dynamic-flat must be >= 0")
    if a.dynamic_flat is not None and a.method != "mean":
        ap.error("--dynamic-flat needs --method mean")
    if a.center_rows < 1:
        ap.error("--center-rows must be >= 1")
    if a.zinger_dif is not None and not a.zinger_dif >= 0:
        ap.error("--zinger-dif must be >= 0")
    if a.zinger_size not in (3, 5, 7):
        ap.error("--zinger-size must be 3, 5 or 7")
    physical = {k: getattr(a, k) for k in ("pixel_size", "dist", "energy", "delta_beta") if getattr(a, k) is not None}
    a.phase = None
    if a.phase_strength is not None:
        if physical:
            ap.error("give --phase-strength or --pixel-size / --dist / --energy / --delta-beta, not both")
        if not a.phase_strength >= 0:
            ap.error("--phase-strength must be >= 0")
        a.phase = dict(strength=a.phase_strength)
    elif physical:
        if not all(k in physical for k in ("pixel_size", "dist", "energy")):
            ap.error("the phase retrieval needs --pixel-size, --dist and --energy (or --phase-strength)")
        a.phase = physical
    if a.stripe_size and (a.stripe_size < 3 or a.stripe_size % 2 == 0):
        ap.error("--stripe-size must be 0 or an odd number >= 3")
    if not (a.stripe_snr > 0 and a.stripe_snr < float("inf")):
        ap.error("--stripe-snr must be finite and > 0")
    if a.stripe == "all" and not a.stripe_size:
        ap.error("--stripe all needs a --stripe-size (the window of its sorting pass)")
    if a.stripe_la_size is not None and (a.stripe_la_size < 3 or a.stripe_la_size % 2 == 0):
        ap.error("--stripe-la-size must be an odd number >= 3")
    if a.crop is not None:
        a.crop = ((a.crop[0], a.crop[1]), (a.crop[2], a.crop[3]))
    return a


def main(argv=None):
    a = parse_args(argv)
    d = run(dict(np.load(a.data)), stripe_size=a.stripe_size, method=a.method, cutoff=a.cutoff, crop=a.crop, verbose=True, phase=a.phase,
            stripe=a.stripe, stripe_snr=a.stripe_snr, la_size=a.stripe_la_size, zinger_dif=a.zinger_dif, zinger_size=a.zinger_size,
            find_center=a.find_center, center_rows=a.center_rows, prealign=a.prealign, dynamic_flat=a.dynamic_flat,
            half_acquisition=a.half_acquisition)
    np.savez(a.out, **d)
    print("wrote %s" % a.out)


if __name__ == "__main__":
    main()
