#!/usr/bin/env python3
"""
Synthetic misaligned tomography data set -- the job of the reference's examples/generate_data.py:6-29 (64^3
Shepp-Logan, 90 angles, alpha/beta jitter of +-1 deg in 0.01-deg steps, x/z jitter of +-2 px in 0.01-px steps), with
the projections computed by the GPU forward projector and, unlike the reference script, actually written to disk
(.npz with the key names of the HDF5 layout examples/align_rigid.py:11-17 reads: projections, alpha, beta, xyz, phi,
phantom).

With raw=True (--raw) the file also holds what a detector gives for the same projections, for examples/preprocess.py: `counts`
(uint16 [n_proj][z][x]), `flats` and `darks` (uint16 stacks of frames) and `mu`, the attenuation per unit of `projections` (the line
integral the counts encode is mu * projections).  counts = Poisson(I0 * gain * exp(-mu p)) + dark, with a per-pixel gain shared by flats
and projections, and a few detector columns whose gain in the projections differs from the flats' by a few percent: the stripes.
dead_columns=K (--dead-columns K) and gain_columns=K (--gain-columns K) add the defects the sorting-based removal leaves and
preprocess.remove_all_stripe handles: K columns stuck at a count of their own in every projection, and K columns whose gain in the
projections is 25 % above the flats'.  They are drawn from a generator of their own, so with both at 0 the frames are those of earlier
versions for the same seed.
zingers=K (--zingers K) adds K zingers to every count frame and to every flat frame: distinct pixels that a scattered photon drove
6 000 ... 30 000 counts above what they recorded (clipped to 65535), what preprocess.remove_outlier is for.  They too come from a
generator of their own, and `zinger_mask` (bool, shaped like counts) says where those of the counts are.
With propagate=A (--propagate A) the noiseless transmission exp(-mu p) is first carried over a propagation distance: the forward model
of preprocess.retrieve_phase with strength A (pixels^2), which puts a bright/dark fringe pair on every edge.
With cor_offset=D (--cor-offset D) the data are projected with Geometry(cor_shift=[D, 0, 0]): the rotation axis is off the detector's
centre column, as in every measured scan, and the file holds D as `cor_offset` -- what rotation_axis.find_center and align_rigid's
cor= are for.  With D = 0 every other key is that of earlier versions for the same seed.
shift_px=S (--shift-px S) and ang_deg=A (--tilt-deg A) set the half-width of the x/z jitter and of the alpha/beta jitter (defaults 2 px
and 1 degree, the reference's): stages of nano-tomography jitter by tens of pixels, what align.consistency and align_rigid's prealign=
are for.  With the defaults every key is that of earlier versions for the same seed.
beam_drift=A (--beam-drift A) lets the illumination move between the frames, what preprocess.normalize_dynamic is for: every flat and
every projection frame is multiplied by a beam profile 0.6 + 0.4 exp(-|r - c|^2 / (2 (0.6 nx)^2)) whose centre c lies uniform(-A, A) px
from the frame's centre in x and in z (beam_profiles).  The draws come from a generator of their own, and n_flat (--flats N) says how
many flats there are (default 10): with A = 0 every array is that of earlier versions for the same seed.
half_acquisition=OV (--half-acquisition OV) writes a half-acquisition (offset-axis) scan, what half_acquisition.find_center_360 and
sino_360_to_180 are for: an even number of projections over [0, 2 pi) without the endpoint, on a detector narrower than the volume whose
rotation axis lies near its right edge, so that the projections at phi and phi + pi overlap by OV columns (half_acquisition_detector:
nx = ceil((size + OV) / 2) columns, the axis at column c = nx - 1 - (OV - 1) / 2, i.e. Geometry(cor_shift=[(nx - 1) / 2 - c, 0, 0]); the
stitched series then has 2 nx - OV = size or size + 1 columns).  The file holds c as `half_center` and OV as `half_overlap`, and
`cor_offset` is the cor_shift used; these keys exist only with the option, and without it every key is that of earlier versions for the
same seed.  OV should be at least the search window (8 columns by default).

    python -m tomography_alignment_amd.examples.generate_data --size 64 --angles 90 --out data.npz
    python -m tomography_alignment_amd.examples.generate_data --size 64 --angles 90 --raw --out raw.npz
    python -m tomography_alignment_amd.examples.generate_data --size 64 --angles 90 --raw --propagate 25 --out fringed.npz
"""
import argparse

import numpy as np

from .. import preprocess
from ..utilities import generate_phantom, geometry, projection_operators


def tie_propagate(T, strength):
    """The intensity a propagation distance downstream of the transmission T [..., nx, nz], float64: the transport-of-intensity
    equation linearised for a homogeneous object, i.e. preprocess.retrieve_phase's padding (edge replication to the same lengths) with
    the spectrum DIVIDED by H = 1 / (1 + strength ((kx/Px)^2 + (kz/Pz)^2)).  tests/phase_model.propagate is the same model, which the
    package cannot import; tests/test_phase.py holds the two together."""
    T = np.asarray(T, np.float64)
    nx, nz = T.shape[-2:]
    (_, px), (_, pz) = preprocess.phase_padding(nx, strength), preprocess.phase_padding(nz, strength)
    ox, oz = (px - nx) // 2, (pz - nz) // 2
    P = np.pad(T, [(0, 0)] * (T.ndim - 2) + [(ox, px - nx - ox), (oz, pz - nz - oz)], mode="edge")
    k2 = np.fft.fftfreq(px)[:, None] ** 2 + np.fft.rfftfreq(pz)[None, :] ** 2
    r = np.fft.irfft2(np.fft.rfft2(P) * (1.0 + strength * k2), s=(px, pz))
    return r[..., ox:ox + nx, oz:oz + nz]


DEFECT_GAIN = 1.25        # the gain of a gain column in the projections, relative to the flats


def defect_columns(nx, dead_columns, gain_columns, seed=None):
    """(dead, gain): distinct column indices at least 4 columns from the detector's edges and 3 columns from each other."""
    k = int(dead_columns) + int(gain_columns)
    if dead_columns < 0 or gain_columns < 0 or 3 * k > nx - 8:
        raise ValueError("dead_columns + gain_columns must be >= 0 and fit 3 columns apart into %d - 8 columns, got %d + %d"
                         % (nx, dead_columns, gain_columns))
    rng = np.random.default_rng(None if seed is None else [int(seed), 0xdead])
    slots = rng.permutation((nx - 8) // 3)[:k] * 3 + 4
    return np.sort(slots[:int(dead_columns)]), np.sort(slots[int(dead_columns):])


ZINGER_COUNTS = (6000, 30000)      # what a zinger adds to its pixel, uniform


def add_zingers(frames, k, rng):
    """Add k zingers to every frame of the uint16 stack frames [n][z][x], in place: k distinct pixels per frame, each raised by a
    uniform ZINGER_COUNTS and clipped to 65535.  Returns the bool mask of the pixels hit."""
    n, nz, nx = frames.shape
    mask = np.zeros(frames.shape, bool)
    for i in range(n):
        pix = rng.choice(nz * nx, size=k, replace=False)
        extra = rng.integers(ZINGER_COUNTS[0], ZINGER_COUNTS[1], size=k, endpoint=True)
        flat = frames[i].reshape(-1)
        flat[pix] = np.minimum(flat[pix].astype(np.int64) + extra, 65535).astype(np.uint16)
        mask[i].reshape(-1)[pix] = True
    return mask


def beam_profiles(n, nz, nx, drift, rng):
    """n beam profiles [n][z][x], float64: 0.6 + 0.4 exp(-|r - c|^2 / (2 (0.6 nx)^2)), the centre c displaced from the frame's centre by
    uniform(-drift, drift) px in x and in z (x drawn first, for all n)."""
    cx = (nx - 1) / 2.0 + rng.uniform(-drift, drift, n)
    cz = (nz - 1) / 2.0 + rng.uniform(-drift, drift, n)
    z, x = np.arange(nz, dtype=np.float64)[None, :, None], np.arange(nx, dtype=np.float64)[None, None, :]
    r2 = (x - cx[:, None, None]) ** 2 + (z - cz[:, None, None]) ** 2
    return 0.6 + 0.4 * np.exp(-r2 / (2.0 * (0.6 * nx) ** 2))


def make_raw(proj, seed=None, i0=2e4, mu=None, n_flat=10, n_dark=5, dark_level=100.0, n_stripes=None, stripe_gain=0.03, propagate=None,
             dead_columns=0, gain_columns=0, zingers=0, beam_drift=0.0):
    """Detector frames of the projections proj [n_proj][nx][nz]: dict(counts, flats, darks, mu) (module docstring).  mu defaults to
    4 / nx, which keeps exp(-mu p) of a phantom of values <= 1 well above the noise floor.  propagate: the strength of the propagation
    applied to the noiseless transmission (None or 0: none, and the frames are those of earlier versions for the same seed).
    dead_columns, gain_columns: how many stuck and how many mis-gained columns to add (module docstring); with any, the dict also holds
    their indices as dead_cols and gain_cols.  zingers: how many zingers every count frame and every flat frame gets (module docstring);
    with any, the dict also holds zinger_mask, and with 0 every array is that of earlier versions for the same seed.  beam_drift: the
    half-width in pixels of the jitter of the beam's centre (module docstring); with 0 there is no beam profile and every array is that
    of earlier versions for the same seed."""
    beam_drift = float(beam_drift)
    if not (np.isfinite(beam_drift) and beam_drift >= 0):
        raise ValueError("beam_drift must be finite and >= 0, got %r" % (beam_drift,))
    zingers = int(zingers)
    if zingers < 0 or zingers > proj.shape[1] * proj.shape[2]:
        raise ValueError("zingers must be >= 0 and at most the pixels of a frame, got %d" % zingers)
    if propagate is not None and not (np.isfinite(propagate) and propagate >= 0):
        raise ValueError("propagate must be a finite strength >= 0 or None, got %r" % (propagate,))
    rng = np.random.default_rng(seed)
    n_proj, nx, nz = proj.shape
    mu = 4.0 / nx if mu is None else float(mu)
    gain = 1.0 + 0.02 * rng.standard_normal((nz, nx))                    # fixed pattern: flats and projections share it
    n_stripes = max(2, nx // 16) if n_stripes is None else int(n_stripes)
    cols = rng.choice(nx, size=min(n_stripes, nx), replace=False)
    drift = np.ones(nx)
    drift[cols] += stripe_gain * rng.choice([-1.0, 1.0], size=cols.size) * rng.uniform(0.5, 1.0, size=cols.size)
    dark_mean = dark_level + 2.0 * rng.standard_normal((nz, nx))

    def frames(mean):
        return np.clip(rng.poisson(mean) + np.rint(dark_mean), 0, 65535).astype(np.uint16)

    att = np.exp(-mu * np.asarray(proj, np.float64))
    if propagate:
        att = np.clip(tie_propagate(att, float(propagate)), 0.0, None)
    att = att.transpose(0, 2, 1)                                          # [n][z][x]
    dead, gained = defect_columns(nx, dead_columns, gain_columns, seed) if (dead_columns or gain_columns) else ((), ())
    if len(gained):
        drift = drift.copy()
        drift[gained] *= DEFECT_GAIN
    if beam_drift:
        brng = np.random.default_rng(None if seed is None else [int(seed), 0x22])
        beam_flats, beam_proj = beam_profiles(n_flat, nz, nx, beam_drift, brng), beam_profiles(n_proj, nz, nx, beam_drift, brng)
        counts = frames(i0 * gain * drift * att * beam_proj)
        flats = frames(i0 * gain * beam_flats)
    else:
        counts = frames(i0 * gain * drift * att)
        flats = frames(np.broadcast_to(i0 * gain, (n_flat, nz, nx)))
    darks = np.clip(rng.poisson(np.broadcast_to(np.maximum(dark_mean, 0), (n_dark, nz, nx))), 0, 65535).astype(np.uint16)
    out = dict(counts=counts, flats=flats, darks=darks, mu=np.float64(mu))
    if len(dead) or len(gained):
        for j, c in enumerate(dead):                                     # stuck: one count per column, between dark and half the flat
            counts[:, :, c] = np.uint16(round(dark_level + i0 * (0.2 + 0.3 * (j + 1) / (len(dead) + 1))))
        out.update(dead_cols=np.asarray(dead, np.int64), gain_cols=np.asarray(gained, np.int64))
    if zingers:
        zrng = np.random.default_rng(None if seed is None else [int(seed), 0x21])
        out["zinger_mask"] = add_zingers(counts, zingers, zrng)
        add_zingers(flats, zingers, zrng)
    return out


def half_acquisition_detector(size, overlap):
    """(nx, c, d) of a half-acquisition scan of a volume `size` wide whose halves overlap by `overlap` columns: the detector's columns,
    the column of the axis (centre convention (nx - 1) / 2, right of the centre) and the x component of Geometry's cor_shift that puts
    it there, (nx - 1) / 2 - c."""
    if isinstance(overlap, (bool, np.bool_)) or not isinstance(overlap, (int, np.integer)) or not 4 <= overlap < size:
        raise ValueError("half_acquisition must be an integer overlap in 4 ... size - 1 = %d columns, got %r" % (size - 1, overlap))
    nx = (int(size) + int(overlap) + 1) // 2
    c = nx - 1 - (int(overlap) - 1) / 2.0
    return nx, c, (nx - 1) / 2.0 - c


def make(size=64, n_proj=90, seed=None, ang_deg=1.0, shift_px=2.0, raw=False, propagate=None, dead_columns=0, gain_columns=0,
         zingers=0, cor_offset=0.0, beam_drift=0.0, n_flat=10, half_acquisition=None):
    cor_offset = float(cor_offset)
    if not np.isfinite(cor_offset):
        raise ValueError("cor_offset must be finite, got %r" % (cor_offset,))
    half = None
    if half_acquisition is not None:
        half = half_acquisition_detector(size, half_acquisition)
        if cor_offset:
            raise ValueError("half_acquisition chooses the axis itself: cor_offset must be 0, got %r" % (cor_offset,))
        if n_proj < 2 or n_proj % 2:
            raise ValueError("half_acquisition needs an even number of projections over 2 pi, got %d" % n_proj)
        cor_offset = half[2]
    rng = np.random.RandomState(seed)
    nx = ny = nz = size
    ndx = nx if half is None else half[0]                               # detector columns
    shepp = generate_phantom.shepp3d(nx)
    geom = geometry.Geometry(n_proj, np.array([nx, ny, nz]), np.ones(3), np.array([ndx, nz]), np.ones(2),
                             cor_shift=np.array([cor_offset, 0.0, 0.0]) if cor_offset else None)
    phi = np.linspace(0.0, np.pi, n_proj) if half is None else np.linspace(0.0, 2.0 * np.pi, n_proj, endpoint=False)
    a100, s100 = int(round(100 * ang_deg)), int(round(100 * shift_px))
    jitter = lambda m: rng.randint(-m, m, n_proj) / 100 if m > 0 else np.zeros(n_proj)      # noqa: E731 (m = 0: nominal poses)
    alpha = np.deg2rad(jitter(a100))                                    # examples/generate_data.py:17-18
    beta = np.deg2rad(jitter(a100))
    xyz = np.zeros((n_proj, 3))
    xyz[:, 0] = jitter(s100)                                            # :22-23 (motion along the beam is invisible)
    xyz[:, 2] = jitter(s100)
    proj_obj = projection_operators.ProjectionMatrix(geom, precision=np.float32)
    pmat = proj_obj.projection_matrix(alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)
    proj = pmat.dot(shepp.ravel()).reshape(n_proj, ndx, nz)             # :29
    d = dict(projections=proj, alpha=alpha, beta=beta, xyz=xyz, phi=phi, phantom=shepp, cor_offset=np.float64(cor_offset))
    if half is not None:
        d.update(half_center=np.float64(half[1]), half_overlap=np.int64(half_acquisition))
    if raw:
        d.update(make_raw(proj, seed=None if seed is None else seed + 1, propagate=propagate, dead_columns=dead_columns,
                          gain_columns=gain_columns, zingers=zingers, beam_drift=beam_drift, n_flat=n_flat))
        # a generator of its own: the other keys do not change
    return d


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--angles", type=int, default=90)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="data.npz")
    ap.add_argument("--raw", action="store_true", help="also write detector counts, flats and darks (examples/preprocess.py)")
    ap.add_argument("--propagate", type=float, default=None, metavar="A",
                    help="with --raw: propagate the transmission with strength A pixels^2 before the counts are drawn (phase-contrast fringes)")
    ap.add_argument("--dead-columns", type=int, default=0, metavar="K", help="with --raw: K detector columns stuck at a count")
    ap.add_argument("--gain-columns", type=int, default=0, metavar="K",
                    help="with --raw: K columns whose gain in the projections is 25 %% above the flats'")
    ap.add_argument("--cor-offset", type=float, default=0.0, metavar="D", help="project with the rotation axis off centre: "
                    "Geometry(cor_shift=[D, 0, 0])")
    ap.add_argument("--zingers", type=int, default=0, metavar="K", help="with --raw: K zingers in every count frame and every flat frame")
    ap.add_argument("--shift-px", type=float, default=2.0, metavar="S", help="half-width of the x and z jitter in pixels (default 2)")
    ap.add_argument("--tilt-deg", type=float, default=1.0, metavar="A", help="half-width of the alpha and beta jitter in degrees (default 1)")
    ap.add_argument("--beam-drift", type=float, default=0.0, metavar="A",
                    help="with --raw: the beam's centre jitters by +-A px between the frames (preprocess.normalize_dynamic)")
    ap.add_argument("--flats", type=int, default=10, metavar="N", help="with --raw: how many flat frames (default 10)")
    ap.add_argument("--half-acquisition", type=int, default=None, metavar="OV", help="a half-acquisition scan over 2 pi on a detector of "
                    "ceil((size + OV) / 2) columns whose halves overlap by OV columns (an even --angles)")
    a = ap.parse_args(argv)
    if a.half_acquisition is not None:
        if not 4 <= a.half_acquisition < a.size:
            ap.error("--half-acquisition must be an overlap of 4 ... size - 1 columns")
        if a.cor_offset:
            ap.error("--half-acquisition chooses the axis itself: leave --cor-offset out")
        if a.angles < 2 or a.angles % 2:
            ap.error("--half-acquisition needs an even number of --angles")
    if not (0 <= a.beam_drift < float("inf")):
        ap.error("--beam-drift must be finite and >= 0")
    if a.beam_drift and not a.raw:
        ap.error("--beam-drift needs --raw")
    if a.flats < 1:
        ap.error("--flats must be >= 1")
    if not (0 <= a.shift_px < float("inf")) or not (0 <= a.tilt_deg < float("inf")):
        ap.error("--shift-px and --tilt-deg must be finite and >= 0")
    if a.zingers < 0:
        ap.error("--zingers must be >= 0")
    if a.zingers and not a.raw:
        ap.error("--zingers needs --raw")
    if a.propagate is not None and not a.raw:
        ap.error("--propagate needs --raw")
    if (a.dead_columns or a.gain_columns) and not a.raw:
        ap.error("--dead-columns and --gain-columns need --raw")
    return a


def main(argv=None):
    a = parse_args(argv)
    d = make(a.size, a.angles, a.seed, ang_deg=a.tilt_deg, shift_px=a.shift_px, raw=a.raw, propagate=a.propagate, dead_columns=a.dead_columns, gain_columns=a.gain_columns,
             zingers=a.zingers, cor_offset=a.cor_offset, beam_drift=a.beam_drift, n_flat=a.flats, half_acquisition=a.half_acquisition)
    np.savez(a.out, **d)
    print("wrote %s: projections %s, phantom %s" % (a.out, d["projections"].shape, d["phantom"].shape))


if __name__ == "__main__":
    main()
