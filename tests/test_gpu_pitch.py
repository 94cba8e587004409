"""The projectors at detector and voxel pitches other than one.  The host code picks its kernels from the pitch (stage_tile_consts and
forward_tiles in csrc/tomo_project.hip, tomo_check_geometry in csrc/tomo_ctx.hip); every row of ROWS below is one way through those
predicates, and every case shows by the profile counters (the names of TOMO_LAUNCH) that the kernel it is meant for ran:

    detector pitch (x, z), step                     forward                      adjoint
    (1.25, 1), (2, 1); step 1.0 and 0.95            gather forward               gather adjoint; adjoint_update fuses
    (1.25, 1); step 0.5                             k_fwd_flat_tab               gather adjoint
    (0.8, 1); angles on both sides of ea = 1.45     k_fwd_flat_tab               gather adjoint and k_adj_tile_flat in one call
    (0.5, 1)                                        k_fwd_flat_tab               k_adj_tile_flat
    (1, 0.5), (0.5, 0.5) step 1 and 0.5,
    (1.3, 1.25), (1, 2)                             k_fwd_tile                   k_adj_tile
    ... with fwd_variant / adj_variant 1 and 2      k_fwd_v1 / k_fwd_v2          k_adj_v1 / k_adj_tile
    voxel pitch (2, 2, 2) with detector (2, 2)      k_fwd_tile                   k_adj_tile
    voxel pitch (1.5, 1, 0.75) with detector (1, 1) gather forward               gather adjoint

(ea = (|cos phi| + |sin phi|) / det_dx: the number of detector rows per voxel across the beam.)  Both flat forwards carry the profile
name k_fwd_tile_flat; the gather one is told from k_fwd_flat_tab as tests/test_gpu_gather_bits.py does it: its bits differ from those
with option "fwd_flat_gather" off.  Where k_fwd_flat_tab is expected the same is shown the other way round, on a volume whose few
voxels lie in one tile (one work-group per ray: nothing for float atomics to reorder): the option changes no bit.

Bars: max|a - b| / max|b| < 1e-5 against the CPU oracle and against golden G16 (the reference itself at these pitches) for forward and
adjoint, 1e-6 for <A x, y> = <x, A^T y>; gradients as tests/test_gpu_fuzz.py (value 1e-5 on all rays, gradient 1e-5 on the rays that keep
2e-5 voxel from a cell face, fused sums 2e-6 against the kernel's own rays); the voxel-driven kernels as A6 / A9 of
tests/test_gpu_parity.py.  Every case asserts that at least a quarter of its rays have a non-zero oracle sum; the measured errors are
printed."""
import numpy as np
import pytest

from conftest import golden, rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5

SHAPES = [(24, 24, 64), (17, 23, 65), (40, 9, 130)]           # the shapes of tests/test_gpu_forward_gather.py: one z chunk, one + a plane, three
SPECIAL = [0.0, np.pi / 2, np.pi,                             # samples on integers
           np.arctan(0.5) - 1e-3, np.arctan(0.5) + 1e-3,      # the 3 / 4-weight switch
           np.pi / 4 - 1e-3, np.pi / 4 + 1e-3,                # the walk switch, inside one group of eight
           3 * np.pi / 4 - 1e-3, 3 * np.pi / 4 + 1e-3]
# detector-x pitch 0.8: (|cos| + |sin|) / 0.8 < 1.45 within 10.1 degrees of an axis.  Both sides of that, about every axis direction
EA_08 = list(np.deg2rad([4.0, 9.0, 11.5, 30.0, 79.0, 81.5, 94.0, 99.5, 101.0, 150.0, 169.0, 171.5]))

FLAT, GATHER, TILE = "k_adj_tile_flat", "k_adj_gather_flat", "k_adj_tile"
# name -> (detector pitch, voxel pitch, step, forward path, adjoint kernels of the untilted poses, angle kind)
ROWS = {
    "dx125_s100": ((1.25, 1.0), (1, 1, 1), 1.0, "gather", (GATHER,), "special"),
    "dx125_s095": ((1.25, 1.0), (1, 1, 1), 0.95, "gather", (GATHER,), "special"),
    "dx200_s100": ((2.0, 1.0), (1, 1, 1), 1.0, "gather", (GATHER,), "special"),
    "dx200_s095": ((2.0, 1.0), (1, 1, 1), 0.95, "gather", (GATHER,), "special"),
    "dx125_s050": ((1.25, 1.0), (1, 1, 1), 0.5, "flat", (GATHER,), "special"),
    "dx080":      ((0.8, 1.0), (1, 1, 1), 1.0, "flat", (GATHER, FLAT), "ea08"),
    "dx050":      ((0.5, 1.0), (1, 1, 1), 1.0, "flat", (FLAT,), "special"),
    "dz050":      ((1.0, 0.5), (1, 1, 1), 1.0, "tile", (TILE,), "special"),
    "d050_s100":  ((0.5, 0.5), (1, 1, 1), 1.0, "tile", (TILE,), "special"),
    "d050_s050":  ((0.5, 0.5), (1, 1, 1), 0.5, "tile", (TILE,), "special"),        # weight_bound = 2 / (0.5 * 0.5 * 0.5) = 16
    "d130_125":   ((1.3, 1.25), (1, 1, 1), 1.0, "tile", (TILE,), "special"),
    "dz200":      ((1.0, 2.0), (1, 1, 1), 1.0, "tile", (TILE,), "special"),
    "vox2":       ((2.0, 2.0), (2, 2, 2), 1.0, "tile", (TILE,), "special"),
    "vox_anis":   ((1.0, 1.0), (1.5, 1.0, 0.75), 1.0, "gather", (GATHER,), "special"),
}
GENERAL_ROWS = ["dz050", "d050_s050", "d130_125", "dz200"]
POSE_KINDS = ["plain", "shift", "cor"]


def det_shape(shape, det_pix, vox_pix):
    """Detector shape x pitch near the volume's footprint."""
    return (max(int(round(shape[0] * vox_pix[0] / det_pix[0])), 2), max(int(round(shape[2] * vox_pix[2] / det_pix[1])), 2))


def geo_pair(n_proj, shape, row, cor_shift=None, step=None):
    from tomography_alignment_amd.utilities.geometry import Geometry
    from oracle import oracle as orc
    det_pix, vox_pix, row_step = ROWS[row][:3]
    args = (n_proj, np.array(shape), np.array(vox_pix, np.float64), np.array(det_shape(shape, det_pix, vox_pix)), np.array(det_pix))
    kw = dict(cor_shift=cor_shift, step_size=row_step if step is None else step)
    return Geometry(*args, **kw), orc.Geo(*args, **kw)


def angles(n, kind, rng):
    a = list(EA_08 if kind == "ea08" else SPECIAL)[:n] if kind != "random" else []
    return np.array(a + list(rng.uniform(0.0, np.pi, n - len(a))))


def pose_kw(n, kind, rng, nz):
    """The pose kinds of tests/test_gpu_forward_gather.py; z translations scaled to the volume's height (+-21 at nz = 64)."""
    xyz = np.zeros((n, 3))
    cor = None
    if kind == "shift":                     # fractional x / z translations
        xyz[:, 0] = rng.uniform(-3.0, 3.0, n)
        xyz[:, 2] = rng.uniform(-21.0, 21.0, n) * min(1.0, nz / 64.0)
    elif kind == "cor":
        cor = np.array([1.37, 0.0, 0.0])
        xyz[:, 2] = np.round(rng.uniform(-9.0, 9.0, n))       # integer z offsets
    return xyz, cor


def case_inputs(row, shape, pkind, n=None, tilt_deg=0.0, seed=0):
    """-> (geo, og, kw of the poses, poses array arguments, x, y, oracle forward, oracle adjoint): all from one seeded generator."""
    rng = np.random.default_rng([seed, sorted(ROWS).index(row), SHAPES.index(shape) if shape in SHAPES else 9, POSE_KINDS.index(pkind)])
    akind = ROWS[row][5]
    n = (17 if akind == "ea08" else 13) if n is None else n
    phi = angles(n, akind, rng)
    xyz, cor = pose_kw(n, pkind, rng, shape[2])
    alpha, beta = np.zeros(n), np.zeros(n)
    if tilt_deg:                             # the second half of the poses tilted: flat and general kernels in one call
        h = n // 2
        alpha[h:], beta[h:] = np.deg2rad(rng.uniform(-tilt_deg, tilt_deg, n - h)), np.deg2rad(rng.uniform(-tilt_deg, tilt_deg, n - h))
    geo, og = geo_pair(n, shape, row, cor_shift=cor)
    kw = dict(alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)
    x = rng.uniform(0.1, 1.0, shape).astype(np.float32)
    y = rng.standard_normal(n * og.n_det).astype(np.float32)
    return geo, og, kw, (phi, alpha, beta, xyz, np.zeros(3) if cor is None else cor), x, y


def oracle_pair(og, kw, x, y):
    from oracle import oracle as orc
    ref_f, ref_a = orc.forward(og, x, **kw).ravel(), orc.adjoint(og, y, **kw)
    live = float(np.mean(ref_f != 0))
    return ref_f, ref_a, live


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def counts(ctx, *names):
    return tuple(ctx.profile_get(k)[0] for k in names)


FWD_NAMES = ("k_fwd_tile_flat", "k_fwd_tile", "k_fwd_v1", "k_fwd_v2")
ADJ_NAMES = (GATHER, FLAT, TILE, "k_adj_v1")


def profiled(ctx, fn):
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        return fn()
    finally:
        ctx.profile_enable(False)


def one_tile_volume(shape, rng):
    """A few voxels, all inside one tile and one z block, values with short mantissas: a ray gets its sum from a single work-group of the
    default flat forward (tests/test_gpu_forward_gather.py::test_declined_calls_keep_the_default_bits)."""
    x = np.zeros(shape, np.float32)
    x[5:9, 2:7, 20:33] = rng.uniform(0.1, 1.0, (4, 5, 13))
    return np.round(x * 64) / 64


def run_forward(be, poses, x, gather=1):
    be.ctx.set_option("fwd_flat_gather", gather)
    try:
        return be.forward(poses, be.upload(x), be.zeros(poses.shape[0] * be.n_det)).download()
    finally:
        be.ctx.set_option("fwd_flat_gather", 1)


def check_forward_path(be, poses, x, fwd, shape, got_counts, has_tilted=False):
    """The counters of the forward call that just ran (got_counts, in the order of FWD_NAMES) and, for the two flat forwards, which one it was."""
    want = {"gather": (1, 0, 0, 0), "flat": (1, 0, 0, 0), "tile": (0, 1, 0, 0)}[fwd]
    if has_tilted:
        want = (want[0], 1, 0, 0)
    assert got_counts == want, (fwd, dict(zip(FWD_NAMES, got_counts)))
    if fwd == "gather" and not has_tilted:
        on, off = run_forward(be, poses, x, 1), run_forward(be, poses, x, 0)
        assert np.any(bits(on) != bits(off)), "option fwd_flat_gather changes no bit: the gather forward did not run"
        return rel_max(on, off)
    if fwd == "flat":
        xs = one_tile_volume(shape, np.random.default_rng(3))
        on, off = run_forward(be, poses, xs, 1), run_forward(be, poses, xs, 0)
        assert np.any(on != 0) and np.array_equal(bits(on), bits(off)), "option fwd_flat_gather changes bits: the call was not left to k_fwd_flat_tab"
    return None


def adj_counts_want(adj, has_tilted=False):
    return (int(GATHER in adj), int(FLAT in adj), int(TILE in adj or has_tilted), 0)


def case_list():
    out = []
    for r, row in enumerate(sorted(ROWS)):
        for s, shape in enumerate(SHAPES):
            if row == "vox2" and s == 2:
                # voxel pitch 2 puts the rotation axis at the index grid's upper corner: of a volume only 9 voxels deep too few rays
                # (18 %, counted on the oracle) cross it for the quarter asked below; the same x and z extent on a square base
                shape = (40, 40, 130)
            out.append((row, shape, POSE_KINDS[(r + s) % 3]))
    return out


@pytest.mark.parametrize("row,shape,pkind", case_list())
def test_forward_adjoint_paths_vs_oracle(row, shape, pkind):
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    fwd, adj = ROWS[row][3], ROWS[row][4]
    geo, og, kw, pa, x, y = case_inputs(row, shape, pkind)
    ref_f, ref_a, live = oracle_pair(og, kw, x, y)
    assert live >= 0.25, "only %.0f %% of the rays cross the volume" % (100 * live)
    be = HipBackend(geo)
    ctx = be.ctx
    poses = _lib.poses_array(*pa)
    got_f = profiled(ctx, lambda: be.forward(poses, be.upload(x), be.zeros(y.size)).download())
    e_gather = check_forward_path(be, poses, x, fwd, shape, counts(ctx, *FWD_NAMES))
    d_y = be.upload(y)
    got_a = profiled(ctx, lambda: be.adjoint(poses, d_y, be.zeros(x.size)).download())
    assert counts(ctx, *ADJ_NAMES) == adj_counts_want(adj), dict(zip(ADJ_NAMES, counts(ctx, *ADJ_NAMES)))
    e_f, e_a = rel_max(got_f, ref_f), rel_max(got_a, ref_a)
    # adjoint_update: one pass of the gather adjoint when every pose takes it, else nothing is launched and nothing changes
    rng = np.random.default_rng(1)
    rec0, V, gt = (rng.standard_normal(x.size).astype(np.float32), rng.uniform(0.1, 1.0, x.size).astype(np.float32),
                   rng.standard_normal(x.size).astype(np.float32))
    rec, d_V, d_gt = be.upload(rec0), be.upload(V), be.upload(gt)
    fused, err = profiled(ctx, lambda: be.adjoint_update(poses, d_y, rec, d_V, True, d_gt))
    assert fused == (adj == (GATHER,))
    if fused:
        assert counts(ctx, GATHER, "k_update") == (1, 0)
        rec2, bp = be.upload(rec0), be.empty(x.size)
        be.adjoint(poses, d_y, bp)
        err2 = be.update(rec2, bp, d_V, True, d_gt)
        assert np.array_equal(bits(rec.download()), bits(rec2.download())) and abs(err - err2) <= 1e-12 * abs(err2)
    else:
        assert counts(ctx, *ADJ_NAMES) == (0, 0, 0, 0) and err is None and np.array_equal(bits(rec.download()), bits(rec0))
    print("[%s %s %s] %d poses, %.0f %% of the rays live: forward (%s) %.2e, adjoint (%s) %.2e vs oracle%s; adjoint_update %s"
          % (row, shape, pkind, poses.shape[0], 100 * live, fwd, e_f, " + ".join(adj), e_a,
             "" if e_gather is None else "; gather vs default forward %.2e" % e_gather, "fused" if fused else "declined"))
    assert e_f < TOL and e_a < TOL


@pytest.mark.parametrize("row", GENERAL_ROWS)
@pytest.mark.parametrize("variant", [1, 2])
def test_ray_driven_variants_vs_oracle(row, variant):
    """fwd_variant / adj_variant 1 and 2 at the pitches of the general tile kernels.  A detector-z pitch above 1 sets TOMO_GEOM_WIDE_ROWS:
    fwd_variant 2 must then run k_fwd_v1 (k_fwd_v2's 24-bit offset multiplies assume rows one voxel apart)."""
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    shape = SHAPES[(GENERAL_ROWS.index(row) + variant) % 3]
    geo, og, kw, pa, x, y = case_inputs(row, shape, POSE_KINDS[variant], n=9, tilt_deg=2.0, seed=variant)
    ref_f, ref_a, live = oracle_pair(og, kw, x, y)
    assert live >= 0.25
    be = HipBackend(geo)
    ctx = be.ctx
    ctx.set_option("fwd_variant", variant)
    ctx.set_option("adj_variant", variant)
    poses = _lib.poses_array(*pa)
    got_f = profiled(ctx, lambda: be.forward(poses, be.upload(x), be.zeros(y.size)).download())
    wide = ROWS[row][0][1] > 1.0
    assert counts(ctx, *FWD_NAMES) == ((0, 0, 1, 0) if variant == 1 or wide else (0, 0, 0, 1)), dict(zip(FWD_NAMES, counts(ctx, *FWD_NAMES)))
    got_a = profiled(ctx, lambda: be.adjoint(poses, be.upload(y), be.zeros(x.size)).download())
    assert counts(ctx, *ADJ_NAMES) == ((0, 0, 0, 1) if variant == 1 else (0, 0, 1, 0)), dict(zip(ADJ_NAMES, counts(ctx, *ADJ_NAMES)))
    e_f, e_a = rel_max(got_f, ref_f), rel_max(got_a, ref_a)
    print("[%s %s variant %d] forward %.2e adjoint %.2e vs oracle (%.0f %% of the rays live)" % (row, shape, variant, e_f, e_a, 100 * live))
    assert e_f < TOL and e_a < TOL


@pytest.mark.parametrize("row", sorted(ROWS))
def test_tilted_poses_on_every_row(row):
    """Half of the poses tilted by up to +-2 degrees: they take the general tile kernels, the untilted half keeps the row's own."""
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    shape = SHAPES[sorted(ROWS).index(row) % 3]
    fwd, adj = ROWS[row][3], ROWS[row][4]
    geo, og, kw, pa, x, y = case_inputs(row, shape, "shift", tilt_deg=2.0, seed=2)
    ref_f, ref_a, live = oracle_pair(og, kw, x, y)
    assert live >= 0.25
    be = HipBackend(geo)
    ctx = be.ctx
    poses = _lib.poses_array(*pa)
    got_f = profiled(ctx, lambda: be.forward(poses, be.upload(x), be.zeros(y.size)).download())
    check_forward_path(be, poses, x, "tile" if fwd == "tile" else "flat", shape, counts(ctx, *FWD_NAMES), has_tilted=True)
    got_a = profiled(ctx, lambda: be.adjoint(poses, be.upload(y), be.zeros(x.size)).download())
    assert counts(ctx, *ADJ_NAMES) == adj_counts_want(adj, True), dict(zip(ADJ_NAMES, counts(ctx, *ADJ_NAMES)))
    e_f, e_a = rel_max(got_f, ref_f), rel_max(got_a, ref_a)
    lhs, rhs = float(np.dot(got_f.astype(np.float64), y.astype(np.float64))), float(np.dot(x.ravel().astype(np.float64), got_a.astype(np.float64)))
    print("[%s %s half tilted] forward %.2e adjoint %.2e vs oracle (%.0f %% of the rays live)" % (row, shape, e_f, e_a, 100 * live))
    assert e_f < TOL and e_a < TOL
    size = float(np.dot(np.abs(got_f).astype(np.float64), np.abs(y).astype(np.float64)))      # y has both signs: compare to the terms
    assert abs(lhs - rhs) <= 1e-5 * size


@pytest.mark.parametrize("row", ["dx125_s100", "dx200_s095", "dx125_s050", "dx080", "dx050", "d050_s050", "dz200", "vox_anis"])
def test_adjointness(row):
    """<A x, y> = <x, A^T y> to 1e-6 with positive x and y, as test_adjointness_with_gather_adjoint."""
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    shape = SHAPES[2]
    geo, og, kw, pa, x, _ = case_inputs(row, shape, "shift", seed=4)
    y = np.random.default_rng(11).uniform(0.1, 1.0, kw["phi"].size * og.n_det).astype(np.float32)
    be = HipBackend(geo)
    poses = _lib.poses_array(*pa)
    Ax = be.forward(poses, be.upload(x), be.zeros(y.size)).download()
    ATy = be.adjoint(poses, be.upload(y), be.zeros(x.size)).download()
    lhs, rhs = float(np.dot(Ax.astype(np.float64), y.astype(np.float64))), float(np.dot(x.ravel().astype(np.float64), ATy.astype(np.float64)))
    print("[%s] adjointness: <Ax, y> = %.10e, <x, A^T y> = %.10e, rel %.2e" % (row, lhs, rhs, abs(lhs - rhs) / abs(lhs)))
    assert lhs > 0 and abs(lhs - rhs) / abs(lhs) < 1e-6


@pytest.mark.parametrize("row", ["dx125_s100", "dx200_s100"])
@pytest.mark.parametrize("shape", SHAPES)
def test_gather_forward_zero_bands_and_determinism(row, shape):
    """As test_zero_bands_exact_zeros_and_determinism: two calls of the gather forward give the same bits; rays through zero planes only
    hold exact zeros, as with the default flat forward; a zero volume gives zeros."""
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    geo, og, kw, pa, x, _ = case_inputs(row, shape, "shift", n=9, seed=7)
    nz = shape[2]
    x[:, :, :20] = 0
    x[:, :, nz - nz // 3:] = 0
    be = HipBackend(geo)
    poses = _lib.poses_array(*pa)
    on, again, off = run_forward(be, poses, x, 1), run_forward(be, poses, x, 1), run_forward(be, poses, x, 0)
    assert np.array_equal(bits(on), bits(again)), "two calls of the gather forward differ"
    assert np.any(bits(on) != bits(off))
    e = rel_max(on, off)
    print("[%s %s] zero bands: gather vs default %.2e; rays that are zero: default %d, gather %d of %d" % (row, shape, e, int((off == 0).sum()), int((on == 0).sum()), on.size))
    assert e < TOL and np.array_equal(on == 0, off == 0) and 0 < int((on == 0).sum()) < on.size
    assert not run_forward(be, poses, np.zeros(shape, np.float32), 1).any()


FGROWS = 24          # lines of one window of k_fwd_gather_flat (kernels_tile_gather.hip.h)


def first_line_spans(og, phis, step):
    """Per (tile of eight detector rows, x slab S): the spread of the first volume line (y index) touched by the samples with |p_x - S| < 1,
    over the eight rows and the poses `phis` -- what one wave of the gather forward has to cover in that step.  From the oracle's own ray
    set-up, no kernel arithmetic."""
    from oracle import oracle as orc
    ndx, ndz = (int(v) for v in og.det_shape)
    nS = int(og.vox_shape[0])
    big = 1 << 29
    L0 = np.full((len(phis), ndx, nS), big, np.int64)
    for k, phi in enumerate(phis):
        p0, rhat, n, _, _, _ = orc.ray_setup(og, 0.0, 0.0, phi, np.zeros(3), og.cor_shift[0])
        rows, d = p0[:, ::ndz], rhat[:, 0] * step
        j = np.arange(n)
        px, py = rows[0][:, None] + j * d[0], rows[1][:, None] + j * d[1]
        for S in range(nS):
            m = np.abs(px - S) < 1.0
            lo = np.floor(np.where(m, py, np.inf).min(axis=1, initial=np.inf))
            ok = m.any(axis=1) & (lo >= -1) & (lo < og.vox_shape[1])
            L0[k, :, S] = np.where(ok, lo, big)
    L0 = L0.reshape(len(phis), ndx // 8, 8, nS)
    val = L0 < big
    span = np.where(val, L0, -big).max(axis=(0, 2)) - np.where(val, L0, big).min(axis=(0, 2))
    return np.where(val.any(axis=(0, 2)), span, 0)


def test_gather_forward_needs_further_windows_at_pitch_2():
    """The eight poses of "win2" in tests/test_gpu_gather_bits.py (one group of the x-walk, three-weight list, 64 .. 116 degrees) on its
    80 x 80 x 64 volume at detector pitch (2, 1): eight rows of a wave now lie 2 sin(phi) lines apart instead of sin(phi), so a wave's
    lanes spread over more lines at every slab: the kernel's rule for a further window (spread >= FGROWS - 3 + 1) holds for 7 of 10
    wave-steps where it held for half at pitch 1, and one step in six takes a third window."""
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    from oracle import oracle as orc
    shape, n = (80, 80, 64), 8
    phi = np.deg2rad(np.linspace(64.0, 116.0, n))
    s, c = np.abs(np.sin(phi)), np.abs(np.cos(phi))
    assert np.all(s >= c) and np.all(2 * c <= s)                    # all eight in the x-walk, NW = 3 list: one group of eight
    geo, og = geo_pair(n, shape, "dx200_s100")
    span = first_line_spans(og, phi, 1.0)
    sw = FGROWS - 3 + 1
    n_two, n_three = int((span >= sw).sum()), int((span >= 2 * sw).sum())
    assert n_two > span.size // 2 and n_three >= 8 and span.max() >= 2 * sw + 8      # (counted: 284 and 66 of 400 steps, widest 54)
    rng = np.random.default_rng(2)
    x = rng.uniform(0.1, 1.0, shape).astype(np.float32)
    kw = dict(alpha=np.zeros(n), beta=np.zeros(n), phi=phi, xyz_shift=np.zeros((n, 3)))
    ref = orc.forward(og, x, **kw).ravel()
    be = HipBackend(geo)
    poses = _lib.poses_array(phi, np.zeros(n), np.zeros(n), np.zeros((n, 3)), np.zeros(3))
    got = profiled(be.ctx, lambda: be.forward(poses, be.upload(x), be.zeros(ref.size)).download())
    e_off = check_forward_path(be, poses, x, "gather", shape, counts(be.ctx, *FWD_NAMES))
    e = rel_max(got, ref)
    print("win2 at detector pitch (2, 1): %d of %d wave-steps need a second window, %d a third (widest first-line spread %d); gather forward vs oracle %.2e, vs default %.2e"
          % (n_two, span.size, n_three, int(span.max()), e, e_off))
    assert np.mean(ref != 0) >= 0.25 and e < TOL and e_off < TOL


@pytest.mark.parametrize("row", ["dx080", "d050_s050", "dx125_s100"])
def test_adjoint_xslabs_add_up_to_the_whole(row):
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    shape = SHAPES[2]                                   # 40 voxels in x: three tile columns
    geo, og, kw, pa, x, y = case_inputs(row, shape, "cor", seed=5)
    be = HipBackend(geo)
    poses = _lib.poses_array(*pa)
    d_y = be.upload(y)
    whole = be.adjoint(poses, d_y, be.zeros(x.size)).download()
    n_xt, _ = be.xslab_info()
    assert n_xt >= 3
    d_v = be.zeros(x.size)
    for i in range(n_xt):
        be.adjoint_xslab(poses, d_y, d_v, i, i + 1, same_sinogram=i > 0)
    e = rel_max(d_v.download(), whole)
    print("[%s] %d x slabs summed vs the whole adjoint: %.2e" % (row, n_xt, e))
    assert np.abs(whole).max() > 0 and e < 2e-6            # the bar of tests/test_gpu_fuzz.py's slab sums


def test_sirt_five_iterations_vs_oracle():
    """Five SIRT iterations at 32^3 x 16 with detector pitch (1.25, 1) against the oracle's restatement of the reference's SIRT."""
    from oracle import oracle as orc
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.recon import sirt
    N, n = 32, 16
    rng = np.random.default_rng(5)
    geo, og = geo_pair(n, (N, N, N), "dx125_s100")
    phi = np.linspace(0.0, np.pi, n)
    xyz = np.zeros((n, 3))
    xyz[:, 0] = rng.uniform(-2.0, 2.0, n)
    xyz[:, 2] = rng.uniform(-2.0, 2.0, n)
    kw = dict(alpha=np.zeros(n), beta=np.zeros(n), phi=phi, xyz_shift=xyz)
    x = orc.shepp3d(N).astype(np.float32)
    b = orc.forward(og, x, **kw).astype(np.float32).ravel()
    want, want_err = orc.sirt(lambda v: orc.forward(og, v.reshape(N, N, N), **kw).astype(np.float32).ravel(),
                              lambda y: orc.adjoint(og, y, **kw).astype(np.float32).ravel(), N ** 3, b, 5)
    be = HipBackend(geo)
    s = sirt.SIRT(geo, b.copy(), np.array([phi, kw["alpha"], kw["beta"]]).T, xyz, options={"_backend": be})
    rec, err = profiled(be.ctx, lambda: s.run_main_iteration(niter=5))
    assert be.ctx.profile_get(GATHER)[0] >= 5 and counts(be.ctx, FLAT, TILE, "k_adj_v1", "k_fwd_tile", "k_fwd_v1", "k_fwd_v2") == (0,) * 6
    e_rec, e_err = rel_max(rec.ravel(), want), float(np.max(np.abs(err - want_err) / want_err))
    print("SIRT x5 at detector pitch (1.25, 1) vs the oracle: rec rel-max %.2e, rms_error rel %.2e" % (e_rec, e_err))
    assert e_rec < 1e-5 and e_err < 1e-5


@pytest.mark.parametrize("tag", ["d05", "d13", "dx08", "dx2", "dz2", "vox2", "vox_anis"])
def test_forward_adjoint_gradient_vs_g16(tag):
    """Golden G16: the reference's own float64 A x, A^T y and projection_gradient at seven pitch combinations, steps 1.0 and 0.7, three of
    the five poses tilted.  The gradient on the rays that keep 2e-5 voxel from a cell face (G16's volume is not smooth)."""
    from oracle import oracle as orc
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.utilities.geometry import Geometry
    g = golden("g16_pitch")
    args = (np.array(g["shape"]), np.array(g[tag + "_vox_pix"]), np.array(g[tag + "_det_shape"]), np.array(g[tag + "_det_pix"]))
    n = g[tag + "_phi"].size
    x, y = g[tag + "_x"], g[tag + "_y"]
    poses = _lib.poses_array(g[tag + "_phi"], g[tag + "_alpha"], g[tag + "_beta"], g[tag + "_xyz"], g["cor"])
    n_det = int(np.prod(g[tag + "_det_shape"]))
    for step in (float(s) for s in g["steps"]):
        s = "%s_s%02d" % (tag, round(10 * step))
        be = HipBackend(Geometry(n, *args, cor_shift=g["cor"], step_size=step))
        d_x = be.upload(x)
        e_f = rel_max(be.forward(poses, d_x, be.zeros(y.size)).download(), g[s + "_Ax"])
        e_a = rel_max(be.adjoint(poses, be.upload(y), be.zeros(x.size)).download(), g[s + "_ATy"])
        line = "[G16 %s step %.1f] forward %.2e adjoint %.2e" % (tag, step, e_f, e_a)
        assert np.mean(g[s + "_Ax"] != 0) >= 0.25
        if s + "_grad" in g.files:
            og = orc.Geo(1, *args, step_size=step)
            for i in range(2):
                pr, gd = be.empty(n_det), be.empty(6 * n_det)
                be.proj_grad(poses[i:i + 1], d_x, pr, gd)
                want_p, want_g = g[s + "_proj"][i], g[s + "_grad"][i]
                well = orc.ray_face_distance(og, g[tag + "_alpha"][i], g[tag + "_beta"][i], g[tag + "_phi"][i], g[tag + "_xyz"][i], g["cor"]) >= 2e-5
                e_p, e_g = rel_max(pr.download(), want_p), grad_error(gd.download().reshape(6, n_det), want_g, well)
                line += "; pose %d value %.2e gradient %.2e (%d of %d rays masked)" % (i, e_p, e_g, int((~well).sum()), well.size)
                assert e_p < TOL and e_g < TOL, line
        print(line)
        assert e_f < TOL and e_a < TOL, line


def grad_error(g, want, well):
    """max over the six rows of |g - want| on the rays `well`, rows of one unit sharing a scale (tests/test_gpu_fuzz.py)."""
    gmax = [max(np.max(np.abs(want[:3])), 1e-30)] * 3 + [max(np.max(np.abs(want[3:])), 1e-30)] * 3
    return max(float(np.max(np.abs(g[r] - want[r])[well], initial=0.0)) / gmax[r] for r in range(6))


# (detector pitch, voxel pitch): anisotropic finer and binned, z finer, z coarser (the WIDE_ROWS twins), neither a simple fraction, voxel pitch
GRAD_PITCHES = {"dx080": ((0.8, 1.0), (1, 1, 1)), "dx200": ((2.0, 1.0), (1, 1, 1)), "dz050": ((1.0, 0.5), (1, 1, 1)), "dz200": ((1.0, 2.0), (1, 1, 1)),
                "d130_125": ((1.3, 1.25), (1, 1, 1)), "vox_anis": ((1.0, 1.0), (1.5, 1.0, 0.75))}
# The rays of one detector row of the untilted pose share their x, y positions: a single sample within 2e-5 voxel of a face masks the whole
# row (5 to 10 % of these small detectors).  With this seed no row is lost (counted on the oracle: at most 0.91 % of a pose's rays masked)
GRAD_SEED = 9001


def grad_case(name, step):
    """-> (generator, Geometry arguments, poses, smooth volume) of one gradient case: 20 x 18 x 22, one untilted and two tilted poses."""
    det_pix, vox_pix = GRAD_PITCHES[name]
    shape = (20, 18, 22)
    rng = np.random.default_rng([GRAD_SEED, sorted(GRAD_PITCHES).index(name), int(round(10 * step))])
    n = 3
    phi = np.array([0.37, 1.23, 2.51]) + rng.uniform(-0.1, 0.1, n)
    # grad_variant 4 sorts the poses by |w_x| + |w_y| > 0.0157, w the detector-z step in voxels (pitch x sin of the tilt): the first pose is
    # below that at any pitch, the last (alpha = +-3 degrees) above it at the finest z pitch used here (0.5 sin 3 deg = 0.026)
    tilt = np.deg2rad([0.0, 0.5, 3.0])
    alpha, beta = rng.choice([-1.0, 1.0], n) * tilt, rng.uniform(-1, 1, n) * tilt
    xyz = rng.uniform(-2, 2, (n, 3))
    cor = np.zeros((n, 3))
    cor[:, 0] = rng.uniform(-1, 1, n)
    args = (n, np.array(shape), np.array(vox_pix, np.float64), np.array(det_shape(shape, det_pix, vox_pix)), np.array(det_pix))
    # a smooth volume keeps the jump of the gradient at a cell face small, not zero
    ii, jj, kk = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    fr, ph = rng.uniform(0.05, 0.35, 3), rng.uniform(0, 6.28, 3)
    x = (0.6 + 0.4 * np.cos(fr[0] * ii + ph[0]) * np.cos(fr[1] * jj + ph[1]) * np.cos(fr[2] * kk + ph[2])).astype(np.float32)
    return rng, args, (phi, alpha, beta, xyz, cor), x


@pytest.mark.parametrize("name", sorted(GRAD_PITCHES))
def test_gradient_kernels_at_non_unit_pitch(name):
    """tomo_proj_grad with all four grad_variants and tomo_cost_grad, arranged as test_gradient_kernels_agree_on_random_geometry: a smooth
    20 x 18 x 22 volume, generic angles (no multiples of pi / 2), one untilted and two tilted poses (0.5 and 3 degrees), steps 1.0 and 0.7.  The kernels multiply
    by the detector pitches (sdx, sdz) where they form a ray's start from its indices; a detector-z pitch above 1 takes the 64-bit twins."""
    from oracle import oracle as orc
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.utilities.geometry import Geometry
    det_pix, vox_pix = GRAD_PITCHES[name]
    worst_p = worst_g = worst_sum = worst_masked = 0.0
    for step in (1.0, 0.7):
        rng, args, (phi, alpha, beta, xyz, cor), x = grad_case(name, step)
        n, n_det = phi.size, int(np.prod(args[3]))
        geo, og = Geometry(*args, cor_shift=cor, step_size=step), orc.Geo(*args, cor_shift=cor, step_size=step)
        want_p, want_g, well = np.zeros((n, n_det)), np.zeros((n, 6, n_det)), np.zeros((n, n_det), bool)
        for i in range(n):
            want_p[i], want_g[i] = orc.projection_gradient(og, x, alpha[i], beta[i], phi[i], xyz[i], cor[i], precision=np.float64)
            well[i] = orc.ray_face_distance(og, alpha[i], beta[i], phi[i], xyz[i], cor[i]) >= 2e-5
            masked = 1.0 - float(np.mean(well[i]))
            worst_masked = max(worst_masked, masked)
            assert masked < 0.02, "the face mask removes %.1f %% of the rays of pose %d" % (100 * masked, i)
            assert np.mean(want_p[i] != 0) >= 0.25
        b = (want_p + 0.05 * np.max(np.abs(want_p)) * rng.standard_normal(want_p.shape)).astype(np.float32)
        want_c = 0.5 * np.sum((b.astype(np.float64) - want_p) ** 2, axis=1)
        poses = _lib.poses_array(phi, alpha, beta, xyz, cor)
        be = HipBackend(geo)
        d_x, d_b = be.upload(x), be.upload(b)
        for v in (1, 2, 3, 4):
            be.ctx.set_option("grad_variant", v)
            cost, g6 = profiled(be.ctx, lambda: be.cost_grad(poses, d_x, d_b))
            ran = tuple(c > 0 for c in counts(be.ctx, "k_cost_grad(v1)", "k_cost_grad(v2)", "k_cost_grad(v3)"))
            wide = det_pix[1] > 1.0              # TOMO_GEOM_WIDE_ROWS: the plain kernel whatever the variant (4: the untilted pose takes 2, the 3-degree one 3)
            assert ran == ((True, False, False) if wide else {1: (True, False, False), 2: (False, True, False), 3: (False, False, True), 4: (False, True, True)}[v]), (v, ran)
            assert np.allclose(cost, want_c, rtol=1e-5), ("cost", name, step, v)
            for i in range(n):
                pr, gd = be.empty(n_det), be.empty(6 * n_det)
                be.proj_grad(poses[i:i + 1], d_x, pr, gd)
                p, g = pr.download().astype(np.float64), gd.download().reshape(6, n_det).astype(np.float64)
                e_p, e_g = rel_max(p, want_p[i]), grad_error(g, want_g[i], well[i])
                worst_p, worst_g = max(worst_p, e_p), max(worst_g, e_g)
                assert e_p < TOL and e_g < TOL, (name, step, "variant", v, "pose", i, e_p, e_g)
                res = b[i].astype(np.float64) - p
                own = -g @ res
                size = np.abs(g) @ np.abs(res)
                size = np.array([size[:3].max()] * 3 + [size[3:].max()] * 3) + 1e-30
                es = float(np.max(np.abs(g6[i] - own) / size))
                worst_sum = max(worst_sum, es)
                assert es < 2e-6, (name, step, "fused sums vs own rays", v, i, es)
    print("[gradient %s] worst: value %.2e, gradient (well-conditioned rays) %.2e, fused sums vs own rays %.2e; masked rays at most %.2f %%"
          % (name, worst_p, worst_g, worst_sum, 100 * worst_masked))


def test_voxel_driven_kernels_at_voxel_pitch_vs_g16_and_oracle():
    """k_bp_voxel and k_vox_splat at voxel pitch (1.5, 1, 0.75) -- the one place `vox_pitch` reaches -- against the reference's back_project_
    and voxel_utilities (golden G16) and the oracle, at the bars of A6 and A9 in tests/test_gpu_parity.py."""
    from scipy import sparse
    from oracle import oracle as orc
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.utilities import voxel_utilities
    from tomography_alignment_amd.utilities.geometry import Geometry
    g = golden("g16_pitch")
    tag = "vox_anis"
    args = (np.array(g["shape"]), np.array(g[tag + "_vox_pix"]), np.array(g[tag + "_det_shape"]), np.array(g[tag + "_det_pix"]))
    n = g["bp_phi"].size
    be = HipBackend(Geometry(n, *args))
    poses = _lib.poses_array(g["bp_phi"], g["bp_alpha"], g["bp_beta"], g["bp_xyz"], np.zeros(3))
    vol = be.empty(int(np.prod(g["shape"])))
    profiled(be.ctx, lambda: be.backproject_voxel(poses, be.upload(g["bp_y"]), vol))
    assert be.ctx.profile_get("k_bp_voxel")[0] == 1
    want = orc.back_project_voxel(orc.Geo(n, *args), g["bp_y"], g["bp_alpha"], g["bp_beta"], g["bp_phi"], g["bp_xyz"])
    e_ref, e_orc = rel_max(vol.download(), g["bp_atx"]), rel_max(vol.download(), want)
    print("A6 back_project at voxel pitch (1.5, 1, 0.75): vs the Fortran %.2e, vs the oracle %.2e" % (e_ref, e_orc))
    assert e_ref < TOL and e_orc < TOL
    for i in range(2):
        geo = Geometry(1, *args)
        geo.cor_shift = g["vs_cor"][i]
        pose = (g["vs_alpha"][i], g["vs_beta"][i], g["vs_phi"][i], g["vs_xyz"][i])
        d, r, w = voxel_utilities.forward_sparse(geo, *pose)
        A = sparse.csr_matrix(sparse.coo_matrix((w, (r, d)), shape=(int(np.prod(g[tag + "_det_shape"])), int(np.prod(g["shape"])))))
        ref = sparse.csr_matrix((g["vs%d_data" % i], g["vs%d_indices" % i], g["vs%d_indptr" % i]), shape=tuple(g["vs%d_shape" % i]))
        A.sum_duplicates(); A.sort_indices()
        D = (A - ref).tocoo()
        e_w = float(np.max(np.abs(D.data))) if D.nnz else 0.0
        assert e_w < 2e-6 and abs(A.nnz - ref.nnz) <= 0.002 * ref.nnz + 4
        img, grad = voxel_utilities.forward_proj_grad(geo, *pose, g["vs_x"])
        o_img, o_grad = orc.vox_forward_proj_grad(orc.Geo(1, *args), *pose, g["vs_cor"][i], g["vs_x"])
        e_i, e_g = rel_max(img, g["vs_img%d" % i]), rel_max(grad, g["vs_grad%d" % i])
        print("A9 voxel splat at voxel pitch (1.5, 1, 0.75), pose %d: weights %.2e, image %.2e, gradient %.2e vs the reference (oracle: %.2e, %.2e)"
              % (i, e_w, e_i, e_g, rel_max(img, o_img), rel_max(grad, o_grad)))
        assert e_i < TOL and e_g < TOL and rel_max(img, o_img) < TOL and rel_max(grad, o_grad) < TOL
