"""half_acquisition on the GPU (libtomo_half.so) against the float64 model of tests/half_model.py: the gathered sinograms, both curves of
every detector row, the integer minimum, the side and the centre; bit-for-bit equality across calls, handles, scratch budgets and the
host and device paths; the stitch on every access path, bit-exact where it copies and within a float32 bound where it blends; the
refusal of an output that overlaps the input; and generate_data --half-acquisition -> preprocess --half-acquisition auto -> FBP.  Every
test prints the figures it measured."""
import numpy as np
import pytest

import half_model as hm

from tomography_alignment_amd import _lib, half_acquisition as ha
from tomography_alignment_amd.examples import generate_data
from tomography_alignment_amd.examples import preprocess as ex_pre
from tomography_alignment_amd.recon import fbp
from tomography_alignment_amd.utilities import projection_operators
from tomography_alignment_amd.utilities.geometry import Geometry

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24

# The five sums of a curve value are N = h w <= 2880 float64 terms each, added in another order than numpy's: each differs from the
# model's by at most N 2^-53 = 3.2e-13 of itself (in practice by a few ulp).  With q = mean square / variance of a block (at most 39 on
# these sinograms) the differences N Sxy - Sx Sy lose a factor q, and r errs by at most 4 q times that: 5e-11.  Measured maximum on the
# MI355X: 2.1e-14.
CURVE_BOUND = 1e-10
# The kernel rounds the four weights to float32 (u = 2^-24 each) and rounds once per product and per fma: b = fma(f, s1, (1 - f) s0)
# errs by at most 3 u max|p| against float64 and out = fma(wA, a, (1 - wA) b) by 2 u more for its second term and 2 u for its first and
# the sum: 7 u max|p|; the bound is 8 u max|p|.  Measured maximum on the MI355X: 2.36 u max|p| (at 16 x 1025 rows).
STITCH_BOUND = 8 * U32


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def half(ctx):
    a = ha.HalfAcquisition(ctx)
    yield a
    a.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _stack(n, nx, c, nz, seed):
    """A stack whose detector rows all have the axis at c but content of their own: noise of 2 % from a seed per row, and a scale."""
    return np.stack([(1.0 + 0.25 * z) * hm.sinogram_360(n, nx, c, noise=0.02 if z % 2 else 0.0, seed=seed + z) for z in range(nz)], axis=2)


# ------------------------------------------------------------------------------------------------------------------------ search

@pytest.mark.parametrize("case,nz", [(0, 5), (1, 8), (2, 5), (3, 8), (4, 5), (5, 8)])
def test_search_equals_the_model(ctx, half, case, nz):
    """Curves within CURVE_BOUND of the model's (measured maximum over the six cases: printed), the integer minimum and the side of
    every detector row identical, the centre within 1e-6 px; for rows=None and for a subset in an order of its own; numpy and device
    input, two calls and a fresh handle give the same bits."""
    n, nx, c, w = hm.CASES[case]
    p = _stack(n, nx, c, nz, seed=10 * case)
    d_p = ctx.to_device(p, np.float32)
    try:
        for rows in (None, [nz - 1, 0, 2]):
            centre, centres, sides, ks, curves = hm.find_center_360(p, rows=rows, win_width=w)
            r = half.find_center_360(d_p, rows=rows, win_width=w, return_curves=True)
            model = np.array([[mr, ml] for mr, ml in curves])
            e = np.abs(r.curves - model).max()
            print("case %d nz %d rows %s: curves differ by at most %.2e; centre %.6f, model %.6f, truth %.2f" % (case, nz, rows, e, r.center, centre, c))
            assert r.curves.shape == (len(ks), 2, nx - w + 1) and e <= CURVE_BOUND
            assert [int(np.argmin(r.curves[i, hm.SIDES.index(sides[i])])) for i in range(len(ks))] == ks
            assert r.sides == sides and r.side == ("right" if c >= (nx - 1) / 2 else "left")
            assert np.abs(r.centers - centres).max() <= 1e-6 and abs(r.center - centre) <= 1e-6 and abs(r.center - c) <= 0.1
            assert r.offset == r.center - (nx - 1) / 2 and r.overlap == 2 * min(r.center, nx - 1 - r.center) + 1
            assert np.array_equal(r.rows, [nz // 2] if rows is None else rows)
            again = half.find_center_360(d_p, rows=rows, win_width=w, return_curves=True)
            host = half.find_center_360(p, rows=rows, win_width=w, return_curves=True)
            tight = half.find_center_360(d_p, rows=rows, win_width=w, return_curves=True, max_scratch_bytes=1)      # one row per batch
            fresh = ha.find_center_360(d_p, rows=rows, win_width=w, return_curves=True, ctx=ctx)
            for other in (again, host, tight, fresh):
                assert np.array_equal(_bits(other.curves), _bits(r.curves)) and other.center == r.center
            one = half.find_center_360(d_p, rows=rows, win_width=w, side=r.side)
            assert one.center == r.center and one.curves is None
        rows = [nz - 1, 0, 2]
        half.curves(d_p, rows=rows, win_width=w)
        for i, z in enumerate(rows):
            assert np.array_equal(half.handle.debug_sinogram(ctx.stream(), i), p[:, :, z])
        assert half.device_bytes() > 0
    finally:
        d_p.free()


def test_search_takes_the_endpoint_and_more_than_one_tile(ctx, half):
    """Angles with the endpoint (the last projection is dropped), a window of 37 columns (five tiles of 8, the last one partial) and 1100
    candidates (two tiles of 1024): against the model on a random stack."""
    rng = np.random.default_rng(3)
    n, nx, nz, w = 7, 1136, 2, 37
    p = rng.uniform(0.0, 2.0, (n, nx, nz)).astype(np.float32)
    angles = np.linspace(0.0, 2 * np.pi, n)
    r = half.find_center_360(p, angles=angles, rows=[0, 1], win_width=w, return_curves=True)
    _, centres, sides, _, curves = hm.find_center_360(p, angles=angles, rows=[0, 1], win_width=w)
    e = np.abs(r.curves - np.array([[mr, ml] for mr, ml in curves])).max()
    print("7 angles with the endpoint, 1136 columns, window 37: curves differ by at most %.2e" % e)
    assert r.curves.shape == (2, 2, 1100) and e <= CURVE_BOUND and r.sides == sides and np.abs(r.centers - centres).max() <= 1e-6
    flat = np.zeros((6, 16, 2), np.float32)                              # no variance anywhere: m = 1, the first candidate of side right
    r = half.find_center_360(flat, rows=[0, 1], win_width=4, return_curves=True)
    assert np.all(r.curves == 1.0) and r.sides == ["right", "right"] and r.center == (16 - 1 + 12) / 2.0


# ------------------------------------------------------------------------------------------------------------------------ stitch

CENTRES = {16: (15.0, 7.5, 12.0, 11.5, 12.62, 8.01, 3.0, 3.5, 2.38, 0.0, 7.49),
           48: (47.0, 23.5, 40.0, 40.5, 33.37, 6.0, 6.5, 14.63),
           64: (63.0, 31.5, 52.0, 55.5, 52.3, 10.2, 11.0, 8.5)}


def _stitch_flat(ctx, half, p, c, offset):
    """The stitch of p through flat device buffers that start `offset` floats into their allocations: offset 0 is 16-byte aligned."""
    n, nx, nz = p.shape
    h, W, _ = ha.stitched_shape(n, nx, c)
    d_in, d_out = ctx.empty(p.size + offset, np.float32), ctx.zeros(h * W * nz + offset + 1, np.float32)
    try:
        src, dst = d_in.view(offset, p.size), d_out.view(offset, h * W * nz)
        src.upload(p)
        res = half.sino_360_to_180(src, c, out=dst, shape=p.shape)
        assert res.projections is dst
        whole = d_out.download()
        assert whole[offset + h * W * nz] == 0.0 and np.all(whole[:offset] == 0.0)      # nothing written outside the output
        return whole[offset:offset + h * W * nz].reshape(h, W, nz), res
    finally:
        d_in.free()
        d_out.free()


# (nx, h, nz) of the stitch.  k_stitch puts zl lanes of four z along z (the rule of tomo_half_stitch, _zl below) and keeps 256 / zl columns
# in flight; past 4 * 256 rows a second chunk of z (blockIdx.x >= 1) follows.  The first list stays within zl 1, 2 and 4.
STITCH_SHAPES = [(16, 1, 1), (16, 4, 5), (16, 45, 8), (48, 4, 12), (48, 1, 8), (64, 4, 5), (64, 45, 12), (64, 1, 1)]
STITCH_SHAPES_TALL = [
    (16, 1, 20),        # zl 8
    (16, 3, 30),        # zl 8, with a tail
    (16, 1, 36),        # zl 16
    (16, 1, 100),       # zl 32
    (16, 3, 130),       # zl 64, with a tail
    (16, 1, 260),       # zl 128
    (48, 3, 516),       # zl 256: one column in flight, three column tiles
    (16, 1, 1024),      # zl 256, exactly one chunk
    (16, 3, 1025),      # two z chunks, the second holds one element
    (48, 1, 1028),      # two z chunks, the 16-byte path
    (48, 3, 2050),      # three z chunks, with a tail
]


def _zl(nz):
    """Lanes along z of k_stitch, as tomo_half_stitch (csrc/half/tomo_half.hip) chooses them: a work-group has 256 lanes of four z."""
    zl = 1
    while zl < 256 and 4 * zl < nz:
        zl *= 2
    return zl


def test_the_stitch_shapes_reach_every_lane_split_and_a_third_chunk():
    """Host only: the lists above reach what they claim, so a change of the kernel's geometry fails here and not silently."""
    nzs = [nz for _, _, nz in STITCH_SHAPES + STITCH_SHAPES_TALL]
    chunks = {nz: -(-nz // (4 * _zl(nz))) for nz in nzs}
    print("zl of the stitch cases %s; z chunks %s" % (sorted(set(_zl(nz) for nz in nzs)), sorted(set(chunks.values()))))
    assert set(_zl(nz) for nz in nzs) == {1, 2, 4, 8, 16, 32, 64, 128, 256}
    assert max(chunks.values()) >= 3
    assert any(c > 1 and nz % 4 == 0 for nz, c in chunks.items()) and any(c > 1 and nz % 4 != 0 for nz, c in chunks.items())


@pytest.mark.parametrize("nx,h,nz", STITCH_SHAPES + STITCH_SHAPES_TALL)
def test_stitch_equals_the_model(ctx, half, nx, h, nz):
    """For every c of CENTRES[nx] -- both sides, integer and half-integer 2 c, fractional values, the detector centre and c = nx - 1,
    where g = 0 -- and for an aligned and a misaligned pair of pointers: the columns the first half alone supplies are its bits, every
    column is within STITCH_BOUND max|p| of the float64 model (measured maximum: printed, in units of 2^-24 max|p|), and the two access
    paths give the same bits."""
    rng = np.random.default_rng(nx + h + nz)
    p = rng.uniform(-1.0, 3.0, (2 * h, nx, nz)).astype(np.float32)
    worst = 0.0
    for c in CENTRES[nx]:
        ref, T = hm.stitch(p, c)
        got = {}
        for offset in (0, 1):
            got[offset], res = _stitch_flat(ctx, half, p, c, offset)
            out = got[offset]
            assert out.shape == (h, T["W"], nz) == ha.stitched_shape(2 * h, nx, c)[:2] + (nz,)
            assert res.center == T["c_out"] and res.cor_offset == T["c_out"] - (T["W"] - 1) / 2 and res.angles is None
            only_a = T["a_valid"] & ~T["b_valid"]
            assert np.array_equal(out[:, only_a].view(np.uint32), p[:h, T["ja"][only_a]].view(np.uint32))
            e = np.abs(out - ref).max() / np.abs(p).max()
            worst = max(worst, e)
            assert e <= STITCH_BOUND, (c, offset, e / U32)
        assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), c
        if c == nx - 1.0:                                                # g = 0: the shared column is the first half's
            assert np.array_equal(got[0][:, :nx], p[:h])
    print("nx %d h %d nz %d: worst error %.2f x 2^-24 max|p| over %d axes" % (nx, h, nz, worst / U32, len(CENTRES[nx])))


def test_stitch_kinds_angles_and_the_overlap_refusal(ctx, half):
    rng = np.random.default_rng(9)
    n, nx, nz, c = 8, 16, 8, 11.3
    p = rng.uniform(0.0, 2.0, (n + 1, nx, nz)).astype(np.float32)
    angles = np.linspace(0.0, 2 * np.pi, n + 1)                          # with the endpoint: the ninth projection is dropped
    h, W, j0 = ha.stitched_shape(n, nx, c)
    ref, _ = hm.stitch(p, c, angles=angles)
    host = half.sino_360_to_180(p, c, angles=angles)
    assert isinstance(host.projections, np.ndarray) and host.projections.dtype == np.float32 and host.projections.shape == (h, W, nz)
    assert np.array_equal(host.angles, angles[:h]) and np.abs(host.projections - ref).max() <= STITCH_BOUND * 2.0
    into = np.zeros((h, W, nz), np.float32)
    assert half.sino_360_to_180(p, c, angles=angles, out=into).projections is into and np.array_equal(into, host.projections)
    d_p = ctx.to_device(p, np.float32)
    try:
        dev = half.sino_360_to_180(d_p, c, angles=angles)
        assert isinstance(dev.projections, _lib.DeviceArray) and dev.projections.shape == (h, W, nz)
        assert np.array_equal(dev.projections.download(), host.projections)
        dev.projections.free()
        own = ha.sino_360_to_180(d_p, c, angles=angles, ctx=ctx)         # a handle of its own
        assert np.array_equal(own.projections.download(), host.projections)
        own.projections.free()
        with pytest.raises(ValueError, match="out must be a DeviceArray"):
            half.sino_360_to_180(d_p, c, angles=angles, out=into)
    finally:
        d_p.free()
    size = n * nx * nz
    buf = ctx.zeros(size + h * W * nz, np.float32)
    try:
        buf.view(0, size).upload(p[:n])
        for start in (0, 4, size - 4):                                   # the output over the input's start, inside it, and over its end
            with pytest.raises(_lib.TomoError, match="out overlaps p: the stitch does not work in place; nothing was launched"):
                half.sino_360_to_180(buf.view(0, size), c, out=buf.view(start, h * W * nz), shape=(n, nx, nz))
        assert np.array_equal(buf.download()[:size], p[:n].ravel()) and np.all(buf.download()[size:] == 0.0)
        res = half.sino_360_to_180(buf.view(0, size), c, out=buf.view(size, h * W * nz), shape=(n, nx, nz))     # adjacent is fine
        assert np.array_equal(res.projections.download().reshape(h, W, nz), host.projections)
    finally:
        buf.free()


# -------------------------------------------------------------------------------------------------------------------- end to end

def test_generate_preprocess_stitch_and_reconstruct(ctx):
    """generate_data --half-acquisition 12 at size 48 (48 projections over 2 pi on 30 columns, no pose jitter), preprocess
    --half-acquisition auto: the written axis is recovered within 0.25 px; the stitched projections equal the phantom's projection over
    [0, pi) on the W columns of the stitched detector, with cor_shift the file's cor_offset, as closely as the float64 model's stitch of
    the same preprocessed series about the same axis does, plus the stitch's parity bound (STITCH_BOUND + 2 u) max|p|; without the
    option preprocess gives what it gave; and FBP of the stitched series is closer to the phantom than FBP of the 2 pi series as it is.
    Measured on the MI355X: axis found at 23.493; error of the model's stitch 2.1497 of a maximum of 12.38 (nearly all of it the sorting
    stripe removal's at the edge columns of the 30-column detector, before any stitch), of the GPU's 2.1497, parity bound 7.4e-6; RMSE
    of FBP 0.0903 stitched, 0.1513 on the 2 pi series."""
    data = generate_data.make(48, 48, seed=0, ang_deg=0.0, shift_px=0.0, raw=True, half_acquisition=12)
    assert data["projections"].shape == (48, 30, 48) and data["half_center"] == 23.5
    plain = ex_pre.run(data, stripe_size=3, ctx=ctx)
    same = ex_pre.run(data, stripe_size=3, ctx=ctx, half_acquisition=None)
    assert sorted(plain) == sorted(same) == sorted(k for k in list(data) + [] if k not in ex_pre.RAW_KEYS)
    for k in plain:
        assert np.asarray(plain[k]).tobytes() == np.asarray(same[k]).tobytes(), k
    out = ex_pre.run(data, stripe_size=3, ctx=ctx, half_acquisition="auto", center_rows=5)
    assert sorted(out) == sorted(list(plain) + ["half_axis"])
    axis = float(out["half_axis"])
    print("axis written %.3f, found %.3f" % (data["half_center"], axis))
    assert abs(axis - data["half_center"]) <= 0.25
    h, W, j0 = ha.stitched_shape(48, 30, axis)
    proj = out["projections"]
    assert proj.shape == (h, W, 48) and proj.dtype == np.float32 and h == 24 and W in (47, 48, 49)
    for k in ("phi", "alpha", "beta", "xyz"):
        assert np.array_equal(out[k], data[k][:h])
    assert out["cor_offset"] == -(axis + j0 - (W - 1) / 2.0)
    given = ex_pre.run(data, stripe_size=3, ctx=ctx, half_acquisition=axis)
    assert np.array_equal(given["projections"], proj) and given["half_axis"] == axis

    geo = Geometry(h, np.array([48, 48, 48]), np.ones(3), np.array([W, 48]), np.ones(2), cor_shift=np.array([float(out["cor_offset"]), 0.0, 0.0]))
    zero = np.zeros(h)
    full = projection_operators.ProjectionMatrix(geo, precision=np.float32).projection_matrix(alpha=zero, beta=zero, phi=out["phi"], xyz_shift=np.zeros((h, 3)))
    full = full.dot(data["phantom"].ravel()).reshape(h, W, 48)
    model, _ = hm.stitch(plain["projections"], axis, angles=data["phi"])
    e_model, e_gpu = np.abs(model - full).max(), np.abs(proj - full).max()
    # the example divides by mu after the stitch, the model's input has been divided before it: one rounding of 2^-24 on either side
    parity = (STITCH_BOUND + 2 * U32) * np.abs(plain["projections"]).max()
    print("stitched against the full-width projection (maximum %.2f): model %.4f, GPU %.4f, parity bound %.2e" % (full.max(), e_model, e_gpu, parity))
    assert e_gpu <= e_model + parity
    assert np.abs(proj - model).max() <= parity

    angles = np.zeros((h, 3))
    angles[:, 0] = out["phi"]
    rec = fbp.FBP(geo, proj, angles, np.zeros((h, 3))).run()
    raw_geo = Geometry(48, np.array([48, 48, 48]), np.ones(3), np.array([30, 48]), np.ones(2), cor_shift=np.array([float(data["cor_offset"]), 0.0, 0.0]))
    raw_angles = np.zeros((48, 3))
    raw_angles[:, 0] = data["phi"]
    raw_rec = fbp.FBP(raw_geo, plain["projections"], raw_angles, np.zeros((48, 3))).run()
    rmse = lambda v: float(np.sqrt(np.mean((np.asarray(v, np.float64) - data["phantom"]) ** 2)))       # noqa: E731
    print("FBP against the phantom: RMSE %.4f stitched, %.4f on the 2 pi series without the stitch" % (rmse(rec), rmse(raw_rec)))
    assert rec.shape == (48, 48, 48) and np.all(np.isfinite(rec)) and rmse(rec) < rmse(raw_rec)
