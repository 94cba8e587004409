"""rotation_axis.find_center on the GPU (libtomo_cor.so) against the float64 model of tests/cor_model.py: the stacked sinograms the
build kernel writes (exact at integer shifts, within one float32 ulp at spline shifts), the metric curves within 16 d32 (d32: what
float32 transforms cost the model itself), the chosen candidate equal to the model's (tests/test_rotation_axis.py asserts the
separation that makes that fair), bit-for-bit equality across scratch budgets, repeats, handles, batching of rows and the host and
device paths, the (n, nx, nz) layout and the endpoint row, the sign against the HIP projector, and align_rigid.run(cor="auto").  Every
test prints the figures it measured."""
import numpy as np
import pytest

import cor_model as cm

from tomography_alignment_amd import _cor_lib, _lib, rotation_axis
from tomography_alignment_amd.examples import align_rigid, generate_data
from tomography_alignment_amd.utilities import generate_phantom, projection_operators
from tomography_alignment_amd.utilities.geometry import Geometry

pytestmark = pytest.mark.gpu

# k_prefilter starts its causal recursion from at most HORIZON = 128 terms (nx - 2 of them where the row is shorter) and moves a row
# through LDS in tiles of TW = 64 columns.  (24, 130): nx - 2 is the horizon exactly, three tiles, the last of two columns; (24, 131):
# one term is cut off, the last tile has three columns; (30, 200): 70 terms are cut off, four tiles, the last of eight columns.
BUILD_SHAPES = [(37, 50), (24, 33), (45, 96), (24, 130), (24, 131), (30, 200)]
PARITY_SHAPES_WIDE = cm.PARITY_SHAPES_WIDE


def test_the_shape_lists_reach_the_truncated_start_and_a_second_pass_of_the_reduction():
    """Host only.  The constants are those of csrc/cor/tomo_cor.hip: HORIZON = 128, TW = 64, and k_reduce's 64 lanes along ku from
    ku = 2 on, whose second pass begins at ku = 66."""
    horizon, tw, second_pass = 128, 64, 2 + 64
    assert any(nx - 2 == horizon for _, nx in BUILD_SHAPES) and any(nx - 2 > horizon for _, nx in BUILD_SHAPES)
    assert any(-(-nx // tw) == 3 and nx % tw for _, nx in BUILD_SHAPES) and any(-(-nx // tw) >= 4 and nx % tw for _, nx in BUILD_SHAPES)
    for n, nx in PARITY_SHAPES_WIDE:
        w, cut = cm.wedge(2 * n, nx)
        widest = int(np.max(np.minimum(w, nx // 2)[~cut]))
        print("(%d, %d): the widest uncut row of the wedge ends at ku = %d" % (n, nx, widest))
        assert widest >= second_pass
    for n, nx in cm.PARITY_SHAPES:                                      # and the narrow list stays what it was: one pass
        w, cut = cm.wedge(2 * n, nx)
        assert int(np.max(np.minimum(w, nx // 2)[~cut])) < second_pass


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def axis(ctx):
    a = rotation_axis.RotationAxis(ctx)
    yield a
    a.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _curves(r):
    """All curves of a CenterResult as one float64 array."""
    return np.concatenate([np.concatenate([c[1] for c in r.coarse]), np.concatenate([f[0] for f in r.fine]), np.concatenate([f[1] for f in r.fine])])


def _search(axis, proj, nx, **kw):
    smin, smax = cm.search_range(nx)
    return axis.find_center(proj, smin=smin, smax=smax, return_curves=True, **kw)


# ------------------------------------------------------------------------------------------------------------------ T1, T2: build

@pytest.mark.parametrize("n,nx", BUILD_SHAPES)
def test_build_integer_shifts_are_the_models_bits(axis, n, nx):
    S = cm.ellipse_sinogram(n, nx, 1.5, seed=5, noise=0.02)
    axis.load(S[:, :, None])
    assert np.array_equal(axis.handle.debug_sinogram(axis.ctx.stream(), 0), S)
    for t in (0, 1, -1, 7, -12):
        got, ref = axis.stack(0, t), cm.stack(S, t)
        bad = int(np.count_nonzero(got != ref))
        print("(%d, %d) t %d: %d of %d elements differ" % (n, nx, t, bad, ref.size))
        assert got.dtype == np.float32 and np.array_equal(got, ref)


@pytest.mark.parametrize("n,nx", BUILD_SHAPES)
def test_build_spline_shifts_within_one_ulp(axis, n, nx):
    """Both sides evaluate in float64 and round once, so only an element at a rounding boundary can differ, by one ulp of its own
    magnitude; the bound is one float32 ulp of the row's largest magnitude."""
    S = cm.ellipse_sinogram(n, nx, 1.5, seed=6, noise=0.02)
    axis.load(S[:, :, None])
    coef = axis.handle.debug_coefficients(axis.ctx.stream(), 0)
    ref_c = cm.spline_coefficients(S[:, ::-1].astype(np.float64))
    print("(%d, %d): spline coefficients, largest difference from the model %.1e (largest value %.3g)"
          % (n, nx, float(np.max(np.abs(coef - ref_c))), float(np.max(np.abs(ref_c)))))
    assert np.max(np.abs(coef - ref_c)) <= 1e-12 * np.max(np.abs(ref_c))
    for t in (0.5, -0.5, 3.5, -7.5, 2.25):
        got, ref = axis.stack(0, t), cm.stack(S, t)
        ulp = np.spacing(np.max(np.abs(ref), axis=1).astype(np.float32)).astype(np.float64)[:, None]
        diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        print("(%d, %d) t %g: %d of %d elements differ, the largest by %.2f ulp of its row's maximum"
              % (n, nx, t, int(np.count_nonzero(diff)), ref.size, float(np.max(diff / ulp))))
        assert np.array_equal(got[:n], S)
        assert np.all(diff <= ulp)


# -------------------------------------------------------------------------------------------------------- T3, T4: curves, result

@pytest.mark.parametrize("noise", [0.0, 0.02])
@pytest.mark.parametrize("n,nx", cm.PARITY_SHAPES + PARITY_SHAPES_WIDE)
def test_metric_curves_and_offset_against_the_float64_model(axis, n, nx, noise):
    worst = 0.0
    for off in cm.OFFSETS:
        S, r64, r32 = cm.found(n, nx, off, noise)
        d32 = cm.d32_of(r64, r32)
        got = _search(axis, S[:, :, None], nx)
        assert np.array_equal(got.coarse[0][0], r64.coarse[0]) and np.array_equal(got.fine[0][0], r64.fine[0])     # the same candidates
        for name, g, m in (("coarse", got.coarse[0][1], r64.coarse[1]), ("fine", got.fine[0][1], r64.fine[1])):
            rel = np.abs(g - m) / m
            worst = max(worst, float(rel.max() / (16 * d32)))
            print("(%d, %d) offset %g noise %g %s: d32 %.2e, GPU minus model at most %.2e = %.2f d32"
                  % (n, nx, off, noise, name, d32, float(rel.max()), float(rel.max() / d32)))
            assert np.all(np.isfinite(g)) and np.all(rel <= 16 * d32)
        print("(%d, %d) offset %g noise %g: offset GPU %g, model %g" % (n, nx, off, noise, got.offset, r64.offset))
        assert got.offset == r64.offset and got.offsets.shape == (1,) and got.center == 0.5 * (nx - 1) + r64.offset
    print("(%d, %d) noise %g: largest fraction of the bound %.3f" % (n, nx, noise, worst))


# ------------------------------------------------------------------------------------------------------------------------ T5: bits

def test_budgets_repeats_handles_batching_and_paths_give_the_same_bits(ctx, axis):
    n, nx, nz = 37, 50, 4
    proj = np.stack([cm.ellipse_sinogram(n, nx, off, seed=10 + z, noise=0.02) for z, off in enumerate((0.0, 3.25, -5.5, 7.75))], axis=2)
    rows = [0, 1, 2, 3]
    fb = 4 * (2 * n) * 2 * (nx // 2 + 1)
    ref = _search(axis, proj, nx, rows=rows, max_scratch_bytes=None)
    want = _bits(_curves(ref))
    print("offsets %s, median %g" % (ref.offsets.tolist(), ref.offset))
    assert ref.offset == float(np.median(ref.offsets)) and ref.offsets.shape == (4,)
    results = {}
    for budget in (1, 2 * fb, 4 * fb, 6 * fb + 5, None):
        results["budget %s" % budget] = _search(axis, proj, nx, rows=rows, max_scratch_bytes=budget)
    _search(axis, cm.ellipse_sinogram(24, 33, 1.0)[:, :, None], 33)                 # another shape and plan between the calls
    results["repeat"] = _search(axis, proj, nx, rows=rows)
    with rotation_axis.RotationAxis(ctx) as fresh:
        results["fresh handle"] = _search(fresh, proj, nx, rows=rows)
    d = ctx.to_device(proj)
    results["device"] = _search(axis, d, nx, rows=rows)
    flat = d.view(0, d.size)
    results["flat device buffer"] = _search(axis, flat, nx, rows=rows, shape=proj.shape)
    smin, smax = cm.search_range(nx)
    results["module level"] = rotation_axis.find_center(proj, rows=rows, smin=smin, smax=smax, return_curves=True, ctx=ctx)
    for name, r in results.items():
        diff = int(np.count_nonzero(_bits(_curves(r)) != want))
        print("%s: %d values differ from the unbatched run" % (name, diff))
        assert diff == 0 and np.array_equal(r.offsets, ref.offsets), name
    for z in rows:                                                                  # one row per call
        one = _search(axis, proj, nx, rows=[z])
        assert np.array_equal(_bits(one.coarse[0][1]), _bits(ref.coarse[z][1])) and np.array_equal(_bits(one.fine[0][1]), _bits(ref.fine[z][1]))
        assert one.offset == ref.offsets[z]
    assert np.array_equal(d.download(), proj)
    d.free()


def test_a_repeated_metric_finds_every_plan_in_the_cache(ctx):
    """The smallest sinogram, five pairs in batches of two: a plan of two and the tail's plan of one.  A wrong cache key would make
    them again, or grow the work area."""
    n, nx = _cor_lib.MIN_N, _cor_lib.MIN_NX
    S = np.random.default_rng(3).uniform(0.0, 1.0, (n, nx)).astype(np.float32)
    budget = 4 * 4 * (2 * n) * 2 * (nx // 2 + 1)
    assert (n, nx) == (8, 16) and _cor_lib.batch(5, n, nx, budget) == 2
    d = ctx.to_device(S[:, :, None])
    slices, ts = [0] * 5, [0.0, 1.0, -2.5, 3.25, -4.0]
    with _cor_lib.CorHandle(ctx.device) as h:
        h.load_rows(ctx.stream(), d.ptr, n, nx, 1, 0, n, [0])
        first = h.metric(ctx.stream(), slices, ts, max_scratch_bytes=budget)
        seconds, held = h.plan_seconds(), h.device_bytes()
        second = h.metric(ctx.stream(), slices, ts, max_scratch_bytes=budget)
        print("m %s, plan seconds %.6f -> %.6f, device bytes %d -> %d" % (first, seconds, h.plan_seconds(), held, h.device_bytes()))
        assert seconds > 0.0 and h.plan_seconds() == seconds and h.device_bytes() == held
    assert np.all(first > 0) and np.array_equal(_bits(second), _bits(first))
    d.free()


# ---------------------------------------------------------------------------------------------------------------------- T6: layout

@pytest.mark.parametrize("nz", [5, 64])
def test_rows_of_a_stack_and_the_endpoint_row(ctx, axis, nz):
    n, nx = 37, 50
    rng = np.random.default_rng(nz)
    proj = rng.uniform(0.0, 0.05, (n, nx, nz)).astype(np.float32)                  # every other row: noise that must not leak in
    rows = [0, nz - 1, nz // 2]
    offs = (3.25, -5.5, 0.0)
    for z, off in zip(rows, offs):
        proj[:, :, z] = cm.ellipse_sinogram(n, nx, off, seed=z, noise=0.02)
    got = _search(axis, proj, nx, rows=rows)
    d = ctx.to_device(proj)
    on_device = _search(axis, d, nx, rows=rows)
    assert np.array_equal(_bits(_curves(on_device)), _bits(_curves(got))) and np.array_equal(got.rows, rows)
    for k, (z, off) in enumerate(zip(rows, offs)):
        alone = _search(axis, np.ascontiguousarray(proj[:, :, z:z + 1]), nx)
        print("nz %d row %d: offset %g (true %g)" % (nz, z, got.offsets[k], off))
        assert np.array_equal(_bits(alone.coarse[0][1]), _bits(got.coarse[k][1])) and np.array_equal(_bits(alone.fine[0][1]), _bits(got.fine[k][1]))
        assert abs(got.offsets[k] - off) <= 0.25
    assert rotation_axis.find_center(proj, smin=-10, smax=10, ctx=ctx).rows.tolist() == [nz // 2]       # the default row
    # n + 1 angles over [0, pi] with the endpoint: the last row is dropped, on the host path and on the device
    with_end = np.concatenate([proj, proj[:1, ::-1, :]], axis=0)
    angles = np.linspace(0.0, np.pi, n + 1)
    for p in (with_end, ctx.to_device(with_end)):
        r = _search(axis, p, nx, rows=rows, angles=angles)
        assert np.array_equal(_bits(_curves(r)), _bits(_curves(got)))
    assert np.array_equal(_bits(_curves(_search(axis, proj, nx, rows=rows, angles=np.arange(n) * np.pi / n))), _bits(_curves(got)))
    d.free()


# ------------------------------------------------------------------------------------------------------------------------ T7: sign

@pytest.mark.parametrize("d", [4.0, -6.5])
def test_sign_against_the_projector(ctx, d):
    N, n = 48, 60
    geom = Geometry(n, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2), cor_shift=np.array([d, 0.0, 0.0]))
    phi = np.arange(n) * np.pi / n
    A = projection_operators.ProjectionMatrix(geom, precision=np.float32).projection_matrix(alpha=np.zeros(n), beta=np.zeros(n), phi=phi,
                                                                                          xyz_shift=np.zeros((n, 3)))
    proj = np.asarray(A.dot(generate_phantom.shepp3d(N).ravel()), np.float32).reshape(n, N, N)
    r = rotation_axis.find_center(proj, angles=phi, smin=-10, smax=10, ctx=ctx)
    cor = rotation_axis.to_cor_shift(r.offset, n)
    print("cor_shift x %g: offset %g, to_cor_shift gives %g" % (d, r.offset, cor[0, 0]))
    assert cor.shape == (n, 3) and np.all(cor[:, 0] == cor[0, 0]) and not cor[:, 1:].any()
    assert abs(cor[0, 0] - d) <= 0.25


# ---------------------------------------------------------------------------------------------------------------------- T8: driver

def _strip(hist):
    return [{k: v for k, v in h.items() if not k.endswith("_wall_s")} for h in hist]


def test_align_rigid_finds_the_axis_first():
    """generate_data.make(64, 90, seed=3, cor_offset=6.5) keeps its +-2 px jitter and +-1 degree tilts.  On this data the model alone
    (the oracle's projections of the same poses, the nine rows the driver searches, +-25 px) gives offsets -6.25, -6.25, 28.0, -10.25,
    -9.25, -10.25, -19.25, 26.0, 25.25: single rows are thrown off by the jitter, their median, -6.25, is within 0.25 px.
    The loop is not bit-reproducible (float-atomic projectors; L-BFGS-B amplifies the last bits of the reconstruction,
    tests/test_gpu_multires.py), so `cor=None` is held to the plain call by what is reproducible: the same keys, no cor_shift in the
    geometry or in the history, the same SIRT iteration counts, and the first SIRT's RMSE at the 1e-5 that test allows two runs.  The
    final poses of the two calls are printed, not asserted: on this data, whose axis offset neither call corrects, they differed by
    0.25 px on the MI355X while the first RMSE agreed to 1.3e-11."""
    data = generate_data.make(64, 90, seed=3, cor_offset=6.5)
    assert float(data["cor_offset"]) == 6.5
    kw = dict(n_outer=2, sirt_iters=30, verbose=False, download=False)
    auto = align_rigid.run(dict(data), cor="auto", **kw)
    none = align_rigid.run(dict(data), cor=None, return_loop=True, **kw)
    plain = align_rigid.run(dict(data), **kw)
    found = auto[4][0]["cor"]
    e_auto, e_none = auto[4][-1]["shift_err_px"], none[4][-1]["shift_err_px"]
    print("cor found %g (true 6.5); final shift error with it %.3f px, without %.3f px" % (found, e_auto, e_none))
    assert abs(found - 6.5) <= 1.5 and all(h["cor"] == found for h in auto[4])
    assert e_auto < e_none
    loop = none[5]
    assert loop.cor is None and not np.any(loop.geom.cor_shift) and all("cor" not in h for h in none[4])
    assert [sorted(h) for h in _strip(none[4])] == [sorted(h) for h in _strip(plain[4])]
    d_rmse = abs(none[4][0]["rmse"] / plain[4][0]["rmse"] - 1)
    d_xyz = float(np.max(np.abs(none[3] - plain[3])))
    print("cor=None against the plain call: first rmse differs by %.2e relative, the poses by %.3e px" % (d_rmse, d_xyz))
    assert d_rmse <= 1e-5 and [h["sirt_iterations"] for h in none[4]] == [h["sirt_iterations"] for h in plain[4]]
    with pytest.raises(ValueError, match="auto"):
        align_rigid.resolve_cor(data, "auto", comm=object())
    assert align_rigid.resolve_cor(data, 2.5, comm=object()) == 2.5 and align_rigid.resolve_cor(data, None) is None


def test_generate_data_without_an_offset_is_what_it_was():
    """make() projects with the float-atomic forward kernel, whose sums depend on the order in which the atomics arrive: two calls of
    make() itself do not give the same bits.  So every key the projector does not write is compared exactly, and `projections` at
    1e-5 of its largest value, the float32 parity every GPU test of the projector is held to (conftest.rel_max).  That cor_offset=0
    hands the projector exactly what make() hands it -- and so gives equal bits with a projector that is a function of its
    arguments -- is asserted without a GPU in tests/test_rotation_axis.py, on the CPU oracle."""
    a, b = generate_data.make(32, 24, seed=1), generate_data.make(32, 24, seed=1, cor_offset=0.0)
    assert sorted(a) == sorted(b) and float(a["cor_offset"]) == 0.0
    for k in a:
        if k != "projections":
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    d = float(np.max(np.abs(a["projections"] - b["projections"])) / np.max(np.abs(a["projections"])))
    print("make() against make(cor_offset=0): projections differ by %.2e of their largest value" % d)
    assert a["projections"].shape == b["projections"].shape and d <= 1e-5
    c = generate_data.make(32, 24, seed=1, cor_offset=3.0)
    assert float(c["cor_offset"]) == 3.0 and np.array_equal(c["xyz"], a["xyz"])
    assert np.max(np.abs(c["projections"] - a["projections"])) > 0.1 * np.max(np.abs(a["projections"]))


# ----------------------------------------------------------------------------------------------------------- refusals and lifetime

def test_refusals_come_before_any_launch(ctx, axis):
    S = cm.ellipse_sinogram(37, 50, 0.0)
    d = ctx.to_device(S[:, :, None])
    before = axis.device_bytes()
    for kw in (dict(smin=-19, smax=5), dict(smin=3, smax=2), dict(smin=-5, smax=5, step=0.0), dict(smin=-5, smax=5, angles=np.linspace(0, 2, 37)),
               dict(smin=-5, smax=5, rows=[1]), dict(smin=-5, smax=5, ratio=0.0)):
        with pytest.raises(ValueError):
            axis.find_center(d, **kw)
    with pytest.raises(rotation_axis.CorUnsupported):
        axis.find_center(ctx.zeros((8200, 16, 1)), smin=-1, smax=1, srad=0)
    with pytest.raises(ValueError):
        axis.find_center(ctx.zeros((6, 50, 1)), smin=-5, smax=5)
    assert axis.device_bytes() == before and np.array_equal(d.download(), S[:, :, None])
    h = _cor_lib.CorHandle(ctx.device)
    with pytest.raises(_lib.TomoError, match="no sinogram is loaded"):
        h.metric(ctx.stream(), [0], [0.0])
    with pytest.raises(_cor_lib.CorUnsupported):
        h.load_rows(ctx.stream(), d.ptr, 37, 8200, 1, 0, 37, [0])
    with pytest.raises(_lib.TomoError, match="not in p"):
        h.load_rows(ctx.stream(), d.ptr, 37, 50, 1, 1, 37, [0])
    h.load_rows(ctx.stream(), d.ptr, 37, 50, 1, 0, 37, [0])
    with pytest.raises(_lib.TomoError, match="not loaded"):
        h.metric(ctx.stream(), [1], [0.0])
    with pytest.raises(_lib.TomoError, match="within"):
        h.metric(ctx.stream(), [0], [51.0])
    m, ms = h.metric(ctx.stream(), [0, 0], [0.0, 0.5], timed=True)
    print("metric %s, pass ms (build, r2c, reduce) %s, plan %.3f s, device bytes %d" % (m, ms, h.plan_seconds(), h.device_bytes()))
    assert np.all(m > 0) and len(ms) == 3 and all(t > 0 for t in ms)
    h.close()
    d.free()


def test_handle_lifetime():
    h = _cor_lib.CorHandle(0)
    assert h.handle and h.device == 0
    h.close()
    h.close()
    with pytest.raises(_lib.TomoError, match="^cor handle closed$"):
        h.handle
    with pytest.raises(_lib.TomoError, match="device out of range"):
        _cor_lib.CorHandle(10**6)
    live = len(_lib.LIVE_CONTEXTS)
    p = rotation_axis.RotationAxis()
    p._ready(None)
    c, hh = p.ctx, p.handle
    assert isinstance(hh, _cor_lib.CorHandle) and hh.handle and c.handle and len(_lib.LIVE_CONTEXTS) == live + 1
    p.close()
    assert p.ctx is None and p.handle is None and len(_lib.LIVE_CONTEXTS) == live
    with pytest.raises(_lib.TomoError, match="handle closed"):
        hh.handle
    p.close()
    given = _lib.Context(0)
    with rotation_axis.RotationAxis(given) as q:
        q._ready(None)
        assert q.ctx is given and q.handle.device == given.device
    assert q.handle is None and q.ctx is given and given.handle
    given.close()
