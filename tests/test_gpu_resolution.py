"""GPU tests of the Fourier shell correlation (tomography_alignment_amd/resolution.py, libtomo_fsc.so) against the numpy model
tests/fsc_model.py: exact shell counts, the curve at the scale float32 transforms allow, bit-identical repeats, device residency, the
batched 2-D form, the half-set FSC of an alignment problem (one GPU and world 2 over gloo) and the driver's --fsc."""
import numpy as np
import pytest

import fsc_model as fm
from gloo_world import run_world

from tomography_alignment_amd import _fsc_lib, _lib, resolution
from tomography_alignment_amd.examples import align_rigid, generate_data
from tomography_alignment_amd.utilities.generate_phantom import shepp3d
from tomography_alignment_amd.utilities.geometry import Geometry

pytestmark = pytest.mark.gpu

# The admissible difference between the GPU (float32 hipFFT) and the float64 model.  d32 is what float32 transforms cost in the MODEL
# (scipy.fft on float32 input, complex64 throughout, against the float64 run, same inputs), computed by every test for its own inputs.
# hipFFT factors the lengths differently from pocketfft, so the same order is expected, not the same value: K_D32 times d32 is allowed
# (the error constants of float32 FFT algorithms differ by small factors; 16 leaves room for that and for the two results' errors
# adding).  A shell of few coefficients does not average its roundings: a float32 transform of these inputs leaves a relative error of
# up to about 2e-6 on a single coefficient (eps log2(N^3) times the ratio of the input's rms to the rms of the weakest shells), so
# FLOOR / sqrt(count) is allowed on top.  Measured on the MI355X (every test prints its own figures): the GPU is 0.5 to 4.0
# d32 away from the model, at most 0.18 of this bound.
K_D32 = 16.0
FLOOR = 4e-6


@pytest.fixture()
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture()
def res(ctx):
    r = resolution.Resolution(ctx)
    yield r
    r.close()


COUNT_SHAPES = [(32, 32, 32), (64, 64, 64), (96, 96, 96), (128, 128, 128), (64, 48, 80), (33, 64, 31), (24, 32, 20), (64, 32, 128)]


@pytest.mark.parametrize("shape", COUNT_SHAPES)
def test_counts_equal_the_model_exactly(res, shape):
    rng = np.random.default_rng(0)
    a = rng.standard_normal(shape).astype(np.float32)
    c = res.fsc(a, a, mask=None, subtract_mean=False)
    s, w, S = fm.shell_index(shape)
    n = np.bincount(s[s < S], w[s < S], S)
    assert c.count.size == S and np.array_equal(c.count, n)
    if len(set(shape)) == 1:
        assert list(c.count[:4]) == [1, 18, 62, 98]
    # identical inputs: C = PA = PB bit for bit, the curve is exactly 1 wherever there is power
    assert np.array_equal(c.C, c.PA) and np.array_equal(c.PA, c.PB) and np.all(c.fsc[c.PA > 0] == 1.0)


@pytest.mark.parametrize("shape", [(24, 40), (33, 31), (64, 64), (48, 20)])
def test_ring_counts_equal_the_model_exactly(res, shape):
    a = np.random.default_rng(1).standard_normal((3,) + shape).astype(np.float32)
    curves = res.frc(a, a, mask=None, subtract_mean=False)
    s, w, S = fm.shell_index(shape)
    n = np.bincount(s[s < S], w[s < S], S)
    assert len(curves) == 3
    for c in curves:
        assert np.array_equal(c.count, n)


def _compare(tag, got, a, b, **kw):
    """Assert the GPU curve `got` against the model of the same inputs at the d32 scale, print both; returns the model's FSCCurve."""
    C, PA, PB, n = fm.sums(a, b, **kw)
    C32, PA32, PB32, _ = fm.sums(a, b, dtype=np.float32, **kw)
    f, f32 = fm.curve(C, PA, PB), fm.curve(C32, PA32, PB32)
    live = PA * PB > 0
    live[0] = live[0] and not kw.get("subtract_mean", True)        # shell 0 of mean-free inputs is rounding noise over rounding noise
    d32 = float(np.max(np.abs(f32 - f)[live]))
    den = np.sqrt(PA * PB)
    d32_sums = max(float(np.max((np.abs(x32 - x) / np.where(live, den, 1.0))[live])) for x32, x in ((C32, C), (PA32, PA), (PB32, PB)))
    assert np.array_equal(got.count, n)
    tol = K_D32 * d32 + FLOOR / np.sqrt(np.maximum(n, 1.0))
    tol_sums = K_D32 * d32_sums + FLOOR / np.sqrt(np.maximum(n, 1.0))
    dc = np.abs(got.fsc - f)
    ds = np.max([np.abs(x_g - x) / np.where(live, den, 1.0) for x_g, x in ((got.C, C), (got.PA, PA), (got.PB, PB))], axis=0)
    print("%s: d32 curve %.2e sums %.2e | GPU - model: curve %.2e (%.1f x d32), sums %.2e (%.1f x d32); largest fraction of the bound: "
          "curve %.3f, sums %.3f" % (tag, d32, d32_sums, dc[live].max(), dc[live].max() / d32, ds[live].max(), ds[live].max() / d32_sums,
                                     (dc / tol)[live].max(), (ds / tol_sums)[live].max()))
    assert np.all(dc[live] <= tol[live])
    assert np.all(ds[live] <= tol_sums[live])
    return resolution.FSCCurve(C, PA, PB, n, got.nmax)


@pytest.mark.parametrize("sigma", [0.02, 0.5])
@pytest.mark.parametrize("masked", [True, False])
def test_curve_equals_the_model_on_a_noisy_phantom(res, sigma, masked):
    N = 128
    rng = np.random.default_rng(11)
    x = shepp3d(N).astype(np.float64)
    a = (x + sigma * rng.standard_normal(x.shape)).astype(np.float32)
    b = (x + sigma * rng.standard_normal(x.shape)).astype(np.float32)
    kw = dict(mask="sphere" if masked else None, subtract_mean=masked)
    got = res.fsc(a, b, **kw)
    model = _compare("shepp %d sigma %.2f %s" % (N, sigma, "masked" if masked else "unmasked"), got, a, b, **kw)
    sm, status_m = model.crossing("0.143")
    sg, status_g = got.crossing("0.143")
    assert status_g == status_m
    if sigma == 0.02:
        print("    the curve stays at or above %.3f" % model.fsc[1:].min())
        assert model.fsc[1:].min() > 0.85 and status_m == "none"
    else:
        # the crossing case: well inside the band on the model, and the two interpolated crossings agree to a fraction of a shell
        assert status_m == "crossed" and sm < 0.8 * (model.fsc.size - 1)
        print("    0.143 crossing: model shell %.6f, GPU shell %.6f, difference %.2e shells" % (sm, sg, abs(sg - sm)))
        assert abs(sg - sm) < 1e-3
        assert abs(got.resolution("0.143") - model.resolution("0.143")) < 1e-3 * model.resolution("0.143")


def test_non_cubic_masked_volume_and_a_mask_array(res, ctx):
    shape = (64, 48, 80)
    rng = np.random.default_rng(12)
    sgn = rng.standard_normal(shape)
    a = (sgn + rng.standard_normal(shape)).astype(np.float32)
    b = (sgn + rng.standard_normal(shape)).astype(np.float32)
    _compare("noise (64, 48, 80) sphere", res.fsc(a, b), a, b)
    _compare("noise (64, 48, 80) sphere R 15 E 3", res.fsc(a, b, radius=15, edge=3), a, b, radius=15, edge=3)
    m = rng.random(shape).astype(np.float32)
    _compare("noise (64, 48, 80) mask array", res.fsc(a, b, mask=m), a, b, mask=m)
    d_m = ctx.to_device(m)
    _compare("noise (64, 48, 80) device mask array", res.fsc(a, b, mask=d_m), a, b, mask=m)
    c = res.fsc(a, b, voxel_size=0.5)
    assert np.allclose(c.freq, np.arange(c.fsc.size) / (80 * 0.5))


def test_sums_are_deterministic(res, ctx):
    rng = np.random.default_rng(13)
    shape = (96, 64, 72)
    a, b = (ctx.to_device(rng.standard_normal(shape).astype(np.float32)) for _ in range(2))
    other = ctx.to_device((100 * rng.standard_normal((64, 64, 64))).astype(np.float32))
    t0 = res.shell_sums(a, b, 3)
    t1 = res.shell_sums(a, b, 3)
    assert np.array_equal(t0, t1)
    res.shell_sums(other, other, 3)                       # other data, another shape: stale accumulators or partial tables would show
    res.shell_sums(b, a, 3, mask=None)
    t2 = res.shell_sums(a, b, 3)
    assert np.array_equal(t0, t2)
    with resolution.Resolution(ctx) as fresh:             # and a handle that has seen nothing else
        assert np.array_equal(fresh.shell_sums(a, b, 3), t0)
    s0 = res.shell_sums(a, b, 2, shape=(96 * 64 // 8, 8, 72))
    assert np.array_equal(s0, res.shell_sums(a, b, 2, shape=(96 * 64 // 8, 8, 72)))


def test_device_residency_and_no_leaks(res, ctx):
    rng = np.random.default_rng(14)
    shape = (32, 40, 48)
    a, b = rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    d_a, d_b = ctx.to_device(a), ctx.to_device(b)
    flat_a = ctx.to_device(a.ravel())                     # a flat buffer, such as a solver's d_rec: needs `shape`
    before = len(ctx._arrays)
    downloads = []
    orig = _lib.DeviceArray.download
    _lib.DeviceArray.download = lambda self, out=None: (downloads.append(self.nbytes), orig(self, out))[1]
    try:
        c_dev = res.fsc(d_a, d_b)
        c_flat = res.fsc(flat_a, d_b, shape=shape)
    finally:
        _lib.DeviceArray.download = orig
    assert downloads == []                                # nothing volume-sized comes back: only the shell table, through fetch()
    assert len(ctx._arrays) == before                     # and no buffer of the context's is left behind
    c_host = res.fsc(a, b)
    assert len(ctx._arrays) == before
    for c in (c_flat, c_host):
        assert np.array_equal(c.C, c_dev.C) and np.array_equal(c.PA, c_dev.PA) and np.array_equal(c.PB, c_dev.PB)
    assert np.array_equal(d_a.download(), a) and np.array_equal(d_b.download(), b)          # the inputs are not written
    bytes_one = res.device_bytes()
    assert bytes_one >= 2 * 8 * 32 * 40 * 25
    plan_seconds = res.handle.plan_seconds()
    res.fsc(d_a, d_b)
    assert res.device_bytes() == bytes_one                # the plan and the buffers are reused
    assert plan_seconds > 0.0 and res.handle.plan_seconds() == plan_seconds
    c_own = resolution.fsc(a, b)                          # a handle and a context of its own, closed again
    assert np.array_equal(c_own.C, c_dev.C)
    with pytest.raises(ValueError):
        res.fsc(flat_a, d_b)
    rows = res.take_rows(d_a, 40 * 48, 1, 2, 16)
    assert np.array_equal(rows.download().reshape(16, 40, 48), a[1::2])
    rows.free()
    with pytest.raises(ValueError):
        res.take_rows(d_a, 40 * 48, 1, 2, 17)


def test_frc_equals_the_per_plane_model(res):
    rng = np.random.default_rng(15)
    for shape in ((5, 48, 64), (4, 33, 31)):
        sgn = rng.standard_normal(shape)
        a = (sgn + 0.7 * rng.standard_normal(shape)).astype(np.float32)
        b = (sgn + 0.7 * rng.standard_normal(shape)).astype(np.float32)
        curves = res.frc(a, b)
        models = [_compare("frc %s plane %d" % (shape, i), curves[i], a[i], b[i]) for i in range(shape[0])]
        pooled = res.frc(a, b, pool=True)
        pm = resolution.pool_curves(models)
        assert np.array_equal(pooled.count, pm.count)
        assert np.array_equal(pooled.C, sum(c.C for c in curves))
        d = np.abs(pooled.fsc - pm.fsc)[1:].max()
        print("frc %s pooled: GPU - model %.2e" % (shape, d))
        assert d < 1e-6
        m = rng.random(shape[1:]).astype(np.float32)
        c1 = res.frc(a, b, mask=m, subtract_mean=False)[1]
        _compare("frc %s plane 1, mask array" % (shape,), c1, a[1], b[1], mask=m, subtract_mean=False)


def test_unsupported_shapes_raise_before_any_launch(ctx):
    r = resolution.Resolution(ctx)
    before = len(ctx._arrays)
    one = np.zeros((8, 1, 8), np.float32)
    with pytest.raises(resolution.FscUnsupported):
        r.fsc(one, one)
    with pytest.raises(resolution.FscUnsupported):
        r.frc(np.zeros((2, 1, 8), np.float32), np.zeros((2, 1, 8), np.float32))
    with pytest.raises(resolution.FscUnsupported):
        _fsc_lib.n_shells(3, 1, _fsc_lib.MAX_N + 1, 8, 8)
    with pytest.raises(resolution.FscUnsupported):
        _fsc_lib.n_shells(2, _fsc_lib.MAX_PLANES + 1, 8, 1, 8)
    assert r.handle is None and len(ctx._arrays) == before            # refused before a handle was made or anything uploaded
    with _fsc_lib.FscHandle(ctx.device) as h:
        with pytest.raises(resolution.FscUnsupported):
            h.set_shape(3, 1, 8, 8, 1)
        assert h.device_bytes() == 0
        with pytest.raises(_lib.TomoError):
            h.reduce(ctx.stream())                                     # no shape set: an error, not a launch


def _refbp_tol(PA, count, n_vox):
    """How far two curves may differ whose half-set FBPs differ by the order of float32 sums (the tilted adjoint adds with atomics, the
    sharded FBP adds the ranks' volumes): tests/test_gpu_fbp.py bounds that at 1e-6 of the largest voxel, below 2e-6 in absolute terms for
    a phantom of values <= 1.  A white perturbation of that size puts at most 2e-6 sqrt(n_vox) on a coefficient, i.e. eps_s = 2e-6
    sqrt(n_vox count_s / PA_s) relative to the shell's rms amplitude; C, PA and PB each move by about sqrt(2) eps_s / sqrt(count_s / 2)
    relative to the shell's power, and 4 standard deviations of that are allowed, plus the floor of single coefficients."""
    return 8 * np.sqrt(2) * 2e-6 * np.sqrt(n_vox / np.maximum(PA, 1e-300)) + FLOOR / np.sqrt(np.maximum(count, 1.0))


def _half_set_problem():
    d = generate_data.make(64, 90, seed=3)
    n = d["phi"].size
    geo = Geometry(n, np.array([64, 64, 64]), np.ones(3), np.array([64, 64]), np.ones(2))
    true = (np.array([d["phi"], d["alpha"], d["beta"]]).T, d["xyz"])
    nominal = (np.array([d["phi"], np.zeros(n), np.zeros(n)]).T, np.zeros((n, 3)))
    return d, geo, true, nominal


def test_half_set_fsc_tells_true_poses_from_uncorrected_ones():
    """Uniform +-2 px shifts (sigma 1.15 px) left uncorrected decorrelate the halves as exp(-4 pi^2 sigma^2 f^2): below the half-bit
    curve (about 0.2) from f = 0.17 / px, a resolution near 6 px; with the true poses the halves differ by the angular sampling of 45
    projections only (Crowther: pi D / 45 = 3.6 px at most).  A ratio of at least 1.25 is asked; the measured values are printed."""
    d, geo, true, nominal = _half_set_problem()
    c_true = resolution.half_set_fsc(geo, d["projections"], true[0], true[1])
    c_nom = resolution.half_set_fsc(geo, d["projections"], nominal[0], nominal[1])
    r_true = c_true.resolution() or c_true.nyquist
    r_nom = c_nom.resolution()
    print("half-set FSC 64^3, 90 projections: half-bit resolution %.2f px (%s) with the true poses, %s px (%s) with the poses uncorrected"
          % (r_true, c_true.crossing()[1], "%.2f" % r_nom if r_nom else "none", c_nom.crossing()[1]))
    assert r_nom is not None and r_nom > 1.25 * r_true
    # device-resident rows give the same curve (up to the order of the tilted adjoint's float32 sums), and SIRT halves run too
    ctx = _lib.Context()
    d_p = ctx.to_device(np.asarray(d["projections"], np.float32).ravel())
    c_dev = resolution.half_set_fsc(geo, d_p, true[0], true[1])
    dlt, tol = np.abs(c_dev.fsc - c_true.fsc)[1:], _refbp_tol(c_true.PA, c_true.count, 64 ** 3)[1:]
    print("    device rows against host rows: curve difference %.2e (largest fraction of the bound %.3f)" % (dlt.max(), (dlt / tol).max()))
    assert np.array_equal(c_dev.count, c_true.count) and np.all(dlt <= tol)
    assert np.array_equal(d_p.download(), np.asarray(d["projections"], np.float32).ravel())
    c_sirt = resolution.half_set_fsc(geo, d["projections"], true[0], true[1], method="sirt", niter=5)
    assert np.all(np.isfinite(c_sirt.fsc)) and c_sirt.fsc[1:8].min() > 0.5
    with pytest.raises(ValueError):
        resolution.half_set_fsc(geo, d["projections"], true[0], true[1], method="sirt")
    ctx.close()


def test_half_set_fsc_world_2_on_one_gpu(tmp_path):
    """World 2 sums each half's volume over the ranks in float32 (tests/test_gpu_fbp.py: 1e-6 rel_max against world 1), so the curves
    agree at the scale of those roundings averaged over a shell (_refbp_tol)."""
    one = run_world("_gloo_gpu_fsc_worker.py", 1, str(tmp_path / "w1"), timeout=300, per_rank=True)[0]
    two = run_world("_gloo_gpu_fsc_worker.py", 2, str(tmp_path / "w2"), timeout=300, per_rank=True)
    assert np.array_equal(two[0]["table"], two[1]["table"])            # both ranks hold the same all-reduced volumes: the same bits
    for key in ("host", "device"):
        for r in range(2):
            assert np.array_equal(two[r][key + "_count"], one[key + "_count"])
            dlt = np.abs(two[r][key + "_fsc"] - one[key + "_fsc"])[1:]
            tol = _refbp_tol(one[key + "_PA"], one[key + "_count"], 64 ** 3)[1:]
            print("half-set FSC (%s rows), world 2 rank %d vs world 1: curve difference %.2e (largest fraction of the bound %.3f)"
                  % (key, r, dlt.max(), (dlt / tol).max()))
            assert np.all(dlt <= tol)
    dlt = np.abs(one["host_fsc"] - one["device_fsc"])[1:]
    assert np.all(dlt <= _refbp_tol(one["host_PA"], one["host_count"], 64 ** 3)[1:])


TODAYS_KEYS = {"outer", "rmse", "sirt_iterations", "residual", "launches", "evals", "driver", "sirt_wall_s", "align_wall_s", "ranks"}


def test_driver_reports_a_resolution_without_a_phantom():
    d = generate_data.make(48, 60, seed=2)
    data = {"projections": d["projections"], "phi": d["phi"]}           # measured data: no phantom, no true poses
    out = align_rigid.run(dict(data), n_outer=2, sirt_iters=10, verbose=False, fsc=True, download=False)
    assert out[0] is None and len(out[4]) == 2
    for h in out[4]:
        assert set(h) == TODAYS_KEYS | {"fsc_resolution", "fsc_curve"}
        assert np.isfinite(h["fsc_resolution"]) and 2.0 <= h["fsc_resolution"] <= 48.0
        assert isinstance(h["fsc_curve"], resolution.FSCCurve)
    print("align_rigid --fsc, 48^3, 60 projections: half-bit resolution per outer iteration %s px"
          % ", ".join("%.2f" % h["fsc_resolution"] for h in out[4]))
    plain = align_rigid.run(dict(data), n_outer=1, sirt_iters=10, verbose=False, download=False)
    assert set(plain[4][0]) == TODAYS_KEYS
    multi = align_rigid.run_multires(dict(data), levels=2, n_outer=1, sirt_iters=10, verbose=False, download=False, fsc=True)
    assert [h["factor"] for h in multi[4]] == [2, 1]
    for h in multi[4]:
        assert set(h) == TODAYS_KEYS | {"fsc_resolution", "fsc_curve", "level", "factor"}
        assert np.isfinite(h["fsc_resolution"]) and 2.0 * h["factor"] <= h["fsc_resolution"] <= 48.0
    assert set(align_rigid.run_multires(dict(data), levels=2, n_outer=1, sirt_iters=5, verbose=False, download=False)[4][0]) == \
        TODAYS_KEYS | {"level", "factor"}
