"""CPU tests of tomography_alignment_amd/multires.py and examples/align_rigid.run_multires: the numpy models (tests/pyr_model.py), the
level convention, argument validation before the library is touched, and the driver's bookkeeping on the oracle-backed stand-in backend
with the device operations replaced by the models."""
import numpy as np
import pytest

import abi
import pyr_model as pm
from backends import OracleBackend

from tomography_alignment_amd import _pyr_lib, alignment, multires
from tomography_alignment_amd.examples import align_rigid
from tomography_alignment_amd.utilities.geometry import Geometry


def test_binning_model_is_the_scaled_float64_sum_of_a_bin():
    rng = np.random.default_rng(0)
    x = (rng.integers(1, 2 ** 14, (3, 8, 16)) / 2 ** 10).astype(np.float32)
    for f in (2, 4, 8):
        b = pm.bin_sino(x, f)
        assert b.shape == (3, 8 // f, 16 // f) and b.dtype == np.float32
        assert b[1, 0, 1] == np.float32(x[1, :f, f:2 * f].astype(np.float64).sum() * (float(np.float32(1.0 / f)) / (f * f)))
        # 14 significant bits between 2^-10 and 2^4: the float64 sum of a bin is exact, so any order of summation gives the same value
        perm = rng.permutation(f * f)
        s = x[:, :f, :f].reshape(3, -1).astype(np.float64)
        assert np.array_equal(np.add.reduce(s[:, perm], axis=1), s.sum(axis=1))
    v = rng.standard_normal((8, 16, 24)).astype(np.float32)
    assert np.allclose(pm.bin_vol(v, 2)[1, 2, 3], v[2:4, 4:6, 6:8].mean(), rtol=1e-6)
    assert np.array_equal(pm.bin_vol(v, 4, scale=2.0), (pm.bin_vol(v, 4).astype(np.float64) * 2).astype(np.float32))


def test_prolongation_model():
    const = pm.prolong(np.full((3, 4, 5), 2.5))
    assert const.shape == (6, 8, 10) and np.array_equal(const, np.full((6, 8, 10), 2.5))
    # linear in the index: coarse cell I has its centre at fine coordinate 2 I + 0.5, so the ramp a I is a (i - 0.5) / 2 on the fine grid
    I, J, K = np.meshgrid(np.arange(6.), np.arange(5.), np.arange(7.), indexing="ij")
    fine = pm.prolong(1.5 * I - 2.0 * J + 0.25 * K + 3.0)
    i, j, k = np.meshgrid(np.arange(12.), np.arange(10.), np.arange(14.), indexing="ij")
    want = 1.5 * (i - 0.5) / 2 - 2.0 * (j - 0.5) / 2 + 0.25 * (k - 0.5) / 2 + 3.0
    assert np.allclose(fine[1:-1, 1:-1, 1:-1], want[1:-1, 1:-1, 1:-1], rtol=0, atol=1e-12)
    assert fine[0, 3, 3] == fine[1, 3, 3] - 0.25 * 1.5 and not np.isclose(fine[0, 3, 3], want[0, 3, 3])      # the face is clamped
    # the outermost fine cell copies its coarse cell
    v = np.random.default_rng(1).standard_normal((4, 3, 5))
    p = pm.prolong(v)
    assert p[0, 0, 0] == v[0, 0, 0] and p[-1, -1, -1] == v[-1, -1, -1]
    # The 3/4, 1/4 weights of the two fine cells of a coarse cell average back to the cell's value plus (left - 2 centre + right) / 8 per
    # axis: bin(prolong(v)) == v away from the faces wherever that second difference vanishes, i.e. on any volume linear in the index.
    lin = (0.5 * I - 0.25 * J + 2.0 * K + 1.0).astype(np.float32)
    back = pm.bin_vol(pm.prolong(lin).astype(np.float32), 2)
    assert np.max(np.abs(back[1:-1, 1:-1, 1:-1] - lin[1:-1, 1:-1, 1:-1])) <= 4 * np.finfo(np.float32).eps * np.abs(lin).max()
    # on a general volume it is the (1/8, 3/4, 1/8) smoothing along each axis, the index clamped
    sm = v.copy()
    for axis in range(3):
        n_ax = sm.shape[axis]
        lo, hi = np.take(sm, np.clip(np.arange(n_ax) - 1, 0, n_ax - 1), axis=axis), np.take(sm, np.clip(np.arange(n_ax) + 1, 0, n_ax - 1), axis=axis)
        sm = 0.75 * sm + 0.125 * (lo + hi)
    assert np.allclose(pm.prolong(v).reshape(4, 2, 3, 2, 5, 2).mean(axis=(1, 3, 5)), sm, rtol=0, atol=1e-12)


@pytest.mark.parametrize("N", [64, 96, 128])
@pytest.mark.parametrize("f", [2, 4, 8])
def test_level_convention_unit_pitch_centres_are_the_bin_centres(N, f):
    full = Geometry(2, np.array([N] * 3), np.ones(3), np.array([N, N]), np.ones(2))
    lvl = multires.level_geometry(2, (N, N, N), f)
    assert list(lvl.vox_shape) == [N // f] * 3 and list(lvl.det_shape) == [N // f] * 2
    assert np.all(np.asarray(lvl.vox_pix) == 1) and np.all(np.asarray(lvl.det_pix) == 1)
    for a in range(3):
        assert np.array_equal(f * lvl._axes[a], full._axes[a].reshape(-1, f).mean(axis=1))
    M = N // f
    xd_full = full.source_centers[0].reshape(N, N)[:, 0]
    zd_full = full.source_centers[2].reshape(N, N)[0]
    assert np.array_equal(f * lvl.source_centers[0].reshape(M, M)[:, 0], xd_full.reshape(-1, f).mean(axis=1))
    assert np.array_equal(f * lvl.source_centers[2].reshape(M, M)[0], zd_full.reshape(-1, f).mean(axis=1))
    # ... which "N / f cells of pitch f" misses by 0.5 (f - 1) full-size pixels
    pitch = Geometry(2, np.array([M] * 3), f * np.ones(3), np.array([M, M]), f * np.ones(2))
    assert np.allclose(pitch._axes[0] - full._axes[0].reshape(-1, f).mean(axis=1), -0.5 * (f - 1))


def test_the_largest_factor_is_the_headers():
    assert max(_pyr_lib.FACTORS) == _pyr_lib.MAX_FACTOR == abi.parse_header(abi.header_path("pyr")).constants["TOMO_PYR_MAX_FACTOR"]


def test_arguments_are_checked_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("the library must not be loaded for an argument error")
    monkeypatch.setattr(_pyr_lib, "load", no_load)
    s, v = np.zeros((2, 8, 12), np.float32), np.zeros((8, 12, 16), np.float32)
    with pytest.raises(ValueError, match="does not divide"):
        multires.bin_projections(s, 8)                       # 12 % 8
    with pytest.raises(ValueError, match="does not divide"):
        multires.bin_volume(np.zeros((8, 12, 18), np.float32), 4)
    for f in (1, 3, 16, 2.5, True):
        with pytest.raises(ValueError, match="2, 4 or 8"):
            multires.bin_projections(s, f)
    with pytest.raises(ValueError, match="dimensions"):
        multires.bin_projections(s[0], 2)
    with pytest.raises(ValueError, match="dimensions"):
        multires.prolong_volume(v.ravel())
    with pytest.raises(ValueError, match="values"):
        multires.bin_volume(v, 2, shape=(8, 12, 8))
    with pytest.raises(ValueError, match="finite"):
        multires.bin_volume(v, 2, scale=np.inf)
    with pytest.raises(ValueError, match="empty"):
        multires.bin_projections(np.zeros((0, 8, 8), np.float32), 2)
    with pytest.raises(ValueError, match="out must be"):
        multires.prolong_volume(v, out=np.zeros(8 * v.size, np.float32))
    with pytest.raises(ValueError, match="divisible by 4"):
        align_rigid.run_multires(dict(projections=np.zeros((3, 8, 10), np.float32), phi=np.zeros(3)), levels=3)
    with pytest.raises(ValueError, match="one entry per level"):
        align_rigid.run_multires(dict(projections=np.zeros((3, 8, 8), np.float32), phi=np.zeros(3)), levels=2)       # n_outer has 3
    with pytest.raises(ValueError, match="levels must be"):
        align_rigid.run_multires(dict(projections=np.zeros((3, 8, 8), np.float32), phi=np.zeros(3)), levels=5, n_outer=1)


def _problem(N=16, n=6, seed=7):
    from oracle import oracle as orc
    rng = np.random.default_rng(seed)
    x = np.zeros((N, N, N), np.float32)
    x[4:12, 5:11, 3:13] = rng.uniform(0.2, 1.0, (8, 6, 10)).astype(np.float32)
    phi = np.linspace(0.2, 2.9, n)
    alpha, beta = np.deg2rad(rng.uniform(-0.8, 0.8, n)), np.deg2rad(rng.uniform(-0.8, 0.8, n))
    xyz = np.zeros((n, 3))
    xyz[:, 0], xyz[:, 2] = rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n)
    og = orc.Geo(n, np.array([N] * 3), np.ones(3), np.array([N, N]), np.ones(2))
    b = orc.forward(og, x, alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz).astype(np.float32).reshape(n, N, N)
    return dict(projections=b, phi=phi, phantom=x, xyz=xyz, alpha=alpha, beta=beta)


def test_run_multires_levels_1_is_run(monkeypatch):
    seen = {}

    def fake_run(data, n_outer, sirt_iters, **kw):
        seen.update(kw, n_outer=n_outer, sirt_iters=sirt_iters)
        return ("rec", "a", "b", "xyz", [{"outer": 0}, {"outer": 1}])
    monkeypatch.setattr(align_rigid, "run", fake_run)
    out = align_rigid.run_multires({"phi": np.zeros(2)}, levels=1, n_outer=2, sirt_iters=7, init="fbp", verbose=False)
    assert out[:4] == ("rec", "a", "b", "xyz") and seen["n_outer"] == 2 and seen["sirt_iters"] == 7 and seen["init"] == "fbp"
    assert out[4] == [{"outer": 0, "level": 0, "factor": 1}, {"outer": 1, "level": 0, "factor": 1}]


def test_run_multires_bookkeeping_on_the_stand_in_backend(monkeypatch):
    """Three levels at 16^3 on the oracle backend, the device operations replaced by their models: level order, what is binned from what,
    x2 on the carried translations and none on the tilts, estimate = base + increment within the bounds, per-level n_outer / sirt_iters."""
    data = _problem()
    n = data["phi"].size
    passes = []
    real = alignment.align_projections

    def spy(backend, rec, projections, phi, **kw):
        res = real(backend, rec, projections, phi, **kw)
        passes.append(dict(n_det=backend.n_det, xyz0=None if kw.get("xyz0") is None else np.array(kw["xyz0"]),
                           angles0=None if kw.get("angles0") is None else np.array(kw["angles0"]), x=res["x"].copy(), bounds=kw["bounds"]))
        return res
    monkeypatch.setattr(alignment, "align_projections", spy)
    iters = []
    real_rec = align_rigid.OuterLoop.reconstruct

    def rec_spy(self, sirt_iters=50, positivity=True, init="zero"):
        iters.append((self.factor, sirt_iters, init, self.d_rec is not None))
        return real_rec(self, sirt_iters, positivity, init)
    monkeypatch.setattr(align_rigid.OuterLoop, "reconstruct", rec_spy)
    pyr = pm.HostPyramid()
    rec, a, b, xyz, hist, loop = align_rigid.run_multires(data, levels=3, n_outer=(2, 1, 2), sirt_iters=(4, 3, 2), verbose=False,
                                                          backend_factory=OracleBackend, pyramid=pyr, return_loop=True)
    assert [(h["level"], h["factor"], h["outer"]) for h in hist] == [(0, 4, 0), (0, 4, 1), (1, 2, 2), (2, 1, 3), (2, 1, 4)]
    assert iters == [(4, 4, "zero", False), (4, 4, "zero", True), (2, 3, "zero", True), (1, 2, "zero", True), (1, 2, "zero", True)]
    # every level's data come from the FULL-SIZE buffers; the reconstruction is prolonged level to level
    assert pyr.calls == [("bin_projections", 4, (n, 16, 16)), ("bin_volume", 4, (16, 16, 16)), ("prolong_volume", 2, (4, 4, 4)),
                         ("bin_projections", 2, (n, 16, 16)), ("bin_volume", 2, (16, 16, 16)), ("prolong_volume", 2, (8, 8, 8))]
    assert [p["n_det"] for p in passes] == [16, 16, 64, 256, 256] and rec.shape == (16, 16, 16)
    assert passes[0]["xyz0"] is None and passes[1]["xyz0"] is None                 # the coarsest level is today's loop on binned data
    est4 = passes[1]["x"]                                                          # the coarsest level's estimate (tx, tz, alpha, beta)
    base2 = passes[2]
    assert np.array_equal(base2["xyz0"][:, [0, 2]], 2.0 * est4[:, :2]) and np.all(base2["xyz0"][:, 1] == 0)
    assert np.array_equal(base2["angles0"], np.column_stack([data["phi"], est4[:, 2], est4[:, 3]]))
    est2 = np.column_stack([base2["xyz0"][:, 0], base2["xyz0"][:, 2], base2["angles0"][:, 1], base2["angles0"][:, 2]]) + base2["x"]
    for p in passes[3:]:                                                           # both passes of the finest level search around the SAME base
        assert np.array_equal(p["xyz0"][:, [0, 2]], 2.0 * est2[:, :2]) and np.array_equal(p["angles0"][:, 1:], est2[:, 2:])
    last = passes[-1]
    assert np.array_equal(xyz[:, [0, 2]], last["xyz0"][:, [0, 2]] + last["x"][:, :2])
    assert np.array_equal(a, last["angles0"][:, 1] + last["x"][:, 2]) and np.array_equal(b, last["angles0"][:, 2] + last["x"][:, 3])
    for p in passes:
        assert p["bounds"] == align_rigid.DEFAULT_BOUNDS
        lo, hi = np.array(p["bounds"]).T
        assert np.all(p["x"] >= lo) and np.all(p["x"] <= hi)
    # pose errors are in full-size pixels at every level
    e0 = np.abs(4 * passes[0]["x"][:, :2] - data["xyz"][:, [0, 2]]).mean()
    assert hist[0]["shift_err_px"] == pytest.approx(e0, rel=1e-12) and loop.factor == 1
    assert hist[-1]["shift_err_px"] == pytest.approx(np.abs(xyz[:, [0, 2]] - data["xyz"][:, [0, 2]]).mean(), rel=1e-12)


def test_outer_loop_defaults_leave_the_plain_loop_as_it_is(monkeypatch):
    data = _problem(n=4)
    seen = []
    real = alignment.align_projections

    def spy(backend, rec, projections, phi, **kw):
        seen.append(sorted(kw))
        return real(backend, rec, projections, phi, **kw)
    monkeypatch.setattr(alignment, "align_projections", spy)
    geo = Geometry(4, np.array([16] * 3), np.ones(3), np.array([16, 16]), np.ones(2))
    out = align_rigid.run(data, n_outer=1, sirt_iters=2, verbose=False, backend=OracleBackend(geo))
    assert seen == [["bounds", "indices", "letters"]]                              # no base pose reaches the optimiser
    assert "level" not in out[4][0] and set(out[4][0]) >= {"outer", "rmse", "shift_err_px", "tilt_err_deg"}
    with pytest.raises(ValueError, match="base must be"):
        align_rigid.OuterLoop(data, backend=OracleBackend(geo), base=(np.zeros((3, 3)), np.zeros(4), np.zeros(4)))
