"""recon/regularized.py::RegularizedRecon and recon/regularized_mpi.py on the CPU: the device-resident driver logic run on the numpy
stand-in backend (tests/reg_standin.py) against the reference's own class (golden G14, tests/golden/make_golden_g14.py), the Armijo
restatement against scipy's, the decisions on the reference's defects, and the angle-sharded class over gloo at worlds 1, 2, 3 and one
world larger than the number of angles."""
import numpy as np
import pytest

from conftest import golden, rel_max
from gloo_world import run_world
from reg_standin import (G14_CASES, RegOracleBackend, SHARD_CASES, SHARD_NPROJ, g14_options, g14_problem, shard_problem)


def _serial(geo, b, angles, xyz, opts):
    from tomography_alignment_amd.recon.regularized import RegularizedRecon
    o = dict(opts)
    o["_backend"] = RegOracleBackend(geo)
    return RegularizedRecon(geo, b, angles, xyz, options=o)


@pytest.mark.parametrize("case", G14_CASES, ids=[c[0] for c in G14_CASES])
def test_g14_serial_class_matches_reference_on_stand_in(capsys, case):
    tag, meth, kw, with_gt, warm = case
    g = golden("g14_regularized_solvers")
    geo, b, angles, xyz, x, x0 = g14_problem()
    r = _serial(geo, b, angles, xyz, g14_options(with_gt, warm, x, x0))
    rec, rms = getattr(r, meth)(**kw)
    k = int(g[tag + "_k"])
    assert len(rms) == k, (tag, len(rms), k)
    e = rel_max(rec, g[tag + "_rec"])
    er = float(np.max(np.abs(rms - g[tag + "_rms"]) / g[tag + "_rms"]))
    with capsys.disabled():
        print("\n[G14 stand-in] %s: k %d, rec rel-max %.1e, rms rel %.1e" % (tag, k, e, er))
    assert e < 1e-5 and er < 1e-5, (tag, e, er)
    assert rec.shape == (g[tag + "_rec"].shape if meth == "run_lasso_ista" else (geo.n_vox,)), tag
    if meth == "run_tikhonov_gd":
        assert np.array_equal(r.n_feval, g[tag + "_n_feval"]), (tag, r.n_feval, g[tag + "_n_feval"])
    if meth == "run_lasso_ista":
        assert np.array_equal(r.step_size, g[tag + "_step_size"]), tag
    if tag == "fista_a":
        assert min(r.tv_iters) < kw["niter_tv"], r.tv_iters          # the TV prox's dual-gap stop fires


def test_g14_fixture_covers_its_conditions():
    """A semi-convergence stop before niter, an Armijo search that interpolates, an ISTA search that backtracks."""
    g = golden("g14_regularized_solvers")
    cases = {c[0]: c for c in G14_CASES}
    assert any(int(g[t + "_k"]) < c[2]["niter"] for t, c in cases.items())
    assert any(np.any(g[t + "_n_feval"] > 1) for t, c in cases.items() if c[1] == "run_tikhonov_gd")
    assert any(np.any(g[t + "_step_size"][:int(g[t + "_k"])] < c[2]["alpha0"]) for t, c in cases.items() if c[1] == "run_lasso_ista")


def test_armijo_restatement_matches_scipy():
    from scipy.optimize import _linesearch as sl
    from tomography_alignment_amd.recon.regularized import scalar_search_armijo
    cases = [
        (lambda a: (a - 0.3) ** 2, 0.09, -0.6, 1.0),              # quadratic interpolation
        (lambda a: (a - 0.5) ** 2 + 0.1 * a ** 4, 0.25, -1.0, 1.0),
        (lambda a: np.exp(4 * a) - 5 * a, 1.0, -1.0, 1.0),          # cubic steps
        (lambda a: 1.0 - a + 3 * a ** 3, 1.0, -1.0, 2.0),
        (lambda a: (a - 2.0) ** 2, 4.0, -4.0, 1.0),                # alpha0 accepted
        (lambda a: 1.0 + 1e-3 * a, 1.0, -1.0, 1.0),                # never decreases ...
        (lambda a: 1.0 + 1e-3 * a, 1.0, -1.0, 1.0, 1e-3),          # ... with a floor on alpha: amin reached -> None
    ]
    nones = 0
    for f, p0, d0, a0, *amin in cases:
        amin = amin[0] if amin else 0
        got_n, want_n = [0], [0]

        def fg(a, f=f):
            got_n[0] += 1
            return f(a)

        def fw(a, f=f):
            want_n[0] += 1
            return f(a)
        a, v = scalar_search_armijo(fg, p0, d0, alpha0=a0, amin=amin)
        wa, wv = sl.scalar_search_armijo(fw, p0, d0, alpha0=a0, amin=amin)
        assert (a is None) == (wa is None) and got_n[0] == want_n[0]
        if a is None:
            nones += 1
        else:
            assert a == wa and v == wv
    assert nones == 1


def test_reference_defect_decisions(capsys):
    """The serial stop prints (the reference reads self.my_rank and raises); ISTA returns vox_shape; make_plot is accepted and ignored;
    voxel_mask is stored and ignored, as the reference's projector never receives it."""
    geo, b, angles, xyz, x, x0 = g14_problem()
    r = _serial(geo, b, angles, xyz, {"ground_truth": x})
    rec, rms = r.run_fista(niter=30, hyper=1.e3, beta_tv=20.0, niter_tv=10)
    assert len(rms) < 30 and "semi-convergence criterion reached" in capsys.readouterr().out
    r = _serial(geo, b, angles, xyz, {})
    rec, rms = r.run_lasso_ista(niter=2, reg_param=0.5, make_plot=True)
    assert rec.shape == tuple(geo.vox_shape) and "make_plot is not supported" in capsys.readouterr().out
    mask = np.zeros(geo.n_vox, np.float32)
    mask[: geo.n_vox // 2] = 1.0
    rm = _serial(geo, b, angles, xyz, {"voxel_mask": mask})
    rec_m, rms_m = rm.run_lasso_ista(niter=2, reg_param=0.5)
    assert rm.voxel_mask is mask and np.array_equal(rec_m, rec) and np.array_equal(rms_m, rms)
    for meth in ("run_fista", "run_tikhonov_gd", "run_lasso_accelerated"):
        getattr(_serial(geo, b, angles, xyz, {}), meth)(niter=1, make_plot=True)
    assert capsys.readouterr().out.count("make_plot is not supported") == 3


def test_tikh_f_fp_on_any_operator():
    from scipy import sparse
    from tomography_alignment_amd.recon import regularized
    rng = np.random.default_rng(0)
    A = sparse.random(30, 20, density=0.3, random_state=1, format="csr")
    x, b = rng.standard_normal(20), rng.standard_normal((5, 6))
    r = A.dot(x) - b.ravel()
    assert np.isclose(regularized.my_tikh_f(x, A, b, 0.7), 0.5 * r @ r + 0.35 * x @ x)
    assert np.allclose(regularized.my_tikh_fp(x, A, b, 0.7), A.T.dot(r) + 0.7 * x)


@pytest.mark.parametrize("world", [1, 2, 3, SHARD_NPROJ + 1])
def test_sharded_regularized_matches_unsharded_gloo(tmp_path, world):
    geo, b, angles, xyz, x = shard_problem()
    ranks = run_world("_gloo_reg_worker.py", world, str(tmp_path / "reg"), timeout=600, per_rank=True, env={"OMP_NUM_THREADS": "1"})
    for tag, meth, kw in SHARD_CASES:
        for gt in (False, True):
            key = "%s_%d" % (tag, int(gt))
            r = _serial(geo, b, angles, xyz, {"ground_truth": x} if gt else {})
            rec, rms = getattr(r, meth)(**kw)
            got = ranks[0]
            assert int(got[key + "_k"]) == len(rms), key
            assert rel_max(got[key + "_rec"], rec) < 1e-5, (key, rel_max(got[key + "_rec"], rec))
            assert np.allclose(got[key + "_rms"], rms, rtol=1e-5, atol=0), key
            for other in ranks[1:]:                     # every rank holds the same bits
                for s in ("_rec", "_rms", "_k"):
                    assert np.array_equal(other[key + s], got[key + s]), (key, s)
    # the collectives used return identical bits on every rank
    for other in ranks[1:]:
        assert np.array_equal(other["probe_vol"], ranks[0]["probe_vol"]) and np.array_equal(other["probe_arr"], ranks[0]["probe_arr"])
