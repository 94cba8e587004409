"""Test helpers for recon/regularized.py (RegularizedRecon) and its sharded twin: a CPU stand-in backend that adds numpy versions of
the fused passes of csrc/tomo_reg.hip to tests/backends.OracleBackend (the same float32 operation order, float64 sums), the G14 cases
and a small problem the sharded tests share.  Nothing in the product imports this module."""
import os

import numpy as np

from backends import OracleBackend
from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32


def _sq(v):
    v = np.asarray(v, np.float64)
    return float(np.dot(v, v))


def _soft(y, l):
    out = np.zeros_like(y)
    up, dn = y > l, y < -l
    out[up] = y[up] - l
    out[dn] = y[dn] + l
    return out


class RegOracleBackend(OracleBackend):
    """OracleBackend + the RegularizedRecon passes (HipBackend.fista_momentum ... tv_prox_det) in numpy."""

    def _acc(self):
        if not hasattr(self, "_accs"):
            self._accs = np.zeros(16)
        return self._accs

    def fista_momentum(self, rec, u, u_old, c, gt=None, slot=0):
        r = u.a + f32(c) * (u.a - u_old.a)
        rec.a[:] = r
        if gt is not None:
            self._acc()[slot] += _sq(gt.a - r)

    def tikh_grad(self, bp, rec, lam, slot=0):
        g = -bp.a + f32(lam) * rec.a
        bp.a[:] = g
        self._acc()[slot] += _sq(g)
        self._acc()[slot + 1] += _sq(rec.a)

    def trial(self, out, x, d, a, slot=0):
        o = x.a + f32(a) * d.a
        out.a[:] = o
        self._acc()[slot] += _sq(o)

    def clamp_err(self, rec, positivity=False, gt=None, slot=0):
        if positivity:
            rec.a[rec.a < 0.] = 0.
        if gt is not None:
            self._acc()[slot] += _sq(gt.a - rec.a)

    def prox_l1_trial(self, xp, x, g, t, t_lambda, slot=0):
        p = _soft(x.a - f32(t) * g.a, f32(t_lambda))
        G = x.a - p
        xp.a[:] = p
        self._acc()[slot] += float(np.dot(g.a.astype(np.float64), G.astype(np.float64)))
        self._acc()[slot + 1] += _sq(G)

    def prox_l1_momentum(self, out, x0, x1, g, c, a, a_lambda, gt=None, slot=0):
        v = x1.a + f32(c) * (x1.a - x0.a)
        o = _soft(v - f32(a) * g.a, f32(a_lambda))
        out.a[:] = o
        if gt is not None:
            self._acc()[slot] += _sq(gt.a - o)

    def residual_acc(self, out, ax, b, negate=False, slot=0):
        o = b.a - ax.a if negate else ax.a - b.a
        if out is not None:
            out.a[:] = o
        self._acc()[slot] += _sq(o)

    def tv_prox_det(self, im, out, shape, weight=50, niter=200, eps=1.e-5, check_gap_frequency=3):
        r, it, gap = orc.tv_denoise_fista(im.a.reshape(shape), weight=weight, niter=niter, eps=eps, check_gap_frequency=check_gap_frequency,
                                          return_info=True)
        out.a[:] = np.asarray(r, np.float32).ravel()
        return it, gap


# (tag, method, kwargs, ground truth?, warm start?) -- tests/golden/make_golden_g14.py
G14_CASES = [
    ("fista_a", "run_fista", dict(niter=12, hyper=2.e3, beta_tv=0.5, niter_tv=20), False, False),
    ("fista_b", "run_fista", dict(niter=30, hyper=1.e3, beta_tv=20.0, niter_tv=10), True, False),
    ("tikh_a", "run_tikhonov_gd", dict(niter=8, reg_param=1.0, positivity=True), False, False),
    ("tikh_b", "run_tikhonov_gd", dict(niter=30, reg_param=300.0, positivity=True), True, True),
    ("ista_a", "run_lasso_ista", dict(niter=8, reg_param=0.5, alpha0=1.0, beta=0.5), False, False),
    ("ista_b", "run_lasso_ista", dict(niter=30, reg_param=20.0, alpha0=0.05, beta=0.5), True, True),
    ("acc_a", "run_lasso_accelerated", dict(niter=8, reg_param=0.5, alpha0=1.0, beta=0.5), False, False),
    ("acc_b", "run_lasso_accelerated", dict(niter=30, reg_param=20.0, alpha0=0.01, beta=0.8), True, True),
]


def g14_problem():
    """(geometry, b, angles, xyz, ground truth, warm start) of G14: G5's sinogram, 32^3 x 16."""
    from tomography_alignment_amd.utilities.geometry import Geometry
    g5 = np.load(os.path.join(HERE, "golden", "g5_sirt.npz"))
    N, n_proj = 32, 16
    geo = Geometry(n_proj, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2))
    angles = np.array([g5["phi"], g5["alpha"], g5["beta"]]).T
    x = orc.shepp3d(N).astype(np.float32).ravel()
    return geo, g5["b"].copy(), angles, g5["xyz"], x, (0.5 * x).astype(np.float32)


def g14_options(with_gt, warm, x, x0):
    opts = {}
    if with_gt:
        opts["ground_truth"] = x.copy()
    if warm:
        opts["rec"] = x0.copy()
    return opts


# the sharded tests' problem: 16^3, 6 angles, per-angle centre-of-rotation shifts (they must follow their angles)
SHARD_N, SHARD_NPROJ = 16, 6
SHARD_CASES = [
    ("fista", "run_fista", dict(niter=5, hyper=5.e2, beta_tv=2.0, niter_tv=10)),
    ("tikh", "run_tikhonov_gd", dict(niter=5, reg_param=0.5, positivity=True)),
    ("ista", "run_lasso_ista", dict(niter=5, reg_param=0.2, alpha0=1.0, beta=0.5)),
    ("acc", "run_lasso_accelerated", dict(niter=5, reg_param=0.2, alpha0=1.0, beta=0.5)),
]


def shard_problem():
    from tomography_alignment_amd.utilities.geometry import Geometry
    N, n_proj = SHARD_N, SHARD_NPROJ
    rng = np.random.default_rng(14)
    cor = np.zeros((n_proj, 3))
    cor[:, 0] = rng.uniform(-1, 1, n_proj)
    geo = Geometry(n_proj, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2), cor_shift=cor)
    phi = np.linspace(0., np.pi, n_proj, endpoint=False)
    alpha = np.deg2rad(rng.uniform(-1, 1, n_proj))
    beta = np.deg2rad(rng.uniform(-1, 1, n_proj))
    xyz = np.zeros((n_proj, 3))
    xyz[:, 0] = rng.uniform(-1, 1, n_proj)
    x = orc.shepp3d(N).astype(np.float32)
    og = orc.Geo(n_proj, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2), cor_shift=cor)
    b = orc.forward(og, x, alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz).astype(np.float32).reshape(n_proj, -1)
    return geo, b, np.array([phi, alpha, beta]).T, xyz, x.ravel()
