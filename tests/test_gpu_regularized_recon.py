"""recon/regularized.py::RegularizedRecon and recon/regularized_mpi.py on the GPU: the reference's own results (golden G14) through
HipBackend, the fused passes of csrc/tomo_reg.hip against numpy (sizes, alignments, bit-reproducible sums), tomo_tv_prox_det against
tomo_tv_denoise_fista, world 2 on one GPU, a 1-rank RCCL run, examples/mpi_reconstruct.py and a 256^3 x 256 TV-FISTA run."""
import os

import numpy as np
import pytest

from conftest import golden, rel_max
from gloo_world import run_world
from reg_standin import G14_CASES, SHARD_CASES, g14_options, g14_problem, shard_problem

pytestmark = pytest.mark.gpu


def test_g14_through_hip_backend(capsys):
    from tomography_alignment_amd.recon.regularized import RegularizedRecon
    g = golden("g14_regularized_solvers")
    geo, b, angles, xyz, x, x0 = g14_problem()
    lines = []
    for tag, meth, kw, with_gt, warm in G14_CASES:
        r = RegularizedRecon(geo, b, angles, xyz, options=g14_options(with_gt, warm, x, x0))
        rec, rms = getattr(r, meth)(**kw)
        assert len(rms) == int(g[tag + "_k"]), (tag, len(rms))
        e = rel_max(rec, g[tag + "_rec"])
        er = float(np.max(np.abs(rms - g[tag + "_rms"]) / g[tag + "_rms"]))
        lines.append("%s %.1e/%.1e" % (tag, e, er))
        assert rec.dtype == np.float32 and e < 1e-5 and er < 1e-5, (tag, e, er)
        if meth == "run_tikhonov_gd":
            assert np.array_equal(r.n_feval, g[tag + "_n_feval"]), tag
        if meth == "run_lasso_ista":
            assert rec.shape == tuple(geo.vox_shape) and np.array_equal(r.step_size, g[tag + "_step_size"]), tag
    with capsys.disabled():
        print("\n[G14 HIP] rec / rms rel-max: " + ", ".join(lines))


def _soft(y, l):
    out = np.zeros_like(y)
    out[y > l] = y[y > l] - l
    out[y < -l] = y[y < -l] + l
    return out


def _d(v):
    return np.asarray(v, np.float64)


@pytest.mark.parametrize("n", [0, 1, 255, 257, 10 ** 7 + 3])
def test_fused_passes_vs_numpy(n):
    """Each pass: float32 outputs bit-equal to numpy's float32 expression (the kernels use no contraction), float64 sums to 1e-12 of
    numpy's float64 sums, and the sums bit-identical over two calls -- aligned operands, operands one float off a 16-byte boundary
    (head / float4 body / tail), and operands of mixed offsets (scalar path)."""
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    ctx = _lib.Context()
    be = HipBackend.__new__(HipBackend)
    be.ctx, be.lib = ctx, ctx.lib
    rng = np.random.default_rng(n % 1000)
    f32 = np.float32
    host = {k: rng.standard_normal(n).astype(f32) for k in ("a", "b", "c", "d")}
    c, al, lam = 0.37, 0.021, 0.6
    for layout in ("aligned", "offset", "mixed"):
        def put(k, i):
            off = 0 if layout == "aligned" else (1 if layout == "offset" else i % 3)
            base = ctx.to_device(np.concatenate([np.zeros(off, f32), host[k], np.zeros(1, f32)]))
            return base.view(off, n)          # the view keeps its base alive
        A, B, C, D = (put(k, i) for i, k in enumerate("abcd"))
        O = put("d", 4)
        a, bb, cc, dd = host["a"], host["b"], host["c"], host["d"]

        def run(fn, nslots):
            outs = []
            for _ in range(2):
                be.acc_zero(0, 4)
                fn()
                outs.append(be.acc_fetch(0, nslots))
            assert np.array_equal(outs[0], outs[1])          # deterministic
            return outs[0]

        def chk(got, want, want_out):
            assert np.allclose(got, want, rtol=1e-12, atol=1e-9 * max(n, 1)), (layout, got, want)
            if want_out is not None:
                assert np.array_equal(O.download(), want_out), layout

        r = f32(c) * (a - bb)
        want = a + r
        chk(run(lambda: be.fista_momentum(O, A, B, c, gt=C, slot=0), 1), [_d(cc - want) @ _d(cc - want)], want)
        gr = -a + f32(lam) * bb
        def tg():
            O.copy_from(A)
            be.tikh_grad(O, B, lam, slot=0)
        chk(run(tg, 2), [_d(gr) @ _d(gr), _d(bb) @ _d(bb)], gr)
        t = a + f32(-al) * bb
        chk(run(lambda: be.trial(O, A, B, -al, slot=1), 2), [0.0, _d(t) @ _d(t)], t)
        cl = np.where(a < 0, f32(0), a)
        def ce():
            O.copy_from(A)
            be.clamp_err(O, True, C, slot=0)
        chk(run(ce, 1), [_d(cc - cl) @ _d(cc - cl)], cl)
        p = _soft(a - f32(al) * bb, f32(al * lam))
        G = a - p
        chk(run(lambda: be.prox_l1_trial(O, A, B, al, al * lam, slot=0), 2), [_d(bb) @ _d(G), _d(G) @ _d(G)], p)
        v = bb + f32(c) * (bb - a)
        m = _soft(v - f32(al) * cc, f32(al * lam))
        chk(run(lambda: be.prox_l1_momentum(O, A, B, C, c, al, al * lam, gt=D, slot=0), 1), [_d(dd - m) @ _d(dd - m)], m)
        def pm_alias():                                    # out aliasing x0, as the solver calls it
            O.copy_from(A)
            be.prox_l1_momentum(O, O, B, C, c, al, al * lam, slot=0)
        run(pm_alias, 1)
        assert np.array_equal(O.download(), m)
        rs = bb - a
        chk(run(lambda: be.residual_acc(O, A, B, negate=True, slot=0), 1), [_d(rs) @ _d(rs)], rs)
        chk(run(lambda: be.residual_acc(None, A, B, slot=0), 1), [_d(rs) @ _d(rs)], None)
    ctx.close()


def test_tv_prox_det_equals_tv_denoise_fista_on_g9():
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    g = golden("g9_regularized")
    im = g["tv_im"]
    ctx = _lib.Context()
    be = HipBackend.__new__(HipBackend)
    be.ctx, be.lib = ctx, ctx.lib
    d_im = ctx.to_device(im)
    cases = [dict(weight=0.2, niter=20, eps=0.0, check_gap_frequency=3), dict(weight=0.05, niter=200, eps=1.e-3, check_gap_frequency=3),
             dict(weight=0.5, niter=1, eps=0.0, check_gap_frequency=1), dict(weight=0.5, niter=0)]
    for kw in cases:
        o1, o2 = ctx.empty(im.shape), ctx.empty(im.shape)
        it1, gap1 = be.tv_denoise_fista(d_im, o1, im.shape, **kw)
        it2, gap2 = be.tv_prox_det(d_im, o2, im.shape, **kw)
        it3, gap3 = be.tv_prox_det(d_im, o2, im.shape, **kw)
        assert it1 == it2 == it3 and gap2 == gap3, (kw, it1, it2, it3)
        assert rel_max(o2.download(), o1.download()) < 1e-6 and abs(gap2 - gap1) <= 1e-6 * max(abs(gap1), 1e-3)
    ctx.close()


def test_sharded_world_2_on_one_gpu(tmp_path):
    one = run_world("_gloo_gpu_reg_worker.py", 1, str(tmp_path / "w1"), timeout=300, per_rank=True)[0]
    two = run_world("_gloo_gpu_reg_worker.py", 2, str(tmp_path / "w2"), timeout=300, per_rank=True)
    for tag, _, _ in SHARD_CASES:
        for gt in (0, 1):
            key = "%s_%d" % (tag, gt)
            assert int(two[0][key + "_k"]) == int(one[key + "_k"]), key
            assert rel_max(two[0][key + "_rec"], one[key + "_rec"]) < 1e-5, key
            assert np.allclose(two[0][key + "_rms"], one[key + "_rms"], rtol=1e-5, atol=0), key
            for s in ("_rec", "_rms", "_k"):
                assert np.array_equal(two[1][key + s], two[0][key + s]), (key, s)


def test_one_rank_rccl_equals_serial():
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.comm import RcclComm
    from tomography_alignment_amd.recon import regularized, regularized_mpi
    geo, b, angles, xyz, x = shard_problem()
    ctx = _lib.Context(0)
    comm = RcclComm(ctx, 0, 1, RcclComm.unique_id(ctx.lib))
    try:
        for tag, meth, kw in SHARD_CASES:
            rm = regularized_mpi.RegularizedRecon(comm, geo, b, angles, xyz, options={"ground_truth": x})
            rec_m, rms_m = getattr(rm, meth)(**kw)
            rs = regularized.RegularizedRecon(geo, b, angles, xyz, options={"ground_truth": x})
            rec_s, rms_s = getattr(rs, meth)(**kw)
            assert len(rms_m) == len(rms_s) and rel_max(rec_m, rec_s) < 1e-5 and np.allclose(rms_m, rms_s, rtol=1e-5, atol=0), tag
    finally:
        comm.close()
        ctx.close()


@pytest.mark.parametrize("penalty", ["TV", "Tikh", "Lasso"])
def test_mpi_reconstruct_example(tmp_path, penalty):
    from tomography_alignment_amd.examples import mpi_reconstruct
    out = str(tmp_path / "recon.npy")
    rec, err = mpi_reconstruct.run(penalty, N=64, n_proj=90, niter=6, out=out)
    assert os.path.exists(out) and np.load(out).size == 64 ** 3
    assert len(err) >= 3 and np.all(np.isfinite(err)) and err[2] < err[0], (penalty, err)


def test_fista_256_device_arrays():
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.recon.regularized import RegularizedRecon
    from tomography_alignment_amd.utilities.generate_phantom import SHEPP_LOGAN
    from tomography_alignment_amd.utilities.geometry import Geometry
    from tomography_alignment_amd.utilities.projection_operators import ProjectionMatrix
    N, n_proj = 256, 256
    phi = np.linspace(0., np.pi, n_proj, endpoint=False)
    z = np.zeros(n_proj)
    geo = Geometry(n_proj, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2))
    be = HipBackend(geo)
    d_gt = be.phantom(be.empty(N ** 3), (N, N, N), SHEPP_LOGAN)
    d_b = ProjectionMatrix(geo, backend=be).projection_matrix(alpha=z, beta=z, phi=phi, xyz_shift=np.zeros((n_proj, 3))).apply(d_gt)
    r = RegularizedRecon(geo, d_b, np.array([phi, z, z]).T, np.zeros((n_proj, 3)), options={"ground_truth": d_gt, "_backend": be})
    rec, rms = r.run_fista(niter=4, hyper=1.e5, beta_tv=0.1, niter_tv=10)
    assert rec.shape == (N ** 3,) and np.all(np.isfinite(rms)) and rms[-1] < rms[0] < 1.0 + 1e-6, rms
