"""The SIRT update as the gather back-projection's store (tomo_adjoint_update) against the two calls it replaces, tomo_adjoint +
tomo_vec_update: the same bits of `rec`; the error sum to 1e-12 relative (double atomics in another order).

Volumes: 20 x 27 x 150 -- partial 8 x 8 column tiles in x and y, three 64-plane chunks, nz % 4 != 0 (the kernel's scalar store path) --
and 16 x 16 x 128 (the float4 store path).  Seven untilted projections, per-projection integer and fractional z shifts, COR shifts."""
import numpy as np
import pytest

from conftest import rel_max

pytestmark = pytest.mark.gpu

PHI = np.array([0.0, 0.4, np.pi / 4, np.pi / 2, 2.0, 2.7, np.pi])
ZSHIFT = np.array([0.0, 3.0, -2.5, 0.6, -4.0, 1.25, 2.0])      # integer and fractional, different per projection
CASES = {"scalar_store": ((20, 27, 150), (36, 150)), "vector_store": ((16, 16, 128), (24, 128))}


def problem(shape, ndet, alpha=None, seed=3):
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.utilities.geometry import Geometry
    rng = np.random.default_rng(seed)
    n = PHI.size
    xyz = np.zeros((n, 3))
    xyz[:, 0] = rng.uniform(-2, 2, n)
    xyz[:, 2] = ZSHIFT
    cor = np.zeros((n, 3))
    cor[:, 0] = rng.uniform(-1.5, 1.5, n)
    geo = Geometry(n, np.array(shape), np.ones(3), np.array(ndet), np.ones(2), cor_shift=cor)
    be = HipBackend(geo)
    poses = _lib.poses_array(PHI, np.zeros(n) if alpha is None else alpha, np.zeros(n), xyz, cor)
    n_vox, n_sino = int(np.prod(shape)), n * int(np.prod(ndet))
    host = {"res": rng.standard_normal(n_sino).astype(np.float32), "rec": rng.standard_normal(n_vox).astype(np.float32),
            "V": rng.uniform(0.1, 1.0, n_vox).astype(np.float32), "gt": rng.standard_normal(n_vox).astype(np.float32)}
    return geo, be, poses, xyz, host


def two_calls(be, poses, d_res, d_V, rec0, positivity, d_gt):
    rec, bp = be.upload(rec0), be.empty(rec0.size)
    be.adjoint(poses, d_res, bp)
    err = be.update(rec, bp, d_V, positivity, d_gt)
    return rec.download(), err


def one_call(be, poses, d_res, d_V, rec0, positivity, d_gt):
    rec = be.upload(rec0)
    ctx = be.ctx
    ctx.profile_reset()
    ctx.profile_enable(True)
    fused, err = be.adjoint_update(poses, d_res, rec, d_V, positivity, d_gt)
    ctx.profile_enable(False)
    assert fused
    assert ctx.profile_get("k_adj_gather_flat")[0] == 1 and ctx.profile_get("k_update")[0] == 0
    return rec.download(), err


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_step_has_the_bits_of_the_two_calls(case):
    shape, ndet = CASES[case]
    _, be, poses, _, h = problem(shape, ndet)
    d_res, d_V, d_gt = be.upload(h["res"]), be.upload(h["V"]), be.upload(h["gt"])
    for positivity in (False, True):
        for gt in (None, d_gt):
            want, e_want = two_calls(be, poses, d_res, d_V, h["rec"], positivity, gt)
            got, e_got = one_call(be, poses, d_res, d_V, h["rec"], positivity, gt)
            assert np.array_equal(bits(got), bits(want)), (positivity, gt is not None, int(np.count_nonzero(bits(got) != bits(want))))
            assert np.count_nonzero(bits(got) != bits(h["rec"])) > got.size // 2      # the step did something
            if gt is None:
                assert e_got is None and e_want is None
            else:
                print("[%s] positivity %d: error sum %.17g (two calls) %.17g (fused)" % (case, positivity, e_want, e_got))
                assert abs(e_got - e_want) <= 1e-12 * abs(e_want)


def test_dead_chunks_keep_their_bits():
    """A residual that is non-zero in the detector planes 96 .. 115 only reaches, with |z shifts| <= 4, the voxel planes of chunk 1
    (64 .. 127) alone: the first live chunk is not a multiple of the kernel's four waves per work-group (its chunk grouping shifts),
    chunks 0 and 2 are dead.  Their voxels keep the bits of `rec` -- and take the clamp and the error sum when those are asked for,
    as k_update gives them."""
    shape, ndet = CASES["scalar_store"]
    _, be, poses, _, h = problem(shape, ndet)
    res = h["res"].reshape(PHI.size, ndet[0], ndet[1]).copy()
    res[:, :, :96] = 0
    res[:, :, 116:] = 0
    d_res, d_V, d_gt = be.upload(res), be.upload(h["V"]), be.upload(h["gt"])
    got, _ = one_call(be, poses, d_res, d_V, h["rec"], False, None)
    got3, rec3 = bits(got).reshape(shape), bits(h["rec"]).reshape(shape)
    assert np.array_equal(got3[:, :, :64], rec3[:, :, :64]) and np.array_equal(got3[:, :, 128:], rec3[:, :, 128:])
    assert np.count_nonzero(got3[:, :, 64:128] != rec3[:, :, 64:128]) > 0
    want, _ = two_calls(be, poses, d_res, d_V, h["rec"], False, None)
    assert np.array_equal(bits(got), bits(want))
    for positivity, gt in ((True, None), (False, d_gt), (True, d_gt)):
        want, e_want = two_calls(be, poses, d_res, d_V, h["rec"], positivity, gt)
        got, e_got = one_call(be, poses, d_res, d_V, h["rec"], positivity, gt)
        assert np.array_equal(bits(got), bits(want)), (positivity, gt is not None)
        if gt is not None:
            assert abs(e_got - e_want) <= 1e-12 * abs(e_want)


def test_a_tilted_pose_declines_and_changes_nothing():
    shape, ndet = CASES["scalar_store"]
    alpha = np.zeros(PHI.size)
    alpha[3] = 0.02
    _, be, poses, _, h = problem(shape, ndet, alpha=alpha)
    d_res, d_V, rec = be.upload(h["res"]), be.upload(h["V"]), be.upload(h["rec"])
    be.ctx.profile_reset()
    be.ctx.profile_enable(True)
    fused, err = be.adjoint_update(poses, d_res, rec, d_V, True, None)
    be.ctx.profile_enable(False)
    assert not fused and err is None
    assert all(be.ctx.profile_get(k)[0] == 0 for k in ("k_adj_gather_flat", "k_adj_tile", "k_adj_tile_flat", "k_update", "k_sino_zflags"))
    assert np.array_equal(bits(rec.download()), bits(h["rec"]))
    # ... and the option that switches the fused path off declines untilted poses the same way
    _, be0, poses0, _, _ = problem(shape, ndet)
    be0.ctx.set_option("fused_update", 0)
    rec0 = be0.upload(h["rec"])
    fused, _ = be0.adjoint_update(poses0, be0.upload(h["res"]), rec0, be0.upload(h["V"]), False, None)
    assert not fused and np.array_equal(bits(rec0.download()), bits(h["rec"]))


def sirt_run(tilted, fused, solver="plain"):
    """Three SIRT iterations with positivity and a ground truth; the ray-driven forward (fwd_variant 2) is deterministic, so with untilted
    poses the whole run is."""
    from tomography_alignment_amd.recon import sirt
    shape, ndet = CASES["scalar_store"]
    alpha = np.zeros(PHI.size)
    if tilted:
        alpha[3] = 0.02
    geo, be, poses, xyz, h = problem(shape, ndet, alpha=alpha)
    x = np.abs(h["gt"])
    be.ctx.set_option("fwd_variant", 2)
    b = be.forward(poses, be.upload(x), be.empty(poses.shape[0] * be.n_det)).download().reshape(poses.shape[0], -1)
    angles = np.array([PHI, alpha, 0 * PHI]).T
    if solver == "plain":
        s = sirt.SIRT(geo, b, angles, xyz, options={"_backend": be, "ground_truth": x})
    else:
        s = solver(geo, b, angles, xyz, {"_backend": be, "ground_truth": x})
    be.ctx.set_option("fused_update", 1 if fused else 0)
    be.ctx.profile_reset()
    be.ctx.profile_enable(True)
    k, rms = s.iterate_device(niter=3, positivity=True)
    be.ctx.profile_enable(False)
    assert k == 3
    return s.d_rec.download(), rms, {n: be.ctx.profile_get(n)[0] for n in ("k_adj_gather_flat", "k_update", "k_sino_zflags")}


def test_sirt_takes_the_fused_step_and_keeps_its_result():
    rec1, rms1, n1 = sirt_run(False, True)
    rec0, rms0, n0 = sirt_run(False, False)
    assert n1["k_adj_gather_flat"] == 3 and n1["k_update"] == 0 and n0["k_update"] == 3 and n0["k_adj_gather_flat"] == 3
    assert np.array_equal(bits(rec1), bits(rec0))
    assert np.allclose(rms1, rms0, rtol=1e-12, atol=0)


def test_sirt_with_a_tilted_pose_falls_back():
    """One tilted pose in the call: the fused step declines in every iteration and the solver makes the two calls, as with the fused path
    switched off.  (The two runs take the same kernels; the tilted pose's back-projection adds with float atomics, whose order is free:
    equal to the float32 bar of the suite, 1e-5 of the maximum, not bit for bit.)"""
    rec1, rms1, n1 = sirt_run(True, True)
    rec0, rms0, n0 = sirt_run(True, False)
    assert n1["k_update"] == 3 and n0["k_update"] == 3
    assert rel_max(rec1, rec0) < 1e-5 and np.allclose(rms1, rms0, rtol=1e-5, atol=0)


def test_sharded_solver_on_one_rank_keeps_the_two_calls(monkeypatch):
    import os
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.comm import RcclComm
    from tomography_alignment_amd.recon import sirt_mpi

    def refuse(self, *a, **kw):
        raise AssertionError("the sharded solver took the fused step")
    monkeypatch.setattr(HipBackend, "adjoint_update", refuse)
    made = []

    def make(geo, b, angles, xyz, options):
        comm = RcclComm(options["_backend"].ctx, 0, 1, RcclComm.unique_id(options["_backend"].ctx.lib))
        made.append(comm)
        return sirt_mpi.SIRT(comm, geo, b, angles, xyz, options)
    try:
        rec_m, rms_m, n_m = sirt_run(False, True, solver=make)
    finally:
        for c in made:
            c.close()
    assert n_m["k_update"] == 3 and n_m["k_adj_gather_flat"] == 3
    monkeypatch.undo()
    # the unsharded solver differs from it in its guard of W and V only (x < 1e-8 -> 0 against x == 0 -> 0): none of either here
    rec_s, rms_s, _ = sirt_run(False, False)
    assert np.array_equal(bits(rec_m), bits(rec_s)) and np.allclose(rms_m, rms_s, rtol=1e-12, atol=0)
