"""k_fwd_flat_tab with a block's footprint clipped to the volume, pinned with option "fwd_flat_gather" 0.  Whole-volume calls of the nominal
scan take the gather-form forward by default, so the clipped-footprint shapes of test_gpu_forward_clip.py (last tile column / row keeping
15, 16, 1 or 2 of its 16 cells: nx = 31, 32, 33, 47, ny = 17, 32; two z blocks, the second nearly empty) reach k_fwd_flat_tab only with the
option off -- yet that kernel still serves tomo_forward_xslab, the sharded solvers, finer steps and mixed calls.  Per shape: a dense volume
and volumes that are non-zero only in x = nx - 1 / y = ny - 1, against the CPU oracle at the flat forward's tolerance (1e-5 of the maximum),
and the dense result adjoint to the gather back-projection at 1e-5.  The measured errors are printed."""
import functools

import numpy as np
import pytest

from conftest import rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5
NZ = 130
PHI = np.array([0.0, np.pi / 4, np.pi / 2, 0.3, 2.2, np.pi])       # 0, 45 and 90 degrees among them
XYZ = np.zeros((6, 3))
XYZ[3] = (2.3, 0.0, -1.6)                                          # one projection translated (x and a fractional z)
XYZ[4] = (-1.0, 0.0, 3.0)
NDET = (62, 134)                                                   # wider than the largest diagonal (47 x 32)
SHAPES = [(nx, ny, NZ) for nx in (31, 32, 33, 47) for ny in (17, 32)]
WHICH = ("dense", "last_x", "last_y")


def geo_pair(shape):
    from tomography_alignment_amd.utilities.geometry import Geometry
    from oracle import oracle as orc
    args = (PHI.size, np.array(shape), np.ones(3), np.array(NDET), np.ones(2))
    return Geometry(*args), orc.Geo(*args)


def volumes(shape):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    dense = rng.uniform(0.1, 1.0, shape).astype(np.float32)
    last_x, last_y = np.zeros_like(dense), np.zeros_like(dense)
    last_x[-1, :, :] = dense[-1, :, :]
    last_y[:, -1, :] = dense[:, -1, :]
    return {"dense": dense, "last_x": last_x, "last_y": last_y}


@functools.lru_cache(maxsize=None)
def oracle_forward(shape, which):
    """Computed once per volume (read-only)."""
    from oracle import oracle as orc
    want = orc.forward(geo_pair(shape)[1], volumes(shape)[which], phi=PHI, xyz_shift=XYZ).ravel()
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_flat_tab_clipped_footprint_with_gather_forward_off(shape):
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    be = HipBackend(geo_pair(shape)[0])
    ctx = be.ctx
    ctx.set_option("fwd_flat_gather", 0)
    poses = _lib.poses_array(PHI, np.zeros(6), np.zeros(6), XYZ, np.zeros(3))
    vols = volumes(shape)
    errs, d_ax = {}, None
    for which in WHICH:
        ctx.profile_reset()
        ctx.profile_enable(True)
        out = be.forward(poses, be.upload(vols[which]), be.empty(poses.shape[0] * be.n_det))
        ctx.profile_enable(False)
        assert ctx.profile_get("k_fwd_tile_flat")[0] == 1 and ctx.profile_get("k_fwd_tile")[0] == 0 and ctx.profile_get("k_fwd_v2")[0] == 0
        want = oracle_forward(shape, which)
        assert np.count_nonzero(want) > 0
        errs[which] = rel_max(out.download(), want)
        if which == "dense":
            d_ax = out
    # adjoint to the gather back-projection: <A x, y> = <x, A^T y>
    y = be.upload(np.random.default_rng(1).uniform(0.1, 1.0, poses.shape[0] * be.n_det).astype(np.float32))
    aty = be.adjoint(poses, y, be.empty(be.n_vox))
    lhs, rhs = be.dot(d_ax, y), be.dot(be.upload(vols["dense"]), aty)
    e_adj = abs(lhs - rhs) / abs(lhs)
    print("[%s] k_fwd_flat_tab vs oracle: dense %.2e, last x %.2e, last y %.2e; adjointness %.2e"
          % (shape, errs["dense"], errs["last_x"], errs["last_y"], e_adj))
    assert all(e < TOL for e in errs.values())
    assert e_adj < TOL
