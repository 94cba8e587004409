"""The flat forward with a block's footprint clipped to the volume (k_fwd_flat_tab): volumes whose last tile column / row keeps 15, 16, 1
or 2 of its 16 cells (nx, ny = 31, 32, 33, 47 / 17, 32 with the tile grid starting at -1), two z blocks of 128 planes, the second nearly
empty.  Against the CPU oracle and the ray-driven forward at the flat forward's tolerance in test_gpu_parity.py (1e-5 of the maximum),
and adjoint to the gather back-projection at the tolerance of test_gpu_configs.py (1e-5).  No bits are compared between two forward
launches: the order of their float atomics is free."""
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
    """Computed once per volume, shared by the tests below (read-only)."""
    from oracle import oracle as orc
    want = orc.forward(geo_pair(shape)[1], volumes(shape)[which], phi=PHI, xyz_shift=XYZ).ravel()
    want.setflags(write=False)
    return want


def backend(shape):
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    be = HipBackend(geo_pair(shape)[0])
    return be, _lib.poses_array(PHI, np.zeros(6), np.zeros(6), XYZ, np.zeros(3))


def flat_forward(be, poses, x):
    ctx = be.ctx
    ctx.profile_reset()
    ctx.profile_enable(True)
    out = be.forward(poses, be.upload(x), be.empty(poses.shape[0] * be.n_det))
    ctx.profile_enable(False)
    assert ctx.profile_get("k_fwd_tile_flat")[0] == 1 and ctx.profile_get("k_fwd_tile")[0] == 0 and ctx.profile_get("k_fwd_v2")[0] == 0
    return out


SHAPES = [(nx, ny, NZ) for nx in (31, 32, 33, 47) for ny in (17, 32)]


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_clipped_forward_dense_volume(shape):
    be, poses = backend(shape)
    x = volumes(shape)["dense"]
    d_ax = flat_forward(be, poses, x)
    ax = d_ax.download()
    e_orc = rel_max(ax, oracle_forward(shape, "dense"))
    be.ctx.set_option("fwd_variant", 2)
    ray = be.forward(poses, be.upload(x), be.empty(ax.size)).download()
    be.ctx.set_option("fwd_variant", 3)
    e_ray = rel_max(ax, ray)
    # adjoint to the gather back-projection: <A x, y> = <x, A^T y>
    y = be.upload(np.random.default_rng(1).uniform(0.1, 1.0, ax.size).astype(np.float32))
    be.ctx.profile_reset()
    be.ctx.profile_enable(True)
    aty = be.adjoint(poses, y, be.empty(be.n_vox))
    be.ctx.profile_enable(False)
    assert be.ctx.profile_get("k_adj_gather_flat")[0] == 1
    lhs, rhs = be.dot(d_ax, y), be.dot(be.upload(x), aty)
    print("[%s] flat forward vs oracle %.2e, vs ray-driven %.2e, adjointness %.2e" % (shape, e_orc, e_ray, abs(lhs - rhs) / abs(lhs)))
    assert e_orc < TOL and e_ray < TOL
    assert abs(lhs - rhs) / abs(lhs) < TOL


@pytest.mark.parametrize("which", ["last_x", "last_y"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s[:2] for s in SHAPES])
def test_clipped_forward_sees_the_last_column_and_row(shape, which):
    """A volume that is non-zero only in x = nx - 1 (y = ny - 1): all of it lies in the cells the clipped footprint of the last tile
    column (row) keeps, and in the neighbouring column's (row's) last cell."""
    be, poses = backend(shape)
    x = volumes(shape)[which]
    ax = flat_forward(be, poses, x).download()
    want = oracle_forward(shape, which)
    assert np.count_nonzero(want) > 0
    e_orc = rel_max(ax, want)
    be.ctx.set_option("fwd_variant", 2)
    e_ray = rel_max(ax, be.forward(poses, be.upload(x), be.empty(ax.size)).download())
    print("[%s %s] flat forward vs oracle %.2e, vs ray-driven %.2e" % (shape, which, e_orc, e_ray))
    assert e_orc < TOL and e_ray < TOL
