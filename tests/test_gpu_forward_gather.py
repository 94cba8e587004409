"""The gather-form flat forward (option "fwd_flat_gather", k_fwd_gather_flat) against the default flat forward (option off) and the CPU
oracle, at the project's bar max|a - b| / max|b| < 1e-5: every group size, both walks, both weight counts and the switches between them,
fractional x / z translations, a COR shift, step 0.95, zero z bands, determinism, adjointness with k_adj_gather_flat, declined calls, and
ten SIRT iterations.  The measured errors are printed."""
import numpy as np
import pytest

from conftest import rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5

SHAPES = [(24, 24, 64), (17, 23, 65), (40, 9, 130),          # nx, ny not multiples of 8; nz = 64, 65, 130 (one chunk, one + 1 plane, three)
          (23, 17, 63)]                                      # ... and 63: the only chunk is one plane short (63 live lanes in the plane mask)
SPECIAL = [0.0, np.pi / 2, np.pi,                             # samples on integers
           np.arctan(0.5) - 1e-3, np.arctan(0.5) + 1e-3,      # the 3 / 4-weight switch
           np.pi / 4 - 1e-3, np.pi / 4 + 1e-3,                # the walk switch, inside one group of eight
           3 * np.pi / 4 - 1e-3, 3 * np.pi / 4 + 1e-3]


def geo_pair(n_proj, shape, ndx, cor_shift=None, step=1.0):
    from tomography_alignment_amd.utilities.geometry import Geometry
    from oracle import oracle as orc
    args = (n_proj, np.array(shape), np.ones(3), np.array([ndx, shape[2]]), np.ones(2))
    return Geometry(*args, cor_shift=cor_shift, step_size=step), orc.Geo(*args, cor_shift=cor_shift, step_size=step)


def angles(n, kind, rng):
    if kind == "special":
        a = list(SPECIAL[:n])
        return np.array(a + list(rng.uniform(0.0, np.pi, n - len(a))))
    return rng.uniform(0.0, np.pi, n)


def volume(shape, rng, band=None):
    x = rng.uniform(0.1, 1.0, shape).astype(np.float32)
    nz = shape[2]
    if band == "bands":             # z planes 0 .. 19 and the top third zero
        x[:, :, :20] = 0
        x[:, :, nz - nz // 3:] = 0
    elif band == "zero":
        x[:] = 0
    return x


def forward(geo, kw, x, gather):
    from tomography_alignment_amd.utilities.projection_operators import ProjectionMatrix
    P = ProjectionMatrix(geo)
    P.backend.ctx.set_option("fwd_flat_gather", gather)
    return P, P.projection_matrix(**kw).dot(x.ravel())


def case_list():
    """(shape, ndx kind, n_proj, angle kind, pose kind, step): every shape x detector width, the group sizes and pose kinds dealt round."""
    counts = [1, 7, 8, 9, 17]
    poses = ["plain", "shift", "cor", "shift"]
    out, k = [], 0
    for shape in SHAPES:
        for wide in (-5, 0, 7):
            n = counts[k % len(counts)]
            out.append((shape, wide, n, "special" if n >= 9 else "random", poses[k % len(poses)], 0.95 if k % 3 == 1 else 1.0))
            k += 1
    for shape in SHAPES:                    # all switches, shifted poses, on every shape
        out.append((shape, 0, 17, "special", "shift", 1.0))
    out.append((SHAPES[2], 0, 9, "special", "plain", 0.95))
    return out


def pose_kw(n, kind, rng):
    xyz = np.zeros((n, 3))
    cor = None
    if kind == "shift":                     # fractional x / z translations: tau != 0, z offsets that are no multiples of 16
        xyz[:, 0] = rng.uniform(-3.0, 3.0, n)
        xyz[:, 2] = rng.uniform(-21.0, 21.0, n)
    elif kind == "cor":
        cor = np.array([1.37, 0.0, 0.0])
        xyz[:, 2] = np.round(rng.uniform(-9.0, 9.0, n))       # integer z offsets: tau = 0, rows not 16-byte aligned
    return xyz, cor


@pytest.mark.parametrize("shape,wide,n,akind,pkind,step", case_list())
def test_gather_forward_vs_default_and_oracle(shape, wide, n, akind, pkind, step):
    from oracle import oracle as orc
    rng = np.random.default_rng(hash((shape, wide, n)) % (1 << 31))
    xyz, cor = pose_kw(n, pkind, rng)
    geo, og = geo_pair(n, shape, shape[0] + wide, cor_shift=cor, step=step)
    kw = dict(alpha=np.zeros(n), beta=np.zeros(n), phi=angles(n, akind, rng), xyz_shift=xyz)
    x = volume(shape, rng)
    _, off = forward(geo, kw, x, 0)
    _, on = forward(geo, kw, x, 1)
    ref = orc.forward(og, x, **kw).ravel()
    e_off, e_ref = rel_max(on, off), rel_max(on, ref)
    print("gather forward %s ndx %+d, %d poses (%s, %s, step %.2f): vs default %.2e, vs oracle %.2e (default vs oracle %.2e)"
          % (shape, wide, n, akind, pkind, step, e_off, e_ref, rel_max(off, ref)))
    assert e_off < TOL and e_ref < TOL


@pytest.mark.parametrize("shape", SHAPES)
def test_zero_bands_exact_zeros_and_determinism(shape):
    n = 9
    rng = np.random.default_rng(7)
    xyz, _ = pose_kw(n, "shift", rng)
    geo, _ = geo_pair(n, shape, shape[0])
    kw = dict(alpha=np.zeros(n), beta=np.zeros(n), phi=angles(n, "special", rng), xyz_shift=xyz)
    x = volume(shape, rng, "bands")
    _, off = forward(geo, kw, x, 0)
    P, on = forward(geo, kw, x, 1)
    again = P.projection_matrix(**kw).dot(x.ravel())
    assert np.array_equal(on.view(np.uint32), again.view(np.uint32)), "two calls of the gather forward differ"
    e = rel_max(on, off)
    print("zero bands %s: vs default %.2e; rays that are zero: default %d, gather %d" % (shape, e, int((off == 0).sum()), int((on == 0).sum())))
    assert e < TOL
    assert np.array_equal(on == 0, off == 0)            # rays through zero planes only hold exact zeros, as on the dense path
    _, z = forward(geo, kw, volume(shape, rng, "zero"), 1)
    assert not z.any()


def test_adjointness_with_gather_adjoint():
    shape, n = SHAPES[2], 17
    rng = np.random.default_rng(11)
    xyz, _ = pose_kw(n, "shift", rng)
    geo, _ = geo_pair(n, shape, shape[0])
    kw = dict(alpha=np.zeros(n), beta=np.zeros(n), phi=angles(n, "special", rng), xyz_shift=xyz)
    x = volume(shape, rng)
    y = rng.uniform(0.1, 1.0, n * shape[0] * shape[2]).astype(np.float32)
    from tomography_alignment_amd.utilities.projection_operators import ProjectionMatrix
    P = ProjectionMatrix(geo)
    P.backend.ctx.set_option("fwd_flat_gather", 1)
    A = P.projection_matrix(**kw)
    Ax, ATy = A.dot(x.ravel()), A.T.dot(y)
    lhs, rhs = float(np.dot(Ax.astype(np.float64), y.astype(np.float64))), float(np.dot(x.ravel().astype(np.float64), ATy.astype(np.float64)))
    print("adjointness: <Ax, y> = %.10e, <x, A^T y> = %.10e, rel %.2e" % (lhs, rhs, abs(lhs - rhs) / abs(lhs)))
    assert abs(lhs - rhs) / abs(lhs) < 1e-6


@pytest.mark.parametrize("kind", ["tilted", "half_step"])
def test_declined_calls_keep_the_default_bits(kind):
    shape, n = SHAPES[0], 8
    rng = np.random.default_rng(3)
    geo, _ = geo_pair(n, shape, shape[0], step=0.5 if kind == "half_step" else 1.0)
    alpha = np.zeros(n)
    if kind == "tilted":
        alpha[3] = np.deg2rad(0.7)
    kw = dict(alpha=alpha, beta=np.zeros(n), phi=angles(n, "random", rng), xyz_shift=np.zeros((n, 3)))
    x = np.zeros(shape, np.float32)
    # few voxels, all inside one tile and one z block: a ray gets its sum from a single work-group, so the free order of the default
    # kernels' float atomics has nothing to reorder (the weights have full mantissas: the sums themselves are not exact).  A call that
    # was not declined would show at once: the gather forward knows neither a tilt nor a half step and would give other values altogether
    x[5:9, 7:12, 20:33] = rng.uniform(0.1, 1.0, (4, 5, 13))
    x = np.round(x * 64) / 64
    _, off = forward(geo, kw, x, 0)
    _, on = forward(geo, kw, x, 1)
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))


def test_sirt_ten_iterations_vs_oracle():
    """Ten SIRT iterations at 64^3 x 24 with the gather forward against the oracle's restatement of the reference's SIRT, at the bar of
    tests/test_gpu_solvers.py (1e-5 on the reconstruction and on the error history)."""
    from oracle import oracle as orc
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.recon import sirt
    N, n = 64, 24
    rng = np.random.default_rng(5)
    geo, og = geo_pair(n, (N, N, N), N)
    phi = np.linspace(0.0, np.pi, n)
    xyz = np.zeros((n, 3))
    xyz[:, 0] = rng.uniform(-2.0, 2.0, n)
    xyz[:, 2] = rng.uniform(-2.0, 2.0, n)
    kw = dict(alpha=np.zeros(n), beta=np.zeros(n), phi=phi, xyz_shift=xyz)
    x = orc.shepp3d(N).astype(np.float32)
    b = orc.forward(og, x, **kw).astype(np.float32).ravel()
    want, want_err = orc.sirt(lambda v: orc.forward(og, v.reshape(N, N, N), **kw).astype(np.float32).ravel(),
                              lambda y: orc.adjoint(og, y, **kw).astype(np.float32).ravel(), N ** 3, b, 10)
    be = HipBackend(geo)
    be.ctx.set_option("fwd_flat_gather", 1)
    s = sirt.SIRT(geo, b.copy(), np.array([phi, kw["alpha"], kw["beta"]]).T, xyz, options={"_backend": be})
    rec, err = s.run_main_iteration(niter=10)
    e_rec, e_err = rel_max(rec.ravel(), want), float(np.max(np.abs(err - want_err) / want_err))
    print("SIRT x10 with the gather forward vs the oracle: rec rel-max %.2e, rms_error rel %.2e" % (e_rec, e_err))
    assert e_rec < 1e-5 and e_err < 1e-5
