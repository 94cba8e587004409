"""GPU parity tests: the HIP path (through the C-ABI of libtomo_hip.so) against
  * the golden vectors produced by the compiled reference (tests/golden), and
  * the CPU oracle on the same seeded inputs,
plus size-independent properties at larger sizes.  Tolerance: 1e-5 relative (max|a-b|/max|b|),
the float32 bar of BASELINE.json:north_star."""
import numpy as np
import pytest

from conftest import golden, rel_max, rel_l2, g10_case, grad_dev_per_ray, FACE_TOL_KERNELS

pytestmark = pytest.mark.gpu
TOL = 1e-5


def geo_pair(n_proj, N, cor_shift=None, step=1.0, ndet=None, shape=None):
    from tomography_alignment_amd.utilities.geometry import Geometry
    from oracle import oracle as orc
    shape = np.array([N, N, N]) if shape is None else np.array(shape)
    ndet = np.array([N, N]) if ndet is None else np.array(ndet)
    args = (n_proj, shape, np.ones(3), ndet, np.ones(2))
    return Geometry(*args, cor_shift=cor_shift, step_size=step), orc.Geo(*args, cor_shift=cor_shift, step_size=step)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def PM():
    from tomography_alignment_amd.utilities.projection_operators import ProjectionMatrix
    return ProjectionMatrix


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_forward_adjoint_vs_reference_golden(PM, shepp32, variant):
    g = golden("g2_fwd_adj")
    geo, _ = geo_pair(6, 32)
    P = PM(geo)
    P.backend.ctx.set_option("fwd_variant", variant)
    A = P.projection_matrix(alpha=g["alpha"], beta=g["beta"], phi=g["phi"], xyz_shift=g["xyz"])
    assert A.shape == (6 * 32 * 32, 32 ** 3)
    Ax = A.dot(shepp32.ravel())
    assert Ax.dtype == np.float32
    assert rel_max(Ax, g["Ax"]) < TOL
    ATy = A.T.dot(g["y"].ravel())
    assert rel_max(ATy, g["ATy"]) < TOL
    A0 = P.projection_matrix()          # unperturbed poses (phi = 0, pi/2, pi among them: integer coordinates)
    assert rel_max(A0.dot(shepp32.ravel()), g["Ax0"]) < TOL
    assert rel_max(A0.T.dot(g["y"].ravel()), g["ATy0"]) < TOL
    P.backend.ctx.set_option("fwd_variant", 3)


def test_scipy_unbound_protocol(PM, shepp32):
    """recon/sirt.py:59,61 call the operator through scipy's unbound methods."""
    from scipy import sparse
    g = golden("g2_fwd_adj")
    geo, _ = geo_pair(6, 32)
    A = PM(geo).projection_matrix(alpha=g["alpha"], beta=g["beta"], phi=g["phi"], xyz_shift=g["xyz"])
    Ax = sparse.csr_matrix.dot(A, shepp32.ravel())
    ATy = sparse.csc_matrix.dot(sparse.csr_matrix.transpose(A), g["y"].ravel())
    assert rel_max(Ax, g["Ax"]) < TOL and rel_max(ATy, g["ATy"]) < TOL


def test_operator_matches_reference_csr_columns(PM):
    """G1: apply the matrix-free operator to unit vectors and compare with the reference's CSR."""
    from scipy import sparse
    g = golden("g1_operator")
    ref = sparse.csr_matrix((g["b_data"], g["b_indices"], g["b_indptr"]), shape=tuple(g["b_shape"]))
    geo, _ = geo_pair(3, 8, cor_shift=g["b_cor"])
    A = PM(geo).projection_matrix(alpha=g["b_alpha"], beta=g["b_beta"], phi=g["b_phi"], xyz_shift=g["b_xyz"])
    rng = np.random.default_rng(0)
    X = rng.standard_normal((8 ** 3, 4)).astype(np.float32)
    for k in range(4):
        assert rel_max(A.dot(X[:, k]), ref.dot(X[:, k])) < TOL
    Y = rng.standard_normal((3 * 64, 4)).astype(np.float32)
    for k in range(4):
        assert rel_max(A.T.dot(Y[:, k]), ref.T.dot(Y[:, k])) < TOL
    dense = ref.toarray()
    cols = [0, 73, 200, 511]
    for c in cols:
        e = np.zeros(512, np.float32)
        e[c] = 1.0
        assert np.max(np.abs(A.dot(e) - dense[:, c])) < 5e-6   # matrix entries are O(1): float32 weights


def test_voxel_mask_step_and_detector_shape(PM, orc):
    """G1 case c: voxel mask, step 0.5, detector 12x12 on a 16^3 volume, float64 precision."""
    from scipy import sparse
    g = golden("g1_operator")
    ref = sparse.csr_matrix((g["c_data"], g["c_indices"], g["c_indptr"]), shape=tuple(g["c_shape"]))
    geo, _ = geo_pair(2, 16, step=0.5, ndet=[12, 12])
    A = PM(geo, precision=np.float64).projection_matrix(alpha=g["c_alpha"], beta=g["c_beta"], phi=g["c_phi"],
                                                        xyz_shift=g["c_xyz"], voxel_mask=g["c_mask"])
    rng = np.random.default_rng(1)
    x = rng.standard_normal(16 ** 3)
    y = rng.standard_normal(2 * 144)
    out = A.dot(x)
    assert out.dtype == np.float64
    assert rel_max(out, ref.dot(x)) < TOL
    assert rel_max(A.T.dot(y), ref.T.dot(y)) < TOL


@pytest.mark.parametrize("grad_variant", [1, 2, 3, 4])
def test_projection_gradient_vs_reference_golden(PM, shepp32, grad_variant):
    g = golden("g3_proj_grad")
    geo, _ = geo_pair(1, 32)
    P = PM(geo, precision=np.float64)
    P.backend.ctx.set_option("grad_variant", grad_variant)
    for i in range(3):          # generic poses
        p, gr = P.projection_gradient(shepp32, g["alpha"][i], g["beta"][i], g["phi"][i], g["xyz"][i], g["cor"][i])
        assert gr.shape == (6, 1024)
        assert rel_max(p, g["proj"][i]) < TOL
        for k in range(6):
            assert rel_max(gr[k], g["grad"][i][k]) < TOL, (i, k)
    # degenerate pose: the value is continuous across integer coordinates, the gradient is not
    p, gr = P.projection_gradient(shepp32, g["alpha"][3], g["beta"][3], g["phi"][3], g["xyz"][3], g["cor"][3])
    assert rel_max(p, g["proj"][3]) < TOL


def test_fortran_row_order_and_matrix_free_golden(PM, shepp32):
    """G4: forward_project_, back_project_, compute_gradient_ of the flang-built reference."""
    from tomography_alignment_amd import _lib
    g2, g3, g4 = golden("g2_fwd_adj"), golden("g3_proj_grad"), golden("g4_matrix_free")
    geo, _ = geo_pair(6, 32)
    P = PM(geo)
    be = P.backend
    A = P.projection_matrix(alpha=g2["alpha"], beta=g2["beta"], phi=g2["phi"], xyz_shift=g2["xyz"])
    assert rel_max(A.dot(shepp32.ravel()), g4["ax"].ravel()) < TOL           # A5
    poses = _lib.poses_array(g2["phi"], g2["alpha"], g2["beta"], g2["xyz"], np.zeros(3))
    det = be.upload(g2["y"])
    vol = be.empty(32 ** 3)
    be.backproject_voxel(poses, det, vol)
    # A6: back_project_ is float32 throughout; k_bp_voxel performs the reference's float32 operations in the reference's order
    e_a6 = rel_max(vol.download(), g4["atx"])
    print("A6 back_project vs the Fortran: rel-max %.2e" % e_a6)
    assert e_a6 < TOL
    vdev = be.upload(shepp32)
    pr, gd = be.empty(1024), be.empty(6 * 1024)
    for i in range(3):                                                          # A7 row order tx,ty,tz,alpha,beta,phi
        pose = _lib.poses_array([g3["phi"][i]], [g3["alpha"][i]], [g3["beta"][i]], g3["xyz"][i], g3["cor"][i])
        be.proj_grad(pose, vdev, pr, gd, 1)
        assert rel_max(pr.download(), g4["grad_ax"][i]) < TOL
        mine = gd.download().reshape(6, -1)
        ref64 = g3["grad"][i][[0, 1, 2, 4, 5, 3]]
        assert rel_max(mine, ref64) < TOL                  # vs the f64 reference, permuted rows
        assert rel_l2(mine, g4["grad_dax"][i]) < 2e-3      # the f32 Fortran twin itself is only this close


def test_cost_grad_fused_vs_oracle(PM, orc, shepp32):
    from tomography_alignment_amd import _lib
    g = golden("g3_proj_grad")
    geo, og = geo_pair(1, 32)
    P = PM(geo)
    be = P.backend
    rng = np.random.default_rng(4)
    n = 3
    b = np.zeros((n, 1024), np.float32)
    want_c, want_g, scale_g = [], [], []
    for i in range(n):
        p, gr = orc.projection_gradient(og, shepp32, g["alpha"][i], g["beta"][i], g["phi"][i], g["xyz"][i], g["cor"][i])
        b[i] = p + 0.05 * rng.standard_normal(1024).astype(np.float32)
        res = b[i].astype(np.float64) - p
        want_c.append(0.5 * np.dot(res, res))
        want_g.append(np.dot(-gr.astype(np.float64), res))
        scale_g.append(np.dot(np.abs(gr.astype(np.float64)), np.abs(res)))     # size of the terms the reduction cancels
    poses = _lib.poses_array(g["phi"][:n], g["alpha"][:n], g["beta"][:n], g["xyz"][:n], g["cor"][:n])
    resid = be.empty(n * 1024)
    cost, g6 = be.cost_grad(poses, be.upload(shepp32), be.upload(b), resid)
    assert np.allclose(cost, want_c, rtol=1e-5)
    assert np.max(np.abs(g6 - np.array(want_g)) / np.array(scale_g)) < TOL
    r = resid.download().reshape(n, -1)
    assert rel_max(r[0], b[0] - orc.projection_gradient(og, shepp32, g["alpha"][0], g["beta"][0], g["phi"][0], g["xyz"][0], g["cor"][0])[0]) < 1e-4
    # row-indexed form (tomo_cost_grad_rows): a subset of the poses against their rows of the resident table
    pick = np.array([2, 0])
    c2, g2 = be.cost_grad(np.ascontiguousarray(poses[pick]), be.upload(shepp32), be.upload(b), rows=pick)
    # round 6: the fused reduction adds the work-groups' partial sums in a fixed order -- a pose's seven numbers do not depend on the batch
    assert np.array_equal(c2, cost[pick]) and np.array_equal(g2, g6[pick])
    with pytest.raises(_lib.TomoError):
        be.cost_grad(np.ascontiguousarray(poses[:1]), be.upload(shepp32), be.upload(b), rows=np.array([3]))


@pytest.mark.parametrize("shape,ndet", [((64, 64, 64), (64, 64)), ((50, 44, 150), (70, 210)), ((400, 380, 340), (402, 350))])
def test_fused_cost_gradient_is_deterministic(PM, shape, ndet):
    """the reference's cost and gradient (utilities/alignment_functions.py:16-37) are deterministic; until round 5
    the fused kernels ended in one float64 atomicAdd per work-group, so two identical calls differed in the last digits and L-BFGS-B turned
    that into 1e-4 px.  Now: work-group partials + a fixed-order second stage (k_cost_grad_reduce) --
      * the same call twice: bit-identical;
      * a pose evaluated alone, in a shuffled batch, in a batch of duplicates, against a row-indexed table: the same seven numbers, bit for bit
        (the partial layout is a function of the rays a work-group owns, not of the launch);
      * every kernel variant on its own (1, 2, 3) and the per-pose choice (4);
      * the third shape takes the cache-ordered grid (z chunk slowest, XCD swizzle off: 101 x groups) when several poses share a launch and the
        plain order for one pose: same numbers."""
    from tomography_alignment_amd import _lib
    rng = np.random.default_rng(23)
    n = 7
    geo, _ = geo_pair(n, None, ndet=ndet, shape=shape)
    be = PM(geo).backend
    x = rng.uniform(0.0, 1.0, shape).astype(np.float32)
    x[: shape[0] // 5] = 0.0                                       # a non-trivial box of non-zero voxels
    phi = np.linspace(0.1, 3.0, n)
    alpha, beta = np.deg2rad(rng.uniform(-2, 2, n)), np.deg2rad(rng.uniform(-2, 2, n))
    alpha[:2] = beta[:2] = 0.0                                     # both tilt groups present (variant 4: v2 for these, v3 for the rest)
    xyz = rng.uniform(-3, 3, (n, 3))
    poses = _lib.poses_array(phi, alpha, beta, xyz, np.zeros(3))
    vol = be.upload(x)
    b = be.forward(poses, vol, be.empty(n * be.n_det))
    b.upload(b.download() + rng.standard_normal(n * be.n_det).astype(np.float32))
    for v in (4, 1, 2, 3):
        be.ctx.set_option("grad_variant", v)
        c0, g0 = be.cost_grad(poses, vol, b)
        assert np.all(np.isfinite(c0)) and np.all(c0 > 0) and np.all(np.abs(g0).max(axis=1) > 0)
        for _ in range(3):
            c1, g1 = be.cost_grad(poses, vol, b)
            assert np.array_equal(c1, c0) and np.array_equal(g1, g0), v
        perm = rng.permutation(n)
        c2, g2 = be.cost_grad(np.ascontiguousarray(poses[perm]), vol, b, rows=perm)
        assert np.array_equal(c2, c0[perm]) and np.array_equal(g2, g0[perm]), v
        for i in (0, n - 1):
            c3, g3 = be.cost_grad(np.ascontiguousarray(poses[i:i + 1]), vol, b, rows=np.array([i]))
            assert c3[0] == c0[i] and np.array_equal(g3[0], g0[i]), (v, i)
        dup = np.array([3, 3, 0, 3, 5, 0])
        c4, g4 = be.cost_grad(np.ascontiguousarray(poses[dup]), vol, b, rows=dup)
        assert np.array_equal(c4, c0[dup]) and np.array_equal(g4, g0[dup]), v
    be.ctx.set_option("grad_variant", 4)


def test_fused_cost_gradient_batches_larger_than_the_partial_buffer(PM):
    """tomo_cost_grad_rows keeps the work-groups' partial sums of at most 512 MB worth of poses at a time (csrc/tomo_project.hip:
    TOMO_RED_PART_BYTES) and sends a larger batch through in several launches.  A 1024 x 1024 detector has 4096 work-groups per pose =
    224 KB of partials: 2500 poses cross the limit (2340).  The call must give, bit for bit, what the same poses give in small batches --
    in both tilt groups, with row indices into a two-row table (the measured rows stay tiny; the volume is a thin slab, most rays miss)."""
    from tomography_alignment_amd import _lib
    rng = np.random.default_rng(31)
    shape, ndet, n = (48, 24, 40), (1024, 1024), 2500
    geo, _ = geo_pair(2, None, ndet=ndet, shape=shape)
    be = PM(geo).backend
    x = rng.uniform(0.1, 1.0, shape).astype(np.float32)
    phi = rng.uniform(0.0, np.pi, n)
    alpha, beta = np.deg2rad(rng.uniform(-2, 2, n)), np.deg2rad(rng.uniform(-2, 2, n))
    alpha[::3] = beta[::3] = 0.0                                   # a third of the poses in the untilted group
    xyz = rng.uniform(-4, 4, (n, 3))
    poses = _lib.poses_array(phi, alpha, beta, xyz, np.zeros(3))
    vol = be.upload(x)
    b = be.upload(rng.standard_normal(2 * be.n_det).astype(np.float32))
    rows = (np.arange(n) % 2).astype(np.int32)
    c_all, g_all = be.cost_grad(poses, vol, b, rows=rows)
    assert np.all(np.isfinite(c_all)) and np.all(c_all > 0)
    for lo in (0, 1200, 2300, 2490):                               # windows on both sides of the internal cut, and the tail
        hi = min(n, lo + 10)
        c, g = be.cost_grad(np.ascontiguousarray(poses[lo:hi]), vol, b, rows=rows[lo:hi])
        assert np.array_equal(c, c_all[lo:hi]) and np.array_equal(g, g_all[lo:hi]), lo
    be.ctx.check(be.lib.tomo_release_workspace(be.ctx.handle))      # hands the 512 MB of partials back


@pytest.mark.parametrize("shape,ndet,step,n_proj", [((20, 24, 70), (20, 70), 1.0, 3),     # ragged, nz > 64, not multiple of 64
                                                    ((16, 16, 5), (16, 5), 1.0, 2),       # nz << 64
                                                    ((24, 24, 24), (30, 40), 0.7, 2),     # detector larger than volume, odd step
                                                    ((33, 31, 65), (33, 65), 1.0, 1)])    # single projection, odd sizes
def test_edge_shapes_vs_oracle(PM, orc, shape, ndet, step, n_proj):
    rng = np.random.default_rng(7)
    geo, og = geo_pair(n_proj, None, step=step, ndet=ndet, shape=shape)
    phi = rng.uniform(0, np.pi, n_proj)
    alpha = np.deg2rad(rng.uniform(-3, 3, n_proj))
    beta = np.deg2rad(rng.uniform(-3, 3, n_proj))
    xyz = rng.uniform(-3, 3, (n_proj, 3))
    x = rng.uniform(0, 1, shape).astype(np.float32)
    y = rng.standard_normal(n_proj * ndet[0] * ndet[1]).astype(np.float32)
    for variant in (1, 2):
        P = PM(geo)
        P.backend.ctx.set_option("fwd_variant", variant)
        A = P.projection_matrix(alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)
        want = orc.forward(og, x, alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz).ravel()
        assert rel_max(A.dot(x.ravel()), want) < TOL
        wantT = orc.adjoint(og, y, alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)
        assert rel_max(A.T.dot(y), wantT) < TOL


def test_rays_missing_the_volume_give_zero(PM):
    geo, _ = geo_pair(2, 16)
    A = PM(geo).projection_matrix(phi=np.array([0.3, 1.0]), xyz_shift=np.array([[40., 0., 0.], [0., 0., -50.]]))
    out = A.dot(np.ones(16 ** 3, np.float32))
    assert np.all(out == 0.0)
    assert np.all(A.T.dot(np.ones(2 * 256, np.float32)) == 0.0)


def test_properties_at_256(PM):
    """Config 2 size (256^3): adjointness <Ax,y> = <x,A^T y>, linearity, variant agreement."""
    N, n_proj = 256, 8
    rng = np.random.default_rng(2)
    geo, _ = geo_pair(n_proj, N)
    phi = np.linspace(0, np.pi, n_proj)
    alpha = np.deg2rad(rng.uniform(-1, 1, n_proj))
    beta = np.deg2rad(rng.uniform(-1, 1, n_proj))
    xyz = np.zeros((n_proj, 3))
    xyz[:, 0] = rng.uniform(-2, 2, n_proj)
    xyz[:, 2] = rng.uniform(-2, 2, n_proj)
    P = PM(geo)
    A = P.projection_matrix(alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)
    x1 = rng.uniform(0, 1, N ** 3).astype(np.float32)
    x2 = rng.uniform(0, 1, N ** 3).astype(np.float32)
    y = rng.uniform(0, 1, n_proj * N * N).astype(np.float32)
    Ax1, Ax2 = A.dot(x1), A.dot(x2)
    ATy = A.T.dot(y)
    lhs = np.dot(Ax1.astype(np.float64), y.astype(np.float64))
    rhs = np.dot(x1.astype(np.float64), ATy.astype(np.float64))
    assert abs(lhs - rhs) / abs(lhs) < 1e-5
    assert rel_max(A.dot(x1 + 2 * x2), Ax1 + 2 * Ax2) < TOL
    for v in (1, 2):
        P.backend.ctx.set_option("fwd_variant", v)
        assert rel_max(A.dot(x1), Ax1) < 2e-6
    P.backend.ctx.set_option("fwd_variant", 3)
    # row sums of a ray through the full volume ~ path length: every central ray of an axis-aligned view crosses N voxels
    A0 = P.projection_matrix(phi=np.array([0.0]))
    ones = A0.dot(np.ones(N ** 3, np.float32)).reshape(N, N)
    assert np.allclose(ones[8:-8, 8:-8], N, rtol=1e-5)


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_csr_materialisation_vs_reference_golden(PM, case):
    """G1: tocsr() against the reference's own projection_matrix CSR (assembled operator, not triplet order)."""
    from scipy import sparse
    g = golden("g1_operator")
    ref = sparse.csr_matrix((g[case + "_data"], g[case + "_indices"], g[case + "_indptr"]), shape=tuple(g[case + "_shape"]))
    if case == "a":
        A = PM(geo_pair(3, 8)[0]).projection_matrix()
    elif case == "b":
        A = PM(geo_pair(3, 8, cor_shift=g["b_cor"])[0]).projection_matrix(alpha=g["b_alpha"], beta=g["b_beta"], phi=g["b_phi"], xyz_shift=g["b_xyz"])
    elif case == "c":
        A = PM(geo_pair(2, 16, step=0.5, ndet=[12, 12])[0], precision=np.float64).projection_matrix(
            alpha=g["c_alpha"], beta=g["c_beta"], phi=g["c_phi"], xyz_shift=g["c_xyz"], voxel_mask=g["c_mask"])
    else:
        A = PM(geo_pair(1, 8)[0]).projection_matrix(phi=np.array([0.4]), alpha=np.array([0.01]), beta=np.array([-0.02]),
                                                    xyz_shift=np.array([[0.5, 0.0, -0.25]]))
    M = A.tocsr()
    assert sparse.isspmatrix_csr(M) and M.shape == ref.shape and M.dtype == ref.dtype
    M.sum_duplicates(); M.sort_indices()
    D = (M - ref).tocoo()
    assert (np.max(np.abs(D.data)) if D.nnz else 0.0) < (1e-12 if case == "c" else 1e-6)
    assert abs(M.nnz - ref.nnz) <= 0.002 * ref.nnz + 8      # integer coordinates: a ~1e-16 weight may sit on either neighbour
    x = np.random.default_rng(0).standard_normal(M.shape[1])
    assert rel_max(A.dot(x), M.dot(x)) < TOL                # the matrix-free kernels are this matrix


def test_triplet_emission_order_vs_oracle(PM, orc):
    from tomography_alignment_amd import _lib
    geo, og = geo_pair(1, 12)
    P = PM(geo)
    pose = _lib.poses_array([0.7], [0.02], [-0.015], np.array([[0.6, 0.3, -1.2]]), np.array([0.4, 0., 0.]))
    dat, det, wts = P.backend.triplets(pose)
    d0, r0, w0 = orc.forward_sparse(og, 0.02, -0.015, 0.7, np.array([0.6, 0.3, -1.2]), np.array([0.4, 0., 0.]))
    assert np.array_equal(dat, d0) and np.array_equal(det, r0) and np.allclose(wts, w0, rtol=0, atol=1e-12)


def test_voxel_splat_vs_reference_golden(PM):
    """G8: utilities/voxel_utilities.forward_sparse / forward_proj_grad of the reference (src/vox_wt_grad.f90)."""
    from scipy import sparse
    from tomography_alignment_amd.utilities import voxel_utilities
    g = golden("g8_voxel_splat")
    x = golden("g7_phantom")["shepp16"]
    for i in range(2):
        geo, _ = geo_pair(1, 16)
        geo.cor_shift = g["cor"][i]
        d, r, w = voxel_utilities.forward_sparse(geo, g["alpha"][i], g["beta"][i], g["phi"][i], g["xyz"][i])
        assert w.dtype == np.float32
        A = sparse.csr_matrix(sparse.coo_matrix((w, (r, d)), shape=(256, 4096)))
        ref = sparse.csr_matrix((g["s%d_data" % i], g["s%d_indices" % i], g["s%d_indptr" % i]), shape=tuple(g["s%d_shape" % i]))
        A.sum_duplicates(); A.sort_indices()
        D = (A - ref).tocoo()
        assert (np.max(np.abs(D.data)) if D.nnz else 0.0) < 2e-6 and abs(A.nnz - ref.nnz) <= 0.002 * ref.nnz + 4
        img, grad = voxel_utilities.forward_proj_grad(geo, g["alpha"][i], g["beta"][i], g["phi"][i], g["xyz"][i], x)
        assert grad.shape == (6, 256)
        assert rel_max(img, g["img%d" % i]) < TOL
        # float32 atomics add the reference's float32 terms in another order; tests/test_oracle_golden.py::
        # test_voxel_splat_gradient_conditioning measures that order to be worth ~1e-7 and the cancellation a factor 4
        e_a9 = rel_max(grad, g["grad%d" % i])
        print("A9 voxel-splat gradient vs the reference, pose %d: rel-max %.2e (image %.2e)" % (i, e_a9, rel_max(img, g["img%d" % i])))
        assert e_a9 < TOL
    P = PM(geo_pair(2, 16)[0])
    P.projection_matrix(alpha=g["alpha"], beta=g["beta"], phi=g["phi"], xyz_shift=g["xyz"])
    wts, dets, dats = P._forward_voxel()
    assert len(wts) == 2 and dets[1].min() >= 256


@pytest.mark.parametrize("shape,ndet", [((32, 32, 32), (32, 32)), ((20, 24, 70), (20, 70)), ((40, 36, 130), (44, 150))])
def test_untilted_poses_take_the_flat_tile_kernels(PM, orc, shape, ndet):
    """alpha = beta = 0 with arbitrary phi, (tx, ty, tz) and centre-of-rotation shifts: the flat tile kernels
    (uniform x,y weights, hoisted z-lerp) against the oracle and against the general tile kernels."""
    rng = np.random.default_rng(12)
    n_proj = 5
    cor = np.zeros((n_proj, 3))
    cor[:, 0] = rng.uniform(-1.5, 1.5, n_proj)
    geo, og = geo_pair(n_proj, None, ndet=ndet, shape=shape, cor_shift=cor)
    phi = np.array([0.0, 0.37, np.pi / 2, 2.2, np.pi])
    xyz = rng.uniform(-3, 3, (n_proj, 3))
    xyz[0] = 0.0                                              # fully degenerate first pose: integer coordinates
    x = rng.uniform(0, 1, shape).astype(np.float32)
    y = rng.standard_normal(n_proj * ndet[0] * ndet[1]).astype(np.float32)
    want = orc.forward(og, x, phi=phi, xyz_shift=xyz).ravel()
    wantT = orc.adjoint(og, y, phi=phi, xyz_shift=xyz)
    res = {}
    for flat, gather in ((1, 1), (1, 0), (0, 0)):     # gather-form adjoint / LDS-atomic flat adjoint / general tile kernels
        P = PM(geo)
        P.backend.ctx.set_option("tile_flat", flat)
        P.backend.ctx.set_option("adj_flat_gather", gather)
        P.backend.ctx.set_option("fwd_flat_ztiles", 2 if gather else 1)     # two-z-tile forward with the gather adjoint, else the one-tile kernel
        P.backend.ctx.profile_reset()
        P.backend.ctx.profile_enable(True)
        A = P.projection_matrix(phi=phi, xyz_shift=xyz)
        res[flat, gather] = (A.dot(x.ravel()), A.T.dot(y))
        P.backend.ctx.profile_enable(False)
        n_launch = {k: P.backend.ctx.profile_get(k)[0] for k in ("k_fwd_tile_flat", "k_adj_tile_flat", "k_adj_gather_flat", "k_adj_tile")}
        assert n_launch == {"k_fwd_tile_flat": flat, "k_adj_tile_flat": flat * (1 - gather), "k_adj_gather_flat": flat * gather,
                            "k_adj_tile": 1 - flat}
        assert rel_max(res[flat, gather][0], want) < TOL and rel_max(res[flat, gather][1], wantT) < TOL
    assert rel_max(res[1, 0][0], res[0, 0][0]) < 2e-6 and rel_max(res[1, 0][1], res[0, 0][1]) < 2e-6
    assert rel_max(res[1, 1][1], res[1, 0][1]) < 2e-6 and rel_max(res[1, 1][0], res[1, 0][0]) < 2e-6


@pytest.mark.parametrize("shape,ndet,step", [((40, 36, 130), (44, 150), 1.0), ((70, 33, 64), (70, 64), 1.0), ((33, 20, 70), (30, 80), 1.0),
                                             ((40, 36, 130), (44, 150), 0.5), ((20, 24, 200), (20, 190), 0.75), ((24, 20, 300), (24, 310), 1.0)])
def test_flat_forward_kernel_variants(PM, orc, shape, ndet, step):
    """The kernels an untilted forward projection can take, each pinned by its options -- "tab": k_fwd_flat_tab (blocks of two z-adjacent
    64-plane images, sample table in LDS; fwd_flat_gather = 0), "one tile": k_tile_flat<true> (fwd_flat_gather = 0, fwd_flat_ztiles = 1),
    "default": the gather forward where all poses qualify (the four shapes at step 1), else k_fwd_flat_tab -- compute the same projections
    as each other and as the oracle: volumes whose x extent is not a multiple of 32, exactly degenerate angles, translations, COR shifts,
    and steps below a voxel (rows with more samples in a tile than one pass of the table holds); z extents of one to three of
    k_fwd_flat_tab's 128-plane work-groups with fractional z translations (the ray between two work-groups receives a part from each)."""
    from tomography_alignment_amd import _lib
    rng = np.random.default_rng(7)
    n_proj = 5
    phi = np.array([0.0, 0.37, np.pi / 2, 2.2, np.pi])
    xyz = rng.uniform(-3, 3, (n_proj, 3))
    cor = np.zeros((n_proj, 3))
    cor[:, 0] = rng.uniform(-1.5, 1.5, n_proj)
    geo, og = geo_pair(n_proj, None, shape=shape, ndet=ndet, cor_shift=cor, step=step)
    x = rng.uniform(0.1, 1.0, shape).astype(np.float32)
    # all-zero images beside non-zero ones (the kernels skip them): the ray between two images / two work-groups of k_fwd_flat_tab
    # must still receive the part of the one that is not zero (planes 0..63 empty, 64..99 full, 100..127 empty, 128.. full)
    xs = x.copy()
    xs[:, :, :64] = 0
    xs[:, :, 100:128] = 0
    P = PM(geo)
    A = P.projection_matrix(phi=phi, xyz_shift=xyz)
    ctx = P.backend.ctx
    variants = {"tab": {"fwd_flat_gather": 0, "fwd_flat_ztiles": 2}, "one tile": {"fwd_flat_gather": 0, "fwd_flat_ztiles": 1},
                "default": {"fwd_flat_gather": 1, "fwd_flat_ztiles": 2}}
    ctx.profile_reset()
    ctx.profile_enable(True)
    n_calls = 0
    try:
        for vol in (x, xs):
            want = orc.forward(og, vol, phi=phi, xyz_shift=xyz).ravel()
            res = {}
            for name, opts in variants.items():
                for key, value in opts.items():
                    ctx.set_option(key, value)
                res[name] = A.dot(vol.ravel())
                n_calls += 1
            for name in variants:
                err = rel_max(res[name], want)
                print("%s, %s volume: vs oracle %.2e, vs tab %.2e" % (name, "dense" if vol is x else "sparse", err, rel_max(res[name], res["tab"])))
                assert err < TOL, name
            assert rel_max(res["one tile"], res["tab"]) < 2e-6 and rel_max(res["default"], res["tab"]) < 2e-6
            assert rel_max(res["default"], res["one tile"]) < 2e-6
    finally:
        for key, value in variants["default"].items():      # the library's defaults
            ctx.set_option(key, value)
        ctx.profile_enable(False)
    assert ctx.profile_get("k_fwd_tile_flat")[0] == n_calls == 6 and ctx.profile_get("k_fwd_tile")[0] == 0
    # the options of the kernel generation that k_fwd_flat_tab replaced are gone: unknown keys are an error
    with pytest.raises(_lib.TomoError):
        ctx.set_option("fwd_flat_tab", 1)
    with pytest.raises(_lib.TomoError):
        ctx.set_option("fwd_flat_wide", 0)


@pytest.mark.parametrize("tilted", [False, True])
@pytest.mark.parametrize("band", [(100, 141), (0, 3), (297, 310), (150, 151)])
def test_adjoint_with_empty_sinogram_planes(PM, orc, band, tilted):
    """The gather back-projection skips the 64-plane chunks of the volume that can only receive from all-zero detector-z planes of the
    sinogram (k_sino_zflags): a sinogram that is non-zero in a band of planes only, integer AND fractional z translations that differ per
    projection (the band reaches different voxel planes per projection), z extent of five chunks -- against the oracle's exact adjoint.
    tilted: the general tile kernel, which skips a (tile, projection) whose rays all lie in all-zero planes (prefix counts of the flags)."""
    rng = np.random.default_rng(11)
    shape, ndet, n_proj = (24, 20, 300), (24, 310), 5
    phi = np.array([0.0, 0.7, np.pi / 2, 2.4, 3.0])
    xyz = np.zeros((n_proj, 3))
    xyz[:, 0] = rng.uniform(-2, 2, n_proj)
    xyz[:, 2] = np.array([0.0, -7.0, 3.4, 12.0, -0.6])
    geo, og = geo_pair(n_proj, None, shape=shape, ndet=ndet)
    y = np.zeros((n_proj, ndet[0], ndet[1]), np.float32)
    y[:, :, band[0]:band[1]] = rng.uniform(0.1, 1.0, (n_proj, ndet[0], band[1] - band[0]))
    alpha = np.deg2rad(np.array([1.5, -2.0, 0.7, 2.0, -1.0])) if tilted else np.zeros(n_proj)
    beta = np.deg2rad(np.array([-1.0, 0.5, 2.0, -2.0, 1.2])) if tilted else np.zeros(n_proj)
    P = PM(geo)
    A = P.projection_matrix(alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)
    ctx = P.backend.ctx
    ctx.profile_reset()
    ctx.profile_enable(True)
    got = A.T.dot(y.ravel())
    ctx.profile_enable(False)
    assert ctx.profile_get("k_adj_tile" if tilted else "k_adj_gather_flat")[0] == 1 and ctx.profile_get("k_sino_zflags")[0] >= 1
    want = orc.adjoint(og, y.ravel(), alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)
    assert rel_max(got, want) < TOL
    assert np.count_nonzero(got) > 0


def test_mixed_tilted_and_untilted_call(PM, orc):
    rng = np.random.default_rng(13)
    geo, og = geo_pair(4, 24)
    phi = np.array([0.3, 1.0, 1.9, 2.7])
    alpha = np.array([0.0, 0.02, 0.0, -0.01])
    beta = np.array([0.0, 0.0, 0.0, 0.015])
    xyz = rng.uniform(-2, 2, (4, 3))
    x = rng.uniform(0, 1, 24 ** 3).astype(np.float32)
    y = rng.standard_normal(4 * 576).astype(np.float32)
    A = PM(geo).projection_matrix(alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)
    assert rel_max(A.dot(x), orc.forward(og, x, alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz).ravel()) < TOL
    assert rel_max(A.T.dot(y), orc.adjoint(og, y, alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)) < TOL


def test_config2_size_vs_oracle(PM, orc):
    """BASELINE config 2 size (256^3 volume, 256x256 detector): forward and adjoint against the CPU oracle on four of
    its angles -- two untilted (flat tile kernels), two perturbed (general tile kernels)."""
    N, n = 256, 4
    rng = np.random.default_rng(256)
    geo, og = geo_pair(n, N)
    phi = np.array([0.0, 0.9, 1.7, 2.6])
    alpha = np.array([0.0, 0.0, np.deg2rad(0.8), np.deg2rad(-0.6)])
    beta = np.array([0.0, 0.0, np.deg2rad(-0.5), np.deg2rad(0.9)])
    xyz = np.zeros((n, 3))
    xyz[1:, 0] = rng.uniform(-2, 2, 3)
    xyz[1:, 2] = rng.uniform(-2, 2, 3)
    from tomography_alignment_amd.utilities.generate_phantom import shepp3d
    x = shepp3d(N) + 0.05 * rng.uniform(0, 1, (N, N, N)).astype(np.float32)      # non-zero to the volume's edges
    y = rng.standard_normal(n * N * N).astype(np.float32)
    A = PM(geo).projection_matrix(alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)
    assert rel_max(A.dot(x.ravel()), orc.forward(og, x, alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz).ravel()) < TOL
    assert rel_max(A.T.dot(y), orc.adjoint(og, y, alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)) < TOL


def test_alignment_gradient_at_128_vs_oracle(PM, orc):
    """projection + 6-DoF gradient on a 128^3 volume (the reference needs 2.6 s per evaluation here)."""
    from tomography_alignment_amd.utilities.generate_phantom import shepp3d
    N = 128
    geo, og = geo_pair(1, N)
    x = shepp3d(N)
    P = PM(geo, precision=np.float64)
    pose = dict(alpha=np.deg2rad(1.3), beta=np.deg2rad(-0.7), phi=1.1, xyz_shift=np.array([3.2, 0.4, -4.1]), cor_shift=np.array([0.6, 0., 0.]))
    p, g = P.projection_gradient(x, **pose)
    p0, g0 = orc.projection_gradient(og, x, pose["alpha"], pose["beta"], pose["phi"], pose["xyz_shift"], pose["cor_shift"], precision=np.float64)
    assert rel_max(p, p0) < TOL
    for k in range(6):
        assert rel_max(g[k], g0[k]) < TOL, k


def test_gradient_at_cell_faces_vs_reference_f64_and_f32(PM, orc, capsys):
    """Golden G10 (64^3, every cell face a jump of the interpolant's gradient): all four kernel variants against the reference's
    float64 `projection_gradient` per ray -- value on ALL rays, gradient on the rays whose samples keep >= 4e-6 voxel (conftest.FACE_TOL_KERNELS)
    from a cell face, at 1e-5.  tests/test_oracle_golden.py::test_g10_... shows on the same fixture that the reference's own float32 routine
    disagrees with its float64 path by 0.4-3 % on rays inside that mask and nowhere else; printed here: how many of the masked rays
    the kernels put on the other side of a face, beside the reference's own count."""
    g, x, g32 = g10_case()
    N = int(g["N"])
    geo, og = geo_pair(1, N)
    P = PM(geo, precision=np.float64)
    rows = []
    for v in (1, 2, 3, 4):
        P.backend.ctx.set_option("grad_variant", v)
        for i in range(2):
            pose = (g["alpha"][i], g["beta"][i], g["phi"][i], g["xyz"][i], np.zeros(3))
            p, gr = P.projection_gradient(x.astype(np.float32), *pose)
            near = orc.ray_face_distance(og, *pose) < FACE_TOL_KERNELS
            dev, dev_ref = grad_dev_per_ray(gr, g["grad64"][i]), grad_dev_per_ray(g32[i], g["grad64"][i])
            e_p = rel_max(p, g["proj64"][i])
            rows.append((v, i, e_p, dev[~near].max(), int((dev > 1e-3).sum()), int((dev_ref > 1e-3).sum()), int(near.sum()), dev[near].max()))
            assert e_p < TOL and dev[~near].max() < TOL, rows[-1]
            assert np.all(near[dev > 1e-3])                                # a kernel's disagreements lie inside the mask, like the reference's
    P.backend.ctx.set_option("grad_variant", 4)
    with capsys.disabled():
        print()
        for r in rows:
            print("[G10 64^3] grad_variant %d pose %d: value %.1e (all rays), gradient %.1e on rays >= 4e-6 from a face; face flips (dev > 1e-3): "
                  "kernel %d, reference's own float32 routine %d, of %d masked rays (largest %.1e)" % r)


@pytest.mark.parametrize("shape,ndet", [((24, 20, 70), (24, 70)), ((16, 16, 5), (20, 9)), ((48, 40, 130), (50, 140))])
def test_gradient_kernel_variants_agree_on_odd_shapes(PM, orc, shape, ndet):
    """grad_variant 1 (plain), 2 (dword gathers, packed lerps) and 3 (four gathers + neighbour-lane DPP shift) against the
    oracle and each other, incl. large tilts where the neighbour lane often does not line up, rays that leave the volume,
    and detector rows shorter than a wave."""
    from tomography_alignment_amd import _lib
    rng = np.random.default_rng(31)
    geo, og = geo_pair(1, None, ndet=ndet, shape=shape)
    x = rng.uniform(0.1, 1, shape).astype(np.float32)
    for pose in ((0.4, 0.0, 0.0, (0.3, 0.2, -0.4)), (1.3, np.deg2rad(3.0), np.deg2rad(-4.0), (2.5, -1.0, 3.0)), (2.4, 0.6, -0.5, (-4., 2., 6.))):
        phi, alpha, beta, t = pose
        t = np.array(t)
        want_p, want_g = orc.projection_gradient(og, x, alpha, beta, phi, t, np.array([0.7, 0., 0.]), precision=np.float64)
        out = {}
        for v in (1, 2, 3):
            P = PM(geo, precision=np.float64)
            P.backend.ctx.set_option("grad_variant", v)
            out[v] = P.projection_gradient(x, alpha, beta, phi, t, np.array([0.7, 0., 0.]))
            assert rel_max(out[v][0], want_p) < TOL
            for k in range(6):
                assert rel_max(out[v][1][k], want_g[k]) < TOL, (v, k)
        assert rel_max(out[2][0], out[1][0]) < 5e-6 and rel_max(out[2][1], out[1][1]) < 5e-6    # float32 lerps in another order
        assert rel_max(out[3][0], out[2][0]) < 2e-6 and rel_max(out[3][1], out[2][1]) < 5e-6    # same positions; lerps z, y, x instead of y, x, z


@pytest.mark.parametrize("case", ["lane63_only", "lane0_only", "short_row", "all_miss", "lane63_only_tilted", "one_row_tilted"])
def test_gradient_kernels_idle_lane_addressing(PM, orc, case):
    """Regression for the GPU abort of round 1 (HISTORY.md section 8): the first neighbour-lane-shift gradient kernel let lanes
    OUTSIDE their own sample range [lo, hi) form gather addresses from their out-of-volume positions -- a wave-uniform sample
    loop with every lane loading -- and faulted as soon as such an address left mapped memory.  Today every lane loads either at
    a sample of its own range or at the borrowed address of a lane that has one.  The shapes here make that path the common
    one: a wave whose only in-range lane is lane 63 at iz = ndz - 1 (or lane 0), rows of rays that all miss the volume,
    a detector row shorter than a wave, and a launch in which no ray hits at all -- for every kernel variant, plain and fused."""
    from tomography_alignment_amd import _lib
    shape, ndet, phi, alpha, beta = (8, 8, 8), (40, 64), 0.4, 0.0, 0.0
    t = np.array([0.3, 0.2, -35.5])                   # only iz = 63 floors into the volume (index z = -0.5)
    if case == "lane0_only":
        t = np.array([0.3, 0.2, 35.5])                # only iz = 0 (index z = 7.5)
    elif case == "short_row":
        shape, ndet, t = (8, 8, 5), (12, 5), np.array([0.4, 0.0, 0.3])
    elif case == "all_miss":
        t = np.array([100.0, 0.0, 0.0])
    elif case == "lane63_only_tilted":
        alpha, beta, t = np.deg2rad(3.0), np.deg2rad(-2.0), np.array([0.3, 0.2, -35.2])
    elif case == "one_row_tilted":
        shape, ndet, alpha, beta, t = (24, 24, 70), (60, 130), np.deg2rad(-4.0), np.deg2rad(5.0), np.array([-14.5, 0.0, 2.0])
    rng = np.random.default_rng(63)
    geo, og = geo_pair(1, None, ndet=ndet, shape=shape)
    x = rng.uniform(0.1, 1, shape).astype(np.float32)
    cor = np.array([0.25, 0., 0.])
    want_p, want_g = orc.projection_gradient(og, x, alpha, beta, phi, t, cor, precision=np.float64)
    hit = int(np.count_nonzero(want_p))
    assert (hit == 0) == (case == "all_miss")
    if case in ("lane63_only", "lane0_only"):
        only = 63 if case == "lane63_only" else 0
        assert set(np.nonzero(want_p.reshape(ndet))[1]) == {only}
    n_det = ndet[0] * ndet[1]
    pose = _lib.poses_array([phi], [alpha], [beta], t, cor)
    b = (want_p + 0.1).astype(np.float32)
    res = b.astype(np.float64) - want_p.astype(np.float32)
    for v in (1, 2, 3, 4):
        P = PM(geo, precision=np.float64)
        be = P.backend
        be.ctx.set_option("grad_variant", v)
        p, g = P.projection_gradient(x, alpha, beta, phi, t, cor)
        if hit:
            assert rel_max(p, want_p) < TOL, (case, v)
            for k in range(6):
                assert rel_max(g[k], want_g[k]) < TOL, (case, v, k)
        else:
            assert not p.any() and not g.any(), (case, v)
        two = np.ascontiguousarray(np.repeat(pose, 2, axis=0))
        two[1, 5] += 200.0                                # second pose of the fused launch misses the volume entirely
        cost, g6 = be.cost_grad(two, be.upload(x), be.upload(np.concatenate([b, b])))
        assert np.isclose(cost[0], 0.5 * np.dot(res, res), rtol=1e-5) and np.isclose(cost[1], 0.5 * np.dot(b.astype(np.float64), b), rtol=1e-5)
        want6 = -np.dot(want_g.astype(np.float32).astype(np.float64), res)
        assert np.max(np.abs(g6[0] - want6)) <= TOL * max(np.dot(np.abs(want_g), np.abs(res)).max(), 1e-30), (case, v)
        assert not g6[1].any()


@pytest.mark.parametrize("case", ["box", "single_voxel", "corner_voxels", "all_zero", "nan"])
def test_rays_are_clipped_to_the_nonzero_box(PM, orc, case):
    """The ray-driven kernels (forward variants 1 / 2, every gradient variant) walk a ray only where it can see a non-zero voxel
    (box found while the volume is staged): same numbers as the oracle, which walks the whole volume."""
    shape, ndet = (40, 36, 70), (44, 80)
    rng = np.random.default_rng(77)
    x = np.zeros(shape, np.float32)
    if case == "box":
        x[12:21, 5:30, 33:61] = rng.uniform(0.1, 1, (9, 25, 28))
    elif case == "single_voxel":
        x[17, 20, 3] = 2.0
    elif case == "corner_voxels":
        x[0, 0, 0] = 1.0
        x[-1, -1, -1] = 3.0
    elif case == "nan":
        x[10:14, 10:14, 10:14] = 1.0
        x[30, 30, 60] = np.nan                           # NaN is "non-zero": rays through it must come out NaN, as in the reference
    geo, og = geo_pair(2, None, ndet=ndet, shape=shape)
    phi, alpha, beta = np.array([0.5, 2.1]), np.deg2rad([1.5, -2.5]), np.deg2rad([-1.0, 2.0])
    xyz = np.array([[1.5, 0.3, -2.0], [-2.5, 0.0, 3.0]])
    want = orc.forward(og, x, alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)
    for fv in (1, 2):
        P = PM(geo)
        P.backend.ctx.set_option("fwd_variant", fv)
        got = P.projection_matrix(alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz).dot(x.ravel()).reshape(want.shape)
        if case == "all_zero":
            assert not got.any()
        elif case == "nan":
            assert np.array_equal(np.isnan(got), np.isnan(want)) and rel_max(got[~np.isnan(want)], want[~np.isnan(want)]) < TOL
        else:
            assert rel_max(got, want) < TOL, (case, fv)
    if case == "nan":
        return
    wp, wg = orc.projection_gradient(og, x, alpha[0], beta[0], phi[0], xyz[0], np.zeros(3), precision=np.float64)
    for v in (1, 2, 3):
        P = PM(geo, precision=np.float64)
        P.backend.ctx.set_option("grad_variant", v)
        p, gr = P.projection_gradient(x, alpha[0], beta[0], phi[0], xyz[0], np.zeros(3))
        if case == "all_zero":
            assert not p.any() and not gr.any()
            continue
        assert rel_max(p, wp) < TOL, (case, v)
        for k in range(6):
            assert np.max(np.abs(gr[k] - wg[k])) <= TOL * np.max(np.abs(wg[3 * (k // 3):3 * (k // 3) + 3])), (case, v, k)


@pytest.mark.parametrize("ndet", [(384, 340), (402, 350)])      # 96 ix groups (XCD swizzle) / 101 (plain)
def test_cost_grad_cache_ordered_grid_vs_oracle(PM, orc, ndet):
    """Volumes whose padded copy exceeds the Infinity Cache make grad_variant 2 walk the grid detector-z-chunk slowest
    (csrc/tomo_project.hip: grad_zslow): same numbers as the oracle and as variant 1, every ray exactly once."""
    from tomography_alignment_amd import _lib
    shape = (400, 380, 340)
    assert (shape[0] + 4) * (shape[1] + 4) * (shape[2] + 4) * 4 > 192 << 20
    rng = np.random.default_rng(17)
    geo, og = geo_pair(1, None, ndet=ndet, shape=shape)
    # a SMOOTH object: the gradient of the trilinear interpolant jumps across cell faces, so on an object with sharp edges a
    # sample within float32 rounding of a face (a few of the 5e7 here) changes a ray's gradient by O(1) against the float64
    # oracle while its value does not move -- that would test luck, not the kernel
    ax = [np.linspace(-1, 1, m) for m in shape]
    X, Y, Z = np.meshgrid(*ax, indexing="ij", sparse=True)
    x = ((1.0 + 0.5 * np.sin(5 * X + 1) * np.cos(4 * Y) * np.sin(3 * Z + 2)) * np.exp(-3.0 * (X ** 2 + 1.3 * Y ** 2 + Z ** 2))).astype(np.float32)
    n, n_det = 3, ndet[0] * ndet[1]
    phi = np.array([0.3, 1.9, 2.8]); alpha = np.deg2rad([1.5, -2.0, 0.0]); beta = np.deg2rad([-1.0, 0.7, 0.0])
    xyz = np.array([[2.0, 0.5, -3.0], [-1.5, 0.0, 2.5], [0.0, 0.0, 0.0]]); cor = np.array([[0.4, 0, 0]] * 3)
    b = np.zeros((n, n_det), np.float32)
    want_c, want_g, scale_g, want_p = [], [], [], []
    for i in range(n):
        p, gr = orc.projection_gradient(og, x, alpha[i], beta[i], phi[i], xyz[i], cor[i])
        b[i] = p + 0.5 * rng.standard_normal(n_det).astype(np.float32)
        res = b[i].astype(np.float64) - p
        want_p.append(p)
        want_c.append(0.5 * np.dot(res, res))
        want_g.append(np.dot(-gr.astype(np.float64), res))
        scale_g.append(np.dot(np.abs(gr.astype(np.float64)), np.abs(res)))
    poses = _lib.poses_array(phi, alpha, beta, xyz, cor)
    P = PM(geo)
    be = P.backend
    vol, bd, resid = be.upload(x), be.upload(b), be.empty(n * n_det)
    out = {}
    for v in (4, 3, 2, 1):                  # 4 = per-pose choice: poses 0, 1 (tilted) -> kernel 3, pose 2 -> kernel 2, two launches
        be.ctx.set_option("grad_variant", v)
        cost, g6 = be.cost_grad(poses, vol, bd, resid)
        out[v] = (cost.copy(), g6.copy())
        assert np.allclose(cost, want_c, rtol=1e-5), v
        # the ray-direction translation telescopes to ~0 on an object that vanishes at the boundary, so errors are measured
        # against the largest component of the same unit (translations / angles), the rel_max convention of this file
        sc = np.array(scale_g)
        sc = np.concatenate([np.repeat(sc[:, 0:3].max(axis=1, keepdims=True), 3, 1), np.repeat(sc[:, 3:6].max(axis=1, keepdims=True), 3, 1)], 1)
        assert np.max(np.abs(g6 - np.array(want_g)) / sc) < TOL, v
        r = resid.download().reshape(n, -1)
        for i in range(n):
            assert np.max(np.abs((b[i] - r[i]) - want_p[i])) / np.max(np.abs(want_p[i])) < TOL, (v, i)
    assert np.allclose(out[1][0], out[2][0], rtol=1e-6)


def test_properties_at_full_size_1024():
    """BASELINE.json configs[2] size (1024^3 volume, 1024^2 detector), a few angles, everything resident on the device:
    adjointness, linearity, the tile kernels against the ray-driven ones, flat against general tile kernels, and the
    x-slab adjoint (the multi-GPU pipeline's unit) against the whole adjoint."""
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.utilities.generate_phantom import SHEPP_LOGAN
    N, n = 1024, 6
    geo, _ = geo_pair(n, N)
    be = HipBackend(geo)
    rng = np.random.default_rng(5)
    phi = np.linspace(0.1, 3.0, n)
    tilt = _lib.poses_array(phi, np.deg2rad(rng.uniform(-1, 1, n)), np.deg2rad(rng.uniform(-1, 1, n)),
                            np.column_stack([rng.uniform(-2, 2, n), np.zeros(n), rng.uniform(-2, 2, n)]), np.zeros((n, 3)))
    flat = _lib.poses_array(phi, np.zeros(n), np.zeros(n), np.column_stack([rng.uniform(-2, 2, n), np.zeros(n), rng.uniform(-2, 2, n)]),
                            np.zeros((n, 3)))
    n_vox, n_sino = N ** 3, n * N * N
    x = be.phantom(be.empty(n_vox), (N, N, N), SHEPP_LOGAN)
    y = be.upload(rng.uniform(0, 1, n_sino).astype(np.float32))
    ax, aty, tmp, tmp2 = be.empty(n_sino), be.empty(n_vox), be.empty(n_sino), be.empty(n_vox)
    for poses in (tilt, flat):
        be.forward(poses, x, ax)
        be.adjoint(poses, y, aty)
        lhs, rhs = be.dot(ax, y), be.dot(x, aty)
        assert abs(lhs - rhs) / abs(lhs) < 1e-5                         # <Ax, y> = <x, A^T y>
        # linearity: A(x + 2 A^T y) = Ax + 2 A(A^T y)
        be.copy(tmp2, x); be.axpy(tmp2, aty, 2.0)
        lin = be.forward(poses, tmp2, be.empty(n_sino)).download()
        want = ax.download() + 2.0 * be.forward(poses, aty, tmp).download()
        assert rel_max(lin, want) < TOL
        del lin, want
        # tile kernels vs the ray-driven kernels (independent code paths, same sums)
        be.ctx.set_option("fwd_variant", 2)
        assert np.sqrt(be.diff_sumsq(be.forward(poses, x, tmp), ax) / be.dot(ax, ax)) < 1e-6
        be.ctx.set_option("fwd_variant", 3)
        be.ctx.set_option("adj_variant", 1)
        assert np.sqrt(be.diff_sumsq(be.adjoint(poses, y, tmp2), aty) / be.dot(aty, aty)) < 1e-5
        be.ctx.set_option("adj_variant", 2)
        # x-slab adjoint: the slabs add up to the whole
        n_xt, _ = be.xslab_info()
        be.fill(tmp2, 0.0)
        for a, b in ((0, n_xt // 3), (n_xt // 3, n_xt - 5), (n_xt - 5, n_xt)):
            be.adjoint_xslab(poses, y, tmp2, a, b)
        assert np.sqrt(be.diff_sumsq(tmp2, aty) / be.dot(aty, aty)) < 1e-6
    # the flat kernels against the general tile kernels on the same untilted poses
    be.forward(flat, x, ax); be.adjoint(flat, y, aty)
    be.ctx.set_option("tile_flat", 0)
    assert np.sqrt(be.diff_sumsq(be.forward(flat, x, tmp), ax) / be.dot(ax, ax)) < 1e-6
    assert np.sqrt(be.diff_sumsq(be.adjoint(flat, y, tmp2), aty) / be.dot(aty, aty)) < 1e-5
    be.ctx.set_option("tile_flat", 1)
    be.ctx.set_option("fwd_flat_ztiles", 1)                      # one-tile forward kernel against the two-tile one used above
    assert np.sqrt(be.diff_sumsq(be.forward(flat, x, tmp), ax) / be.dot(ax, ax)) < 1e-6
    be.ctx.set_option("fwd_flat_ztiles", 2)
    # ... and the gather-form flat adjoint (default, used above) against the LDS-atomic flat adjoint
    be.ctx.set_option("adj_flat_gather", 0)
    assert np.sqrt(be.diff_sumsq(be.adjoint(flat, y, tmp2), aty) / be.dot(aty, aty)) < 1e-6
    be.ctx.set_option("adj_flat_gather", 1)


def _sample_tables(og, alpha, beta, phi, xyz, cor3):
    """The (3, n_rays, n) tables the reference builds in numpy before it calls its f2py routines
    (utilities/ray_voxel_utilities.py:85-99,151), from the oracle's restated ray set-up."""
    from oracle import oracle as orc
    p0, rhat, n, r_len0, src, det = orc.ray_setup(og, alpha, beta, phi, xyz, cor3)
    n_rays = p0.shape[1]
    r_points = np.zeros((3, n_rays, n))
    r_points[:, :, :] = p0[:, :, np.newaxis]
    step = np.zeros((n_rays, n))
    for j in range(n):
        r_points[:, :, j] += j * og.step_size * rhat
        step[:, j] = j * og.step_size / r_len0
    floor_points = np.floor(r_points).astype(np.int32)
    w_floor = 1. - (r_points - floor_points.astype(np.float64))
    der = orc.derivative_ray_points(src, (det - src)[:, 0], alpha, beta, phi, xyz)
    return floor_points, w_floor, step, der, n_rays, n


def test_f2py_signature_twins_vs_reference_golden(shepp32):
    """VERDICT r3 "missing" #5: `src.ray_wt_grad.trilinear_ray_interp / trilinear_ray_sparse` with the f2py module's call signatures
    (src/ray_wt_grad.f90:1-92,95-223; called at utilities/ray_voxel_utilities.py:103,164), on the library (csrc/tomo_f2py.hip):
    fed with the sample tables the reference's Python builds, against the reference's own outputs -- G3 (`projection_gradient`, all
    three generic poses; the degenerate one by value) and G1 b (the assembled CSR of generic poses with per-projection cor_shift) -- and against the oracle."""
    from oracle import oracle as orc
    from scipy import sparse
    from tomography_alignment_amd.src import ray_wt_grad
    g3 = golden("g3_proj_grad")
    og = orc.Geo(1, np.array([32] * 3), np.ones(3), np.array([32, 32]), np.ones(2))
    worst = 0.0
    for i in range(4):
        fp, wf, step, der, n_rays, n = _sample_tables(og, g3["alpha"][i], g3["beta"][i], g3["phi"][i], g3["xyz"][i], g3["cor"][i])
        img, grad = ray_wt_grad.trilinear_ray_interp(np.asfortranarray(fp), np.asfortranarray(wf), 32, 32, 32, n_rays, n,
                                                     np.asfortranarray(shepp32.ravel().astype(np.float64)), np.asfortranarray(step), np.asfortranarray(der))
        assert img.shape == (n_rays,) and grad.shape == (6, n_rays) and img.dtype == np.float64
        want_p, want_g = orc.projection_gradient(og, shepp32, g3["alpha"][i], g3["beta"][i], g3["phi"][i], g3["xyz"][i], g3["cor"][i], precision=np.float64)
        if i == 3:      # degenerate pose (samples ON integer coordinates: a last-bit difference in a position flips a cell): the value only
            assert rel_max(img, want_p) < 1e-9 and rel_max(img, g3["proj"][i]) < 2e-7
            continue
        e_o = max(rel_max(img, want_p), rel_max(grad, want_g))
        e_r = max(rel_max(img, g3["proj"][i]), rel_max(grad, g3["grad"][i]))       # the reference's outputs (stored in its `precision`, float32)
        worst = max(worst, e_o)
        assert e_o < 1e-11 and e_r < 2e-7, (i, e_o, e_r)
    # trilinear_ray_sparse: G1 b, per projection -> COO -> the reference's CSR (duplicates summed), and the raw emission order vs the oracle
    g1 = golden("g1_operator")
    N = 8
    n_proj = len(g1["b_phi"])
    og = orc.Geo(n_proj, np.array([N] * 3), np.ones(3), np.array([N, N]), np.ones(2), cor_shift=g1["b_cor"])
    rows, cols, vals = [], [], []
    for ip in range(n_proj):
        fp, wf, step, der, n_rays, n = _sample_tables(og, g1["b_alpha"][ip], g1["b_beta"][ip], g1["b_phi"][ip], g1["b_xyz"][ip], g1["b_cor"][ip])
        dat, det, wts, n_inds = ray_wt_grad.trilinear_ray_sparse(np.asfortranarray(fp), np.asfortranarray(wf), N, N, N, n_rays, n)
        assert dat.shape == (8 * n_rays * n,) and dat.dtype == np.int32 and wts.dtype == np.float64
        assert np.all(dat[n_inds:] == -999) and np.all(det[n_inds:] == -999) and np.all(wts[n_inds:] == -999.0)      # src/ray_wt_grad.f90:15-17
        o_dat, o_det, o_wts = orc.forward_sparse(og, g1["b_alpha"][ip], g1["b_beta"][ip], g1["b_phi"][ip], g1["b_xyz"][ip], g1["b_cor"][ip])
        assert n_inds == o_dat.size and np.array_equal(dat[:n_inds], o_dat) and np.array_equal(det[:n_inds], o_det) and np.allclose(wts[:n_inds], o_wts, rtol=1e-11, atol=1e-15)
        rows.append(det[:n_inds].astype(np.int64) + ip * n_rays)
        cols.append(dat[:n_inds].astype(np.int64))
        vals.append(wts[:n_inds])
    A = sparse.csr_matrix(sparse.coo_matrix((np.concatenate(vals).astype(np.float32), (np.concatenate(rows), np.concatenate(cols))), shape=tuple(g1["b_shape"])))
    A.sum_duplicates()
    A.sort_indices()
    assert np.array_equal(A.indptr, g1["b_indptr"]) and np.array_equal(A.indices, g1["b_indices"]) and rel_max(A.data, g1["b_data"]) < 1e-6
    print("f2py twins: trilinear_ray_interp vs the float64 oracle %.1e; trilinear_ray_sparse reproduces G1 b's CSR" % worst)


def test_vox_wt_grad_twin_vs_reference_golden():
    """VERDICT r5 missing 3 / next 3: `src.vox_wt_grad.bilinear_sparse / bilinear_vox_interp` with the f2py module's call signatures
    (src/vox_wt_grad.f90:1-55,58-112; called at utilities/voxel_utilities.py:69,98) on the library (tomo_bilinear_sparse / tomo_bilinear_vox_interp,
    csrc/tomo_f2py.hip):
      * G13 -- fed the very arrays the reference's Python handed to its f2py module, against what that module returned: BIT-IDENTICAL (float32 in
        the reference's operation order, additions into a pixel in voxel order), -999 tails, shapes and Fortran memory order of the returns;
      * G8 -- through the numpy of utilities/voxel_utilities.py:59-67,88-96 (restated by this package's mirror helpers) against the reference's
        forward_sparse CSR and forward_proj_grad outputs;
      * edge cases: n_vox = 0, every voxel off the detector, a 1 x 1 detector."""
    from scipy import sparse
    from tomography_alignment_amd.src import vox_wt_grad
    from tomography_alignment_amd.utilities import voxel_utilities as vu
    g = golden("g13_vox_wt_grad_arrays")
    for i in range(2):
        a = lambda k: g["p%d_%s" % (i, k)]      # noqa: E731
        n, ndx, ndz = int(a("n_vox")), int(a("ndim_x")), int(a("ndim_z"))
        dat, det, wts, k = vox_wt_grad.bilinear_sparse(n, np.asfortranarray(a("floor_x")), np.asfortranarray(a("floor_z")), np.asfortranarray(a("alpha_x")),
                                                       np.asfortranarray(a("alpha_z")), ndx, ndz)
        assert k == int(a("n_inds")) and dat.shape == (4 * n,) and dat.dtype == np.int32 and det.dtype == np.int32 and wts.dtype == np.float32
        assert np.array_equal(dat, a("dat_inds")) and np.array_equal(det, a("det_inds")) and np.array_equal(wts, a("wts"))
        img, grad = vox_wt_grad.bilinear_vox_interp(n, a("floor_x"), a("floor_z"), a("alpha_x"), a("alpha_z"), np.asfortranarray(a("rec_arg")), ndx, ndz,
                                                    np.asfortranarray(a("der")))
        assert img.shape == (ndz, ndx) and grad.shape == (6, ndz, ndx) and img.dtype == np.float32 and img.flags["F_CONTIGUOUS"] and grad.flags["F_CONTIGUOUS"]
        assert np.array_equal(img, a("det_img")) and np.array_equal(grad, a("grad_det_img"))
        assert np.array_equal(img.ravel(), a("caller_img")) and np.array_equal(grad.reshape(6, -1), a("caller_grad"))
        # a C-ordered der_points is converted as f2py converts it
        img2, grad2 = vox_wt_grad.bilinear_vox_interp(n, a("floor_x"), a("floor_z"), a("alpha_x"), a("alpha_z"), a("rec_arg"), ndx, ndz, np.ascontiguousarray(a("der")))
        assert np.array_equal(img2, img) and np.array_equal(grad2, grad)
    # G8 through the caller's numpy (utilities/voxel_utilities.py:59-67,88-96)
    g8 = golden("g8_voxel_splat")
    x = golden("g7_phantom")["shepp16"].astype(np.float32)
    for i in range(2):
        geo, _ = geo_pair(1, 16)
        rc = vu.rigid_transformation(geo.vox_centers, g8["alpha"][i], g8["beta"][i], g8["phi"][i], g8["xyz"][i])
        orig = geo.vox_origin - g8["cor"][i]
        fx, fz = np.floor(rc[0] - orig[0]).astype(np.int32), np.floor(rc[2] - orig[2]).astype(np.int32)
        ax, az = (rc[0] - orig[0] - fx).astype(np.float32), (rc[2] - orig[2] - fz).astype(np.float32)
        dat, det, wts, k = vox_wt_grad.bilinear_sparse(geo.n_vox, fx, fz, ax, az, 16, 16)
        A = sparse.csr_matrix(sparse.coo_matrix((wts[:k], (det[:k], dat[:k])), shape=(256, 4096)))
        ref = sparse.csr_matrix((g8["s%d_data" % i], g8["s%d_indices" % i], g8["s%d_indptr" % i]), shape=tuple(g8["s%d_shape" % i]))
        A.sum_duplicates(); A.sort_indices()
        assert np.array_equal(A.indptr, ref.indptr) and np.array_equal(A.indices, ref.indices) and np.array_equal(A.data, ref.data)
        der = vu.derivative_rigid(geo.vox_centers, g8["alpha"][i], g8["beta"][i], g8["phi"][i], g8["xyz"][i]).astype(np.float32)
        img, grad = vox_wt_grad.bilinear_vox_interp(geo.n_vox, fx, fz, ax, az, np.asfortranarray(x.ravel()), 16, 16, np.asfortranarray(der))
        assert np.array_equal(img.ravel(), g8["img%d" % i]) and rel_max(grad.reshape(6, -1), g8["grad%d" % i]) < 1e-6
        print("vox_wt_grad twin, G8 pose %d: image identical, gradient rel-max %.1e" % (i, rel_max(grad.reshape(6, -1), g8["grad%d" % i])))
    # a size at which the device path matters (262 144 voxels -> a million (pixel, entry) pairs to sort; several hundred voxels per pixel, so the ORDER of
    # the single-precision additions decides the last bits): against the oracle's serial restatement, which G13 pins to the f2py module bit for bit
    from oracle import oracle as orc
    rng = np.random.default_rng(13)
    nv, ndx, ndz = 64 ** 3, 70, 50
    fxr = rng.integers(-3, ndx + 2, nv).astype(np.int32)
    fzr = rng.integers(-3, ndz + 2, nv).astype(np.int32)
    axr, azr = rng.uniform(0, 1, nv).astype(np.float32), rng.uniform(0, 1, nv).astype(np.float32)
    rr = rng.uniform(-1, 1, nv).astype(np.float32)
    derr = rng.standard_normal((6, 3, nv)).astype(np.float32)
    dat, det, wts, k = vox_wt_grad.bilinear_sparse(nv, fxr, fzr, axr, azr, ndx, ndz)
    o_dat, o_det, o_wts, o_k = orc.bilinear_sparse(nv, fxr, fzr, axr, azr, ndx, ndz)
    assert k == o_k and np.array_equal(dat, o_dat) and np.array_equal(det, o_det) and np.array_equal(wts, o_wts)
    img, grad = vox_wt_grad.bilinear_vox_interp(nv, fxr, fzr, axr, azr, rr, ndx, ndz, derr)
    o_img, o_grad = orc.bilinear_vox_interp(nv, fxr, fzr, axr, azr, rr, ndx, ndz, derr)
    assert np.array_equal(img, o_img) and np.array_equal(grad, o_grad)
    # edge cases
    z = np.zeros(0, np.int32)
    dat, det, wts, k = vox_wt_grad.bilinear_sparse(0, z, z, z.astype(np.float32), z.astype(np.float32), 3, 2)
    assert k == 0 and dat.size == 0
    img, grad = vox_wt_grad.bilinear_vox_interp(0, z, z, z.astype(np.float32), z.astype(np.float32), z.astype(np.float32), 3, 2, np.zeros((6, 3, 0), np.float32))
    assert img.shape == (2, 3) and not img.any() and not grad.any()
    far = np.full(5, 100, np.int32)
    h = np.full(5, 0.25, np.float32)
    dat, det, wts, k = vox_wt_grad.bilinear_sparse(5, far, -far, h, h, 4, 4)
    assert k == 0 and np.all(dat == -999) and np.all(wts == -999.0)
    # 1 x 1 detector: voxels at floor (-1, -1), (0, -1), (-1, 0), (0, 0) reach pixel (0, 0) through corners 3, 2, 1, 0 in that voxel order
    fx1, fz1 = np.array([-1, 0, -1, 0, 5], np.int32), np.array([-1, -1, 0, 0, 5], np.int32)
    a1, b1 = np.array([0.3, 0.6, 0.1, 0.9, 0.5], np.float32), np.array([0.2, 0.7, 0.4, 0.8, 0.5], np.float32)
    r1 = np.array([1.5, 2.5, 3.5, 4.5, 9.0], np.float32)
    dat, det, wts, k = vox_wt_grad.bilinear_sparse(5, fx1, fz1, a1, b1, 1, 1)
    assert k == 4 and list(dat[:4]) == [0, 1, 2, 3] and list(det[:4]) == [0, 0, 0, 0]
    f = np.float32
    want_w = [a1[0] * b1[0], (f(1) - a1[1]) * b1[1], a1[2] * (f(1) - b1[2]), (f(1) - a1[3]) * (f(1) - b1[3])]
    assert np.array_equal(wts[:4], np.array(want_w, np.float32))
    img, _ = vox_wt_grad.bilinear_vox_interp(5, fx1, fz1, a1, b1, r1, 1, 1, np.zeros((6, 3, 5), np.float32))
    acc = f(0)
    for j, (wx, wz) in enumerate([(a1[0], b1[0]), (f(1) - a1[1], b1[1]), (a1[2], f(1) - b1[2]), (f(1) - a1[3], f(1) - b1[3])]):
        acc = f(acc + f(f(r1[j] * wx) * wz))
    assert img.shape == (1, 1) and img[0, 0] == acc


def test_gather_back_projection_of_untilted_poses_is_bit_reproducible(PM):
    """INTEGRATION.md "reproducibility": the gather-form back-projection of untilted poses (k_adj_gather_flat: every voxel column sums its own
    projections, no atomics) returns the same bits on every call; the forward projector's float32 atomics do not promise that (and are not asked to)."""
    from tomography_alignment_amd import _lib
    rng = np.random.default_rng(41)
    shape, ndet, n = (96, 80, 200), (100, 210), 24
    geo, _ = geo_pair(n, None, ndet=ndet, shape=shape)
    be = PM(geo).backend
    phi = np.linspace(0.0, np.pi, n)
    xyz = np.zeros((n, 3))
    xyz[:, 0], xyz[:, 2] = rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)
    poses = _lib.poses_array(phi, np.zeros(n), np.zeros(n), xyz, np.zeros(3))
    y = be.upload(rng.standard_normal(n * ndet[0] * ndet[1]).astype(np.float32))
    first = be.adjoint(poses, y, be.empty(int(np.prod(shape)))).download()
    assert np.abs(first).max() > 0
    for _ in range(3):
        again = be.adjoint(poses, y, be.empty(int(np.prod(shape)))).download()
        assert np.array_equal(again, first)


def test_empty_inputs(PM, shepp32):
    """Zero projections (a rank of a sharded run that owns no angle: np.array_split hands out empty blocks when there are more ranks than angles,
    recon/sirt_mpi.py:40) and zero-sized buffers: every entry point returns without touching anything it should not -- forward writes nothing, the
    back-projection of nothing is the zero volume (or leaves an accumulating target alone), the fused evaluation returns empty tables, the solver's
    vector lines accept empty segments."""
    from tomography_alignment_amd import _lib
    geo, _ = geo_pair(3, 32)
    be = PM(geo).backend
    none = np.zeros((0, _lib.POSE_STRIDE))
    vol = be.upload(shepp32)
    e0 = be.empty(0)
    assert e0.size == 0 and e0.download().size == 0
    be.forward(none, vol, e0)
    tgt = be.upload(np.full(32 ** 3, 7.0, np.float32))
    be.adjoint(none, e0, tgt, accumulate=True)
    assert np.all(tgt.download() == 7.0)
    be.adjoint(none, e0, tgt)
    assert not tgt.download().any()
    c, g = be.cost_grad(none, vol, e0)
    assert c.shape == (0,) and g.shape == (0, 6)
    c, g = be.cost_grad(none, vol, be.upload(np.zeros(1024, np.float32)), rows=np.zeros(0, np.int32))
    assert c.shape == (0,)
    assert be.dot(e0, e0) == 0.0
    be.axpy(e0, e0, 2.0)
    be.fill(e0, 1.0)
    # a sharded solver on a shard without angles: construction and the local parts of an iteration
    from tomography_alignment_amd.comm import SingleComm
    from tomography_alignment_amd.recon import sirt_mpi
    sh = sirt_mpi.SIRT._shard_geometry(geo, np.zeros(0, np.int64))
    assert sh.n_proj == 0 and sh.cor_shift.shape == (0, 3)


def test_roctx_ranges_on_demand(PM, shepp32):
    """SURVEY section 5 / VERDICT r5 next 8: roctx ranges around the projector / gradient entry points, loaded on demand (no link-time dependency):
    switching them on must find a roctx library on a ROCm box, change no result, and switching them off again must work."""
    geo, _ = geo_pair(3, 32)
    P = PM(geo)
    be = P.backend
    A = P.projection_matrix()
    want = A.dot(shepp32.ravel())
    be.ctx.set_option("roctx", 1)
    try:
        got = A.dot(shepp32.ravel())
        back = A.T.dot(got)
    finally:
        be.ctx.set_option("roctx", 0)
    assert np.array_equal(got, want) or rel_max(got, want) < 1e-6
    assert np.all(np.isfinite(back)) and np.abs(back).max() > 0


def test_context_used_from_a_helper_thread(PM, orc, shepp32):
    """HIP's current device is per thread: a context created in one thread and used from another (alignment.py evaluates its batches from a
    helper thread) binds the thread with tomo_ctx_make_current; entry points that need a geometry do it themselves.  Same results either way."""
    import threading
    from tomography_alignment_amd import _lib
    geo, og = geo_pair(2, 32)
    P = PM(geo)
    be = P.backend
    poses = _lib.poses_array(np.array([0.4, 1.9]), np.array([0.01, -0.02]), np.array([-0.015, 0.01]), np.array([[0.5, 0., -1.], [-1.5, 0., 0.7]]), np.zeros(3))
    vol = be.upload(shepp32)
    want = be.forward(poses, vol, be.empty(2 * 1024)).download()
    got = {}

    def work():
        be.ctx.make_current()
        d = be.upload(shepp32)                      # allocation + copy + launch + download, all from this thread
        got["fwd"] = be.forward(poses, d, be.empty(2 * 1024)).download()
        got["cg"] = be.cost_grad(poses, d, be.upload(want))
    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert rel_max(got["fwd"], want) < 1e-6                                          # (float atomics: equal up to the order of the additions)
    assert np.all(got["cg"][0] < 1e-6 * np.sum(want.astype(np.float64) ** 2))       # cost of the exact projections ~ 0


def test_ray_voxel_utilities_mirror_gpu(shepp32):
    """utilities/ray_voxel_utilities.py::forward_sparse / forward_proj_grad (the reference's names and returns, :53-170) on the library:
    G1 b's assembled CSR from the per-projection triplets, G3's projection + 6-row gradient, geometry not shifted in place."""
    import copy
    from scipy import sparse
    from tomography_alignment_amd.utilities import ray_voxel_utilities as rvu
    from tomography_alignment_amd.utilities.geometry import Geometry
    g1 = golden("g1_operator")
    N, n_proj = 8, len(g1["b_phi"])
    rows, cols, vals = [], [], []
    for ip in range(n_proj):
        geo = Geometry(1, np.array([N] * 3), np.ones(3), np.array([N, N]), np.ones(2))
        geo.cor_shift = g1["b_cor"][ip]
        before = copy.deepcopy(geo.source_centers)
        dat, det, wts = rvu.forward_sparse(geo, g1["b_alpha"][ip], g1["b_beta"][ip], g1["b_phi"][ip], g1["b_xyz"][ip])
        assert np.array_equal(geo.source_centers, before)
        rows.append(det.astype(np.int64) + ip * N * N)
        cols.append(dat.astype(np.int64))
        vals.append(wts)
    A = sparse.csr_matrix(sparse.coo_matrix((np.concatenate(vals).astype(np.float32), (np.concatenate(rows), np.concatenate(cols))), shape=tuple(g1["b_shape"])))
    A.sum_duplicates()
    A.sort_indices()
    assert np.array_equal(A.indptr, g1["b_indptr"]) and np.array_equal(A.indices, g1["b_indices"]) and rel_max(A.data, g1["b_data"]) < 1e-6
    g3 = golden("g3_proj_grad")
    for i in range(3):
        geo = Geometry(1, np.array([32] * 3), np.ones(3), np.array([32, 32]), np.ones(2))
        geo.cor_shift = g3["cor"][i]
        p, gr = rvu.forward_proj_grad(geo, g3["alpha"][i], g3["beta"][i], g3["phi"][i], g3["xyz"][i], shepp32)
        assert p.dtype == np.float64 and gr.shape == (6, 1024) and rel_max(p, g3["proj"][i]) < TOL and rel_max(gr, g3["grad"][i]) < TOL


def test_csr_assembled_on_the_device_equals_host_assembly(PM, capsys):
    """SURVEY 8f row N3 in full (round 4): RayOperator.tocsr() builds the reference's CSR (utilities/projection_operators.py:54-76) ON THE
    DEVICE -- triplets of all projections, mask filter, radix sort, duplicate sums, row pointers (csrc/tomo_csr.hip) -- against round 3's
    form (device triplets, scipy sort + merge on the host): same structure bit for bit, data to one float32 / float64 rounding of a duplicate
    sum; ragged shape, tilted poses, a voxel mask, both precisions, the all-masked case (the reference keeps every entry with weight 0,
    :63-65), the transposed operator; and what it buys at 64^3 x 8 (printed)."""
    import time
    from scipy import sparse
    rng = np.random.default_rng(77)
    shape, ndet, n = (24, 20, 28), (26, 30), 5
    geo, _ = geo_pair(n, None, ndet=ndet, shape=shape)
    phi = rng.uniform(0, np.pi, n)
    alpha, beta = np.deg2rad(rng.uniform(-2, 2, n)), np.deg2rad(rng.uniform(-2, 2, n))
    xyz = rng.uniform(-2, 2, (n, 3))
    mask = rng.uniform(size=shape) > 0.4
    for prec, tol in ((np.float32, 3e-7), (np.float64, 1e-15)):
        for m in (None, mask, np.zeros(shape, bool)):
            A = PM(geo, precision=prec).projection_matrix(alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz, voxel_mask=m)
            D, H = A.tocsr(), A.tocsr(device=False)
            H.sum_duplicates()
            H.sort_indices()
            assert D.dtype == H.dtype == np.dtype(prec) and D.shape == H.shape and D.has_sorted_indices
            assert np.array_equal(D.indptr, H.indptr) and np.array_equal(D.indices, H.indices), (prec, m is None)
            assert np.max(np.abs(D.data - H.data), initial=0.0) <= tol * max(1.0, np.max(np.abs(H.data), initial=0.0))
            if m is not None and not m.any():
                assert D.nnz > 0 and not D.data.any()                      # every entry kept, all weights zero
            T = A.T.tocsr()
            assert T.shape == (D.shape[1], D.shape[0]) and abs(T.sum() - D.sum()) <= 1e-5 * abs(D.sum()) + 1e-12
    # max_nnz is enforced BEFORE anything is allocated on the host or downloaded, the device copy is dropped on refusal
    # (a second fetch finds nothing), and the operator assembles again afterwards
    from tomography_alignment_amd import _lib
    with pytest.raises(MemoryError):
        A.tocsr(max_nnz=D.nnz - 1)
    be_ = A.backend
    with pytest.raises(_lib.TomoError, match="nothing assembled"):
        be_.ctx.check(be_.lib.tomo_csr_fetch(be_.ctx.handle, None, None, np.zeros(4, np.int64).ctypes.data_as(_lib._c_vp)))
    assert A.tocsr(max_nnz=D.nnz).nnz == D.nnz
    # what it buys: 64^3 x 8 (the reference itself: 35 s for 90 angles at this size)
    geo64, _ = geo_pair(8, 64)
    A = PM(geo64).projection_matrix()
    t0 = time.perf_counter(); D = A.tocsr(); t1 = time.perf_counter(); H = A.tocsr(device=False); t2 = time.perf_counter()
    with capsys.disabled():
        print("\n[CSR 64^3 x 8] %d stored entries: assembled on the device in %.2f s (incl. download), device triplets + scipy on the host %.2f s"
              % (D.nnz, t1 - t0, t2 - t1))
    assert D.nnz == H.nnz
