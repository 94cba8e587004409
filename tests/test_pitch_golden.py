"""Detector and voxel pitches other than one, on the CPU: the oracle against golden G16 (the reference's own routines at seven pitch
combinations, tests/golden/make_golden_g16.py), and the geometry struct the library is handed against what the oracle's `Geo` implies.
Bars: those of tests/test_oracle_golden.py -- float64 restatements 1e-11, the float32 routines as G4 (back_project_) and G8 (voxel splat)."""
import numpy as np
from scipy import sparse

from conftest import golden, rel_max
from oracle import oracle as orc
from test_oracle_golden import assert_same_operator, csr_of


def g16_geo(g, tag, n_proj, step=1.0, cor=None, cls=orc.Geo):
    return cls(n_proj, np.array(g["shape"]), np.array(g[tag + "_vox_pix"]), np.array(g[tag + "_det_shape"]), np.array(g[tag + "_det_pix"]),
               cor_shift=cor, step_size=step)


def test_g16_oracle_at_non_unit_pitch():
    g = golden("g16_pitch")
    tags = [str(t) for t in g["tags"]]
    assert len(tags) == 7
    n_grad = 0
    for tag in tags:
        kw = dict(alpha=g[tag + "_alpha"], beta=g[tag + "_beta"], phi=g[tag + "_phi"], xyz_shift=g[tag + "_xyz"])
        n = kw["phi"].size
        for step in g["steps"]:
            s = "%s_s%02d" % (tag, round(10 * float(step)))
            G = g16_geo(g, tag, n, float(step), g["cor"])
            e_f = rel_max(orc.forward(G, g[tag + "_x"], **kw).ravel(), g[s + "_Ax"])
            e_a = rel_max(orc.adjoint(G, g[tag + "_y"], **kw), g[s + "_ATy"])
            A = orc.projection_matrix(G, precision=np.float64, **kw)
            line = "G16 %-8s step %.1f: forward %.1e adjoint %.1e, nnz %d (reference %d)" % (tag, step, e_f, e_a, A.nnz, int(g[s + "_nnz"]))
            assert e_f <= 1e-11 and e_a <= 1e-11, line
            assert abs(A.nnz - int(g[s + "_nnz"])) <= 0.002 * int(g[s + "_nnz"]) + 8, line
            assert np.mean(g[s + "_Ax"] != 0) > 0.25                 # no case holds on zeros
            if s + "_grad" in g.files:
                G1 = g16_geo(g, tag, 1, float(step))
                for i in range(2):
                    p, gr = orc.projection_gradient(G1, g[tag + "_x"], kw["alpha"][i], kw["beta"][i], kw["phi"][i], kw["xyz_shift"][i], g["cor"], precision=np.float64)
                    e_p, e_g = rel_max(p, g[s + "_proj"][i]), rel_max(gr, g[s + "_grad"][i])
                    line += "; pose %d value %.1e gradient %.1e" % (i, e_p, e_g)
                    assert e_p <= 1e-11 and e_g <= 1e-11, line
                    n_grad += 1
            print(line)
    assert n_grad == 2 * len(tags)


def test_g16_oracle_voxel_driven_at_non_unit_voxel_pitch():
    g = golden("g16_pitch")
    tag = "vox_anis"
    assert np.array_equal(g[tag + "_vox_pix"], [1.5, 1.0, 0.75])
    n = g["bp_phi"].size
    G = g16_geo(g, tag, n)
    atx = orc.back_project_voxel(G, g["bp_y"], g["bp_alpha"], g["bp_beta"], g["bp_phi"], g["bp_xyz"])
    e_bp = rel_max(atx, g["bp_atx"])
    print("G16 back_project_ at voxel pitch (1.5, 1, 0.75): rel-max %.2e" % e_bp)
    assert e_bp < 2e-5                                              # A6: float32 both sides (the bar of G4)
    for i in range(2):
        G = g16_geo(g, tag, 1)
        pose = (g["vs_alpha"][i], g["vs_beta"][i], g["vs_phi"][i], g["vs_xyz"][i], g["vs_cor"][i])
        d, r, w = orc.vox_forward_sparse(G, *pose)
        A = sparse.csr_matrix(sparse.coo_matrix((w, (r, d)), shape=(G.n_det, G.n_vox)))
        assert_same_operator(A, csr_of(g, "vs%d" % i), 1e-6)
        img, grad = orc.vox_forward_proj_grad(G, *pose, g["vs_x"])
        e_i, e_g = rel_max(img, g["vs_img%d" % i]), rel_max(grad, g["vs_grad%d" % i])
        print("G16 voxel splat %d: image %.2e gradient %.2e" % (i, e_i, e_g))
        assert e_i < 2e-6 and e_g < 2e-5                            # the bars of G8


def test_geom_struct_matches_the_oracles_geometry_at_every_g16_pitch():
    """What `_lib.geom_struct` hands to tomo_set_geometry from the package's Geometry, against the oracle's independent `Geo` of the same
    arguments: origin, detector origin and pitches, source / detector planes, voxel pitch.  The detector pitches are differences of
    linspace values (the grid the rays start from), equal to `det_pix` only up to rounding."""
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.utilities.geometry import Geometry
    g = golden("g16_pitch")
    for tag in (str(t) for t in g["tags"]):
        s = _lib.geom_struct(g16_geo(g, tag, 3, 0.7, g["cor"], cls=Geometry))
        og = g16_geo(g, tag, 3, 0.7, g["cor"])
        ndx, ndz = (int(v) for v in og.det_shape)
        assert (s.nx, s.ny, s.nz, s.ndx, s.ndz) == tuple(int(v) for v in og.vox_shape) + (ndx, ndz) and s.step == 0.7
        src, det = og.source_centers, og.det_centers
        want = dict(det_x0=src[0, 0], det_z0=src[2, 0], det_dx=src[0, ndz] - src[0, 0], det_dz=src[2, 1] - src[2, 0], src_y=src[1, 0], det_y=det[1, 0])
        for k, v in want.items():
            assert getattr(s, k) == v, (tag, k, getattr(s, k), v)
        assert [s.vox_origin[a] for a in range(3)] == list(og.vox_origin) and [s.vox_pitch[a] for a in range(3)] == list(og.vox_pix)
        # the rays of the last row and plane start where the oracle's do
        assert np.isclose(s.det_x0 + (ndx - 1) * s.det_dx, src[0, -1], rtol=0, atol=1e-12) and np.isclose(s.det_z0 + (ndz - 1) * s.det_dz, src[2, -1], rtol=0, atol=1e-12)
        assert abs(s.det_dx - og.det_pix[0]) < 1e-12 and abs(s.det_dz - og.det_pix[1]) < 1e-12
        assert s.src_y == -og.vox_size[1] and s.det_y == og.vox_size[1]
