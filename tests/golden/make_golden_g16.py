#!/usr/bin/env python3
"""
G16: the reference at detector and voxel pitches other than one -- its own Python (utilities/geometry.py, projection_operators.py,
voxel_utilities.py), its two f2py modules and `back_project_` of libref_mf.so, run on a 12 x 10 x 14 volume.  Imports make_golden for
its shims and helpers.  Written: g16_pitch.npz, data only.

Per pitch combination (CASES) and per step (1.0 and 0.7), with `cor_shift` x = 0.6 and five poses (three with tilts up to +-2 deg and
x / z shifts, two untilted, one of them at phi = 0):
  * `A . x` and `A^T . y` of `ProjectionMatrix(geo, precision=float64).projection_matrix(...)` in float64 for seeded x, y (stored as
    float32: the values are float32 numbers, so that float32 and float64 routines see the same inputs).  The CSR itself is not stored;
  * `projection_gradient` (value and six rows, float64) of the first two poses, at one of the two steps (they alternate from one
    combination to the next: the file stays below the size of the largest golden before it).
For the combination with voxel pitch (1.5, 1, 0.75) also the voxel-driven routines, as G4 / G8 hold them at unit pitch: `back_project_`
(float32) for three poses, and `voxel_utilities.forward_sparse` (as a canonical CSR) / `forward_proj_grad` for two.

Run in the authoring container:  oracle/build_ref.sh && python tests/golden/make_golden_g16.py
"""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (shims + reference on sys.path)
import numpy as np  # noqa: E402
from scipy import sparse  # noqa: E402
from utilities import geometry, projection_operators, voxel_utilities  # noqa: E402

SHAPE = (12, 10, 14)
STEPS = (1.0, 0.7)
COR = np.array([0.6, 0.0, 0.0])
# tag -> (detector pitch (x, z), voxel pitch, detector shape): detector shape x pitch is near the volume's footprint
CASES = {
    "dx08":     ((0.8, 1.0), (1.0, 1.0, 1.0), (15, 14)),        # anisotropic, finer in x
    "dx2":      ((2.0, 1.0), (1.0, 1.0, 1.0), (6, 14)),         # anisotropic, binned in x
    "d05":      ((0.5, 0.5), (1.0, 1.0, 1.0), (24, 28)),        # detector-z pitch < 1
    "dz2":      ((1.0, 2.0), (1.0, 1.0, 1.0), (12, 7)),         # detector-z pitch > 1
    "d13":      ((1.3, 1.25), (1.0, 1.0, 1.0), (9, 11)),        # neither pitch a simple fraction
    "vox2":     ((2.0, 2.0), (2.0, 2.0, 2.0), (12, 14)),        # voxel pitch 2: the rotation axis leaves the index grid's centre
    "vox_anis": ((1.0, 1.0), (1.5, 1.0, 0.75), (14, 12)),       # anisotropic voxel pitch; the voxel-driven routines too
}
VOXEL_DRIVEN = "vox_anis"


def poses(seed):
    rng = np.random.default_rng(seed)
    n = 5
    phi = np.array([0.45, 1.3, 2.6, 0.0, 2.0])
    alpha, beta = np.zeros(n), np.zeros(n)
    alpha[:3], beta[:3] = np.deg2rad(rng.uniform(-2, 2, 3)), np.deg2rad(rng.uniform(-2, 2, 3))
    xyz = np.zeros((n, 3))
    xyz[:, 0], xyz[:, 2] = rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n)
    return phi, alpha, beta, xyz


def main():
    out = {"shape": np.array(SHAPE), "steps": np.array(STEPS), "cor": COR, "tags": np.array(sorted(CASES))}
    for k, tag in enumerate(sorted(CASES)):
        det_pix, vox_pix, det_shape = CASES[tag]
        rng = np.random.default_rng(1600 + k)
        phi, alpha, beta, xyz = poses(1650 + k)
        n = phi.size
        n_det = det_shape[0] * det_shape[1]
        x = rng.uniform(0.1, 1.0, SHAPE).astype(np.float32)
        y = rng.standard_normal(n * n_det).astype(np.float32)
        out.update({tag + "_det_pix": np.array(det_pix), tag + "_vox_pix": np.array(vox_pix), tag + "_det_shape": np.array(det_shape),
                    tag + "_phi": phi, tag + "_alpha": alpha, tag + "_beta": beta, tag + "_xyz": xyz, tag + "_x": x, tag + "_y": y})
        for step in STEPS:
            geo = geometry.Geometry(n, np.array(SHAPE), np.array(vox_pix), np.array(det_shape), np.array(det_pix), cor_shift=COR, step_size=step)
            P = projection_operators.ProjectionMatrix(geo, precision=np.float64)
            A = P.projection_matrix(alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz)
            assert A.dtype == np.float64 and A.shape == (n * n_det, int(np.prod(SHAPE)))
            Ax = sparse.csr_matrix.dot(A, x.ravel().astype(np.float64))
            ATy = sparse.csc_matrix.dot(sparse.csr_matrix.transpose(A), y.astype(np.float64))
            s = "%s_s%02d" % (tag, round(10 * step))
            out[s + "_Ax"], out[s + "_ATy"], out[s + "_nnz"] = Ax, ATy, np.array(A.nnz)
            if step != STEPS[k % 2]:
                print("   g16 %-8s step %.1f: nnz %6d, rays with a non-zero sum %4.0f %%, max|Ax| %.3f" % (tag, step, A.nnz, 100.0 * np.mean(Ax != 0), np.abs(Ax).max()))
                continue
            P1 = projection_operators.ProjectionMatrix(geometry.Geometry(1, np.array(SHAPE), np.array(vox_pix), np.array(det_shape), np.array(det_pix),
                                                                         step_size=step), precision=np.float64)
            pg = [P1.projection_gradient(x.astype(np.float64), alpha[i], beta[i], phi[i], xyz[i], COR) for i in range(2)]
            out[s + "_proj"], out[s + "_grad"] = np.array([p for p, _ in pg]), np.array([g for _, g in pg])
            print("   g16 %-8s step %.1f: nnz %6d, rays with a non-zero sum %4.0f %%, max|Ax| %.3f, max|grad| %.3f"
                  % (tag, step, A.nnz, 100.0 * np.mean(Ax != 0), np.abs(Ax).max(), np.abs(out[s + "_grad"]).max()))
    out.update(voxel_driven(VOXEL_DRIVEN))
    mg.save("g16_pitch", **out)


def voxel_driven(tag):
    det_pix, vox_pix, det_shape = CASES[tag]
    ndx, ndz = det_shape
    rng = np.random.default_rng(1699)
    out = {}
    # back_project_ (src/back_projection.f90), float32, as G4 calls it
    lib = ctypes.CDLL(os.path.join(mg.ROOT, "oracle", "_ref", "libref_mf.so"))
    n = 3
    phi = np.array([0.6, 1.7, 2.9])
    alpha, beta, xyz = mg.jitter(rng, n, 2.0, 1.5)
    geo = geometry.Geometry(n, np.array(SHAPE), np.array(vox_pix), np.array(det_shape), np.array(det_pix))
    y = rng.standard_normal((n, ndx, ndz)).astype(np.float32)
    f32 = np.float32
    F = lambda a: np.asfortranarray(a, dtype=f32)  # noqa: E731
    I = lambda v: ctypes.byref(ctypes.c_int32(int(v)))  # noqa: E731
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    atx = np.zeros(geo.n_vox, dtype=f32)
    lib.back_project_(P(F(alpha)), P(F(beta)), P(F(phi)), P(F(xyz.T)), P(F(geo.vox_centers)), P(F(geo.vox_origin)), P(F(y)), I(n), I(geo.n_vox), I(ndx), I(ndz), P(atx))
    assert np.abs(atx).max() > 0
    out.update(bp_phi=phi, bp_alpha=alpha, bp_beta=beta, bp_xyz=xyz, bp_y=y, bp_atx=atx)
    # the voxel splat (utilities/voxel_utilities.py + src/vox_wt_grad.f90), as G8 holds it
    phi = np.array([0.6, 2.2])
    alpha, beta, xyz = mg.jitter(rng, 2, 2.0, 1.5)
    cor = rng.uniform(-1, 1, (2, 3))
    x = rng.uniform(0.1, 1.0, SHAPE).astype(np.float32)
    out.update(vs_phi=phi, vs_alpha=alpha, vs_beta=beta, vs_xyz=xyz, vs_cor=cor, vs_x=x)
    for i in range(2):
        geo = geometry.Geometry(1, np.array(SHAPE), np.array(vox_pix), np.array(det_shape), np.array(det_pix))
        geo.cor_shift = cor[i]
        d, r, w = voxel_utilities.forward_sparse(geo, alpha[i], beta[i], phi[i], xyz[i])
        A = sparse.csr_matrix(sparse.coo_matrix((w, (r, d)), shape=(geo.n_det, geo.n_vox)))
        for k, v in mg.csr_canon(A).items():
            out["vs%d_%s" % (i, k)] = v
        img, grad = voxel_utilities.forward_proj_grad(geo, alpha[i], beta[i], phi[i], xyz[i], x)
        out["vs_img%d" % i], out["vs_grad%d" % i] = img, grad
        print("   g16 voxel splat %d: %d entries, max|img| %.3f, max|grad| %.3f" % (i, A.nnz, np.abs(img).max(), np.abs(grad).max()))
    return out


if __name__ == "__main__":
    main()
