"""Worker of tests/test_gpu_fbp.py: one rank of the angle-sharded FBP (recon/fbp_mpi.py) with the REAL HIP backend (every rank opens its
own context on GPU 0) and tests/backends.py's host-staged gloo communicator standing in for RCCL.  Every rank writes what it
computed to <out>.rank<r>.npz."""
import numpy as np

from gloo_world import rank_main


def problem():
    """32^3 blobs, 37 angles over [0, pi] with tilts, shifts and a centre-of-rotation offset (projections from the oracle)."""
    from fbp_model import blob_phantom
    from oracle import oracle as orc
    N, n = 32, 37
    rng = np.random.default_rng(7)
    phi = np.linspace(0, np.pi, n)
    alpha, beta = np.deg2rad(rng.uniform(-1, 1, n)), np.deg2rad(rng.uniform(-1, 1, n))
    xyz = np.zeros((n, 3))
    xyz[:, 0], xyz[:, 2] = rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)
    cor = np.array([0.7, 0.0, 0.0])
    og = orc.Geo(n, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2), cor_shift=cor)
    x = blob_phantom(N, seed=3, n_blobs=5)
    p = orc.forward(og, x, alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz).reshape(n, N, N).astype(np.float32)
    return N, phi, alpha, beta, xyz, cor, p


def body(comm, ctx):
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.recon import fbp_mpi
    from tomography_alignment_amd.utilities.geometry import Geometry

    N, phi, alpha, beta, xyz, cor, p = problem()
    geo = Geometry(phi.size, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2), cor_shift=cor)
    angles = np.array([phi, alpha, beta]).T
    out = {}
    for filt in ("ramp", "hann"):
        f = fbp_mpi.FBP(comm, geo, p, angles, xyz, options={"filter": filt})
        out[filt] = f.run()
        out[filt + "_rows"] = np.asarray(f.my_index)
    return out


if __name__ == "__main__":
    rank_main(body, gpu=True, per_rank=True)
