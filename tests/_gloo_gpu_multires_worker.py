"""Worker of tests/test_gpu_multires.py: one rank of the angle-sharded examples/align_rigid.run_multires with the REAL HIP backend (every
rank opens its own context on GPU 0) and tests/backends.py's host-staged gloo communicator standing in for RCCL.  Every rank
writes what it computed to <out>.rank<r>.npz."""
import numpy as np

from gloo_world import rank_main


def body(comm, ctx):
    import torch
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.examples import align_rigid
    from tomography_alignment_amd.utilities.geometry import Geometry
    from tomography_alignment_amd.utilities.generate_phantom import shepp3d

    N, n_proj = 48, 12                                                    # the problem of _gloo_gpu_worker.align_rigid_stages
    rng = np.random.default_rng(17)
    x = shepp3d(N).astype(np.float32)
    phi = np.linspace(0.0, np.pi, n_proj)
    alpha, beta = np.deg2rad(rng.uniform(-0.8, 0.8, n_proj)), np.deg2rad(rng.uniform(-0.8, 0.8, n_proj))
    xyz = np.zeros((n_proj, 3))
    xyz[:, 0], xyz[:, 2] = rng.uniform(-1.5, 1.5, n_proj), rng.uniform(-1.5, 1.5, n_proj)
    geo = Geometry(n_proj, np.array([N] * 3), np.ones(3), np.array([N, N]), np.ones(2))
    full = HipBackend(geo, ctx=ctx)
    b = full.forward(_lib.poses_array(phi, alpha, beta, xyz, np.zeros(3)), full.upload(x), full.empty(n_proj * N * N)).download().reshape(n_proj, N, N)
    t = torch.from_numpy(np.ascontiguousarray(b))                         # rank 0's copy on every rank (float32 atomics in the forward projector)
    comm.dist.broadcast(t, src=0)
    data = dict(projections=t.numpy(), phi=phi, phantom=x, xyz=xyz, alpha=alpha, beta=beta)
    rec, a, bb, tt, hist = align_rigid.run_multires(data, levels=3, n_outer=(2, 2, 2), sirt_iters=8, verbose=False, comm=comm)
    spread = max(comm.allreduce_max(float(v)) + comm.allreduce_max(-float(v)) for v in np.concatenate([a, bb, tt.ravel()]))
    return dict(rec=rec, alpha=a, beta=bb, xyz=tt, spread=spread, injected=np.abs(xyz[:, [0, 2]]).mean(),
                rmse=np.array([h["rmse"] for h in hist]), shift_err=np.array([h["shift_err_px"] for h in hist]),
                tilt_err=np.array([h["tilt_err_deg"] for h in hist]), factor=np.array([h["factor"] for h in hist]),
                ranks=np.array([h["ranks"] for h in hist]))


if __name__ == "__main__":
    rank_main(body, gpu=True, per_rank=True)
