"""Worker of tests/test_gpu_regularized_recon.py: one rank of the angle-sharded RegularizedRecon with the REAL HIP backend (every rank
opens its own context on GPU 0) and tests/backends.py's host-staged gloo communicator standing in for RCCL.  Every rank writes
what it computed to <out>.rank<r>.npz."""
import numpy as np

from gloo_world import rank_main


def body(comm, ctx):
    from reg_standin import SHARD_CASES, shard_problem
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.recon import regularized_mpi

    geo, b, angles, xyz, x = shard_problem()
    out = {}
    for tag, meth, kw in SHARD_CASES:
        for gt in (False, True):
            r = regularized_mpi.RegularizedRecon(comm, geo, b, angles, xyz, options={"ground_truth": x} if gt else {})
            rec, rms = getattr(r, meth)(**kw)
            key = "%s_%d" % (tag, int(gt))
            out[key + "_rec"], out[key + "_rms"], out[key + "_k"] = np.asarray(rec), np.asarray(rms), np.array(len(rms))
    return out


if __name__ == "__main__":
    rank_main(body, gpu=True, per_rank=True)
