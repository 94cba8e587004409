"""Worker of tests/test_gpu_regularized_recon.py: one rank of the angle-sharded RegularizedRecon with the REAL HIP backend (every rank
opens its own context on GPU 0) and tests/_gloo_gpu_worker.py's host-staged gloo communicator standing in for RCCL.  Every rank writes
what it computed to <out>.rank<r>.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(out_path):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="env://")
    from _gloo_gpu_worker import HostStagedComm
    from reg_standin import SHARD_CASES, shard_problem
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.recon import regularized_mpi

    ctx = _lib.Context(0)
    comm = HostStagedComm(ctx)
    geo, b, angles, xyz, x = shard_problem()
    out = {}
    for tag, meth, kw in SHARD_CASES:
        for gt in (False, True):
            r = regularized_mpi.RegularizedRecon(comm, geo, b, angles, xyz, options={"ground_truth": x} if gt else {})
            rec, rms = getattr(r, meth)(**kw)
            key = "%s_%d" % (tag, int(gt))
            out[key + "_rec"], out[key + "_rms"], out[key + "_k"] = np.asarray(rec), np.asarray(rms), np.array(len(rms))
    np.savez(out_path + ".rank%d.npz" % comm.rank, **out)
    dist.barrier()
    ctx.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
