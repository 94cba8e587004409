"""Worker of tests/test_regularized_recon.py: one rank of the angle-sharded RegularizedRecon over torch.distributed (gloo, CPU) with the
numpy stand-in backend.  Every rank writes what it computed to <out>.rank<r>.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(out_path):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="env://")
    from backends import Buf, GlooComm
    from reg_standin import RegOracleBackend, SHARD_CASES, shard_problem
    from tomography_alignment_amd.recon import regularized_mpi

    comm = GlooComm()
    geo, b, angles, xyz, x = shard_problem()
    my = np.array_split(np.arange(angles.shape[0]), comm.size)[comm.rank]
    shard = regularized_mpi._shard_geometry(geo, my)
    out = {}
    for tag, meth, kw in SHARD_CASES:
        for gt in (False, True):
            opts = {"_backend": RegOracleBackend(shard)}
            if gt:
                opts["ground_truth"] = x
            r = regularized_mpi.RegularizedRecon(comm, geo, b, angles, xyz, options=opts)
            assert np.array_equal(r.my_index, my)
            rec, rms = getattr(r, meth)(**kw)
            key = "%s_%d" % (tag, int(gt))
            out[key + "_rec"], out[key + "_rms"], out[key + "_k"] = np.asarray(rec), np.asarray(rms), np.array(len(rms))
    # the collectives themselves: identical bits on every rank (rank-dependent, non-representable inputs)
    rng = np.random.default_rng(100 + comm.rank)
    v = Buf(rng.standard_normal(10007).astype(np.float32) * np.float32(1.1))
    comm.allreduce_sum_(v)
    a = rng.standard_normal(37) * 1.1
    comm.allreduce_array(a)
    out["probe_vol"], out["probe_arr"] = v.a.copy(), a
    np.savez(out_path + ".rank%d.npz" % comm.rank, **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
