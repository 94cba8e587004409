"""Worker of tests/test_regularized_recon.py: one rank of the angle-sharded RegularizedRecon over torch.distributed (gloo, CPU) with the
numpy stand-in backend.  Every rank writes what it computed to <out>.rank<r>.npz."""
import numpy as np

from gloo_world import rank_main


def body(comm, ctx):
    from backends import Buf
    from reg_standin import RegOracleBackend, SHARD_CASES, shard_problem
    from tomography_alignment_amd.recon import regularized_mpi

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
    return out


if __name__ == "__main__":
    rank_main(body, per_rank=True)
