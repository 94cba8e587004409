"""Worker of tests/test_gpu_resolution.py: one rank of resolution.half_set_fsc with the REAL HIP backend (every rank opens its own context
on GPU 0) and tests/backends.py's host-staged gloo communicator standing in for RCCL.  The rank computes the curve once from the
host array of all projections and once from a device buffer that holds only its own np.array_split block, and writes both, and the raw
table of the second, to <out>.rank<r>.npz."""
import numpy as np

from gloo_world import rank_main


def body(comm, ctx):
    from tomography_alignment_amd import _lib, resolution
    from tomography_alignment_amd.examples import generate_data
    from tomography_alignment_amd.utilities.geometry import Geometry

    d = generate_data.make(64, 90, seed=3)
    n = d["phi"].size
    geo = Geometry(n, np.array([64, 64, 64]), np.ones(3), np.array([64, 64]), np.ones(2))
    angles = np.array([d["phi"], d["alpha"], d["beta"]]).T
    proj = np.asarray(d["projections"], np.float32)
    out = {}
    c = resolution.half_set_fsc(geo, proj, angles, d["xyz"], comm=comm)
    out.update(host_fsc=c.fsc, host_count=c.count, host_PA=c.PA)
    mine = np.array_split(np.arange(n), comm.size)[comm.rank]
    d_p = ctx.to_device(proj.reshape(n, -1)[mine].ravel())
    c = resolution.half_set_fsc(geo, d_p, angles, d["xyz"], comm=comm)
    out.update(device_fsc=c.fsc, device_count=c.count, device_PA=c.PA, table=np.array([c.C, c.PA, c.PB, c.count]), rows=mine)
    return out


if __name__ == "__main__":
    rank_main(body, gpu=True, per_rank=True)
