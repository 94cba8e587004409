"""
The reference's examples/mpi_reconstruct.py (:14-71): reconstruct a Shepp-Logan phantom from 90 untilted projections with one of
the three penalties of recon/regularized_mpi.RegularizedRecon -- 'Tikh' (Tikhonov gradient descent, positivity), 'Lasso' (accelerated
ISTA) or 'TV' (TV-FISTA) -- with the reference's parameters, and write recon.npy.

Differences: the phantom is generated on the device; each rank projects and keeps only its own sinogram rows (the reference projects
its rows into a full-size zero array and all-reduces it as an all-gather); the recon runs on the device.  One process per GPU under
torch.distributed.run picks up the RCCL communicator (RcclComm.from_env(), as examples/align_rigid.py does); without one the serial class
runs.  Plotting (the reference's make_plot=True) is not provided.
    python -m tomography_alignment_amd.examples.mpi_reconstruct [TV|Tikh|Lasso] [N] [n_proj] [niter]
"""
import sys

import numpy as np

from ..backend import HipBackend
from ..recon import regularized, regularized_mpi
from ..utilities.geometry import Geometry
from ..utilities.generate_phantom import SHEPP_LOGAN
from ..utilities.projection_operators import ProjectionMatrix

PENALTIES = ('Tikh', 'Lasso', 'TV')


def run(penalty='TV', N=64, n_proj=90, niter=500, comm=None, out='recon.npy'):
    """-> (rec, rms_error) of `penalty` (rank 0 writes `out` unless it is None)."""
    if penalty not in PENALTIES:
        raise ValueError('%s penalty not implemented' % penalty)                                   # :68-70
    phi = np.linspace(0.0, np.pi, n_proj)                                                          # :20-24
    alpha, beta, xyz = np.zeros(n_proj), np.zeros(n_proj), np.zeros((n_proj, 3))
    geom = Geometry(n_proj, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2))       # :27-28
    rank, size = (0, 1) if comm is None else (comm.rank, comm.size)
    my = np.array_split(np.arange(n_proj), size)[rank]                                              # :35
    my_geom = regularized_mpi._shard_geometry(geom, my)
    be = HipBackend(my_geom, ctx=None if comm is None else comm.ctx)
    d_truth = be.phantom(be.empty(N ** 3), (N, N, N), SHEPP_LOGAN)                                 # :15
    A = ProjectionMatrix(my_geom, backend=be).projection_matrix(alpha=alpha[my], beta=beta[my], phi=phi[my], xyz_shift=xyz[my])
    d_proj = A.apply(d_truth)                                                                      # :38-39: this rank's rows only
    angles = np.array([phi, alpha, beta]).T
    opts = {'ground_truth': d_truth, 'rec': None, '_backend': be}                                  # :47-48
    if comm is None:
        rec_obj = regularized.RegularizedRecon(geom, d_proj, angles, xyz, options=opts)
    else:
        rec_obj = regularized_mpi.RegularizedRecon(comm, geom, d_proj, angles, xyz, options=opts)
    if penalty == 'Tikh':                                                                          # :52-66
        rec, err = rec_obj.run_tikhonov_gd(niter=niter, reg_param=0.1, positivity=True)
    elif penalty == 'Lasso':
        rec, err = rec_obj.run_lasso_accelerated(niter=niter, reg_param=1.0, beta=0.8)
    else:
        rec, err = rec_obj.run_fista(niter=niter, hyper=1.e4, beta_tv=0.1)
    if rank == 0 and out is not None:
        np.save(out, rec)                                                                          # :72-73
    return rec, err


def main(argv=None):
    import os
    a = list(sys.argv[1:] if argv is None else argv)
    penalty = a[0] if a else 'TV'
    N, n_proj, niter = (int(v) for v in (a[1:4] + ['64', '90', '500'][len(a[1:4]):]))
    comm = None
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:       # python -m torch.distributed.run --nproc-per-node N -m ...mpi_reconstruct
        from ..comm import RcclComm
        comm = RcclComm.from_env()
    rec, err = run(penalty, N, n_proj, niter, comm=comm)
    if comm is None or comm.rank == 0:
        print('%s: %d iterations, rms %.5f -> %.5f' % (penalty, len(err), err[0], err[-1]))
    if comm is not None:
        comm.close()


if __name__ == '__main__':
    main()
