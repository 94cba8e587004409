"""
Angle-sharded RegularizedRecon: the constructor / method signatures of the reference's recon/regularized_mpi.py (`comm` first), with the
mpi4py communicator replaced by RCCL (tomography_alignment_amd.comm.RcclComm) -- or any object exposing `size`, `rank`,
`allreduce_sum_(buffer)` and `allreduce_array(float64 array)`.

Decomposition (regularized_mpi.py:57-66): rank r owns the angle block np.array_split(arange(n_proj), size)[r] and its sinogram rows, and a
full replica of every volume.  Per gradient ONE whole-volume all-reduce of A_r^T res_r (:115-116, 222-223, 327-328, 438-439); the
sums over sinogram rows (||res||^2, the line searches' data terms) are summed over the ranks once per point where the reference
all-reduces, all of a point's slots in one collective (recon/cgls_mpi.py's _sum_accs pattern).

Where the reference runs the TV prox (:130-137) and the accelerated update (:452-457) on rank 0 and broadcasts the pickled volume, here
EVERY rank computes them, redundantly, on the all-reduced gradient: the all-reduce hands every rank the same bits, the kernels are
deterministic (csrc/tomo_reg.hip), so every rank holds the same volume bit for bit and no broadcast is needed.  Every control decision
(stop rule, Armijo acceptance, the backtracking test g <= gp, FISTA's t, the TV prox's dual-gap stop) is taken from all-reduced scalars
or from deterministic sums over those identical volumes, so no rank can stop, or accept a step, alone.
"""
import numpy as np

from .regularized import RegularizedRecon as _RR
from .sirt_mpi import SIRT as _SIRTM

_shard_geometry = _SIRTM._shard_geometry


class RegularizedRecon(_RR):

    def __init__(self, comm, geometry, projections, angles, xyz_shifts, options={}):
        self.comm = comm
        self.size = comm.Get_size() if hasattr(comm, "Get_size") else comm.size
        self.my_rank = comm.Get_rank() if hasattr(comm, "Get_rank") else comm.rank
        self.my_index = np.array_split(np.arange(angles.shape[0]), self.size)[self.my_rank]     # regularized_mpi.py:59
        self.my_n_proj = np.size(self.my_index)
        opts = dict(options)
        if '_backend' not in opts and getattr(comm, "ctx", None) is not None:
            try:
                from ..backend import HipBackend
            except ImportError:
                from backend import HipBackend
            opts['_backend'] = HipBackend(_shard_geometry(geometry, self.my_index), ctx=comm.ctx)
        super(RegularizedRecon, self).__init__(geometry, projections, angles, xyz_shifts, opts)

    def _my_rows(self):
        return self.my_index

    def _local_geometry(self, rows):
        return _shard_geometry(self.geometry, rows)              # regularized_mpi.py:62-66

    def _allreduce_vol(self, buf):
        return self.comm.allreduce_sum_(buf)

    def _sum_accs(self, slot0, n):
        """Accumulators [slot0, slot0 + n) summed over the ranks: one device-side all-reduce where the communicator is the backend's own
        RCCL one, else the fetched values through the communicator's small host all-reduce."""
        be, comm = self.be, self.comm
        if getattr(comm, "device_scalars", False) and getattr(be, "ctx", None) is getattr(comm, "ctx", None):
            return be.acc_fetch(slot0, n, allreduce=True)
        vals = np.array(be.acc_fetch(slot0, n), np.float64)
        if self.size > 1:
            comm.allreduce_array(vals)
        return vals

    def _scalars(self, n_row, n_vol):
        """Row slots summed over the ranks (one collective), then the whole-volume slots as this rank has them -- identical on every
        rank already, so they are not reduced."""
        out = [float(v) for v in self._sum_accs(0, n_row)] if n_row else []
        if n_vol:
            out += [float(v) for v in self.be.acc_fetch(n_row, n_vol)]
        return out

    def _is_root(self):
        return self.my_rank == 0
