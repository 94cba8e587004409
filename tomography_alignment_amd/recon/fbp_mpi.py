"""
Angle-sharded filtered back-projection: recon/fbp.py's FBP with the communicator first, as recon/sirt_mpi.py's SIRT.  Rank r filters and
back-projects its np.array_split block of the projections (recon/sirt_mpi.py:40) and one all-reduce of the volume (the communicator's
`allreduce_sum_`: comm.RcclComm, comm.SingleComm or anything with that method) gives every rank the full FBP.  The angle weights are
computed from ALL the angles, so the sum over the ranks is the unsharded FBP.
"""
import numpy as np

from . import fbp as _fbp
from .sirt_mpi import SIRT as _ShardedSIRT


class FBP(_fbp.FBP):

    def __init__(self, comm, geometry, projections, angles, xyz_shifts, options={}):
        self.comm = comm
        self.size = comm.Get_size() if hasattr(comm, "Get_size") else comm.size
        self.my_rank = comm.Get_rank() if hasattr(comm, "Get_rank") else comm.rank
        n_proj = np.asarray(angles).reshape(-1, 3).shape[0]
        self.my_index = np.array_split(np.arange(n_proj), self.size)[self.my_rank]     # sirt_mpi.py:40
        self.my_n_proj = np.size(self.my_index)
        opts = dict(options)
        if '_backend' not in opts and getattr(comm, "ctx", None) is not None:
            from ..backend import HipBackend
            opts['_backend'] = HipBackend(self._local_geometry(self.my_index, geometry), ctx=comm.ctx)
        super(FBP, self).__init__(geometry, projections, angles, xyz_shifts, opts)

    def _my_rows(self):
        return self.my_index

    def _local_geometry(self, rows, geometry=None):
        return _ShardedSIRT._shard_geometry(self.geometry if geometry is None else geometry, rows)

    def _allreduce_vol(self, buf):
        return self.comm.allreduce_sum_(buf)
