"""numpy models of libtomo_pyr.so's three operations (include/tomo_pyr.h), used by tests/test_multires.py and tests/test_gpu_multires.py,
and a host stand-in of multires.Pyramid over tests/backends.Buf for the CPU test of examples/align_rigid.run_multires."""
import numpy as np


def bin_sino(x, f, scale=None):
    """[n][nx][nz] -> [n][nx/f][nz/f]: float32(S * c), S the float64 sum of a bin, c = double(float32(scale)) / f^2; scale None: 1 / f."""
    x = np.asarray(x, np.float32)
    n, nx, nz = x.shape
    c = float(np.float32(1.0 / f if scale is None else scale)) / (f * f)
    return (x.astype(np.float64).reshape(n, nx // f, f, nz // f, f).sum(axis=(2, 4)) * c).astype(np.float32)


def bin_vol(x, f, scale=1.0):
    x = np.asarray(x, np.float32)
    nx, ny, nz = x.shape
    c = float(np.float32(scale)) / (f * f * f)
    return (x.astype(np.float64).reshape(nx // f, f, ny // f, f, nz // f, f).sum(axis=(1, 3, 5)) * c).astype(np.float32)


def _prolong_axis(v, axis):
    """Fine index i samples the coarse axis at (i + 0.5) / 2 - 0.5: 3/4 of cell i // 2, 1/4 of its neighbour on i's side, index clamped."""
    n = v.shape[axis]
    i = np.arange(2 * n)
    near = i // 2
    far = np.clip(near + np.where(i % 2 == 1, 1, -1), 0, n - 1)
    return 0.75 * np.take(v, near, axis=axis) + 0.25 * np.take(v, far, axis=axis)


def prolong(v, scale=1.0):
    """[nx][ny][nz] -> [2nx][2ny][2nz] in float64 (the GPU works in float32)."""
    v = np.asarray(v, np.float64)
    for axis in range(3):
        v = _prolong_axis(v, axis)
    return v * float(np.float32(scale))


class HostPyramid(object):
    """multires.Pyramid's three methods on tests/backends.Buf buffers, through the models above; records its calls."""

    def __init__(self):
        self.calls = []

    def bin_projections(self, proj, f, scale=None, out=None, shape=None):
        from backends import Buf
        self.calls.append(("bin_projections", f, tuple(shape)))
        return Buf(bin_sino(proj.a.reshape(shape), f, scale))

    def bin_volume(self, vol, f, shape=None, scale=1.0, out=None):
        from backends import Buf
        self.calls.append(("bin_volume", f, tuple(shape)))
        return Buf(bin_vol(vol.a.reshape(shape), f, scale))

    def prolong_volume(self, vol, shape=None, scale=1.0, out=None):
        from backends import Buf
        self.calls.append(("prolong_volume", 2, tuple(shape)))
        return Buf(prolong(vol.a.reshape(shape), scale).astype(np.float32))

    def close(self):
        pass
