"""float64 model of recon/fbp.py (numpy FFT filter + the CPU oracle's adjoint), the per-column-pair error measure of the filter tests and
the blob phantom the FBP accuracy tests use.
Used by tests/test_fbp.py (CPU) and tests/test_gpu_fbp.py."""
import numpy as np

from oracle import oracle as orc
from tomography_alignment_amd.recon import fbp


def filter_model(p, filter="ramp", scales=None):
    """q = s * IDFT(H . DFT(pad(p)))[:ndx] along axis 1 of p (n_proj, ndx, ndz), float64."""
    p = np.asarray(p, np.float64)
    n_proj, ndx, ndz = p.shape
    npad = fbp.padded_length(ndx)
    H = fbp.filter_response(ndx, filter)
    Hf = np.concatenate([H, H[1:-1][::-1]])             # even: H[Npad - j] = H[j]
    q = np.real(np.fft.ifft(np.fft.fft(p, n=npad, axis=1) * Hf[None, :, None], axis=1))[:, :ndx]
    if scales is not None:
        q = q * np.asarray(scales, np.float64)[:, None, None]
    return q


def pair_errs(got, ref):
    """max|got - ref| / max|ref| per projection and column pair (2s, 2s+1) -- the two columns one complex signal of the kernel carries --
    both maxima over the pair's two columns and all rows; a trailing lone column is a pair of its own.  Shape (n_proj, ceil(ndz / 2))."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    out = np.empty((ref.shape[0], (ref.shape[2] + 1) // 2))
    for s in range(out.shape[1]):
        r = ref[:, :, 2 * s:2 * s + 2]
        out[:, s] = np.max(np.abs(got[:, :, 2 * s:2 * s + 2] - r), axis=(1, 2)) / np.maximum(np.max(np.abs(r), axis=(1, 2)), 1e-300)
    return out


def pair_err(got, ref):
    """The worst pair of pair_errs."""
    return float(np.max(pair_errs(got, ref)))


def fbp_model(og, proj, phi, alpha=None, beta=None, xyz=None, filter="ramp", weights=None):
    """FBP of proj (n_proj, ndx, ndz) on the oracle geometry og: filter_model with the scales of recon/fbp.py, then the oracle's
    adjoint (which reads float32 values)."""
    phi = np.asarray(phi, np.float64)
    w = fbp.angle_weights(phi) if weights is None else np.asarray(weights, np.float64)
    q = filter_model(proj, filter, fbp.projection_scales(og, w))
    return orc.adjoint(og, q.reshape(phi.size, -1), alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz).reshape(tuple(int(v) for v in og.vox_shape))


def blob_phantom(N, seed=0, n_blobs=12):
    """Sum of Gaussian blobs, sigma 3-6 voxels, centres inside radius 0.7 N/2 of the rotation axis (x, y) and of the z middle."""
    rng = np.random.default_rng(seed)
    c = (np.arange(N) - (N - 1) / 2.0)
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    vol = np.zeros((N, N, N))
    r_max = 0.7 * N / 2
    for _ in range(n_blobs):
        sig = rng.uniform(3, 6)
        rr = rng.uniform(0, r_max - 2 * sig) if r_max > 2 * sig else 0.0
        th = rng.uniform(0, 2 * np.pi)
        cx, cy = rr * np.cos(th), rr * np.sin(th)
        cz = rng.uniform(-(N / 2 - 2 * sig), N / 2 - 2 * sig)
        vol += rng.uniform(0.5, 1.0) * np.exp(-((X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2) / (2 * sig ** 2))
    return vol


def cylinder_mask(N, frac=1.0):
    """Voxels inside the cylinder of radius frac * N/2 about the rotation axis (z)."""
    c = (np.arange(N) - (N - 1) / 2.0)
    X, Y = np.meshgrid(c, c, indexing="ij")
    return np.broadcast_to(((X ** 2 + Y ** 2) <= (frac * N / 2) ** 2)[:, :, None], (N, N, N))


def accuracy(rec, truth):
    """(rel-L2 error, mean ratio) inside the inscribed cylinder."""
    m = cylinder_mask(truth.shape[0])
    r, t = np.asarray(rec, np.float64)[m], np.asarray(truth, np.float64)[m]
    return float(np.linalg.norm(r - t) / np.linalg.norm(t)), float(r.mean() / t.mean())
