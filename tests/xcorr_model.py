"""numpy models of the two align_cc chains (float64, numpy.fft + scipy.ndimage + the pcc stand-in), with the GPU module's decisions:
float64 means, filters in image-axis order, each aligned image rounded to the input dtype.  Used by tests/test_gpu_align_cc.py."""
import numpy as np
from scipy import ndimage

import pcc_standin as ps


def chain_numpy(proj):
    n, nx, nz = proj.shape
    fr, fk = ps.cc_filters(nx, nz)
    off = np.zeros((n, 2))
    out = proj.copy()
    margins = [np.inf]
    for i in range(1, n):
        img = proj[i].astype(np.float64)
        ref = out[i - 1].astype(np.float64)
        a = np.fft.fft2((img - img.mean()) * fr)
        b = np.fft.fft2((ref - ref.mean()) * fr)
        xcor = np.abs(np.fft.ifft2(np.conj(a) * b * fk))
        k, m = ps._argmax_margin(xcor)
        s = np.unravel_index(k, xcor.shape)
        off[i] = s
        margins.append(m)
        out[i] = np.roll(np.roll(proj[i], s[0], axis=0), s[1], axis=1)
    off[off[:, 0] > nx / 2, 0] -= nx
    off[off[:, 1] > nz / 2, 1] -= nz
    return off, out, np.array(margins)


def chain_skimage(proj, u=100):
    n = proj.shape[0]
    off = np.zeros((n, 2))
    out = proj.copy()
    margins = [(np.inf, np.inf)]
    for i in range(1, n):
        s, _, _, m = ps.phase_cross_correlation_margins(out[i - 1], out[i], u)
        off[i] = s
        margins.append(m)
        out[i] = ndimage.shift(out[i], s)
    return off, out, np.array(margins)
