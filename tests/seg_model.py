"""The definitions of include/tomo_seg.h / tomography_alignment_amd/segment.py in plain numpy and Python (no scipy): float32 comparisons
for the threshold, integers for the region and the tables, a breadth-first flood in linear-index order for the labels (which numbers
the components by their smallest linear index by construction), math.fsum for the sums.  Volumes are [nx][ny][nz], z fastest."""
import itertools
import math

import numpy as np

from tomography_alignment_amd import _seg_lib

import vol_model as vm

TX, TY, TZ = _seg_lib.TILE_X, _seg_lib.TILE_Y, _seg_lib.TILE_Z

# The degenerate ones; per axis one below, at and one above the brick edge with the other two small and no multiple of 4; one shape that
# crosses a brick edge in all three axes; nz % 4 == 0 with small and with brick-crossing x, y (the 16-byte path); two bricks and a bit
# along every axis, the largest.
GPU_SHAPES = ([(1, 1, 1), (1, 1, 7), (5, 1, 1), (3, 4, 5)]
              + [(TX + d, 3, 5) for d in (-1, 0, 1)] + [(3, TY + d, 5) for d in (-1, 0, 1)] + [(3, 5, TZ + d) for d in (-1, 0, 1)]
              + [(TX + 1, TY + 2, TZ + 3), (5, 6, 8), (TX + 2, TY + 1, TZ + 8), (2 * TX + 1, 2 * TY + 2, 2 * TZ + 2)])
LARGEST = GPU_SHAPES[-1]
CROSSING = (TX + 1, TY + 2, TZ + 3)


# ------------------------------------------------------------------------------------------------------------------------ definitions

def threshold(v, lo=None, hi=None, R4=-1):
    """uint8: inside the region, not NaN, lo <= v and v <= hi in float32 for the bounds that are given.  So +inf (-inf) passes only
    when hi (lo) is missing."""
    v = np.asarray(v, np.float32)
    assert lo is not None or hi is not None
    ok = ~np.isnan(v)
    with np.errstate(invalid="ignore"):
        if lo is not None:
            ok &= v >= np.float32(lo)
        if hi is not None:
            ok &= v <= np.float32(hi)
    ok &= vm.region(v.shape[0], v.shape[1], R4)[:, :, None]
    return ok.astype(np.uint8)


def _j(classes_counts):
    """sum over the classes in order of M M / W in float64, M and W exact integers; an empty class adds 0."""
    total = 0.0
    first = True
    for lo, c in classes_counts:
        w = int(c.sum())
        m = int((c * np.arange(lo, lo + c.size, dtype=np.int64)).sum())
        term = np.float64(m) * np.float64(m) / np.float64(w) if w > 0 else np.float64(0.0)
        total = term if first else total + term
        first = False
    return total


def otsu(counts, edges, classes=2):
    """Brute force over every cut (every ordered pair of cuts) after bins 0 ... nbins - 2; the first maximum in index order."""
    c = np.asarray(counts).astype(np.int64)
    nb = c.size
    best, cuts = None, None
    if classes == 2:
        for t in range(nb - 1):
            j = _j([(0, c[:t + 1]), (t + 1, c[t + 1:])])
            if best is None or j > best:
                best, cuts = j, (t,)
    else:
        for t1 in range(nb - 2):
            for t2 in range(t1 + 1, nb - 1):
                j = _j([(0, c[:t1 + 1]), (t1 + 1, c[t1 + 1:t2 + 1])])
                j = j + _j([(t2 + 1, c[t2 + 1:])])
                if best is None or j > best:
                    best, cuts = j, (t1, t2)
    return tuple(np.float32(edges[t + 1]) for t in cuts)


def offsets(connectivity):
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(abs(a) for a in d) <= connectivity]


def label(mask, connectivity=1):
    """-> (labels int32, n): flood from every unlabelled foreground voxel in ascending linear index."""
    m = np.asarray(mask) != 0
    nx, ny, nz = m.shape
    pad = np.zeros((nx + 2, ny + 2, nz + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = m
    sx, sy = (ny + 2) * (nz + 2), nz + 2
    offs = [dx * sx + dy * sy + dz for dx, dy, dz in offsets(connectivity)]
    flat = pad.ravel()
    fg = flat.tolist()
    lab = [0] * len(fg)
    n = 0
    for i in np.flatnonzero(flat).tolist():                  # the padded index rises with the linear index
        if lab[i]:
            continue
        n += 1
        lab[i] = n
        queue = [i]
        while queue:
            nxt = []
            for j in queue:
                for o in offs:
                    k = j + o
                    if fg[k] and not lab[k]:
                        lab[k] = n
                        nxt.append(k)
            queue = nxt
    return np.array(lab, np.int32).reshape(pad.shape)[1:-1, 1:-1, 1:-1].copy(), n


def measure(labels, n, vol=None):
    """-> dict: count int64 (n,), bbox int32 (n, 6), coord_sum int64 (n, 3), centroid float64 (n, 3); with vol: min, max float32 (NaN
    without a finite value), sum (math.fsum of the finite values, float64) and sumabs (of their magnitudes)."""
    labels = np.asarray(labels, np.int32)
    fg = (labels >= 1) & (labels <= n)
    k = labels[fg].astype(np.int64) - 1
    coords = [c[fg].astype(np.int64) for c in np.indices(labels.shape)]
    out = {"count": np.bincount(k, minlength=n).astype(np.int64)}
    bbox = np.zeros((n, 6), np.int32)
    csum = np.zeros((n, 3), np.int64)
    for a, c in enumerate(coords):
        lo, hi = np.full(n, np.iinfo(np.int32).max, np.int64), np.full(n, np.iinfo(np.int32).min, np.int64)
        np.minimum.at(lo, k, c)
        np.maximum.at(hi, k, c)
        np.add.at(csum[:, a], k, c)
        bbox[:, 2 * a], bbox[:, 2 * a + 1] = lo, hi
    out["bbox"], out["coord_sum"] = bbox, csum
    with np.errstate(invalid="ignore", divide="ignore"):
        out["centroid"] = csum.astype(np.float64) / out["count"].astype(np.float64)[:, None]
    if vol is not None:
        v = np.asarray(vol, np.float32)[fg]
        fin = np.isfinite(v)
        kf, vf = k[fin], v[fin]
        mn, mx = np.full(n, np.inf, np.float32), np.full(n, -np.inf, np.float32)
        np.minimum.at(mn, kf, vf)
        np.maximum.at(mx, kf, vf)
        none = np.bincount(kf, minlength=n) == 0
        mn[none], mx[none] = np.nan, np.nan
        order = np.argsort(kf, kind="stable")
        parts = np.split(vf[order].astype(np.float64), np.cumsum(np.bincount(kf, minlength=n))[:-1]) if n else []
        out["min"], out["max"] = mn, mx
        out["sum"] = np.array([math.fsum(p) for p in parts], np.float64)
        out["sumabs"] = np.array([math.fsum(np.abs(p)) for p in parts], np.float64)
        out["n_finite"] = np.bincount(kf, minlength=n).astype(np.int64)
    return out


def remove_small(labels, n, min_size):
    labels = np.asarray(labels, np.int32)
    count = np.bincount(labels[(labels >= 1) & (labels <= n)].astype(np.int64) - 1, minlength=n)
    keep = count >= min_size
    new = np.zeros(n + 1, np.int32)
    new[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    return new[np.where((labels >= 1) & (labels <= n), labels, 0)], int(keep.sum())


def largest(labels, n):
    labels = np.asarray(labels, np.int32)
    if n == 0:
        return np.zeros(labels.shape, np.uint8)
    count = np.bincount(labels[(labels >= 1) & (labels <= n)].astype(np.int64) - 1, minlength=n)
    return (labels == int(np.argmax(count)) + 1).astype(np.uint8)          # argmax: the first of equals


# ------------------------------------------------------------------------------------------------------------------------ masks

def bernoulli(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def checkerboard(shape):
    x, y, z = np.indices(shape)
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def even_lattice(shape):
    x, y, z = np.indices(shape)
    return ((x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0)).astype(np.uint8)


def serpentine(shape, cut=False):
    """A one-voxel-wide path through the whole volume: along z in the rows of even y, a connector on every odd y between two of them at
    alternating z ends; that in every plane of even x, the planes joined on the odd x at the plane path's end and start in turn.
    cut: the voxel in the middle of the middle row of the middle plane removed."""
    nx, ny, nz = shape
    m = np.zeros(shape, np.uint8)
    rows = list(range(0, ny, 2))
    for x in range(0, nx, 2):
        for r, y in enumerate(rows):
            m[x, y, :] = 1
            if y + 2 < ny:
                m[x, y + 1, nz - 1 if r % 2 == 0 else 0] = 1
    start = (0, 0)
    end = (rows[-1], nz - 1 if len(rows) % 2 == 1 else 0)
    for p, x in enumerate(range(1, nx - 1, 2)):
        m[(x,) + (end if p % 2 == 0 else start)] = 1
    if cut:
        m[(nx // 2) // 2 * 2, rows[len(rows) // 2], nz // 2] = 0
    return m


def rods(shape, axis, joined=True):
    """Rods along `axis` at the even positions of the other two axes, which meet (joined) only in the last plane of the axis: they are
    trees of their own through every brick but the last."""
    idx = np.indices(shape)
    others = [a for a in range(3) if a != axis]
    last = idx[axis] == shape[axis] - 1
    m = (idx[others[0]] % 2 == 0) & (idx[others[1]] % 2 == 0) & ~last
    if joined:
        m |= last
    return m.astype(np.uint8)


def nested_u(shape):
    """In every plane of even z: U shapes nested in each other in (x, y), arms along x at y = 2k and ny - 1 - 2k that meet only in
    their bottom at x = nx - 1 - 2k.  Every U of every plane is a component of its own."""
    nx, ny, nz = shape
    m = np.zeros(shape, np.uint8)
    k = 0
    while 2 * k < nx and 2 * k <= ny - 1 - 2 * k:
        a, b, bottom = 2 * k, ny - 1 - 2 * k, nx - 1 - 2 * k
        if b - a == 1:
            break                                            # the two arms would touch
        m[:bottom + 1, a, ::2] = 1
        m[:bottom + 1, b, ::2] = 1
        m[bottom, a:b + 1, ::2] = 1
        k += 1
    return m


EDGE_PAIRS = [(1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1)]
CORNER_PAIRS = [(1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)]


def pairs_at_corner(shape, corner):
    """Masks of two voxels that share only an edge (first) or only a corner: the first voxel at corner + {-1, 0}^3.
    -> list of (kind, mask)."""
    out = []
    for base in itertools.product((-1, 0), repeat=3):
        p = tuple(c + b for c, b in zip(corner, base))
        for kind, ds in (("edge", EDGE_PAIRS), ("corner", CORNER_PAIRS)):
            for d in ds:
                q = tuple(a + b for a, b in zip(p, d))
                if all(0 <= a < n for a, n in zip(p + q, shape + shape)):
                    m = np.zeros(shape, np.uint8)
                    m[p], m[q] = 1, 1
                    out.append((kind, m))
    return out


def structured(shape):
    """name -> mask: the patterns that separate the connectivities and the ones that force long chains and late merges."""
    return {"zeros": np.zeros(shape, np.uint8), "ones": np.ones(shape, np.uint8), "checkerboard": checkerboard(shape),
            "even lattice": even_lattice(shape), "serpentine": serpentine(shape), "serpentine cut": serpentine(shape, True),
            "rods x": rods(shape, 0), "rods y": rods(shape, 1), "rods z": rods(shape, 2), "rods x apart": rods(shape, 0, False),
            "nested u": nested_u(shape)}
