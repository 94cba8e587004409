"""The definitions of include/tomo_morph.h in numpy, the yardstick of test_morphology.py and test_gpu_morphology.py: the squared Euclidean
distance transform as three exact integer min-plus line passes (an O(n^2) broadcast per axis), the ball by its integer test, hole
filling by scipy-free flood labels (seg_model.label), and the shapes and masks the GPU tests run."""
import numpy as np

from tomography_alignment_amd import _morph_lib

import seg_model as sm

INF = _morph_lib.INF
W, MAX_WQ, GROUP, LINE_LIMIT = _morph_lib.W, _morph_lib.MAX_WQ, _morph_lib.GROUP, _morph_lib.LINE_LIMIT
CHUNK = GROUP // MAX_WQ             # the line length at which a full work-group's lanes each own one group of W columns
R2 = (0, 1, 2, 3, 4, 5, 6, 8, 9, 12)

# the degenerate ones; per axis one below, at and one above W and CHUNK with the other axes small and no multiple of 4 (nz = 4 and 32
# are the shapes with nz % 4 == 0); a line longer than a work-group, and than the length from which a work-group owns fewer than MAX_WQ
# groups (LINE_LIMIT / MAX_WQ = 256), on each axis alone; 64 and 68 columns: exactly MAX_WQ groups and one more, nz % 4 == 0; and one
# shape past every edge at once, several work-groups in every pass.
GPU_SHAPES = ([(1, 1, 1), (1, 1, 7), (5, 1, 1), (7, 1, 3)]
              + [tuple(n if a == axis else (3, 5, 3)[a] for a in range(3)) for axis in range(3)
                 for n in (W - 1, W, W + 1, CHUNK - 1, CHUNK, CHUNK + 1)]
              + [(300, 3, 5), (3, 300, 5), (3, 5, 300), (6, 5, W * MAX_WQ), (5, 6, W * MAX_WQ + 4)]
              + [(CHUNK + 1, CHUNK + 2, W * MAX_WQ + 3)])
GPU_SHAPES = list(dict.fromkeys(GPU_SHAPES))                           # the three small ones of the axis sweeps coincide
CROSSING = GPU_SHAPES[-1]
assert LINE_LIMIT // MAX_WQ < 300


def _line_pass(f, axis, border):
    """g[i] = min_j f[j] + (i - j)^2 along `axis`; border: positions -1 and n hold 0.  int64 in, int64 out, clamped to INF."""
    f = np.moveaxis(f, axis, -1)
    n = f.shape[-1]
    i = np.arange(n, dtype=np.int64)
    cost = (i[:, None] - i[None, :]) ** 2                                 # [i][j]
    flat = f.reshape(-1, n)
    out = np.empty_like(flat)
    step = max(1, (1 << 22) // (n * n))
    for a in range(0, flat.shape[0], step):
        out[a:a + step] = (flat[a:a + step, None, :] + cost[None]).min(axis=2)
    if border:
        out = np.minimum(out, np.minimum(i + 1, n - i) ** 2)
    out = np.minimum(out, INF)
    return np.moveaxis(out.reshape(f.shape), -1, axis)


def distance_sq(mask, border="ignore"):
    """int32: 0 on the background, else min |p - b|^2 over the background voxels b (border "background": and every position outside
    the volume); INF where there is none."""
    if border not in ("ignore", "background"):
        raise ValueError(border)
    f = np.where(np.asarray(mask) != 0, np.int64(INF), np.int64(0))
    for axis in (2, 1, 0):
        f = _line_pass(f, axis, border == "background")
    return f.astype(np.int32)


def root(d2):
    """float32: the correctly rounded root, INF -> +inf."""
    d2 = np.asarray(d2)
    with np.errstate(invalid="ignore"):
        r = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    return np.where(d2 == INF, np.float32(np.inf), r).astype(np.float32)


def distance(mask, border="ignore"):
    return root(distance_sq(mask, border))


def brute_distance_sq(mask, border="ignore"):
    """The definition itself: every foreground voxel against every background voxel (tiny shapes)."""
    mask = np.asarray(mask) != 0
    shape = mask.shape
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.int64) for n in shape], indexing="ij"), -1).reshape(-1, 3)
    bg = grid[~mask.reshape(-1)]
    out = np.full(grid.shape[0], INF, np.int64)
    if bg.shape[0]:
        out = ((grid[:, None, :] - bg[None, :, :]) ** 2).sum(-1).min(1)
    if border == "background":
        n = np.array(shape, np.int64)
        out = np.minimum(out, np.minimum(grid + 1, n - grid).min(1) ** 2)
    out[~mask.reshape(-1)] = 0
    return out.reshape(shape).astype(np.int32)


def ball_offsets(r2):
    """Every o in Z^3 with |o|^2 <= r2."""
    r = int(np.floor(np.sqrt(r2)))
    a = np.arange(-r, r + 1)
    o = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
    return o[(o ** 2).sum(1) <= r2]


def ball(r2):
    """The ball as a structuring element for scipy: (2r + 1)^3 bool."""
    r = int(np.floor(np.sqrt(r2)))
    a = np.arange(-r, r + 1)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    return x * x + y * y + z * z <= r2


def brute_erode(mask, r2, border_value=0):
    """The ball's integer test itself (tiny shapes)."""
    mask = np.asarray(mask) != 0
    r = int(np.floor(np.sqrt(r2)))
    p = np.pad(mask, r, constant_values=bool(border_value))
    out = np.ones(mask.shape, bool)
    for o in ball_offsets(r2):
        out &= p[tuple(slice(r + int(d), r + int(d) + n) for d, n in zip(o, mask.shape))]
    return out.astype(np.uint8)


def erode(mask, r2, border_value=0):
    return (distance_sq(mask, "background" if border_value == 0 else "ignore") > r2).astype(np.uint8)


def dilate(mask, r2):
    return (distance_sq(np.asarray(mask) == 0, "ignore") <= r2).astype(np.uint8)


def open_(mask, r2, border_value=0):
    return dilate(erode(mask, r2, border_value), r2)


def close_(mask, r2, border_value=0):
    return erode(dilate(mask, r2), r2, border_value)


def fill_holes(mask):
    """-> (uint8 filled mask, the number of voxels filled): the background components (6 neighbours) that touch no face."""
    mask = np.asarray(mask) != 0
    lab, n = sm.label((~mask).astype(np.uint8), 1)
    face = np.zeros(mask.shape, bool)
    for axis in range(3):
        idx = [slice(None)] * 3
        for at in (0, -1):
            idx[axis] = at
            face[tuple(idx)] = True
    outer = np.unique(lab[face & (lab > 0)])
    holes = (lab > 0) & ~np.isin(lab, outer)
    return (mask | holes).astype(np.uint8), int(holes.sum())


# ---------------------------------------------------------------------------------------------------------------------------- masks

def bernoulli(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def slabs(shape):
    """Foreground slabs three thick along every axis in turn, two apart."""
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return (((x % 5) < 3) & ((y % 7) < 5) | ((z % 6) < 2)).astype(np.uint8)


def solid_ball(shape):
    """A ball around the centre that reaches the nearest face: many equidistant background voxels."""
    c = [(n - 1) / 2.0 for n in shape]
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    r = max(min(shape) / 2.0, 1.0)
    return ((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= r * r).astype(np.uint8)


def masks(shape):
    """name -> uint8 mask (values 0 / 1, one of them 0 / 200): the cases of the GPU tests."""
    out = {"zeros": np.zeros(shape, np.uint8), "ones": np.ones(shape, np.uint8)}
    corners = sorted(set(tuple(0 if b == 0 else n - 1 for b, n in zip(bits, shape)) for bits in np.ndindex(2, 2, 2)))
    for at in corners + [tuple(n // 2 for n in shape)]:
        m = np.ones(shape, np.uint8)
        m[at] = 0
        out["one background voxel at %s" % (at,)] = m
    m = np.zeros(shape, np.uint8)
    m[tuple(n // 2 for n in shape)] = 200
    out["one foreground voxel"] = m
    for p in (0.5, 0.9, 0.99):
        out["bernoulli %g" % p] = bernoulli(shape, p, 7)
    out["slabs"] = slabs(shape)
    out["checkerboard"] = sm.checkerboard(shape).astype(np.uint8)
    out["ball"] = solid_ball(shape)
    return out


def nested_shells(shape):
    """Cubic shells one voxel thick inside one another, two apart: holes within holes."""
    m = np.zeros(shape, np.uint8)
    k = 1
    while all(n - 2 * k >= 1 for n in shape):
        box = np.zeros(shape, bool)
        box[tuple(slice(k, n - k) for n in shape)] = True
        inner = np.zeros(shape, bool)
        if all(n - 2 * (k + 1) >= 1 for n in shape):
            inner[tuple(slice(k + 1, n - k - 1) for n in shape)] = True
        m[box & ~inner] = 1
        k += 3
    return m


def corner_hole(shape):
    """A full volume (at least 5 x 5 x 5) with the corner voxel (0, 0, 0) open and a cavity at (1, 1, 1) that meets it only across the
    corner -- with 6 neighbours still a hole; a tunnel of three voxels that reaches the face x = 0 with one voxel -- no hole; and a cavity
    deep inside."""
    m = np.ones(shape, np.uint8)
    m[0, 0, 0] = 0
    m[1, 1, 1] = 0
    m[0:3, 3, 3] = 0
    m[3, 1:3, 1:4] = 0
    return m
