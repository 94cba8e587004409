"""The isosurface of include/tomo_mesh.h in numpy: marching tetrahedra, six per cell around the cell's main diagonal, orientation from
the case alone.  What tests/test_mesh.py checks on its own and tests/test_gpu_mesh.py holds libtomo_mesh.so against, bit for bit.

A volume is [nx][ny][nz]; voxel (i, j, k) is the lattice point (i, j, k).  A float32 volume is taken at `level`, a uint8 / bool mask as
0 / 1 at 0.5.  A corner is inside when v >= level (NaN: outside).  border "open": cell origins 0 ... n - 2; "closed": the volume stands
in one layer of -inf and cell origins are -1 ... n - 1, coordinates staying in the unpadded frame.
"""
import itertools

import numpy as np

BORDERS = ("open", "closed")
PERMS = list(itertools.permutations(range(3)))            # lexicographic: the six tetrahedra of a cell
BRICK = (8, 8, 32)                                        # TOMO_MESH_BRICK_X / Y / Z: the cells of a work-group's brick


def tet_corners(perm):
    """The four corners of the tetrahedron of `perm` as offsets from the cell origin, in corner order."""
    a, b, _ = perm
    e = np.eye(3, dtype=np.int64)
    return np.array([0 * e[0], e[a], e[a] + e[b], e[0] + e[1] + e[2]])


def case_triangles(inside):
    """The triangles of one tetrahedron before orientation: inside[i] says whether corner i is inside.  Each triangle is three edges,
    an edge a pair (i, j) of corner indices with i < j -- corner i is the end with the smaller lattice coordinates."""
    ins = [i for i in range(4) if inside[i]]
    out = [i for i in range(4) if not inside[i]]
    edge = lambda p, q: (min(p, q), max(p, q))      # noqa: E731
    if len(ins) == 1:
        return [[edge(ins[0], o) for o in out]]
    if len(ins) == 3:
        return [[edge(i, out[0]) for i in ins]]
    if len(ins) == 2:
        a, b = ins
        c, d = out
        return [[edge(a, c), edge(a, d), edge(b, d)], [edge(a, c), edge(b, d), edge(b, c)]]
    return []


def oriented_case(perm, inside):
    """case_triangles with the last two vertices swapped where (p1 - p0) x (p2 - p0), every vertex at its edge's midpoint, does not point
    away from the inside corners."""
    corners = tet_corners(perm).astype(np.float64)
    ins = np.array(inside, bool)
    away = corners[~ins].mean(0) - corners[ins].mean(0) if ins.any() and not ins.all() else None
    tris = []
    for tri in case_triangles(inside):
        p = [0.5 * (corners[i] + corners[j]) for i, j in tri]
        if np.dot(np.cross(p[1] - p[0], p[2] - p[0]), away) < 0:
            tri = [tri[0], tri[2], tri[1]]
        tris.append(tri)
    return tris


def as_field(vol, level):
    """(float32 volume, float32 level) of a float32 volume at `level` or of a mask at 0.5."""
    vol = np.asarray(vol)
    if vol.dtype == np.float32:
        if level is None:
            raise ValueError("a float32 volume needs a level")
        return vol, np.float32(level)
    if vol.dtype not in (np.uint8, np.bool_):
        raise ValueError("float32, uint8 or bool")
    return (vol != 0).astype(np.float32), np.float32(0.5)


def isosurface(vol, level=None, border="closed"):
    """float32 (n, 3, 3): the triangles, in no particular order."""
    f, level = as_field(vol, level)
    if f.ndim != 3 or border not in BORDERS:
        raise ValueError("a 3-D volume and border 'open' or 'closed'")
    shift = 0
    if border == "closed":
        f = np.pad(f, 1, constant_values=-np.inf)
        shift = -1
    cells = tuple(n - 1 for n in f.shape)
    if min(cells) < 1:
        return np.zeros((0, 3, 3), np.float32)
    cx, cy, cz = cells

    def corner(off):                                    # the values at corner `off` of every cell
        return f[off[0]:off[0] + cx, off[1]:off[1] + cy, off[2]:off[2] + cz]

    origin = np.stack(np.meshgrid(*[np.arange(c, dtype=np.int64) + shift for c in cells], indexing="ij"), -1)
    out = []
    with np.errstate(all="ignore"):
        for perm in PERMS:
            corners = tet_corners(perm)
            vals = [corner(c) for c in corners]
            ins = [v >= level for v in vals]
            case = sum(ins[i].astype(np.int64) << i for i in range(4))
            for c in range(1, 15):
                sel = case == c
                if not sel.any():
                    continue
                o = origin[sel]
                for tri in oriented_case(perm, [(c >> i) & 1 for i in range(4)]):
                    verts = []
                    for i, j in tri:
                        lo, hi = vals[i][sel], vals[j][sel]
                        den = hi - lo
                        t = (level - lo) / den
                        t = np.where(np.isfinite(lo) & np.isfinite(hi) & np.isfinite(den), t, np.float32(0.5)).astype(np.float32)
                        base = (o + corners[i]).astype(np.float32)
                        moved = (corners[j] != corners[i])
                        verts.append(np.where(moved, base + t[:, None], base).astype(np.float32))
                    out.append(np.stack(verts, 1))
    if not out:
        return np.zeros((0, 3, 3), np.float32)
    return np.ascontiguousarray(np.concatenate(out, 0), np.float32)


def measures(triangles):
    """(area, volume) in float64 from the float32 vertices: sum of |e| / 2 and of p0 . e / 6 with e = (p1 - p0) x (p2 - p0), which is
    p0 . (p1 x p2) / 6."""
    t = np.asarray(triangles, np.float32).reshape(-1, 3, 3).astype(np.float64)
    if len(t) == 0:
        return 0.0, 0.0
    e = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return float(0.5 * np.sqrt((e * e).sum(1)).sum()), float((t[:, 0] * e).sum() / 6.0)


def _keys(v):
    """A sortable byte key of every float32 vertex (..., 3): the twelve bytes as they lie."""
    v = np.ascontiguousarray(v, np.float32)
    return v.view(np.dtype((np.void, 12))).reshape(v.shape[:-1])


def canonical(triangles):
    """Every triangle rotated so that its byte-wise smallest vertex comes first (which keeps the orientation), then the triangles sorted
    by bytes: two surfaces are the same set of oriented triangles iff their canonical forms are equal bit for bit."""
    t = np.ascontiguousarray(triangles, np.float32).reshape(-1, 3, 3)
    if len(t) == 0:
        return t
    raw = t.view(np.uint8).reshape(len(t), 3, 12)
    first = np.zeros(len(t), np.int64)
    for k in (1, 2):                                     # lexicographic compare of vertex k with the smallest so far
        cur = raw[np.arange(len(t)), first].astype(np.int16)
        d = raw[:, k].astype(np.int16) - cur
        nz = d != 0
        where = nz.argmax(1)
        less = nz.any(1) & (d[np.arange(len(t)), where] < 0)
        first = np.where(less, k, first)
    idx = (first[:, None] + np.arange(3)) % 3
    t = t[np.arange(len(t))[:, None], idx]
    order = np.argsort(np.ascontiguousarray(t).reshape(len(t), 9).view(np.dtype((np.void, 36))).ravel(), kind="stable")
    return np.ascontiguousarray(t[order])


def closed(triangles):
    """Every directed edge whose ends differ in their bits occurs as often as its reverse."""
    t = np.ascontiguousarray(triangles, np.float32).reshape(-1, 3, 3)
    if len(t) == 0:
        return True
    bits = t.view(np.uint32)
    a = bits.reshape(-1, 3)                                         # the start of every directed edge
    b = bits[:, [1, 2, 0]].reshape(-1, 3)                           # its end
    keep = (a != b).any(1)
    fwd = np.concatenate([a[keep], b[keep]], 1)
    rev = np.concatenate([b[keep], a[keep]], 1)
    key = np.dtype((np.void, 24))
    f = np.sort(np.ascontiguousarray(fwd).view(key).ravel())
    r = np.sort(np.ascontiguousarray(rev).view(key).ravel())
    return bool(np.array_equal(f, r))


# ---------------------------------------------------------------------------------------------------------------------- inputs
def ball_field(n, radius, offset=(0.3, 0.1, -0.2)):
    """R - r on n^3 about the centre (n - 1) / 2 - offset: level 0 is the sphere."""
    g = [np.arange(n, dtype=np.float64) - ((n - 1) / 2.0 - o) for o in offset]
    x, y, z = np.meshgrid(*g, indexing="ij")
    return (radius - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


def bernoulli(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def checkerboard(shape):
    i, j, k = np.indices(shape)
    return ((i + j + k) % 2).astype(np.uint8)


def corners_mask(shape):
    m = np.zeros(shape, np.uint8)
    for c in itertools.product(*[(0, n - 1) for n in shape]):
        m[c] = 1
    return m


def noise(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def integers(shape, seed):
    """Integer-valued floats 0 ... 3: at level 1 or 2 many voxels equal the level."""
    return np.random.default_rng(seed).integers(0, 4, shape).astype(np.float32)


def nonfinite(shape, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape).astype(np.float32)
    kind = rng.integers(0, 8, shape)
    v[kind == 0] = np.nan
    v[kind == 1] = np.inf
    v[kind == 2] = -np.inf
    return v


def _gpu_shapes():
    bx, by, bz = BRICK
    s = [(1, 1, 1), (1, 5, 6), (5, 1, 6), (5, 6, 1)]
    # closed has n + 1 cells and open n - 1: cell counts one below, at and one above the brick edge under both borders
    for axis, b in enumerate(BRICK):
        for n in sorted(set([b - 2, b - 1, b, b + 1, b + 2])):
            shape = [3, 4, 5]
            shape[axis] = n
            s.append(tuple(shape))
    s += [(3, 4, 3), (3, 4, 4), (4, 3, 5), (3, 3, 67)]
    s.append((bx + 3, by + 2, bz + 5))                   # past every brick edge at once
    return s


GPU_SHAPES = _gpu_shapes()
