#!/usr/bin/env python
"""Derives the tables of tomography_alignment_amd/csrc/tomo_side_tets.h from the rule of include/tomo_mesh.h and prints them as the
block that stands between the two `generated` lines of that header (tests/test_mesh.py holds the header against this output).

The six tetrahedra of a cell: for the permutations (a, b, c) of the axes in lexicographic order the corners o, o + e_a, o + e_a + e_b,
o + (1, 1, 1).  A cube corner is coded dx + 2 dy + 4 dz.  A tetrahedron of an odd permutation is the mirror image of the first, so it
takes the first one's triangles with the last two vertices swapped (TETS_ODD).

The 16 cases (bit i: corner i is inside), for the tetrahedron of the identity permutation:
    one inside corner a, outside o1 < o2 < o3:       (a o1, a o2, a o3)
    three inside i1 < i2 < i3, one outside o:        (i1 o, i2 o, i3 o)
    two inside a < b, two outside c < d:             (ac, ad, bd) and (ac, bd, bc)
and the last two vertices swapped where (p1 - p0) x (p2 - p0), with every vertex at the midpoint of its edge, does not point from the
inside corners to the outside ones.  A case is packed as: bits 0-1 the number of triangles, then four bits a vertex, (i << 2) | j for
the edge between corners i < j, the first vertex lowest.

    python tools/tets_table.py            print the block
"""
import itertools

PERMS = list(itertools.permutations(range(3)))


def corners(perm):
    a, b, _ = perm
    e = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    add = lambda p, q: tuple(x + y for x, y in zip(p, q))      # noqa: E731
    return [(0, 0, 0), e[a], add(e[a], e[b]), (1, 1, 1)]


def det(u, v, w):
    return (u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0]))


def sub(p, q):
    return tuple(x - y for x, y in zip(p, q))


def triangles(case):
    ins = [i for i in range(4) if (case >> i) & 1]
    out = [i for i in range(4) if not (case >> i) & 1]
    edge = lambda p, q: (min(p, q), max(p, q))                 # noqa: E731
    if len(ins) == 1:
        return [[edge(ins[0], o) for o in out]]
    if len(ins) == 3:
        return [[edge(i, out[0]) for i in ins]]
    if len(ins) == 2:
        (a, b), (c, d) = ins, out
        return [[edge(a, c), edge(a, d), edge(b, d)], [edge(a, c), edge(b, d), edge(b, c)]]
    return []


def oriented(case, perm=PERMS[0]):
    """The triangles of `case` in the tetrahedron of `perm`, turned by geometry at t = 0.5 (coordinates doubled: integers)."""
    c = corners(perm)
    ins = [c[i] for i in range(4) if (case >> i) & 1]
    out = [c[i] for i in range(4) if not (case >> i) & 1]
    res = []
    for tri in triangles(case):
        p = [tuple(x + y for x, y in zip(c[i], c[j])) for i, j in tri]
        # away: mean(out) - mean(in), times len(ins) len(out)
        away = tuple(len(ins) * sum(q[k] for q in out) - len(out) * sum(q[k] for q in ins) for k in range(3))
        s = det(sub(p[1], p[0]), sub(p[2], p[0]), away)
        assert s != 0
        res.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
    return res


def pack(tris):
    w = len(tris)
    for k, (i, j) in enumerate(v for tri in tris for v in tri):
        w |= ((i << 2) | j) << (2 + 4 * k)
    return w


def block():
    lines = ["constexpr unsigned TETS_CASES[16] = {"]
    words = [pack(oriented(case)) for case in range(16)]
    for r in range(0, 16, 4):
        lines.append("    " + " ".join("0x%07xu," % w for w in words[r:r + 4]))
    lines.append("};")
    codes = [[x + 2 * y + 4 * z for x, y, z in corners(p)] for p in PERMS]
    lines.append("constexpr unsigned char TETS_CORNERS[6][4] = {" + ", ".join("{%d, %d, %d, %d}" % tuple(c) for c in codes) + "};")
    odd = [det(*[sub(q, corners(p)[0]) for q in corners(p)[1:]]) < 0 for p in PERMS]
    lines.append("constexpr bool TETS_ODD[6] = {" + ", ".join("true" if o else "false" for o in odd) + "};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    # the mirror rule the header relies on, for every case of every tetrahedron
    for n, perm in enumerate(PERMS):
        flip = det(*[sub(q, corners(perm)[0]) for q in corners(perm)[1:]]) < 0
        for case in range(16):
            want = oriented(case, perm)
            got = [[t[0], t[2], t[1]] if flip else t for t in oriented(case)]
            assert want == got, (perm, case)
    print(block(), end="")
