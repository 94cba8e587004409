#!/usr/bin/env python3
"""Cost model of the gather-form flat forward (k_fwd_gather_flat), CPU only.

Emulates the kernel's tiling for a parallel-beam scan of an N^3 volume with N detector rows and A angles: a wave owns
8 projections x 8 detector rows x 64 planes and walks the volume one slab at a time (x slabs where |d_x| >= |d_y|, y slabs
otherwise; projections are grouped per walk, in pose order).  Per (ray, slab) the kernel needs the lines L0 .. L0 + NW - 1
(L0 = lowest node touched by the <= 3 samples with |p_s - S| < 1); per wave-step it stages the lines wave_min(L0) ..
wave_max(L0) + NW - 1 in windows of FROWS.  Prints what the kernel's constants were chosen from, and, for the work-group order
(patches of G groups x R row tiles per XCD), how many of the lines a patch requests per slab are distinct:

  python tools/fwd_gather_model.py [--n 1024] [--angles 1024] > profiles/fwd_gather_model.md
"""
import argparse

import numpy as np

GP, GR = 8, 8          # projections x rows of a wave
CHUNK = 64             # planes of a wave
LINE_BYTES = 256


def lattice(phi, tx, n, step=1.0):
    """Ray lattice p(ix, j) = a + ix u + j d of an untilted pose, index space, volume and detector centred.  The first sample sits
    0.75 n steps before the centre line: this tool's own choice, not the project's ray start, so the phase of the samples along a ray
    differs from the kernel's; the counts below are statistics over all phases and do not depend on it."""
    c = (n - 1) / 2.0
    u = np.array([np.cos(phi), np.sin(phi)])
    d = step * np.array([-np.sin(phi), np.cos(phi)])
    a = np.array([c, c]) + (-(n - 1) / 2.0 + tx) * u - (0.75 * n) * d / step
    return a, u, d


def group_stats(poses, walk, n, frows_list, nbins):
    """poses: list of (phi, tx) of one group (<= 8, same walk).  Returns per-slab arrays over (row tiles, slabs)."""
    s_ax, l_ax = (0, 1) if walk == 0 else (1, 0)
    S = np.arange(n, dtype=np.float64)[None, :]                        # slabs
    ix = np.arange(n, dtype=np.float64)[:, None]                       # rows
    L0 = np.full((GP, n, n), 1 << 30, dtype=np.int64)
    nodes = np.zeros((GP, n, n), dtype=np.int64)
    for k, (phi, tx) in enumerate(poses):
        a, u, d = lattice(phi, tx, n)
        bs, bl = a[s_ax] + ix * u[s_ax], a[l_ax] + ix * u[l_ax]
        ds, dl = d[s_ax], d[l_ax]
        t0, t1 = (S - 1.0 - bs) / ds, (S + 1.0 - bs) / ds
        tlo, thi = np.minimum(t0, t1), np.maximum(t0, t1)
        jlo, jhi = np.floor(tlo) + 1.0, np.ceil(thi) - 1.0                # samples strictly inside the slab's footprint
        has = jhi >= jlo
        pa, pb = bl + jlo * dl, bl + jhi * dl
        lo, hi = np.floor(np.minimum(pa, pb)), np.floor(np.maximum(pa, pb)) + 1.0
        valid = has & (hi >= 0) & (lo <= n - 1)
        L0[k] = np.where(valid, lo, 1 << 30).astype(np.int64)
        nodes[k] = np.where(valid, hi - lo + 1.0, 0).astype(np.int64)
    # waves: row tiles of 8
    L0t = L0.reshape(GP, n // GR, GR, n)
    val = L0t < (1 << 29)
    lmin = np.where(val, L0t, 1 << 30).min(axis=(0, 2))
    lmax = np.where(val, L0t, -(1 << 30)).max(axis=(0, 2))
    live = lmax >= lmin
    return lmin, lmax, live, nodes.max()


def patch_reuse(lmin, lmax, live, nw, n, fpg, fpr):
    """Lines requested and distinct lines touched per patch-slab, summed over the patches of fpg groups x fpr row tiles of one list
    (groups and row tiles split evenly over the patches, as the kernel does).  lmin, lmax, live: [groups, row tiles, slabs] of the
    list's waves.  A wave requests its first window's lines lmin .. lmax + nw - 1, clamped to the volume as the kernel clamps them;
    the distinct lines of a patch-slab are the union of those intervals over the patch's waves.  Requested / distinct is the reuse
    one XCD's L2 can give IF the work-groups of a patch walk their slabs together; nothing here says whether they do."""
    npg, nrt, ns = lmin.shape
    npp, nrp = (npg + fpg - 1) // fpg, (nrt + fpr - 1) // fpr
    lo = np.clip(np.where(live, lmin, 0), 0, n)
    hi = np.clip(np.where(live, lmax + nw, 0), 0, n)            # exclusive
    req = dist = 0.0
    n_ps = 0
    for a in range(npp):
        g0, g1 = a * npg // npp, (a + 1) * npg // npp
        for b in range(nrp):
            r0, r1 = b * nrt // nrp, (b + 1) * nrt // nrp
            l = lo[g0:g1, r0:r1].reshape(-1, ns)
            h = hi[g0:g1, r0:r1].reshape(-1, ns)
            cover = np.zeros((n + 1, ns), dtype=np.int32)
            cols = np.broadcast_to(np.arange(ns), l.shape)
            np.add.at(cover, (l, cols), 1)
            np.add.at(cover, (h, cols), -1)
            d = (np.cumsum(cover, axis=0) > 0).sum(axis=0)
            req += float((h - l).sum())
            dist += float(d.sum())
            n_ps += int((d > 0).sum())
    return req, dist, n_ps, (-(-npg // npp), -(-nrt // nrp))       # ... and the largest patch actually formed (groups, row tiles)


def run(name, phis, txs, n, frows_list, out, patches=()):
    A = len(phis)
    dsx = np.abs(np.sin(phis)) >= np.abs(np.cos(phis))                  # |d_x| >= |d_y|: x walk
    ratio = np.where(dsx, np.abs(np.cos(phis) / np.maximum(np.abs(np.sin(phis)), 1e-300)),
                     np.abs(np.sin(phis) / np.maximum(np.abs(np.cos(phis)), 1e-300)))
    nw3 = ratio <= 0.5
    lists = {}
    for walk in (0, 1):
        for nw in (3, 4):
            sel = np.nonzero((dsx == (walk == 0)) & (nw3 == (nw == 3)))[0]
            if len(sel):
                lists[(walk, nw)] = sel
    nbins = 8
    cdist = np.abs(np.arange(n) - (n - 1) / 2.0)
    bins = np.minimum((cdist / (n / 2.0) * nbins).astype(int), nbins - 1)
    tot_steps = tot_live = 0
    sum_lines = 0.0
    max_lines = 0
    bin_sum, bin_cnt = np.zeros(nbins), np.zeros(nbins)
    over = {f: 0 for f in frows_list}
    staged = {f: 0.0 for f in frows_list}
    w_steps = {3: 0, 4: 0}
    max_nodes = {3: 0, 4: 0}
    per_list = {}
    for (walk, nw), sel in sorted(lists.items()):
        # groups of eight in pose order; a new group starts where the list jumps to another range of poses (as the host pads its lists)
        groups, cur = [], []
        for i in sel:
            if cur and (len(cur) == GP or i != cur[-1] + 1):
                groups.append(cur)
                cur = []
            cur.append(i)
        groups.append(cur)
        per_list[(walk, nw)] = ([], [], [])
        for grp in groups:
            poses = [(phis[i], txs[i]) for i in grp]
            lmin, lmax, live, mx = group_stats(poses, walk, n, frows_list, nbins)
            for store, arr in zip(per_list[(walk, nw)], (lmin, lmax, live)):
                store.append(arr)
            max_nodes[nw] = max(max_nodes[nw], int(mx))
            lines = np.where(live, lmax - lmin + nw, 0)
            tot_steps += live.size
            nl = int(live.sum())
            tot_live += nl
            w_steps[nw] += nl
            sum_lines += float(lines.sum())
            max_lines = max(max_lines, int(lines.max()))
            for b in range(nbins):
                m = live & (bins[None, :] == b)
                bin_sum[b] += float(lines[m].sum())
                bin_cnt[b] += float(m.sum())
            for f in frows_list:
                sw = f - nw + 1
                nwin = np.where(live, (lmax - lmin) // sw + 1, 0)
                over[f] += int((nwin > 1).sum())
                staged[f] += float(nwin.sum()) * f
    n_chunk = (n + CHUNK - 1) // CHUNK
    p = lambda *a: print(*a, file=out)
    p(f"## {name}: {n}^3 volume, {n} rows, {A} angles")
    p()
    p(f"- projections at 3 weights: {int(nw3.sum())} ({100.0 * nw3.mean():.1f} %), at 4: {int((~nw3).sum())}; "
      f"x-walk {int(dsx.sum())}, y-walk {int((~dsx).sum())}")
    p(f"- live wave-steps at 3 weights: {100.0 * w_steps[3] / max(tot_live, 1):.1f} %, at 4: {100.0 * w_steps[4] / max(tot_live, 1):.1f} %")
    p(f"- most nodes any ray needs in one slab: {max_nodes[3]} in the 3-weight lists, {max_nodes[4]} in the 4-weight lists")
    p(f"- wave-steps in which no lane has a weight: {100.0 * (1.0 - tot_live / max(tot_steps, 1)):.1f} % of {tot_steps}")
    p(f"- lines needed per live wave-step: mean {sum_lines / max(tot_live, 1):.2f}, max {max_lines}")
    p()
    p("| slab distance from the rotation centre (fraction of N/2) | mean lines |")
    p("|---|---|")
    for b in range(nbins):
        p(f"| {b / nbins:.3f} - {(b + 1) / nbins:.3f} | {bin_sum[b] / max(bin_cnt[b], 1):.2f} |")
    p()
    p("| FROWS | wave-steps needing a second window | lines staged per live wave-step | wave loads per launch, all z chunks live | with 11 of 16 chunks live (the headline) |")
    p("|---|---|---|---|---|")
    for f in frows_list:
        gb = staged[f] * LINE_BYTES * n_chunk / 1e9
        p(f"| {f} | {100.0 * over[f] / max(tot_live, 1):.1f} % | {staged[f] / max(tot_live, 1):.2f} | {gb:.0f} GB | {gb * 11 / 16:.0f} GB |")
    p()
    if patches:
        # the work-group order of the kernel (option fwd_gather_patch): which waves are resident on one XCD together
        p("Patches of G projection groups x R row tiles that one XCD's work-groups cover together: lines requested / distinct lines touched, "
          "per patch-slab.  In brackets: distinct lines per patch-slab; the largest patch actually formed -- groups and row tiles are split "
          "evenly over ceil(groups / G) x ceil(row tiles / R) patches, as the kernel does, so G x R is an upper limit "
          "(the plain order's resident set, one group x 96 consecutive row tiles, is evaluated as the 1 x 96 row's 1 x 64 at 128 row tiles):")
        p()
        keys = sorted(per_list)
        p("| patch G x R | " + " | ".join("%s walk, NW %d" % ("xy"[w], nw) for w, nw in keys) + " |")
        p("|---|" + "---|" * len(keys))
        for fpg, fpr in patches:
            cells = []
            for k in keys:
                lmin, lmax, live = (np.stack(a) for a in per_list[k])
                req, dist, n_ps, eff = patch_reuse(lmin, lmax, live, k[1], n, fpg, fpr)
                cells.append("%.2f (%.0f; %d x %d)" % (req / max(dist, 1.0), dist / max(n_ps, 1), eff[0], eff[1]))
            p("| %d x %d | " % (fpg, fpr) + " | ".join(cells) + " |")
        p()
    return sum_lines / max(tot_live, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--angles", type=int, default=1024)
    ap.add_argument("--frows", type=int, nargs="*", default=[16, 20, 24, 28, 32])
    ap.add_argument("--patches", nargs="*", default=["1x96", "2x48", "4x24", "8x12", "12x8", "16x6", "24x4", "16x4", "32x3", "48x2"],
                    help="patch shapes GxR (projection groups x row tiles) of the work-group order table")
    args = ap.parse_args()
    patches = [tuple(int(v) for v in s.split("x")) for s in args.patches]
    import sys
    out = sys.stdout
    print("# Cost model of the gather-form flat forward (tools/fwd_gather_model.py)", file=out)
    print(file=out)
    print("The gather adjoint, for comparison: 14 sinogram rows staged per wave-step, 660 GB of wave loads per launch with the headline's "
          "live z chunks (960 GB with all chunks live), 506 GB by FETCH_SIZE.", file=out)
    print(file=out)
    phis = np.linspace(0.0, np.pi, args.angles)
    run("headline poses", phis, np.zeros(args.angles), args.n, args.frows, out, patches)
    rng = np.random.default_rng(0)                              # bench.py --perturbed draws alpha, beta, then tx from this generator
    rng.uniform(-1, 1, args.angles)
    rng.uniform(-1, 1, args.angles)
    tx = rng.uniform(-2, 2, args.angles)
    run("perturbed translations (the tx of bench.py --perturbed, default_rng(0); alpha = beta = 0)", phis, tx, args.n, args.frows, out, patches)


if __name__ == "__main__":
    main()
