"""numpy statements of the point-cloud metric rules, the yardstick of csrc/point_metrics.hip:

1. ``greedy_mis`` / ``mis_rounds``: the radius maximal independent set of ``metrics.reduce_pts`` (|p - q| <= dst in fp64), as the
   reference's sequential pass in ``randOrd`` order and as the parallel rounds the GPU runs;
2. ``nn_bounded``: the distance to the nearest target when strictly below ``maxdist``, else inf (``chamfer_imw``);
3. ``chamfer_blocked``: ``metrics.chamfer``'s loop over the cells of ``bb``, with a brute-force search in place of cKDTree.

Distances are fp64 from the float32 coordinates.  Pure numpy: no SciPy.  ``fragile`` marks the pairs whose squared distance lies
within ``REL`` of the bound, where a kd-tree and the kernel may round differently."""
from __future__ import annotations

import numpy as np

REL = 1e-9


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _d2_rows(a, b):
    """[len(a), len(b)] squared distances, summed x, y, z in that order."""
    d = a[:, None, :] - b[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def neighbours(pts, dst, chunk=512):
    """Radius graph: list of index arrays (each point's neighbours, itself included) and whether any pair is fragile."""
    p = _f64(pts)
    r2 = float(dst) * float(dst)
    out, fragile = [], False
    for s in range(0, p.shape[0], chunk):
        d2 = _d2_rows(p[s:s + chunk], p)
        fragile |= bool((np.abs(d2 - r2) <= REL * max(r2, 1e-300)).any())
        out += [np.nonzero(row <= r2)[0] for row in d2]
    return out, fragile


def greedy_mis(nbrs, rand_ord):
    """The reference's pass (metrics.reduce_pts, chunked=False): bool mask in index order."""
    keep = np.ones(len(nbrs), dtype=bool)
    for j in range(len(nbrs)):
        i = rand_ord[j]
        if keep[i]:
            keep[nbrs[i]] = False
            keep[i] = True
    return keep


def mis_rounds(nbrs, rank):
    """Parallel rounds: an undecided point ranked below all its undecided neighbours is kept, then the undecided neighbours of
    the newly kept points are removed.  -> (mask, rounds)."""
    n = len(nbrs)
    und = np.ones(n, dtype=bool)
    keep = np.zeros(n, dtype=bool)
    rounds = 0
    while und.any():
        rounds += 1
        new = [i for i in np.nonzero(und)[0] if all(rank[j] >= rank[i] or not und[j] for j in nbrs[i])]
        keep[new] = True
        und[new] = False
        for i in new:
            und[nbrs[i]] = False
    return keep, rounds


def nn_bounded(q, t, maxdist, chunk=256):
    """(dist float64 [m], fragile bool [m]): nearest target distance when d^2 < maxdist^2, else inf."""
    q, t = _f64(q), _f64(t)
    m = q.shape[0]
    out = np.full(m, np.inf)
    fragile = np.zeros(m, dtype=bool)
    if t.shape[0] == 0:
        return out, fragile
    b2 = float(maxdist) ** 2
    for s in range(0, m, chunk):
        d2 = _d2_rows(q[s:s + chunk], t).min(axis=1)
        ok = d2 < b2
        out[s:s + chunk][ok] = np.sqrt(d2[ok])
        fragile[s:s + chunk] = np.isfinite(b2) & (np.abs(d2 - b2) <= REL * b2)
    return out, fragile


def chamfer_blocked(pts_from, pts_to, bb, maxdist):
    """metrics.chamfer with brute force for the kd-tree: (dist float64 [m], fragile bool [m])."""
    bb = np.asarray(bb, dtype=np.float64)
    f = np.asarray(pts_from, dtype=np.float32)
    t = np.asarray(pts_to, dtype=np.float32)
    rx, ry, rz = np.floor((bb[1, :] - bb[0, :]) / maxdist).astype(int)
    dist = np.ones(f.shape[0]) * maxdist
    fragile = np.zeros(f.shape[0], dtype=bool)
    for x in range(rx + 1):
        for y in range(ry + 1):
            for z in range(rz + 1):
                low = bb[0, :] + np.array([x, y, z]) * maxdist
                high = low + maxdist
                vf = (f >= low[None]).all(axis=1) & (f < high[None]).all(axis=1)
                low = low - maxdist
                high = high + maxdist
                vt = (t >= low[None]).all(axis=1) & (t < high[None]).all(axis=1)
                if vt.sum() == 0:
                    dist[vf] = maxdist
                    fragile[vf] = False
                elif vf.sum() == 0:
                    pass
                else:
                    dist[vf], fragile[vf] = nn_bounded(f[vf], t[vt], maxdist)
    return dist, fragile
