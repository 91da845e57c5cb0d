"""Numpy restatement of the GPU PatchMatch stereo rule (wild_deep_mvs_amd/csrc/patch_match.hip).

Costs are fp64 from the fp32 inputs; the counter hash is uint32, so every random draw (and hence every candidate hypothesis) is
the kernel's own, bit for bit.  Pixels are handled as flat index arrays so that one half-step is a handful of vectorised passes.

State of a view: fp32-valued [h, w, 4] = (depth, nx, ny, nz) in the reference camera frame.  Cameras: ``cams`` [S+1, 30] rows of
(K, K^-1, R, t) as ``ops.geo_filter_cams`` builds them, row 0 = the reference view.
"""
from __future__ import annotations

import math

import numpy as np

from tests._fusion_ref import cam_parts

SIGMA_COLOR = 0.2
MIN_VAR = 1e-5
MIN_TRI_DEG = 1.0
GEOM_LAMBDA = 0.3
GEOM_EMAX = 3.0
FILTER_MAX_COST = 0.9
FILTER_MIN_TRI_DEG = 3.0
FILTER_MAX_ERR = 1.0
FILTER_MIN_CONSISTENT = 2
NUM_CAND = 11
NEIGHBOURS = ((0, -1), (0, 1), (-1, 0), (1, 0), (0, -3), (0, 3), (-3, 0), (3, 0))    # (drow, dcol) of candidates 1-8
DELTA0, THETA0_DEG = 0.25, 30.0                                                    # perturbation schedule: x 0.5 per iteration
INIT_ITERATION = 0xFFFFFFFF
SLOT_PHI, SLOT_ALPHA, SLOT_DEPTH, SLOT_RDEPTH, SLOT_RZ, SLOT_RAZ = range(6)

M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------------------------
# randomness
# ---------------------------------------------------------------------------------------------------------------------------
def lowbias32(x):
    """Wellons' lowbias32 finaliser on uint32 values (computed in uint64 and masked, so numpy never warns on overflow)."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def pm_hash(seed, view, pixel, iteration, colour, slot):
    """h = H(H(H(H(H(H(seed ^ 0x9E3779B9) ^ view) ^ pixel) ^ iteration) ^ colour) ^ slot), H = lowbias32, all uint32 -> uint32
    array (the golden-ratio constant keeps an all-zero key away from H's fixed point 0)."""
    h = lowbias32((np.uint64(seed) & M32) ^ np.uint64(0x9E3779B9))
    for word in (view, pixel, iteration, colour, slot):
        h = lowbias32(h ^ (np.asarray(word, dtype=np.uint64) & M32))
    return h.astype(np.uint32)


def pm_uniform(seed, view, pixel, iteration, colour, slot):
    """(h >> 8) * 2^-24: a float in [0, 1) exact in fp32."""
    return (pm_hash(seed, view, pixel, iteration, colour, slot) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def schedule(t: int):
    """(delta_t, theta_t) of pass-local iteration t: the inverse-depth fraction and the normal angle (radians) of candidate 9."""
    return DELTA0 * 0.5 ** t, math.radians(THETA0_DEG) * 0.5 ** t


# ---------------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------------
def grey(img):
    """[3,H,W] float image in [0,1] -> fp32 grey [H,W]: x255 truncated to bytes, (0.299 R + 0.587 G + 0.114 B) / 255."""
    b = np.floor(np.asarray(img, dtype=np.float32) * np.float32(255.0)).clip(0, 255).astype(np.float32)
    return ((np.float32(0.299) * b[0] + np.float32(0.587) * b[1] + np.float32(0.114) * b[2]) / np.float32(255.0)).astype(np.float32)


def source_geometry(cams):
    """Per source s (rows 1..S): A = K_s R_rel K_r^-1, b = K_s t_rel, C = -R_rel^T t_rel (s's centre in r's frame),
    G = K_r R_rel^T K_s^-1, c = K_r C, with R_rel = R_s R_r^T, t_rel = t_s - R_rel t_r.  Also K_r^-1."""
    K, Ki, R, t = cam_parts(cams)
    out = []
    for s in range(1, K.shape[0]):
        Rr = R[s] @ R[0].T
        tr = t[s] - Rr @ t[0]
        C = -Rr.T @ tr
        out.append(dict(A=K[s] @ Rr @ Ki[0], b=K[s] @ tr, C=C, G=K[0] @ Rr.T @ Ki[s], c=K[0] @ C))
    return out, Ki[0]


def offsets(radius: int, step: int):
    k = np.arange(-(radius // step), radius // step + 1) * step
    oy, ox = np.meshgrid(k, k, indexing="ij")
    return oy.reshape(-1), ox.reshape(-1)


def _rays(Kinv, rows, cols):
    p = np.stack([cols.astype(np.float64), rows.astype(np.float64), np.ones(rows.shape)], axis=-1)
    return p @ Kinv.T                                   # K^-1 p, [N,3]


def _bilinear(img, u, v):
    h, w = img.shape
    u = np.clip(np.nan_to_num(u, nan=0.0), 0.0, w - 1.0)        # NaN -> 0 as fmaxf(NaN, 0) does
    v = np.clip(np.nan_to_num(v, nan=0.0), 0.0, h - 1.0)
    x0 = np.floor(u).astype(np.int64)
    y0 = np.floor(v).astype(np.int64)
    x1 = np.minimum(x0 + 1, w - 1)
    y1 = np.minimum(y0 + 1, h - 1)
    fx, fy = u - x0, v - y0
    I = img.astype(np.float64)
    top = (1 - fx) * I[y0, x0] + fx * I[y0, x1]
    bot = (1 - fx) * I[y1, x0] + fx * I[y1, x1]
    return (1 - fy) * top + fy * bot


def ref_window(ref, rows, cols, radius, step):
    """Bilateral weights [N,T] and centred reference values r' = I_r(p+o) - I_r(p) [N,T] (integer reads, clamped to the edge)."""
    h, w = ref.shape
    oy, ox = offsets(radius, step)
    R = ref.astype(np.float64)
    rr = np.clip(rows[:, None] + oy[None], 0, h - 1)
    cc = np.clip(cols[:, None] + ox[None], 0, w - 1)
    rp = R[rr, cc] - R[rows, cols][:, None]
    wgt = np.exp(-(oy ** 2 + ox ** 2)[None].astype(np.float64) / (2.0 * radius * radius) - rp ** 2 / (2.0 * SIGMA_COLOR ** 2))
    return wgt, rp


def source_costs(ref, srcs, cams, rows, cols, depth, normal, radius=5, step=1, window=None):
    """Photometric per-source costs c_s [S,N] of hypotheses (depth [N], normal [N,3]) at pixels (rows, cols), with the reference
    variance [N], the source variances [S,N] (nan where the centre test already failed) and the cosines of the triangulation
    angles [S,N]."""
    geo, Kinv = source_geometry(cams)
    oy, ox = offsets(radius, step)
    wgt, rp = ref_window(ref, rows, cols, radius, step) if window is None else window
    W = wgt.sum(1)
    mr = (wgt * rp).sum(1) / W
    vr = (wgt * rp * rp).sum(1) / W - mr * mr
    d = np.asarray(depth, dtype=np.float64)
    n = np.asarray(normal, dtype=np.float64)
    m = _rays(Kinv, rows, cols)
    X0 = d[:, None] * m
    rho = d * (n * m).sum(1)
    g = (n @ Kinv) / rho[:, None]                               # g^T q = n^T K^-1 q / rho
    qx = cols[:, None] + ox[None]
    qy = rows[:, None] + oy[None]
    S = len(srcs)
    cost = np.full((S, len(rows)), 2.0)
    vs_out = np.full((S, len(rows)), np.nan)
    cosang = np.zeros((S, len(rows)))
    for s in range(S):
        A, b, C = geo[s]["A"], geo[s]["b"], geo[s]["C"]
        H = A[None] + b[None, :, None] * g[:, None, :]          # [N,3,3]
        x = [H[:, i, 0, None] * qx + H[:, i, 1, None] * qy + H[:, i, 2, None] for i in range(3)]
        pos = x[2] > 0
        u = np.where(pos, x[0] / np.where(pos, x[2], 1.0), 0.0)
        v = np.where(pos, x[1] / np.where(pos, x[2], 1.0), 0.0)
        hs, ws = srcs[s].shape
        ci = len(oy) // 2
        centre_ok = pos[:, ci] & (u[:, ci] >= 0) & (u[:, ci] <= ws - 1) & (v[:, ci] >= 0) & (v[:, ci] <= hs - 1)
        val = _bilinear(srcs[s], u, v)
        sp = val - val[:, ci, None]
        ms = (wgt * sp).sum(1) / W
        vs = (wgt * sp * sp).sum(1) / W - ms * ms
        cov = (wgt * rp * sp).sum(1) / W - mr * ms
        r2 = X0 - C[None]
        ca = (X0 * r2).sum(1) / (np.linalg.norm(X0, axis=1) * np.linalg.norm(r2, axis=1))
        cosang[s] = ca
        ok = centre_ok & (vr >= MIN_VAR) & (vs >= MIN_VAR) & (ca <= math.cos(math.radians(MIN_TRI_DEG)))
        with np.errstate(invalid="ignore", divide="ignore"):
            ncc = cov / np.sqrt(vr * vs)
        cost[s] = np.where(ok, np.clip(1.0 - ncc, 0.0, 2.0), 2.0)
        vs_out[s] = np.where(centre_ok, vs, np.nan)
    return cost, vr, vs_out, cosang


def geom_errors(cams, src_depths, rows, cols, depth, normal, margin=1e-4):
    """Forward-backward errors e_s [S,N] (capped at GEOM_EMAX) against the sources' depth maps, and a flag [N] for pixels where a
    rounding of the forward projection lies within ``margin`` of a half-integer (fp32 and fp64 may round it differently)."""
    geo, Kinv = source_geometry(cams)
    d = np.asarray(depth, dtype=np.float64)
    p = np.stack([cols, rows], axis=-1).astype(np.float64)
    e = np.full((len(geo), len(rows)), GEOM_EMAX)
    amb = np.zeros(len(rows), dtype=bool)
    for s, gs in enumerate(geo):
        Ds = np.asarray(src_depths[s], dtype=np.float64)
        hs, ws = Ds.shape
        p3 = np.stack([cols, rows, np.ones(rows.shape)], axis=-1).astype(np.float64)
        y = d[:, None] * (p3 @ gs["A"].T) + gs["b"][None]               # K_s (R_rel X0 + t_rel)
        ok = y[:, 2] > 0
        z = np.where(ok, y[:, 2], 1.0)
        u, v = y[:, 0] / z, y[:, 1] / z
        ok &= np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 2 ** 30) & (np.abs(v) < 2 ** 30)
        u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
        amb |= ok & ((np.abs(np.abs(u - np.trunc(u)) - 0.5) < margin) | (np.abs(np.abs(v - np.trunc(v)) - 0.5) < margin))
        qx = np.where(u >= 0, np.floor(u + 0.5), np.ceil(u - 0.5)).astype(np.int64)
        qy = np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)
        ok &= (qx >= 0) & (qx < ws) & (qy >= 0) & (qy < hs)
        ds = np.where(ok, Ds[np.clip(qy, 0, hs - 1), np.clip(qx, 0, ws - 1)], 0.0)
        ok &= ds > 0
        q = np.stack([qx, qy, np.ones_like(qx)], axis=-1).astype(np.float64)
        yr = ds[:, None] * (q @ gs["G"].T) + gs["c"][None]
        ok &= yr[:, 2] > 0
        zr = np.where(ok, yr[:, 2], 1.0)
        err = np.hypot(yr[:, 0] / zr - p[:, 0], yr[:, 1] / zr - p[:, 1])
        e[s] = np.where(ok, np.minimum(err, GEOM_EMAX), GEOM_EMAX)
    return e, amb


def aggregate(cost, top_k):
    """Mean of the top_k smallest per-source costs, [S,N] -> [N]."""
    return np.sort(cost, axis=0)[:top_k].mean(0)


# ---------------------------------------------------------------------------------------------------------------------------
# hypotheses
# ---------------------------------------------------------------------------------------------------------------------------
def random_hypothesis(Kinv, rows, cols, w, depth_min, depth_max, seed, view, iteration, colour):
    """Candidate 10 (and the initialisation): inverse depth uniform in [1/dmax, 1/dmin], normal uniform on the sphere, flipped to
    face the camera.  -> depth [N], normal [N,3]."""
    pix = rows.astype(np.int64) * w + cols
    u_d = pm_uniform(seed, view, pix, iteration, colour, SLOT_RDEPTH)
    u_z = pm_uniform(seed, view, pix, iteration, colour, SLOT_RZ)
    u_a = pm_uniform(seed, view, pix, iteration, colour, SLOT_RAZ)
    lo, hi = 1.0 / np.float64(np.float32(depth_max)), 1.0 / np.float64(np.float32(depth_min))
    d = 1.0 / (lo + u_d * (hi - lo))
    z = 1.0 - 2.0 * u_z
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    a = 2.0 * math.pi * u_a
    n = np.stack([r * np.cos(a), r * np.sin(a), z], axis=-1)
    m = _rays(Kinv, rows, cols)
    n = np.where(((n * m).sum(1) > 0)[:, None], -n, n)
    return d, n


def perturbed_hypothesis(Kinv, rows, cols, w, d, n, depth_min, depth_max, delta, theta, seed, view, iteration, colour):
    """Candidate 9: n rotated by phi = theta u about the axis at angle alpha = 2 pi u' in the tangent plane (basis e1 =
    normalise(n x a), a = x if |n_x| < 0.9 else y; e2 = n x e1), kept unrotated when the result does not face the camera; inverse
    depth moved by (2u'' - 1) delta (1/dmin - 1/dmax) and clamped into the range."""
    pix = rows.astype(np.int64) * w + cols
    u_p = pm_uniform(seed, view, pix, iteration, colour, SLOT_PHI)
    u_a = pm_uniform(seed, view, pix, iteration, colour, SLOT_ALPHA)
    u_d = pm_uniform(seed, view, pix, iteration, colour, SLOT_DEPTH)
    # 0.9 as the fp32 number the kernel compares with: the two differ only for |n_x| = 0.9f exactly
    axis = np.where((np.abs(n[:, 0]) < float(np.float32(0.9)))[:, None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    e1 = np.cross(n, axis)
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(n, e1)
    phi, al = theta * u_p, 2.0 * math.pi * u_a
    t = np.cos(al)[:, None] * e1 + np.sin(al)[:, None] * e2
    n2 = np.cos(phi)[:, None] * n + np.sin(phi)[:, None] * t
    n2 /= np.linalg.norm(n2, axis=1, keepdims=True)
    m = _rays(Kinv, rows, cols)
    n2 = np.where(((n2 * m).sum(1) < 0)[:, None], n2, n)
    lo, hi = 1.0 / np.float64(np.float32(depth_max)), 1.0 / np.float64(np.float32(depth_min))
    inv = np.clip(1.0 / d + (2.0 * u_d - 1.0) * delta * (hi - lo), lo, hi)
    return 1.0 / inv, n2


def init_state(h, w, cams, depth_min, depth_max, seed, view):
    _, Kinv = source_geometry(cams)
    rows, cols = np.divmod(np.arange(h * w), w)
    d, n = random_hypothesis(Kinv, rows, cols, w, depth_min, depth_max, seed, view, INIT_ITERATION, 0)
    return np.concatenate([d[:, None], n], axis=1).reshape(h, w, 4)


def candidates(state, cams, rows, cols, depth_min, depth_max, delta, theta, seed, view, iteration, colour):
    """[11,N,4] candidate hypotheses and [11,N] skip flags of the pixels (rows, cols) (section 2h, in index order)."""
    h, w, _ = state.shape
    _, Kinv = source_geometry(cams)
    st = np.asarray(state, dtype=np.float64)
    N = len(rows)
    cand = np.zeros((NUM_CAND, N, 4))
    skip = np.zeros((NUM_CAND, N), dtype=bool)
    cur = st[rows, cols]
    cand[0] = cur
    m = _rays(Kinv, rows, cols)
    dmin, dmax = float(np.float32(depth_min)), float(np.float32(depth_max))
    for k, (dr, dc) in enumerate(NEIGHBOURS, start=1):
        qr, qc = rows + dr, cols + dc
        inside = (qr >= 0) & (qr < h) & (qc >= 0) & (qc < w)
        q = st[np.clip(qr, 0, h - 1), np.clip(qc, 0, w - 1)]
        nq = q[:, 1:]
        Xq = q[:, :1] * _rays(Kinv, np.clip(qr, 0, h - 1), np.clip(qc, 0, w - 1))
        with np.errstate(invalid="ignore", divide="ignore"):
            d = (nq * Xq).sum(1) / (nq * m).sum(1)
        ok = inside & (d >= dmin) & (d <= dmax)
        cand[k, :, 0] = np.where(ok, d, 0.0)
        cand[k, :, 1:] = np.where(ok[:, None], nq, 0.0)
        skip[k] = ~ok
    d9, n9 = perturbed_hypothesis(Kinv, rows, cols, w, cur[:, 0], cur[:, 1:], depth_min, depth_max, delta, theta, seed, view,
                                  iteration, colour)
    cand[9, :, 0], cand[9, :, 1:] = d9, n9
    d10, n10 = random_hypothesis(Kinv, rows, cols, w, depth_min, depth_max, seed, view, iteration, colour)
    cand[10, :, 0], cand[10, :, 1:] = d10, n10
    return cand, skip


def colour_pixels(h, w, colour):
    rows, cols = np.divmod(np.arange(h * w), w)
    sel = ((rows + cols) & 1) == colour
    return rows[sel], cols[sel]


def half_step(state, ref, srcs, cams, depth_min, depth_max, *, colour, iteration, delta, theta, seed, view, src_depths=None,
              radius=5, step=1, top_k=None):
    """One half-step on a copy of ``state`` -> (new state, choice [h,w] int (-1 on the other colour), candidates [h,w,11,4]
    (0 where skipped or on the other colour), gap [h,w] between the best two aggregated costs (inf where fewer than two),
    ambiguous [h,w] geometric rounding flag)."""
    h, w, _ = state.shape
    top_k = min(len(srcs), 3) if top_k is None else top_k
    rows, cols = colour_pixels(h, w, colour)
    cand, skip = candidates(state, cams, rows, cols, depth_min, depth_max, delta, theta, seed, view, iteration, colour)
    win = ref_window(ref, rows, cols, radius, step)
    agg = np.full((NUM_CAND, len(rows)), np.inf)
    amb = np.zeros(len(rows), dtype=bool)
    for k in range(NUM_CAND):
        live = ~skip[k]
        if not live.any():
            continue
        idx = np.nonzero(live)[0]
        c, _, _, _ = source_costs(ref, srcs, cams, rows[idx], cols[idx], cand[k, idx, 0], cand[k, idx, 1:], radius, step,
                                  window=(win[0][idx], win[1][idx]))
        if src_depths is not None:
            e, a = geom_errors(cams, src_depths, rows[idx], cols[idx], cand[k, idx, 0], cand[k, idx, 1:])
            c = c + GEOM_LAMBDA * np.minimum(e, GEOM_EMAX)
            amb[idx] |= a
        agg[k, idx] = aggregate(c, top_k)
    choice = np.argmin(agg, axis=0)               # first minimum: ties go to the lowest index
    srt = np.sort(agg, axis=0)
    gap = srt[1] - srt[0]
    new = np.array(state, dtype=np.float64, copy=True)
    new[rows, cols] = cand[choice, np.arange(len(rows))]
    ch = np.full((h, w), -1, dtype=np.int64)
    ch[rows, cols] = choice
    cd = np.zeros((h, w, NUM_CAND, 4))
    cd[rows, cols] = np.where(skip[..., None], 0.0, cand).transpose(1, 0, 2)
    gp = np.full((h, w), np.inf)
    gp[rows, cols] = gap
    am = np.zeros((h, w), dtype=bool)
    am[rows, cols] = amb
    return new, ch, cd, gp, am


def patch_match(ref, srcs, cams, depth_min, depth_max, *, num_iterations=8, seed=0, view=0, src_depths=None, state=None,
                radius=5, step=1, top_k=None):
    """The photometric pass (src_depths None, from the random initialisation) or the geometric pass (from ``state``)."""
    h, w = ref.shape
    pas = 0 if src_depths is None else 1
    if state is None:
        state = init_state(h, w, cams, depth_min, depth_max, seed, view)
    for t in range(num_iterations):
        delta, theta = schedule(t)
        for colour in (0, 1):
            state = half_step(state, ref, srcs, cams, depth_min, depth_max, colour=colour, iteration=(pas << 16) | t,
                              delta=delta, theta=theta, seed=seed, view=view, src_depths=src_depths, radius=radius, step=step,
                              top_k=top_k)[0]
    return state


def filter_counts(state, ref, srcs, cams, src_depths, radius=5, step=1):
    """Per pixel: the number of sources passing all three filter tests, and a margin flag for pixels where a test value lies
    within a small band of its threshold (or a rounding is ambiguous)."""
    h, w, _ = state.shape
    rows, cols = np.divmod(np.arange(h * w), w)
    st = np.asarray(state, dtype=np.float64).reshape(-1, 4)
    live = st[:, 0] > 0
    c, _, vs, ca = source_costs(ref, srcs, cams, rows, cols, np.where(live, st[:, 0], 1.0), np.where(live[:, None], st[:, 1:],
                                np.array([0.0, 0.0, -1.0])), radius, step)
    e, amb = geom_errors(cams, src_depths, rows, cols, np.where(live, st[:, 0], 1.0), np.where(live[:, None], st[:, 1:],
                         np.array([0.0, 0.0, -1.0])))
    cmin = math.cos(math.radians(FILTER_MIN_TRI_DEG))
    ok = (c <= FILTER_MAX_COST) & (ca <= cmin) & (e <= FILTER_MAX_ERR)
    count = np.where(live, ok.sum(0), 0)
    near = (np.abs(c - FILTER_MAX_COST) < 1e-3) | (np.abs(ca - cmin) < 1e-6) | (np.abs(e - FILTER_MAX_ERR) < 1e-3) \
        | ((np.abs(vs - MIN_VAR) < 0.01 * MIN_VAR) & np.isfinite(vs))
    margin = live & (near.any(0) | amb)
    return count.reshape(h, w), margin.reshape(h, w)


def filter_state(state, ref, srcs, cams, src_depths, radius=5, step=1):
    """COLMAP's filter: (depth [h,w], normal [h,w,3]) with pixels of fewer than FILTER_MIN_CONSISTENT passing sources zeroed."""
    count, _ = filter_counts(state, ref, srcs, cams, src_depths, radius, step)
    keep = count >= FILTER_MIN_CONSISTENT
    st = np.asarray(state, dtype=np.float64)
    return np.where(keep, st[..., 0], 0.0), np.where(keep[..., None], st[..., 1:], 0.0)


def reconstruct(greys, cams_all, src_lists, depth_min, depth_max, *, num_iterations=8, seed=0, top_k=None):
    """The full rule over a scene: the photometric pass of every view, then each view's geometric pass against its sources'
    photometric depths, then the filter.  cams_all [V,30]; src_lists per view; depth ranges [V].
    -> (photometric states, geometric states, filtered depths, filtered normals), lists over the views."""
    V = len(greys)
    photo = []
    for v in range(V):
        ids = [v] + list(src_lists[v])
        photo.append(patch_match(greys[v], [greys[s] for s in src_lists[v]], cams_all[ids], depth_min[v], depth_max[v],
                                 num_iterations=num_iterations, seed=seed, view=v, top_k=top_k))
    geom, depth, normal = [], [], []
    for v in range(V):
        ids = [v] + list(src_lists[v])
        srcs = [greys[s] for s in src_lists[v]]
        sd = [photo[s][..., 0] for s in src_lists[v]]
        g = patch_match(greys[v], srcs, cams_all[ids], depth_min[v], depth_max[v], num_iterations=num_iterations, seed=seed,
                        view=v, src_depths=sd, state=photo[v], top_k=top_k)
        d, n = filter_state(g, greys[v], srcs, cams_all[ids], sd)
        geom.append(g); depth.append(d); normal.append(n)
    return photo, geom, depth, normal


def accuracy(depth, normal, gt_depth, gt_normal, untextured, vis):
    """The accuracy bars' four numbers over the views: (fraction of kept textured pixels within 1 % relative depth, fraction of
    textured pixels seen by >= 2 sources that are kept, median normal error in degrees over kept textured pixels, fraction of the
    untextured patch filtered out)."""
    d, gd = np.stack(depth), np.asarray(gt_depth, dtype=np.float64)
    n, gn = np.stack(normal), np.asarray(gt_normal, dtype=np.float64)
    unt, vis = np.asarray(untextured, dtype=bool), np.asarray(vis)
    kept = d > 0
    tex_kept = kept & ~unt
    within = (np.abs(d - gd) <= 0.01 * gd) & tex_kept
    cand = ~unt & (vis >= 2)
    cosn = np.clip((n * gn).sum(-1) / np.maximum(np.linalg.norm(n, axis=-1), 1e-12), -1.0, 1.0)
    return (within.sum() / max(tex_kept.sum(), 1), (kept & cand).sum() / max(cand.sum(), 1),
            float(np.median(np.degrees(np.arccos(cosn[tex_kept])))) if tex_kept.any() else 180.0,
            1.0 - (kept & unt).sum() / max(unt.sum(), 1))
