"""The two rules of csrc/tsdf_fusion.hip in numpy float64: depth maps into a dense TSDF volume, and
the volume into an indexed triangle mesh by marching tetrahedra.  Vectorised over the voxels; every product and sum is its own
float64 operation in the stated order (numpy fuses nothing), the views are walked in order in chunks of 64 with tsdf_sum rounded
to float32 after each chunk, and nothing is culled -- so the kernels, built without contractions, have to reproduce every bit."""
import functools

import numpy as np

CAM_K, CAM_KINV, CAM_R, CAM_T = 0, 9, 18, 27
F32_MAX = np.float32(3.402823466e38)
MAX_VIEWS = 64
ORDERS = ((1, 2, 4), (1, 4, 2), (2, 1, 4), (2, 4, 1), (4, 1, 2), (4, 2, 1))


def depth_ok(d):
    """cf_depth_ok of geo_common.h on a float32 array: 0 < d finite."""
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (d > np.float32(0.0)) & (d <= F32_MAX)


def volume(dims):
    nx, ny, nz = dims
    return dict(tsdf_sum=np.zeros((nz, ny, nx), np.float32), weight=np.zeros((nz, ny, nx), np.int32),
                rgb_sum=np.zeros((nz, ny, nx, 3), np.float32), cweight=np.zeros((nz, ny, nx), np.int32))


def lattice(dims, origin, voxel):
    """X, Y, Z [nz,ny,nx] float64: o + i s, the product first."""
    nx, ny, nz = dims
    s = float(voxel)
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return float(origin[0]) + i * s, float(origin[1]) + j * s, float(origin[2]) + k * s


def project(cam, X, Y, Z):
    """cf_project: K (R X + t), float64 sums left to right."""
    c = np.asarray(cam, dtype=np.float32).astype(np.float64)
    K, R, t = c[CAM_K:CAM_K + 9], c[CAM_R:CAM_R + 9], c[CAM_T:CAM_T + 3]
    e = [R[3 * r] * X + R[3 * r + 1] * Y + R[3 * r + 2] * Z + t[r] for r in range(3)]
    return tuple(K[3 * r] * e[0] + K[3 * r + 1] * e[1] + K[3 * r + 2] * e[2] for r in range(3))


def integrate(state, depths, colors, cams, origin, voxel, trunc):
    """Adds the views to ``state`` in place.  depths V x float32 [h,w], colors V x uint8 [h,w,3], cams [V,30]."""
    nz, ny, nx = state["weight"].shape
    X, Y, Z = lattice((nx, ny, nz), origin, voxel)
    trunc = float(trunc)
    for first in range(0, len(depths), MAX_VIEWS):
        S = state["tsdf_sum"].astype(np.float64)
        rgb = state["rgb_sum"].astype(np.int64)
        for v in range(first, min(first + MAX_VIEWS, len(depths))):
            d32 = np.asarray(depths[v], dtype=np.float32)
            h, w = d32.shape
            x, y, z = project(cams[v], X, Y, Z)
            with np.errstate(all="ignore"):
                px, py = np.floor(x / z + 0.5), np.floor(y / z + 0.5)
                on = (z > 0.0) & (px >= 0.0) & (px < float(w)) & (py >= 0.0) & (py < float(h))
            ix, iy = np.where(on, px, 0.0).astype(np.int64), np.where(on, py, 0.0).astype(np.int64)
            d = d32[iy, ix]
            on &= depth_ok(d)
            with np.errstate(all="ignore"):
                sd = d.astype(np.float64) - z
                on &= ~(sd < -trunc)
                q = sd / trunc
                phi = np.where(q < 1.0, q, 1.0)
                S = np.where(on, S + phi, S)
                near = on & (sd <= trunc)
            state["weight"] += on
            rgb += np.where(near[..., None], np.asarray(colors[v])[iy, ix].astype(np.int64), 0)
            state["cweight"] += near
        state["tsdf_sum"][...] = S.astype(np.float32)
        state["rgb_sum"][...] = rgb.astype(np.float32)
    return state


# ---- marching tetrahedra ---------------------------------------------------------------------------------------------------------
def offset(c):
    return np.array((c & 1, c >> 1 & 1, c >> 2 & 1))


def tet_corners(T):
    a, b, _ = ORDERS[T]
    return (0, a, a | b, 7)


@functools.lru_cache(maxsize=None)
def tet_case(T, neg):
    """The oriented cycle of tetrahedron T for the set ``neg`` (bit u = corner position u is negative): a tuple of (u, v) position
    pairs, u < v, decided on the lattice as the issue states it."""
    cc = tet_corners(T)
    N = [u for u in range(4) if neg >> u & 1]
    P = [u for u in range(4) if not neg >> u & 1]
    if len(N) in (1, 3):
        lone = N[0] if len(N) == 1 else P[0]
        cyc = [(min(u, lone), max(u, lone)) for u in range(4) if u != lone]
    elif len(N) == 2:
        cyc = [(N[0], P[0]), (N[0], P[1]), (N[1], P[1]), (N[1], P[0])]
        cyc = [(min(a, b), max(a, b)) for a, b in cyc]
    else:
        return ()
    mid2 = [offset(cc[u]) + offset(cc[v]) for u, v in cyc[:3]]
    normal = np.cross(mid2[1] - mid2[0], mid2[2] - mid2[0])
    towards = len(N) * sum(offset(cc[u]) for u in P) - len(P) * sum(offset(cc[u]) for u in N)
    dot = int(normal @ towards)
    assert dot != 0
    return tuple(cyc if dot > 0 else cyc[::-1])


def case_table():
    """The 6 x 16 table in the encoding of pscv_tsdf_case_table."""
    tab = np.zeros(96, dtype=np.uint32)
    for T in range(6):
        cc = tet_corners(T)
        for neg in range(16):
            cyc = tet_case(T, neg)
            e = len(cyc)
            for k, (u, v) in enumerate(cyc):
                e |= (cc[u] | (cc[v] ^ cc[u]) << 3) << (3 + 6 * k)
            tab[T * 16 + neg] = e
    return tab


def extract(state, origin, voxel, min_weight=1):
    """-> (xyz float32 [V,3], rgb uint8 [V,3], faces int32 [F,3]) in the defined order."""
    w = state["weight"]
    nz, ny, nx = w.shape
    with np.errstate(all="ignore"):
        f = state["tsdf_sum"].astype(np.float64) / w.astype(np.float64)
        obs = w >= int(min_weight)
        neg = obs & (f < 0.0)
        cw = state["cweight"]
        mean = state["rgb_sum"].astype(np.float64) / cw.astype(np.float64)[..., None]
    X = np.stack(lattice((nx, ny, nz), origin, voxel), axis=-1)
    nvox = nx * ny * nz
    has = np.zeros((nz, ny, nx, 7), dtype=bool)
    for d in range(1, 8):
        ox, oy, oz = offset(d)
        sp = (slice(0, nz - oz), slice(0, ny - oy), slice(0, nx - ox))
        sq = (slice(oz, nz), slice(oy, ny), slice(ox, nx))
        has[sp + (d - 1,)] = obs[sp] & obs[sq] & (neg[sp] != neg[sq])
    keys = np.flatnonzero(has.reshape(-1))
    vid = np.full(nvox * 7, -1, dtype=np.int64)
    vid[keys] = np.arange(keys.size)
    lin, d = keys // 7, keys % 7 + 1
    pk, pj, pi = lin // (nx * ny), lin // nx % ny, lin % nx
    qk, qj, qi = pk + (d >> 2 & 1), pj + (d >> 1 & 1), pi + (d & 1)
    fp, fq = f[pk, pj, pi], f[qk, qj, qi]
    t = fp / (fp - fq)
    Xp, Xq = X[pk, pj, pi], X[qk, qj, qi]
    xyz = (Xp + t[:, None] * (Xq - Xp)).astype(np.float32)
    mp, mq = mean[pk, pj, pi], mean[qk, qj, qi]
    cp, cq = (cw[pk, pj, pi] > 0)[:, None], (cw[qk, qj, qi] > 0)[:, None]
    with np.errstate(all="ignore"):
        val = np.where(cp & cq, mp + t[:, None] * (mq - mp), np.where(cp, mp, np.where(cq, mq, 0.0)))
    rgb = np.clip(np.floor(val + 0.5), 0.0, 255.0).astype(np.uint8)

    faces = []
    obs_l, neg_l = obs.reshape(-1).tolist(), neg.reshape(-1).tolist()
    step = (1, nx, nx * ny)
    clin = [sum(int(o) * s for o, s in zip(offset(c), step)) for c in range(8)]
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                p = (k * ny + j) * nx + i
                if not any(obs_l[p + c] for c in clin):
                    continue
                for T in range(6):
                    cc = tet_corners(T)
                    if not all(obs_l[p + clin[c]] for c in cc):
                        continue
                    case = sum(int(neg_l[p + clin[c]]) << u for u, c in enumerate(cc))
                    cyc = tet_case(T, case)
                    if not cyc:
                        continue
                    q = [int(vid[(p + clin[cc[u]]) * 7 + (cc[v] ^ cc[u]) - 1]) for u, v in cyc]
                    assert min(q) >= 0
                    m = q.index(min(q))
                    q = q[m:] + q[:m]
                    faces.append(q[:3])
                    if len(q) == 4:
                        faces.append([q[0], q[2], q[3]])
    return xyz, rgb, np.asarray(faces, dtype=np.int32).reshape(-1, 3)


# ---- mesh properties the tests assert --------------------------------------------------------------------------------------------
def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))


def unmatched_edges(faces):
    """The directed edges whose reverse does not appear exactly once (and the edges that appear twice themselves)."""
    e = directed_edges(faces)
    n = int(e.max()) + 1 if e.size else 1
    key, rev = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    count = dict(zip(uniq.tolist(), cnt.tolist()))
    bad = [k for k, (a, b) in enumerate(zip(key.tolist(), rev.tolist())) if count[a] != 1 or count.get(b, 0) != 1]
    return e[bad]


def signed_volume(xyz, faces):
    p = np.asarray(xyz, dtype=np.float64)
    a, b, c = (p[np.asarray(faces)[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
