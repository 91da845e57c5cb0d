"""The rules of csrc/mesh_metrics.hip in numpy: surface samples proportional to area from a
counter-based splitmix64 hash, and the exact bounded distance from points to the surface of an indexed triangle mesh, brute force
over all faces with the lexicographic minimum over (d^2, face).  Every product and sum is its own float64 operation in the order
the kernels use (numpy fuses nothing; the kernels are built without contractions), the hashes are numpy uint64 arithmetic."""
import numpy as np

from tests._mesh_ref import valid_faces

MASK = (1 << 64) - 1
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MAX_COUNT = 2 ** 31 - 1
MAX_SAMPLES = 2 ** 31 - 2
REL = 1e-9          # a squared distance within REL (relative) of maxdist^2 is fragile


# ---- hash -----------------------------------------------------------------------------------------------------------------------
def mix(k):
    """splitmix64 finaliser on uint64 arrays (wrapping products)."""
    k = np.asarray(k, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k = (k ^ (k >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        k = (k ^ (k >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return k ^ (k >> np.uint64(31))


def step(x):
    """One splitmix64 step from state x: mix(x + 0x9e3779b97f4a7c15)."""
    with np.errstate(over="ignore"):
        return mix(np.asarray(x, dtype=np.uint64) + GOLDEN)


def unit(h):
    """uint64 -> float64 in [0, 1): (h >> 11) * 2^-53 (exact)."""
    return (np.asarray(h, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def face_hash(seed, f):
    """h_f = step(step(seed) ^ f)."""
    return step(step(np.uint64(int(seed) & MASK)) ^ np.asarray(f, dtype=np.uint64))


def sample_hash(hf, k):
    """h_fk = step(h_f ^ (k + 1))."""
    with np.errstate(over="ignore"):
        return step(np.asarray(hf, dtype=np.uint64) ^ (np.asarray(k, dtype=np.uint64) + np.uint64(1)))


# ---- sampling -------------------------------------------------------------------------------------------------------------------
def _corners(xyz, faces):
    p = np.asarray(xyz, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    ok = valid_faces(f, p.shape[0])
    g = np.where(ok[:, None], f, 0)
    if p.shape[0] == 0:
        z = np.zeros((f.shape[0], 3))
        return z, z.copy(), z.copy(), ok
    return p[g[:, 0]], p[g[:, 1]], p[g[:, 2]], ok


def _cross(u, v):
    return np.stack((u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]), axis=-1)


def _dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def areas(xyz, faces):
    """(A float64 [F], good bool [F]): 0.5 * sqrt(n . n), n = (b - a) x (c - a); good = valid, area finite and > 0."""
    a, b, c, ok = _corners(xyz, faces)
    with np.errstate(all="ignore"):
        n = _cross(b - a, c - a)
        A = 0.5 * np.sqrt(_dot(n, n))
        good = ok & (A > 0.0) & np.isfinite(A)
    return A, good


def _count_arg(xyz, faces, spacing, seed):
    A, good = areas(xyz, faces)
    s2 = float(spacing) * float(spacing)
    r = unit(face_hash(seed, np.arange(A.shape[0], dtype=np.uint64)))
    with np.errstate(all="ignore"):
        return np.where(good, A, 0.0) / s2 + r, good


def counts(xyz, faces, spacing, seed=0):
    """int64 [F]: n_f = floor(A_f / spacing^2 + r_f), 0 for a face that gives no samples, saturated at 2^31 - 1."""
    x, good = _count_arg(xyz, faces, spacing, seed)
    return np.where(good, np.minimum(np.floor(x), float(MAX_COUNT)), 0.0).astype(np.int64)


def fragile_faces(xyz, faces, spacing, seed=0):
    """The faces whose A_f / spacing^2 + r_f lies within 1e-9 of an integer: a last-bit difference of the area could change n_f."""
    x, good = _count_arg(xyz, faces, spacing, seed)
    return np.flatnonzero(good & (np.abs(x - np.rint(x)) <= 1e-9))


def sample(xyz, faces, spacing, seed=0, return_uv=False):
    """(points float32 [N,3], face int32 [N]) and, with return_uv, the folded (u, v) float64 [N,2]: face-major, k ascending."""
    n = counts(xyz, faces, spacing, seed)
    total = int(n.sum())
    if total > MAX_SAMPLES:
        raise ValueError(f"spacing {spacing} gives {total} samples")
    face = np.repeat(np.arange(n.shape[0], dtype=np.int64), n)
    off = np.cumsum(n) - n
    k = np.arange(total, dtype=np.int64) - off[face]
    hk = sample_hash(face_hash(seed, face.astype(np.uint64)), k.astype(np.uint64))
    u, v = unit(hk), unit(step(hk))
    fold = u + v > 1.0
    u, v = np.where(fold, 1.0 - u, u), np.where(fold, 1.0 - v, v)
    a, b, c, _ = _corners(xyz, faces)
    a, b, c = a[face], b[face], c[face]
    pts = ((a + u[:, None] * (b - a)) + v[:, None] * (c - a)).astype(np.float32)
    out = (pts.reshape(-1, 3), face.astype(np.int32))
    return out + (np.stack((u, v), axis=1),) if return_uv else out


# ---- distance -------------------------------------------------------------------------------------------------------------------
def segment_d2(q, p0, p1):
    """Squared distance from q [..,3] to the segments p0 p1 [..,3]: parameter clamped to [0, 1], 0 for a segment of length 0."""
    d, w = p1 - p0, q - p0
    dd = _dot(d, d)
    with np.errstate(all="ignore"):
        t = np.where(dd > 0.0, np.minimum(np.maximum(_dot(w, d) / np.where(dd > 0.0, dd, 1.0), 0.0), 1.0), 0.0)
    r = w - t[..., None] * d
    return _dot(r, r)


def face_d2(q, a, b, c):
    """Squared distance from q [..,3] to the triangles a b c [..,3] (broadcast), the kernel's expression order."""
    e0, e1 = b - a, c - a
    n = _cross(e0, e1)
    nn = _dot(n, n)
    wa, wb, wc = q - a, q - b, q - c
    s0 = _dot(_cross(e0, wa), n)
    s1 = _dot(_cross(c - b, wb), n)
    s2 = _dot(_cross(a - c, wc), n)
    inside = (nn > 0.0) & (s0 >= 0.0) & (s1 >= 0.0) & (s2 >= 0.0)
    h = _dot(wa, n)
    with np.errstate(all="ignore"):
        plane = (h * h) / np.where(nn > 0.0, nn, 1.0)
    edges = np.minimum(np.minimum(segment_d2(q, a, b), segment_d2(q, b, c)), segment_d2(q, c, a))
    return np.where(inside, plane, edges)


def dist_d2(query, xyz, faces, chunk=128):
    """(d2 float64 [m], face int64 [m]): the lexicographic minimum of (d^2, face) over the valid faces; (inf, -1) without any."""
    q = np.asarray(query, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    a, b, c, ok = _corners(xyz, faces)
    idx = np.flatnonzero(ok)
    best = np.full(q.shape[0], np.inf)
    face = np.full(q.shape[0], -1, dtype=np.int64)
    if idx.size == 0 or q.shape[0] == 0:
        return best, face
    a, b, c = a[idx][None], b[idx][None], c[idx][None]
    for s in range(0, q.shape[0], chunk):
        d2 = face_d2(q[s:s + chunk, None, :], a, b, c)            # [chunk, valid faces]
        j = np.argmin(d2, axis=1)                                  # the first minimum: the lowest face index among equals
        best[s:s + chunk] = d2[np.arange(d2.shape[0]), j]
        face[s:s + chunk] = idx[j]
    return best, face


def dist(query, xyz, faces, maxdist):
    """(distance float64 [m], face int32 [m], fragile bool [m]): sqrt(d^2) and the face where d^2 < maxdist^2 (strict), else
    (inf, -1); fragile where d^2 lies within REL (relative) of maxdist^2."""
    d2, face = dist_d2(query, xyz, faces)
    b2 = float(maxdist) * float(maxdist)
    hit = d2 < b2
    with np.errstate(invalid="ignore"):
        fragile = np.abs(d2 - b2) <= REL * b2 if np.isfinite(b2) else np.zeros(d2.shape, dtype=bool)
    return np.where(hit, np.sqrt(np.where(hit, d2, 0.0)), np.inf), np.where(hit, face, -1).astype(np.int32), fragile


# ---- the inputs the tests share ---------------------------------------------------------------------------------------------------
TRI_XYZ = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], dtype=np.float32)
TRI_FACES = np.array([[0, 1, 2]], dtype=np.int32)
# (query, closed-form distance to TRI): the face region, the three edge regions, the three vertex regions, then on the plane
# inside, on an edge, at a vertex and on the long edge
REGIONS = [((0.5, 0.5, 0.75), 0.75), ((1.0, -1.0, 0.5), np.sqrt(1.25)), ((2.0, 2.0, 1.0), np.sqrt(3.0)), ((-1.0, 1.0, 0.0), 1.0),
           ((-1.0, -1.0, 0.0), np.sqrt(2.0)), ((3.0, -1.0, 0.0), np.sqrt(2.0)), ((-1.0, 3.0, 2.0), np.sqrt(6.0)),
           ((0.5, 0.5, 0.0), 0.0), ((1.0, 0.0, 0.0), 0.0), ((2.0, 0.0, 0.0), 0.0), ((1.0, 1.0, 0.0), 0.0)]
BIG_TRI_XYZ = np.array([[1, 2, 3], [9, 3, 4], [2, 11, 5]], dtype=np.float32)           # area 36.6...: 5000 samples at spacing ~0.0856
DEGENERATE_XYZ = np.array([[0, 0, 0], [2, 1, -1], [1, 0.5, -0.5], [0.25, 0.5, 0.75]], dtype=np.float32)
DEGENERATE_FACES = np.array([[0, 1, 1], [0, 0, 1], [0, 2, 1], [1, 0, 2], [3, 3, 3]], dtype=np.int32)    # four segments 0-1, one point


def sphere_gt(n, seed):
    """n float32 points of the analytic sphere behind _mesh_ref.sphere_mesh()."""
    from tests._mesh_ref import SPHERE_N, SPHERE_ORIGIN
    v = np.random.default_rng(seed).normal(size=(n, 3))
    centre = (SPHERE_N - 1) / 2.0 + np.array(SPHERE_ORIGIN)
    return (centre + 4.7 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def dtu_gt(gt):
    """(gt, ObsMask, BB, Res, Plane) as metrics.load_gt returns them, for the sphere: a mask that hides the voxels with x index
    >= 8, the plane z = 6.5."""
    mask = np.ones((16, 16, 16), dtype=np.uint8)
    mask[8:] = 0
    return gt, mask, np.array([[0.0, 0.0, 0.0], [14.0, 14.0, 14.0]]), np.array([[1.0]]), np.array([[0.0], [0.0], [1.0], [-6.5]])


def write_cloud(path, pts):
    from wild_deep_mvs_amd.utils.point_cloud import write_point_cloud
    path.parent.mkdir(parents=True, exist_ok=True)
    write_point_cloud(path, pts, np.zeros(pts.shape, dtype=np.uint8))


def write_mesh(path, xyz, faces):
    from wild_deep_mvs_amd.utils.point_cloud import write_mesh as write
    path.parent.mkdir(parents=True, exist_ok=True)
    write(path, xyz, np.zeros(xyz.shape, dtype=np.uint8), faces)
