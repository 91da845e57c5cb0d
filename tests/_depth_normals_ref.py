"""The rule of csrc/depth_normals.hip in numpy float64: normal maps from depth maps by a linear
least-squares fit of the inverse depth over a gated window, and the world normals of fused points.  Vectorised over the pixels;
the taps are walked in the stated order (j outer, i inner), every product and sum is its own float64 operation (numpy fuses
nothing), so the kernel, built without contractions, has to reproduce every bit."""
import numpy as np

CAM_K, CAM_KINV, CAM_R, CAM_T = 0, 9, 18, 27
F32_MAX = np.float32(3.402823466e38)


def depth_ok(d):
    """cf_depth_ok of geo_common.h on a float32 array: 0 < d finite."""
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (d > np.float32(0.0)) & (d <= F32_MAX)


def window_sums(depth, radius, rel_gate):
    """The gated window sums of every pixel of a float32 depth map -> dict of [h,w] arrays: ``ok``, ``n`` and the six geometric
    sums (int64), ``Se``, ``Sie``, ``Sje`` (float64)."""
    d32 = np.asarray(depth, dtype=np.float32)
    h, w = d32.shape
    r, tau = int(radius), float(rel_gate)
    ok = depth_ok(d32)
    d = np.where(ok, d32, np.float32(1.0)).astype(np.float64)
    rho = np.where(ok, 1.0 / d, 0.0)                       # once per valid pixel
    d = np.where(ok, d, 0.0)
    dP, rP, oP = (np.pad(a, r, mode="constant") for a in (d, rho, ok))
    thr = tau * d
    S = {k: np.zeros((h, w), dtype=np.int64) for k in ("n", "Si", "Sj", "Sii", "Sij", "Sjj")}
    Se, Sie, Sje = (np.zeros((h, w), dtype=np.float64) for _ in range(3))
    for j in range(-r, r + 1):
        for i in range(-r, r + 1):
            sl = (slice(r + j, r + j + h), slice(r + i, r + i + w))
            dq, rq, oq = dP[sl], rP[sl], oP[sl]
            on = ok & oq & (np.abs(dq - d) <= thr)
            if i == 0 and j == 0:
                on = ok.copy()                             # the centre always counts
            e = d * rq - 1.0
            S["n"] += on
            S["Si"] += on * i
            S["Sj"] += on * j
            S["Sii"] += on * (i * i)
            S["Sij"] += on * (i * j)
            S["Sjj"] += on * (j * j)
            Se = np.where(on, Se + e, Se)
            Sie = np.where(on, Sie + float(i) * e, Sie)
            Sje = np.where(on, Sje + float(j) * e, Sje)
    return dict(S, ok=ok, Se=Se, Sie=Sie, Sje=Sje)


def solve(s):
    """Cofactors, determinant and the scaled solution of the 3 x 3 normal equations, float64 in the stated order."""
    S1, Si, Sj, Sii, Sij, Sjj = (s[k].astype(np.float64) for k in ("n", "Si", "Sj", "Sii", "Sij", "Sjj"))
    Se, Sie, Sje = s["Se"], s["Sie"], s["Sje"]
    C00 = Sjj * S1 - Sj * Sj
    C01 = Sj * Si - Sij * S1
    C02 = Sij * Sj - Sjj * Si
    C11 = Sii * S1 - Si * Si
    C12 = Sij * Si - Sii * Sj
    C22 = Sii * Sjj - Sij * Sij
    det = Sii * C00 + Sij * C01 + Si * C02
    A = C00 * Sie + C01 * Sje + C02 * Se
    B = C01 * Sie + C11 * Sje + C12 * Se
    Cc = C02 * Sie + C12 * Sje + C22 * Se
    return det, A, B, det + Cc


def depth_normals(depth, cam, radius=2, rel_gate=0.05, min_support=6, want_parts=False):
    """depth float32 [h,w], cam the 30 floats of ops.geo_filter_cams -> (normal float32 [h,w,3], support int32 [h,w])."""
    cam = np.asarray(cam, dtype=np.float32).astype(np.float64)
    K, Ki = cam[CAM_K:CAM_K + 9], cam[CAM_KINV:CAM_KINV + 9]
    s = window_sums(depth, radius, rel_gate)
    ok, n = s["ok"], s["n"]
    h, w = ok.shape
    det, A, B, g2 = solve(s)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        fit = ok & (n >= int(min_support)) & (det > 0.0) & (g2 > 0.0)
        g0, g1, gc = A, B, g2 - A * x - B * y
        vf = [-(K[k] * g0 + K[3 + k] * g1 + K[6 + k] * gc) for k in range(3)]
        vb = [-(Ki[3 * k] * x + Ki[3 * k + 1] * y + Ki[3 * k + 2] * 1.0) for k in range(3)]
        v = [np.where(fit, a, b) for a, b in zip(vf, vb)]
        norm = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        normal = np.stack([np.where(ok, c / norm, 0.0) for c in v], axis=-1).astype(np.float32)
    support = np.where(ok, np.where(fit, n, -n), 0).astype(np.int32)
    if want_parts:
        return normal, support, dict(s, det=det, A=A, B=B, g2=g2, fit=fit)
    return normal, support


def world_normal(cam, n):
    """cf_world_normal: w = R^T n, float64 sums left to right, rounded to float32.  n [..., 3] float32."""
    R = np.asarray(cam, dtype=np.float32)[CAM_R:CAM_R + 9].astype(np.float64)
    n = np.asarray(n, dtype=np.float32).astype(np.float64)
    return np.stack([R[k] * n[..., 0] + R[3 + k] * n[..., 1] + R[6 + k] * n[..., 2] for k in range(3)], axis=-1).astype(np.float32)


def point_world_normals(view, pixel, normals, cams):
    """view, pixel int [M]; normals V x float32 [h_v,w_v,3]; cams [V,30] -> float32 [M,3]; an index outside its range gives 0."""
    out = np.zeros((len(view), 3), dtype=np.float32)
    for k, (v, p) in enumerate(zip(view, pixel)):
        if 0 <= v < len(normals) and 0 <= p < normals[v].shape[0] * normals[v].shape[1]:
            out[k] = world_normal(cams[v], normals[v].reshape(-1, 3)[p])
    return out
