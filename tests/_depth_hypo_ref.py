"""Float64 reference of pscv_cvp_depth_hypos (csrc/depth_hypo.hip) in numpy, from the same fp64 [B,39] constants the kernel receives.
It never imports ``wild_deep_mvs_amd.ops``; ``host_cams`` builds the constants on the host in float64 (numpy's LAPACK inverse, not
pscv_cvp_cams).  Per batch item: per-pixel validity and |step| (the kernel's own formulation: Cramer's rule on rows 1..2 where the
oracle inverts a 2x2 matrix), the LOWER median at rank (n_valid - 1) // 2, the fallback where nothing is valid, and the eight planes
float32(d + (k - 4) s).

The bar of the step.  tests/test_depth_hypo_ref_cpu.py measures the worst relative distance between this float64 evaluation and the
oracle's (oracle.cvpmvsnet.cal_depth_hypo, another operation order: LAPACK inverses, a batched 2x2 inverse) over every case below;
STEP_DIST holds that measurement (the CPU test fails if it is exceeded), and the kernel -- which contracts multiply-adds, a rounding
difference of the same order -- is held to STEP_BAR = 8 STEP_DIST, far below the 1e-9 the planes' tie rule assumes and below the 10 %
by which every rank error moves the step in the few-valid cases.

The planes: the kernel rounds the fp64 sum once, so a plane is the reference's fp32 value bit for bit unless the reference's fp64 sum
lies within TIE_REL = 1e-9 (relative) of the midpoint of two fp32 neighbours; there it is within one fp32 ulp."""
import numpy as np

STEP_DIST = 1.62e-13        # measured on the CPU: 1.611e-13, the worst of CASES (partly_invalid, item 0); asserted by the CPU test
STEP_BAR = 8.0 * STEP_DIST
TIE_REL = 1e-9
H, W = 72, 97               # 6984 pixels: two select workgroups (one per 4096 keys, striding by 512), 28 key workgroups, the last ragged (72 of 256)
F = np.float64


def host_cams(ref_in, src_in, ref_ex, src_ex):
    """fp32-valued [B,3,3], [B,3,3], [B,4,4], [B,4,4] (the FIRST source view) -> float64 [B,39]:
    K_ref^-1, rows 0..2 of E_src E_ref^-1, K_src, (K_ref R_ref)(K_src R_src)^-1."""
    Kr, Ks, Er, Es = (np.asarray(a, dtype=F) for a in (ref_in, src_in, ref_ex, src_ex))
    out = []
    for b in range(Kr.shape[0]):
        T = Es[b] @ np.linalg.inv(Er[b])
        A = (Kr[b] @ Er[b][:3, :3]) @ np.linalg.inv(Ks[b] @ Es[b][:3, :3])
        out.append(np.concatenate((np.linalg.inv(Kr[b]).reshape(-1), T[:3].reshape(-1), Ks[b].reshape(-1), A.reshape(-1))))
    return np.stack(out)


def _steps(depth, c):
    """depth [H,W] float64, c [39] -> valid [H,W], |step| [H,W]"""
    h, w = depth.shape
    Kinv, T, Ks, A = c[0:9].reshape(3, 3), c[9:21].reshape(3, 4), c[21:30].reshape(3, 3), c[30:39].reshape(3, 3)
    y, x = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")

    def project(d):
        cam = np.einsum("jk,khw->jhw", Kinv, np.stack((x * d, y * d, d)))
        s = np.einsum("jk,khw->jhw", T[:, :3], cam) + T[:, 3].reshape(3, 1, 1)
        p = np.einsum("jk,khw->jhw", Ks, s)
        return p[0] / p[2], p[1] / p[2], p[2]
    with np.errstate(all="ignore"):
        u1, v1, z1 = project(depth)
        u2, v2, z2 = project(depth + 1.0)
        dx, dy = u2 - u1, v2 - v1
        nrm = np.sqrt(dx * dx + dy * dy)
        inv = 1.0 / np.maximum(nrm, 1e-8)
        u3, v3 = u1 + dx * inv, v1 + dy * inv
        r = np.einsum("jk,khw->jhw", A, np.stack((u1, v1, np.ones_like(u1)))) * z1
        cc = np.einsum("jk,khw->jhw", A, np.stack((u3, v3, np.ones_like(u3))))
        det = y * cc[2] - cc[1]
        delta = np.abs((cc[2] * r[1] - cc[1] * r[2]) / det)
        valid = (nrm > 1e-8) & (z1 > 1e-8) & (z2 > 1e-8) & (np.abs(det) > 1e-8) & ~np.isnan(delta)
    return valid, delta


def reference(depth, cams, fallback):
    """depth [B,H,W] (fp32 values), cams [B,39] float64, fallback [B] (fp32 values) -> dict: valid [B,H,W], abs_step [B,H,W],
    n_valid [B], steps [B] float64, sorted (list of the sorted valid steps), planes64 [B,8,H,W] and planes [B,8,H,W] float32."""
    depth = np.asarray(depth, dtype=F)
    B = depth.shape[0]
    out = {k: [] for k in ("valid", "abs_step", "n_valid", "steps", "sorted", "planes64")}
    for b in range(B):
        valid, delta = _steps(depth[b], np.asarray(cams[b], dtype=F))
        vals = np.sort(delta[valid])
        n = vals.size
        s = float(vals[(n - 1) // 2]) if n else float(np.float32(np.asarray(fallback).reshape(-1)[b]))
        with np.errstate(all="ignore"):
            planes = np.stack([depth[b] + float(k - 4) * s for k in range(8)])
        for k, v in zip(out, (valid, delta, n, s, vals, planes)):
            out[k].append(v)
    res = {k: (v if k == "sorted" else np.stack(v) if k in ("valid", "abs_step", "planes64") else np.asarray(v)) for k, v in out.items()}
    with np.errstate(all="ignore"):
        res["planes"] = res["planes64"].astype(np.float32)
    return res


def check_steps(tag, got, ref):
    """got [B] float64 from the kernel against ref['steps']: inside STEP_BAR relative, the fallback exactly.  Returns the worst
    distance in units of the bar."""
    got = np.asarray(got, dtype=F)
    worst = 0.0
    for b, (g, s, n) in enumerate(zip(got, ref["steps"], ref["n_valid"])):
        if n == 0:
            assert g == s, f"{tag}[{b}]: fallback {g!r} != {s!r}"
            continue
        rel = abs(g - s) / abs(s)
        worst = max(worst, rel / STEP_BAR)
        assert rel <= STEP_BAR, f"{tag}[{b}]: step {g!r} against {s!r}: relative distance {rel:.3e}, bar {STEP_BAR:.1e} (n_valid {n})"
    return worst


def check_planes(tag, got, ref):
    """got [B,8,H,W] float32 from the kernel: NaN / inf exactly where the reference has them, within one fp32 ulp everywhere, bit-equal
    wherever the reference's fp64 value is not within TIE_REL of a rounding tie.  Returns (number of near-tie elements, of differing)."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref["planes"].shape, (tag, got.dtype, got.shape)
    x, r32 = ref["planes64"], ref["planes"]
    fin = np.isfinite(x)
    assert np.array_equal(np.isnan(got), np.isnan(x)), f"{tag}: NaN planes differ"
    assert np.array_equal(got[np.isinf(x)], r32[np.isinf(x)]), f"{tag}: inf planes differ"
    g, rr, xx = got[fin], r32[fin], x[fin]
    other = np.where(xx >= rr.astype(F), np.nextafter(rr, np.float32(np.inf)), np.nextafter(rr, np.float32(-np.inf)))
    mid = 0.5 * (rr.astype(F) + other.astype(F))
    tie = np.abs(xx - mid) <= TIE_REL * np.abs(xx)
    diff = g != rr
    assert not np.any(diff & ~tie), f"{tag}: {int((diff & ~tie).sum())} planes differ from the rounded float64 value away from any tie"
    assert np.all(np.abs(g.astype(F) - rr.astype(F)) <= np.spacing(np.abs(rr)).astype(F)), f"{tag}: a plane is more than one ulp away"
    return int(tie.sum()), int(diff.sum())


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
FEW = (0, 1, 2, 3, 4, 5)
FEW_PIX = (0, H * W - 1, 256, 4095, 3000)           # first and last pixel, the first key of the second select workgroup, ...
FEW_DEPTH = (2.5, 3.4, 4.6, 6.2, 8.3)                 # the steps grow with the depth: every rank gives another step by > 10 %
EXPECT_RANK = {1: 0, 2: 0, 3: 1, 4: 1, 5: 2}          # the lower median: lower of two, second of four, third of five
CASES = tuple(f"valid-{n}" for n in FEW) + ("valid-all-but-one", "valid-all", "tie-constant", "tie-two-levels", "batch", "non-finite",
                                           "scene", "degenerate", "partly_invalid")


def _rig(B, h, w, seed=4):
    import torch
    from wild_deep_mvs_amd import synthetic
    scene = synthetic.make_scene(B, 3, h, w, seed=seed)
    scene["t"] = scene["t"] * 8
    row = torch.tensor([0., 0., 0., 1.])
    ref_ex = torch.cat((torch.cat((scene["R"][:, 0], scene["t"][:, 0]), 2), row.view(1, 1, 4).expand(B, 1, 4)), 1)
    src_ex = torch.cat((torch.cat((scene["R"][:, 1:], scene["t"][:, 1:]), 3), row.view(1, 1, 1, 4).expand(B, 2, 1, 4)), 2)
    return scene, ref_ex, src_ex


def _few(n, gen=None):
    import torch
    d = torch.full((H * W,), -5.0)                    # depth -5 projects behind the source camera (and so does -5 + 1): invalid
    for k in range(n):
        d[FEW_PIX[k]] = FEW_DEPTH[k]
    return d.view(1, H, W)


def make_case(name):
    """-> dict of torch tensors: depth [B,h,w], ref_in [B,3,3], src_in [B,N,3,3], ref_ex [B,4,4], src_ex [B,N,4,4], dmin, dmax [B]"""
    import torch
    gen = torch.Generator().manual_seed(8)
    if name in ("scene", "degenerate", "partly_invalid"):        # the three cases of tests/test_gpu_cvp.py, 48 x 64
        B, h, w = (1 if name == "degenerate" else 2), 48, 64
        scene, ref_ex, src_ex = _rig(B, h, w)
        ref_ex[B - 1, :3, 3] *= 0.5
        src_ex[B - 1, :, :3, 3] *= 0.5
        depth = 2.5 + 3.0 * torch.rand(B, h, w, generator=gen)
        if name == "degenerate":
            src_ex = ref_ex.unsqueeze(1).repeat(1, 2, 1, 1)
        if name == "partly_invalid":
            src_ex[:, 0, 2, 3] -= 4.0
    else:
        B = 3 if name == "batch" else 1
        scene, ref_ex, src_ex = _rig(B, H, W)
        full = 2.5 + 3.0 * torch.rand(1, H, W, generator=gen)
        if name.startswith("valid-") and name[6:].isdigit():
            depth = _few(int(name[6:]))
        elif name == "valid-all-but-one":
            depth = full.clone()
            depth.view(-1)[1234] = -5.0
        elif name == "valid-all":
            depth = full
        elif name.startswith("tie-"):
            # identity rotations, equal intrinsics, a translation in the image plane (a purely horizontal one makes rows 1..2 singular)
            eye = torch.eye(4).view(1, 4, 4)
            ref_ex, src_ex = eye.clone(), eye.view(1, 1, 4, 4).repeat(1, 2, 1, 1)
            src_ex[:, :, 0, 3], src_ex[:, :, 1, 3] = 0.3, 0.5
            scene["K"] = scene["K"][:, :1].repeat(1, 3, 1, 1)
            depth = torch.full((1, H, W), 4.0)
            if name == "tie-two-levels":
                low = torch.randperm(H * W, generator=gen)[:int(0.4 * H * W)]
                depth = torch.full((H * W,), 5.0)
                depth[low] = 3.0
                depth = depth.view(1, H, W)
        elif name == "batch":
            depth = torch.cat((_few(0), _few(2), full))
            ref_ex[1, :3, 3] *= 0.5
            src_ex[1, :, :3, 3] *= 0.5
        elif name == "non-finite":
            depth = full.clone()
            idx = torch.randperm(H * W, generator=gen)[:10]
            depth.view(-1)[idx[:5]] = float("nan")
            depth.view(-1)[idx[5:]] = float("inf")
        else:
            raise KeyError(name)
    K = scene["K"]
    return {"depth": depth.contiguous(), "ref_in": K[:, 0].contiguous(), "src_in": K[:, 1:].contiguous(), "ref_ex": ref_ex.contiguous(),
            "src_ex": src_ex.contiguous(), "dmin": scene["depth_min"][:, 0].contiguous(), "dmax": scene["depth_max"][:, 0].contiguous()}


def inputs(case):
    """-> (depth float32 [B,h,w] array, cams float64 [B,39], fallback float32 [B]) of a case: what the kernel is given"""
    c = case if isinstance(case, dict) else make_case(case)
    cams = host_cams(c["ref_in"].numpy(), c["src_in"][:, 0].numpy(), c["ref_ex"].numpy(), c["src_ex"][:, 0].numpy())
    fallback = ((c["dmax"] - c["dmin"]) / 128).float().reshape(-1).numpy()
    return c["depth"].numpy(), cams, fallback
