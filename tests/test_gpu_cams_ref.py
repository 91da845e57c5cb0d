"""The camera-block kernels of csrc/cams.hip -- pscv_homog_cams, pscv_proj_cams, the warp blocks of pscv_cvp_cams -- against a float64
closed form per element.  The kernels compute in fp64 from fp32 inputs and round ONCE, so the bound is derived, not measured:

    |got - ref| <= 2^-24 U + C64 2^-53 cond(M) U

U is the sum of the absolute terms of the element (|K_s| |R_s| |R_r^T| |K_r^-1| for A; |b_s| + |rot| |b_r| for trans; ...), the first
term is the one fp32 rounding (half an ulp of a value no larger than U), the second the fp64 error of the chain: the 3x3 inverse of M
(K_r, or the reference projection's A_r) loses cond(M) = |M|_inf |M^-1|_inf units of 2^-53, and C64 = 64 covers that inverse (adjugate
and determinant: < 16 roundings) and the < 48 roundings of the up to four 3x3 products behind it.  Entries 12..17 of a PROJ block are
exactly 0.

For pscv_cvp_cams the fp32 steps in front of the fp64 part are part of the contract (cams.hip: cvp_level_k, cvp_projection): the level
intrinsics K * (1.0f / level_scale) and the projections K E[:3] with a product and two fused multiply-adds per entry.  They are
restated exactly (rational arithmetic, one rounding to fp32 per step)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS32, EPS64, C64 = 2.0 ** -24, 2.0 ** -53, 64.0
F = np.float64


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wild_deep_mvs_amd import _lib as L, ops, synthetic
    L.lib()
    return L, ops, synthetic


def cond(M):
    return float(np.abs(M).sum(1).max() * np.abs(np.linalg.inv(M)).sum(1).max())


def compare(tag, got, ref, U, kappa):
    got = np.asarray(got, dtype=F)
    bound = EPS32 * U + C64 * EPS64 * kappa * U
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"[parity] {tag}: worst |got - ref| / (2^-24 U + {C64:.0f} 2^-53 cond U) = {float(ratio.max()):.3f} (bound 1), "
          f"fp64 share of the bound {float(C64 * EPS64 * kappa / EPS32):.2e}", flush=True)
    assert float(ratio.max()) <= 1.0, f"{tag}: {float(ratio.max()):.3f} x the derived bound at {np.unravel_index(int(ratio.argmax()), ratio.shape)}"


# ---- HOMOG blocks -----------------------------------------------------------------------------------------------------------------------
def homog_ref(ref_cam, src_cam, scale):
    """one [2,4,4] pair -> A, Bm, U_A, U_Bm, cond(K_r): models/VisMVSNet/homography.py:23-74 after scale_camera (preproc.py:63-92)"""
    L_, S_ = np.asarray(ref_cam, dtype=F), np.asarray(src_cam, dtype=F)

    def parts(c):
        K = c[1, :3, :3].copy()
        K[0, 0] *= scale; K[1, 1] *= scale; K[0, 2] *= scale; K[1, 2] *= scale
        return K, c[0, :3, :3], c[0, :3, 3:4]
    Kl, Rl, tl = parts(L_)
    Ks, Rs, ts = parts(S_)
    M1 = Rl.T @ np.linalg.inv(Kl)
    aM1 = np.abs(Rl.T) @ np.abs(np.linalg.inv(Kl))
    KR, aKR = Ks @ Rs, np.abs(Ks) @ np.abs(Rs)
    crel = -Rs.T @ ts + Rl.T @ tl
    acrel = np.abs(Rs.T) @ np.abs(ts) + np.abs(Rl.T) @ np.abs(tl)
    T, aT = crel @ Rl[2:3, :], acrel @ np.abs(Rl[2:3, :])
    return KR @ M1, KR @ (T @ M1), aKR @ aM1, aKR @ (aT @ aM1), cond(Kl)


@pytest.mark.parametrize("scale", [1.0 / 8.0, 1.0 / 3.0])
def test_homog_cams_against_float64(env, scale):
    """B = 2, three sources, the last one EQUAL to the reference view: Bm exactly 0 there, A the identity to one rounding."""
    L, ops, synthetic = env
    B, V = 2, 4
    sc = synthetic.make_scene(B, V, 64, 80, seed=21)
    sc["t"] = sc["t"] * 6
    cam = torch.zeros(B, V, 2, 4, 4)
    cam[:, :, 0, :3, :3], cam[:, :, 0, :3, 3:4], cam[:, :, 0, 3, 3] = sc["R"], sc["t"], 1.0
    cam[:, :, 1, :3, :3] = sc["K"]
    cam[:, 3] = cam[:, 0]
    scale32 = float(np.float32(scale))                      # the ABI takes an fp32 scale: the reference gets the same value
    got = ops.homog_cams_device(cam[:, 0].cuda(), [cam[:, v].cuda() for v in range(1, V)], scale32).cpu().numpy()
    assert got.shape == (V - 1, B, L.CAM_FLOATS)
    for j in range(V - 1):
        for b in range(B):
            A, Bm, UA, UB, kappa = homog_ref(cam[b, 0].numpy(), cam[b, j + 1].numpy(), scale32)
            compare(f"homog_cams scale {scale:.3f} src {j} item {b} A", got[j, b, :9].reshape(3, 3), A, UA, kappa)
            compare(f"homog_cams scale {scale:.3f} src {j} item {b} Bm", got[j, b, 9:].reshape(3, 3), Bm, UB, kappa)
            if j == V - 2:
                assert np.all(got[j, b, 9:] == 0.0), "Bm of a source equal to the reference is exactly 0"
                assert np.all(np.abs(got[j, b, :9].reshape(3, 3) - np.eye(3)) <= EPS32 * UA * (1.0 + 1e-6)), "A is the identity to one rounding"


# ---- PROJ blocks ------------------------------------------------------------------------------------------------------------------------
def proj_ref(Pr, Ps):
    """[4,4] fp32-valued projections -> rot, trans, U_rot, U_trans, cond(A_r)"""
    Pr, Ps = np.asarray(Pr, dtype=F), np.asarray(Ps, dtype=F)
    Ai = np.linalg.inv(Pr[:3, :3])
    rot, Urot = Ps[:3, :3] @ Ai, np.abs(Ps[:3, :3]) @ np.abs(Ai)
    trans = Ps[:3, 3] - rot @ Pr[:3, 3]
    Utrans = np.abs(Ps[:3, 3]) + Urot @ np.abs(Pr[:3, 3])      # |b_s| + |rot| |b_r|, with the absolute terms of rot
    return rot, trans, Urot, Utrans, cond(Pr[:3, :3])


def check_proj_block(tag, blk, Pr, Ps):
    rot, trans, Urot, Utrans, kappa = proj_ref(Pr, Ps)
    compare(f"{tag} rot", blk[:9].reshape(3, 3), rot, Urot, kappa)
    compare(f"{tag} trans", blk[9:12], trans, Utrans, kappa)
    assert np.all(blk[12:] == 0.0), f"{tag}: entries 12..17 are exactly 0"


def f32(fr):
    """a rational, rounded once to fp32 (nearest, ties to even; normal range), as a Fraction"""
    if fr == 0:
        return Fraction(0)
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    q = Fraction(2) ** (e - 23)
    n = round(a / q)                                      # Fraction rounds half to even
    return (n * q) * (1 if fr > 0 else -1)


def cvp_projection(K, E, inv_s):
    """cams.hip cvp_level_k + cvp_projection: rows 0..2 of [[K_l E[:3]]] in fp32 -> float64 [3,4] (exact fp32 values)"""
    Kf = [[Fraction(float(K[r, c])) for c in range(3)] for r in range(3)]
    s = Fraction(float(inv_s))
    Kl = [[f32(Kf[r][c] * s) if r < 2 else Kf[r][c] for c in range(3)] for r in range(3)]
    Ef = [[Fraction(float(E[r, c])) for c in range(4)] for r in range(3)]
    P = np.zeros((4, 4))
    for r in range(3):
        for c in range(4):
            acc = f32(Kl[r][0] * Ef[0][c])
            acc = f32(Kl[r][1] * Ef[1][c] + acc)
            acc = f32(Kl[r][2] * Ef[2][c] + acc)
            P[r, c] = float(acc)
    P[3, 3] = 1.0
    return P


def _rig(synthetic):
    B, V = 2, 4
    sc = synthetic.make_scene(B, V, 96, 120, seed=11)
    sc["t"][1] *= 0.5
    row = torch.tensor([0., 0., 0., 1.]).view(1, 1, 1, 4).expand(B, V, 1, 4)
    E = torch.cat((torch.cat((sc["R"], sc["t"]), 3), row), 2).contiguous()          # [B,V,4,4]
    return B, V, sc["K"].contiguous(), E


@pytest.mark.parametrize("ref", [0, 1])
def test_cvp_cams_warp_blocks_against_float64(env, ref):
    """B = 2, three sources, level scales {1, 2, 3, 8} (1 / 3 is an inexact fp32 reciprocal), reference frame 0 and 1."""
    L, ops, synthetic = env
    B, V, K, E = _rig(synthetic)
    srcs = [v for v in range(V) if v != ref]
    scales = [1.0, 2.0, 3.0, 8.0]
    warp, _ = ops.cvp_cams(K[:, ref].cuda(), K[:, srcs].cuda(), E[:, ref].cuda(), E[:, srcs].cuda(), scales)
    warp = warp.cpu().numpy()
    assert warp.shape == (len(scales), V - 1, B, L.CAM_FLOATS)
    for l, s in enumerate(scales):
        inv_s = np.float32(1.0) / np.float32(s)
        for b in range(B):
            Pr = cvp_projection(K[b, ref].numpy(), E[b, ref].numpy(), inv_s)
            for j, v in enumerate(srcs):
                Ps = cvp_projection(K[b, v].numpy(), E[b, v].numpy(), inv_s)
                check_proj_block(f"cvp_cams ref {ref} level 1/{s:.0f} src {j} item {b}", warp[l, j, b], Pr, Ps)


@pytest.mark.parametrize("ref", [0, 1])
def test_proj_cams_device_against_float64(env, ref):
    """pscv_proj_cams on fp32 projections [B,V,4,4] (here the level-1/3 projections of the CVP rig), reference frame 0 and 1: sources in
    view order with the reference skipped."""
    L, ops, synthetic = env
    B, V, K, E = _rig(synthetic)
    inv_s = np.float32(1.0) / np.float32(3.0)
    P = np.stack([np.stack([cvp_projection(K[b, v].numpy(), E[b, v].numpy(), inv_s) for v in range(V)]) for b in range(B)])
    got = ops.proj_cams_device(torch.from_numpy(P.astype(np.float32)).cuda(), ref).cpu().numpy()
    assert got.shape == (V - 1, B, L.CAM_FLOATS)
    for j, v in enumerate([v for v in range(V) if v != ref]):
        for b in range(B):
            check_proj_block(f"proj_cams_device ref {ref} src {j} item {b}", got[j, b], P[b, ref], P[b, v])
