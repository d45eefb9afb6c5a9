"""The rules of the image term (smplpp_image_sample, smplpp_image_term, smplpp_image_term_vjp; include/smplpp_hip.h) restated in numpy,
operation by operation, with the dtype as a parameter: in float32 it is the bit reference of the library, in float64 the reference of the
CPU tests.  The image's dtype decides.  The frame sum is sum_rules.sum1024; grad_image is a plain loop in ascending point index.
sample_t / energy_t are the DEFINITION in torch (any dtype), for autograd in uv and in the image.  blobs / heatmaps make smooth images."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sum_rules import sum1024  # noqa: E402

f32 = np.float32


def _cell(I, uv, channel):
    """(inside [n,K], i, j, fx, fy [n,K], b [n], ch [K] or None) of uv [n,K,2] on the image I [B,H,W,C], in the dtype of I."""
    dt = I.dtype.type
    uv = np.asarray(uv, dt)
    n = uv.shape[0]
    B, H, W, C = I.shape
    assert B in (1, n)
    inside, idx, frac = np.ones(uv.shape[:2], bool), [], []
    for a, G in ((0, W), (1, H)):
        g = uv[..., a] - dt(0.5)
        ok = (g >= 0) & (g <= dt(G - 1))  # (a NaN fails both, an infinity one)
        inside &= ok
        g = np.where(ok, g, dt(0))
        i = np.minimum(np.floor(g).astype(np.int64), G - 2)
        idx.append(i), frac.append(g - i.astype(dt))
    ch = None
    if channel is not None:
        ch = np.asarray(channel, np.int64)
        okc = (ch >= 0) & (ch < C)
        inside &= okc[None]
        ch = np.where(okc, ch, 0)
    b = np.arange(n) if B == n and n > 1 else np.zeros(n, np.int64)
    return inside, idx[0], idx[1], frac[0], frac[1], b, ch


def _sample(I, uv, channel):
    """The cell and, per sampled channel, s, ds/du, ds/dv [n,K,Cs] before the valid rule is applied."""
    inside, i, j, fx, fy, b, ch = _cell(I, uv, channel)

    def v(x, y):  # the pixel (j + y, i + x)
        t = I[b[:, None], j + y, i + x]
        return t if ch is None else np.take_along_axis(t, np.broadcast_to(ch[None, :, None], t.shape[:2] + (1,)), 2)

    FX, FY = fx[..., None], fy[..., None]
    d0, d1 = v(1, 0) - v(0, 0), v(1, 1) - v(0, 1)
    c0, c1 = v(0, 0) + FX * d0, v(0, 1) + FX * d1
    e = c1 - c0
    s = c0 + FY * e
    du = d0 + FY * (d1 - d0)
    valid = inside & np.isfinite(s).all(-1)
    return dict(s=s, du=du, dv=e, valid=valid, i=i, j=j, fx=fx, fy=fy, b=b, ch=ch)


def sample(I, uv, channel=None):
    """(value [n,K,Cs], gradient [n,K,Cs,2], valid [n,K] uint8) of uv [n,K,2] on I [B,H,W,C]."""
    dt = I.dtype.type
    with np.errstate(all="ignore"):
        r = _sample(I, uv, channel)
        ok = r["valid"][..., None]
        value = np.where(ok, r["s"], dt(0)).astype(dt)
        grad = np.where(ok[..., None], np.stack([r["du"], r["dv"]], -1), dt(0)).astype(dt)
    return value, grad, r["valid"].astype(np.uint8)


def _rows(a, n, shape, fill, dt):
    """target / weight: None reads as `fill`; a leading 1 is shared by the n frames."""
    if a is None:
        return np.full((n,) + shape, fill, dt)
    a = np.asarray(a, dt)
    assert a.shape[1:] == shape and a.shape[0] in (1, n), (a.shape, shape)
    return np.broadcast_to(a, (n,) + shape)


def _residual(I, uv, channel, target, weight):
    dt = I.dtype.type
    r = _sample(I, uv, channel)
    n, K, Cs = r["s"].shape
    w, t = _rows(weight, n, (K,), 1, dt), _rows(target, n, (K, Cs), 0, dt)
    res = r["s"] - t
    q = np.zeros((n, K), dt)
    for c in range(Cs):
        q = q + res[..., c] * res[..., c]
    return r, w, res, q


def term(I, uv, channel=None, target=None, weight=None, rho=0.0):
    """(energy [n], point_energy [n,K], value [n,K,Cs], valid [n,K] uint8)."""
    dt = I.dtype.type
    with np.errstate(all="ignore"):
        r, w, _, q = _residual(I, uv, channel, target, weight)
        if rho == 0:
            pe = w * q
        else:
            p2 = dt(rho) * dt(rho)
            pe = w * ((p2 * q) / (p2 + q))
        pe = np.where((w != 0) & r["valid"], pe, dt(0)).astype(dt)
        energy = sum1024(pe, axis=1)
        value = np.where(r["valid"][..., None], r["s"], dt(0)).astype(dt)
    return energy, pe, value, r["valid"].astype(np.uint8)


def term_vjp(I, uv, channel, target, weight, rho, grad_energy, grad_point_energy, grad_value, grad_uv=None, grad_image=None, accumulate=0):
    """grad_uv [n,K,2] and grad_image [B,H,W,C] written (or added into) by smplpp_image_term_vjp; either may be None.  Returns both."""
    dt = I.dtype.type
    with np.errstate(all="ignore"):
        r, w, res, q = _residual(I, uv, channel, target, weight)
        n, K, Cs = res.shape
        ge = np.zeros(n, dt) if grad_energy is None else np.asarray(grad_energy, dt)
        gpe = np.zeros((n, K), dt) if grad_point_energy is None else np.asarray(grad_point_energy, dt)
        g = ge[:, None] + gpe
        if rho == 0:
            m = w
        else:
            p2 = dt(rho) * dt(rho)
            d = p2 / (p2 + q)
            m = w * (d * d)
        live = w != 0
        coef = (dt(2) * g) * m
        gv = np.zeros((n, K, Cs), dt) if grad_value is None else np.asarray(grad_value, dt)
        gamma = gv + np.where(live[..., None], coef[..., None] * res, dt(0))
        reads = r["valid"] & (live | (grad_value is not None))
        if grad_uv is not None:
            su, sv = np.zeros((n, K), dt), np.zeros((n, K), dt)
            for c in range(Cs):
                su = su + gamma[..., c] * r["du"][..., c]
                sv = sv + gamma[..., c] * r["dv"][..., c]
            el = np.where(reads[..., None], np.stack([su, sv], -1), dt(0)).astype(dt)
            grad_uv[...] = grad_uv + el if accumulate else el
        if grad_image is not None:
            acc = np.zeros(I.shape, dt)
            ax, ay = dt(1) - r["fx"], dt(1) - r["fy"]
            taps = np.stack([ax * ay, r["fx"] * ay, ax * r["fy"], r["fx"] * r["fy"]], -1)  # [n,K,4]: the pixels (j, i), (j, i+1), (j+1, i), (j+1, i+1)
            share = taps[..., None] * gamma[:, :, None, :]                                  # [n,K,4,Cs]: every product, rounded once
            I_, J_, B_ = r["i"].tolist(), r["j"].tolist(), r["b"].tolist()
            CH = None if r["ch"] is None else r["ch"].tolist()
            for f in range(n):
                for k in range(K):  # ascending flat point index f K + k
                    if not reads[f, k]:
                        continue
                    cs = slice(None) if CH is None else slice(CH[k], CH[k] + 1)
                    for t in range(4):
                        px = acc[B_[f], J_[f][k] + (t >> 1), I_[f][k] + (t & 1), cs]  # (a view: the sum is written in place)
                        px += share[f, k, t]
            grad_image[...] = grad_image + acc if accumulate else acc
    return grad_uv, grad_image


# ---------------------------------------------------------------------------------------------------- the definition, in torch
def sample_t(I, uv, channel=None):
    """Bilinear interpolation of the torch image I [B,H,W,C] at the torch points uv [n,K,2] (inside points only), as the sum of the four
    taps times their weights: differentiable in uv at a fixed cell, and in I.  [n,K,Cs]."""
    import torch

    dt = uv.dtype
    n = uv.shape[0]
    B, H, W, C = I.shape
    g = uv - 0.5
    i = torch.clamp(torch.floor(g[..., 0].detach()).long(), 0, W - 2)
    j = torch.clamp(torch.floor(g[..., 1].detach()).long(), 0, H - 2)
    fx, fy = (g[..., 0] - i.to(dt))[..., None], (g[..., 1] - j.to(dt))[..., None]
    b = (torch.arange(n) if B == n and n > 1 else torch.zeros(n, dtype=torch.long))[:, None]
    out = 0
    for y in (0, 1):
        for x in (0, 1):
            t = I[b, j + y, i + x]
            if channel is not None:
                ch = torch.as_tensor(np.asarray(channel, np.int64))
                t = torch.gather(t, 2, ch[None, :, None].expand(n, -1, 1))
            out = out + (fx if x else 1 - fx) * (fy if y else 1 - fy) * t
    return out


def energy_t(I, uv, channel=None, target=None, weight=None, rho=0.0):
    """The definition of the term in torch: point energies [n,K] (inside points only).  target and weight: arrays or tensors."""
    import torch

    s = sample_t(I, uv, channel)
    T = lambda a: a.to(uv.dtype) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, np.float64), dtype=uv.dtype)  # noqa: E731
    r = s if target is None else s - T(target)
    q = (r * r).sum(-1)
    e = q if rho == 0 else (rho * rho * q) / (rho * rho + q)
    return e if weight is None else T(weight) * e


def cell_margin(uv):
    """[...] float64: the distance of gx and gy from the nearest cell edge, in pixels (float64 arithmetic)."""
    g = np.asarray(uv, np.float64) - 0.5
    f = g - np.floor(g)
    return np.minimum(f, 1 - f).min(-1)


# ---------------------------------------------------------------------------------------------------- images
def blobs(H, W, centres, sigma, amplitude=None):
    """[H,W,len(centres)] float64: channel c is a Gaussian of width sigma (pixels) at the image point centres[c] = (u, v), sampled at the
    pixel centres (i + 0.5, j + 0.5)."""
    centres = np.asarray(centres, np.float64).reshape(-1, 2)
    amplitude = np.ones(len(centres)) if amplitude is None else np.asarray(amplitude, np.float64)
    v, u = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    d2 = (u[..., None] - centres[:, 0]) ** 2 + (v[..., None] - centres[:, 1]) ** 2
    return amplitude * np.exp(-d2 / (2.0 * sigma * sigma))


def random_image(B, H, W, C, seed):
    return np.random.default_rng(seed).normal(0, 0.5, (B, H, W, C))


# ---------------------------------------------------------------------------------------------------- the two chains on the synthetic model
NEAR = 0.05
SIZE = 96                      # both chains use 96 x 96 images
GRADIENT_SEED, MARGIN = 3, 0.02  # a point within MARGIN pixels of a cell edge (float64) gets weight 0


def _fk64(model, beta, theta):
    import torch

    import fk_vjp_oracle as FK

    return FK.fk(FK.model_tensors(model, torch.float64), torch.as_tensor(beta, dtype=torch.float64), torch.as_tensor(theta, dtype=torch.float64))


def _cameras(n, rng, turn=0.1):
    """n cameras 3 m in front of the body, y down, each turned a little, with the body (about 1.2 m of extent) inside 96 x 96 pixels."""
    cam = np.empty((n, 16), f32)
    for f in range(n):
        a = rng.normal(0, turn)
        c, s = np.cos(a), np.sin(a)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([1.0, -1.0, -1.0])
        cam[f] = np.concatenate([R.reshape(9), [0.02 * f, -0.25, 3.0], [150.0, 145.0, 48.0 + f, 40.0 - f]])
    return cam


def regressor(model):
    """The 53-row landmark regressor of the keypoint tests, and its dense form [53, V + 24]."""
    import keypoints_oracle as KP

    reg = KP.regressor_53(model)
    return reg, KP.dense(reg, model["vertices_template"].shape[0] + 24)


def landmarks64(model, dense, beta, theta):
    """[n,53,3] float64 torch landmarks of (beta, theta)."""
    import torch

    import keypoints_oracle as KP

    out = _fk64(model, beta, theta)
    return KP.landmarks_t(torch.tensor(dense), out["verts"], out["joints"])


def gradient_case(model):
    """theta, beta, camera -> FK -> landmarks -> projection -> the image term -> sum, n = 2: a per-frame image of three Gaussian blobs
    per channel pair on 96 x 96, C = 3, per-frame targets and weights, rho = 0.05.  keep [2,53] bool comes from the float64 run alone: the
    points that are inside the image and at least MARGIN pixels from a cell edge."""
    import torch

    import keypoints_oracle as KP

    rng = np.random.default_rng(GRADIENT_SEED)
    n = 2
    beta = rng.normal(0, 1, (n, 10)).astype(f32)
    theta = np.zeros((n, 25, 3), f32)
    theta[:, 1:] = rng.normal(0, 0.2, (n, 24, 3))
    cam = _cameras(n, rng)
    reg, dense = regressor(model)
    with torch.no_grad():
        uv, ok = KP.project_t(landmarks64(model, dense, beta, theta), torch.tensor(cam, dtype=torch.float64), NEAR)
    uv, ok = uv.numpy(), ok.numpy()
    K = uv.shape[1]
    image = np.stack([sum(blobs(SIZE, SIZE, rng.uniform(16, 80, (3, 2)), rng.uniform(6, 14), rng.uniform(0.5, 1.5, 3)) for _ in range(3)) for _ in range(n)])
    g = uv - 0.5
    inside = ok & (g >= 0).all(-1) & (g[..., 0] <= SIZE - 1) & (g[..., 1] <= SIZE - 1)
    keep = inside & (cell_margin(uv) >= MARGIN)
    target = rng.normal(0.5, 0.3, (n, K, 3)).astype(f32)
    weight = rng.uniform(0.5, 2.0, (n, K)).astype(f32)
    return dict(beta=beta, theta=theta, camera=cam, reg=reg, dense=dense, image=image.astype(f32), target=target, weight=weight, rho=0.05, keep=keep,
                inside=inside)


FIT_STEPS, FIT_LR, FIT_SIGMA = 80, 0.01, 4.0


def joint_rows(model):
    """The fit's 24 "joints": the rows of the model's own joint_regressor applied to the POSED vertices, as a CSR regressor (ascending
    vertex), with the vertices they read and the model restricted to those (the same numbers as on the whole body, a tenth of the work)."""
    import keypoints_oracle as KP

    J = np.asarray(model["joint_regressor"], f32)
    reg = KP.csr([[(int(c), J[j, c]) for c in np.nonzero(J[j])[0]] for j in range(24)])
    used = np.unique(reg[1])
    sub = {k: model[k][used] for k in ("vertices_template", "shape_blend_shapes", "pose_blend_shapes", "weights")}
    sub["joint_regressor"], sub["kinematic_tree"] = model["joint_regressor"][:, used], model["kinematic_tree"]
    return reg, sub, J[:, used].astype(np.float64)


def _joints64(m, A, beta, theta):
    import torch

    import fk_vjp_oracle as FK

    return torch.einsum("jv,nvx->njx", A, FK.fk(m, beta, theta)["verts"])


def fit_case(model):
    """The fit of test_image_gpu: n = 2 bodies; 24 joint heatmaps per frame (Gaussians of sigma = 4 px at the true projections of
    joint_rows' points, 96 x 96), read through channel = 0..23.  The start moves trans and the rotations so that every joint starts
    within about 1.5 sigma of its heatmap's peak."""
    import torch

    import fk_vjp_oracle as FK
    import keypoints_oracle as KP

    rng = np.random.default_rng(11)
    n = 2
    beta = np.zeros((n, 10), f32)
    theta_true = np.zeros((n, 25, 3), f32)
    theta_true[:, 1:] = rng.normal(0, 0.15, (n, 24, 3))
    cam = _cameras(n, rng, turn=0.0)
    reg, sub, A = joint_rows(model)
    m = FK.model_tensors(sub, torch.float64)
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731

    def project(theta):
        with torch.no_grad():
            uv, ok = KP.project_t(_joints64(m, t64(A), t64(beta), t64(theta)), t64(cam), NEAR)
        assert bool(ok.all())
        return uv.numpy()

    uv_true = project(theta_true)
    heat = np.stack([blobs(SIZE, SIZE, uv_true[f], FIT_SIGMA) for f in range(n)]).astype(f32)
    start = theta_true.copy()
    start[:, 0] += np.array([0.015, -0.01, 0.0], f32)
    start[:, 1:] += rng.normal(0, 0.03, (n, 24, 3)).astype(f32)
    return dict(beta=beta, theta=start, camera=cam, heat=heat, uv_true=uv_true, uv_start=project(start), channel=np.arange(24), reg=reg, sub=sub, A=A)


def fit_float64(case):
    """FIT_STEPS Adam steps on trans and the rotations in float64 on the CPU with the term's definition (target 1, weight = valid): the
    mean reprojection error in pixels before every step and after the last, [FIT_STEPS + 1]."""
    import torch

    import fk_vjp_oracle as FK
    import keypoints_oracle as KP

    m = FK.model_tensors(case["sub"], torch.float64)
    A = torch.tensor(case["A"])
    beta = torch.tensor(case["beta"], dtype=torch.float64)
    cam = torch.tensor(case["camera"], dtype=torch.float64)
    heat = torch.tensor(case["heat"], dtype=torch.float64)
    I64 = case["heat"].astype(np.float64)
    trans = torch.tensor(case["theta"][:, :1], dtype=torch.float64, requires_grad=True)
    rot = torch.tensor(case["theta"][:, 1:], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([trans, rot], lr=FIT_LR)
    target = np.ones((1, 24, 1))
    errors = []

    def evaluate():
        uv, _ = KP.project_t(_joints64(m, A, beta, torch.cat([trans, rot], 1)), cam, NEAR)
        errors.append(float(np.linalg.norm(uv.detach().numpy() - case["uv_true"], axis=-1).mean()))
        valid = sample(I64, uv.detach().numpy(), case["channel"])[2]
        safe = torch.where(torch.tensor(valid[..., None] != 0), uv, torch.full_like(uv, 1.0))  # (a point that is not valid has weight 0)
        return energy_t(heat, safe, case["channel"], target, valid.astype(np.float64), 0.0).sum()

    for _ in range(FIT_STEPS):
        opt.zero_grad()
        evaluate().backward()
        opt.step()
    with torch.no_grad():
        evaluate()
    return np.array(errors)
