"""The rules of the scene term (smplpp_volume_sample, smplpp_scene_term, smplpp_scene_term_vjp; include/smplpp_hip.h) restated in numpy,
operation by operation, with the dtype as a parameter: in float32 it is the bit reference of the library, in float64 the reference of the
CPU tests.  The frame sum is sum_rules.sum1024.  sample_t / energy_t are the DEFINITION in torch (any dtype), for autograd.
plane / sphere / random_field fill grids with analytic fields."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sum_rules import sum1024  # noqa: E402

f32 = np.float32


def volume(values, origin, spacing, world_to_volume=None, dtype=f32):
    """values [Gz,Gy,Gx]; world_to_volume [3,4] (or [12]) row-major [R|t], None: the identity."""
    xf = None if world_to_volume is None else np.asarray(world_to_volume, dtype).reshape(3, 4)
    return dict(v=np.asarray(values, dtype), o=np.asarray(origin, dtype).reshape(3), h=np.asarray(spacing, dtype).reshape(3), xf=xf)


def as_dtype(V, dtype):
    return volume(V["v"], V["o"], V["h"], V["xf"], dtype)


def node_positions(G, origin, spacing):
    """[Gz,Gy,Gx,3] float64: the volume coordinates of the nodes, G = (Gx, Gy, Gz)."""
    o, h = np.asarray(origin, np.float64), np.asarray(spacing, np.float64)
    k, j, i = np.meshgrid(np.arange(G[2]), np.arange(G[1]), np.arange(G[0]), indexing="ij")
    return np.stack([o[0] + i * h[0], o[1] + j * h[1], o[2] + k * h[2]], -1)


def plane(G, origin, spacing, normal, c):
    """n . p - c at the nodes (n is normalised here); returns (values float64, n)."""
    nrm = np.asarray(normal, np.float64)
    nrm = nrm / np.linalg.norm(nrm)
    return node_positions(G, origin, spacing) @ nrm - c, nrm


def sphere(G, origin, spacing, centre, r):
    return np.linalg.norm(node_positions(G, origin, spacing) - np.asarray(centre, np.float64), axis=-1) - r


def random_field(G, seed):
    return np.random.default_rng(seed).normal(0, 0.2, (G[2], G[1], G[0]))


def _cell(V, P):
    """(inside, (ix, iy, iz), (fx, fy, fz)) of points P [..., 3] in the dtype of V: the transform, the grid coordinate, the cell."""
    dt = V["v"].dtype.type
    P = np.asarray(P, dt)
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    if V["xf"] is not None:
        R, t = V["xf"][:, :3], V["xf"][:, 3]
        q = [((R[a, 0] * x + R[a, 1] * y) + R[a, 2] * z) + t[a] for a in range(3)]
    else:
        q = [x, y, z]
    Gz, Gy, Gx = V["v"].shape
    inside, idx, frac = np.ones(x.shape, bool), [], []
    for a, G in enumerate((Gx, Gy, Gz)):
        g = (q[a] - V["o"][a]) / V["h"][a]
        ok = (g >= 0) & (g <= dt(G - 1))  # (a NaN fails both, an infinity one)
        inside &= ok
        g = np.where(ok, g, dt(0))
        i = np.minimum(np.floor(g).astype(np.int64), G - 2)
        idx.append(i), frac.append(g - i.astype(dt))
    return inside, idx, frac


def sample(V, P):
    """(value [...], gradient [..., 3] to the world point, valid [...] uint8) of points P [..., 3]."""
    dt = V["v"].dtype.type
    with np.errstate(all="ignore"):
        inside, (ix, iy, iz), (fx, fy, fz) = _cell(V, P)
        v = lambda dx, dy, dz: V["v"][iz + dz, iy + dy, ix + dx]  # noqa: E731
        d = {(y, z): v(1, y, z) - v(0, y, z) for y in (0, 1) for z in (0, 1)}
        c = {(y, z): v(0, y, z) + fx * d[y, z] for y in (0, 1) for z in (0, 1)}
        e0, e1 = c[1, 0] - c[0, 0], c[1, 1] - c[0, 1]
        c0, c1 = c[0, 0] + fy * e0, c[0, 1] + fy * e1
        ez = c1 - c0
        s = c0 + fz * ez
        x0, x1 = d[0, 0] + fy * (d[1, 0] - d[0, 0]), d[0, 1] + fy * (d[1, 1] - d[0, 1])
        gv = [(x0 + fz * (x1 - x0)) / V["h"][0], (e0 + fz * (e1 - e0)) / V["h"][1], ez / V["h"][2]]
        if V["xf"] is not None:
            R = V["xf"][:, :3]
            gv = [(R[0, a] * gv[0] + R[1, a] * gv[1]) + R[2, a] * gv[2] for a in range(3)]
        valid = inside & np.isfinite(s)
        value = np.where(valid, s, dt(0)).astype(dt)
        grad = np.where(valid[..., None], np.stack(gv, -1), dt(0)).astype(dt)
    return value, grad, valid.astype(np.uint8)


def _weights(w_pen, w_con, K, dt):
    return (np.ones(K, dt) if w_pen is None else np.asarray(w_pen, dt)), (np.zeros(K, dt) if w_con is None else np.asarray(w_con, dt))


def term(V, P, w_pen=None, w_con=None, rho=0.0):
    """P [n,K,3] -> (energy [n], point_energy [n,K], value [n,K], valid [n,K] uint8)."""
    dt = V["v"].dtype.type
    n, K = P.shape[:2]
    wp, wc = _weights(w_pen, w_con, K, dt)
    value, _, valid = sample(V, P)
    with np.errstate(all="ignore"):
        s = value
        q = s * s
        e_pen = np.where(s < 0, wp[None] * q, dt(0))
        if rho == 0:
            e_con = wc[None] * q
        else:
            p2 = dt(rho) * dt(rho)
            e_con = wc[None] * ((p2 * q) / (p2 + q))
        live = ((wp != 0) | (wc != 0))[None] & (valid != 0)
        pe = np.where(live, e_pen + e_con, dt(0)).astype(dt)
        energy = sum1024(pe, axis=1)
    return energy, pe, value, valid


def term_vjp(V, P, w_pen, w_con, rho, grad_energy, grad_point_energy, grad_value, out, accumulate):
    """out [n,K,3] written (or added into) by smplpp_scene_term_vjp."""
    dt = V["v"].dtype.type
    n, K = P.shape[:2]
    wp, wc = _weights(w_pen, w_con, K, dt)
    s, grad, valid = sample(V, P)
    with np.errstate(all="ignore"):
        ge = np.zeros(n, dt) if grad_energy is None else np.asarray(grad_energy, dt)
        gpe = np.zeros((n, K), dt) if grad_point_energy is None else np.asarray(grad_point_energy, dt)
        g = ge[:, None] + gpe
        pen = np.where(s < 0, (dt(2) * wp)[None] * s, dt(0))
        if rho == 0:
            con = (dt(2) * wc)[None] * s
        else:
            p2 = dt(rho) * dt(rho)
            d = p2 / (p2 + s * s)
            con = ((dt(2) * wc)[None] * (d * d)) * s
        live = ((wp != 0) | (wc != 0))[None]
        t = np.where(live, g * (pen + con), dt(0))
        kk = (np.zeros((n, K), dt) if grad_value is None else np.asarray(grad_value, dt)) + t
        reads = live | (grad_value is not None)
        el = np.where(((valid != 0) & reads)[..., None], kk[..., None] * grad, dt(0)).astype(dt)
        out[...] = out + el if accumulate else el
    return out


# ---------------------------------------------------------------------------------------------------- the definition, in torch
def sample_t(V, P):
    """Trilinear interpolation of V at the torch points P [..., 3] (inside points only), differentiable in P at a fixed cell."""
    import torch

    dt = P.dtype
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dt)  # noqa: E731
    q = P
    if V["xf"] is not None:
        q = P @ T(V["xf"][:, :3]).T + T(V["xf"][:, 3])
    g = (q - T(V["o"])) / T(V["h"])
    Gz, Gy, Gx = V["v"].shape
    vals = T(V["v"])
    idx = [torch.clamp(torch.floor(g[..., a].detach()).long(), 0, G - 2) for a, G in enumerate((Gx, Gy, Gz))]
    f = [g[..., a] - idx[a].to(dt) for a in range(3)]
    out = 0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (f[0] if dx else 1 - f[0]) * (f[1] if dy else 1 - f[1]) * (f[2] if dz else 1 - f[2])
                out = out + w * vals[idx[2] + dz, idx[1] + dy, idx[0] + dx]
    return out


def energy_t(V, P, w_pen=None, w_con=None, rho=0.0):
    """The definition of the term in torch: point energies [n,K] of P [n,K,3] (inside points only)."""
    import torch

    K = P.shape[1]
    wp, wc = _weights(w_pen, w_con, K, np.float64)
    wp, wc = torch.as_tensor(wp, dtype=P.dtype), torch.as_tensor(wc, dtype=P.dtype)
    s = sample_t(V, P)
    q = s * s
    con = q if rho == 0 else (rho * rho * q) / (rho * rho + q)
    return wp * torch.where(s < 0, q, torch.zeros_like(q)) + wc * con


def cell_margin(V, P):
    """[...] float64: the distance of each point's fractional grid coordinates from the nearest cell face, in cells (float64 arithmetic)."""
    V64 = as_dtype(V, np.float64)
    _, _, frac = _cell(V64, np.asarray(P, np.float64))
    return np.min([np.minimum(f, 1 - f) for f in frac], 0)


# ---------------------------------------------------------------------------------------------------- the two chains on the synthetic model
GRADIENT_SEED = 0
MARGIN, S_MIN = 0.05, 1e-3  # a vertex closer than MARGIN (in cells) to a cell face, or with |s| < S_MIN, is left out of the comparison


def _fk64(model, beta, theta):
    import torch

    import fk_vjp_oracle as FK

    return FK.fk(FK.model_tensors(model, torch.float64), torch.as_tensor(beta, dtype=torch.float64), torch.as_tensor(theta, dtype=torch.float64))["verts"]


def gradient_case(model):
    """theta, beta -> FK -> the term on a sphere field -> sum, n = 2: dict(beta [2,10], theta [2,25,3], V (float32 volume), w_pen, w_con
    [K], rho, keep [2,K] bool).  keep comes from the float64 run alone.  A condition that leaves out every vertex within 0.05 cells of a
    face leaves out 1 - 0.9^3 = 27 % of a body that spans many cells, whatever the seed; and a weight is per vertex, so a vertex stays
    only when it is clear in both frames.  So the 24^3 grid is coarse (cells of 0.95 x 2.1 x 1.3 m) and placed with the centre of the
    bodies' bounding box on a node plane in x and in the middle of a cell in y and z: the bodies lie in two cells, and one face plane
    cuts them."""
    rng = np.random.default_rng(GRADIENT_SEED)
    beta = rng.normal(0, 1, (2, 10)).astype(f32)
    theta = np.zeros((2, 25, 3), f32)
    theta[:, 1:] = rng.normal(0, 0.2, (2, 24, 3))
    theta[:, 0] = rng.normal(0, 0.05, (2, 3))
    v = _fk64(model, beta, theta).numpy()
    K = v.shape[1]
    centre = 0.5 * (v.min((0, 1)) + v.max((0, 1)))
    G, h = (24, 24, 24), np.array([0.95, 2.1, 1.3])
    origin = centre - np.array([12.0, 11.5, 11.5]) * h
    V = volume(sphere(G, origin, h, centre + np.array([1.5, -1.0, 2.0]), 2.7), origin, h)  # (its surface passes through the bodies)
    w_pen, w_con = rng.uniform(0.5, 2.0, K).astype(f32), rng.uniform(0.0, 1.0, K).astype(f32)
    w_con[::3] = 0
    s, _, valid = sample(as_dtype(V, np.float64), v)
    keep = (cell_margin(V, v) >= MARGIN) & (np.abs(s) >= S_MIN) & (valid != 0)
    return dict(beta=beta, theta=theta, V=V, w_pen=w_pen, w_con=w_con, rho=0.05, keep=keep, verts64=v)


FIT_STEPS, FIT_LR, FIT_RHO, FIT_DEPTH, FIT_SHARE = 60, 0.005, 0.05, 0.05, 0.05


def fit_case(model):
    """The fit of test_scene_gpu: n = 2 bodies, each translated so that its lowest vertex touches the plane n . p = 0, a 32^3 grid around
    them, then both moved FIT_DEPTH through the plane.  Weights: 1 on the FIT_SHARE of the vertices that come lowest along n above their
    body's lowest vertex (the lower of the two frames counts), for penetration and contact alike."""
    rng = np.random.default_rng(7)
    beta = rng.normal(0, 1, (2, 10)).astype(f32)
    theta = np.zeros((2, 25, 3), f32)
    theta[:, 1:] = rng.normal(0, 0.2, (2, 24, 3))
    v = _fk64(model, beta, theta).numpy()
    nrm = np.array([0.1, 1.0, 0.05])
    nrm = nrm / np.linalg.norm(nrm)
    height = v @ nrm
    stand = -height.min(1)[:, None] * nrm[None]  # [2,3]: the translation that puts each body on the plane
    v = v + stand[:, None]
    lo, hi = v.min((0, 1)) - 0.25, v.max((0, 1)) + 0.25
    G, h = (32, 32, 32), (hi - lo) / 31
    values, _ = plane(G, lo, h, nrm, 0.0)
    K = v.shape[1]
    w = np.zeros(K, f32)
    w[np.argsort((height - height.min(1, keepdims=True)).min(0))[:int(FIT_SHARE * K)]] = 1
    start = theta.copy()
    start[:, 0] = stand - FIT_DEPTH * nrm
    return dict(beta=beta, theta=start, V=volume(values, lo, h), w=w, normal=nrm)


def fit_float64(model, case):
    """FIT_STEPS Adam steps on trans and the rotations in float64 on the CPU: the largest penetration depth (metres) before every step
    and after the last, [FIT_STEPS + 1]."""
    import torch

    import fk_vjp_oracle as FK

    m = FK.model_tensors(model, torch.float64)
    V64 = as_dtype(case["V"], np.float64)
    beta = torch.tensor(case["beta"], dtype=torch.float64)
    trans = torch.tensor(case["theta"][:, :1], dtype=torch.float64, requires_grad=True)
    rot = torch.tensor(case["theta"][:, 1:], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([trans, rot], lr=FIT_LR)
    depth = []

    def evaluate():
        verts = FK.fk(m, beta, torch.cat([trans, rot], 1))["verts"]
        depth.append(float(-sample(V64, verts.detach().numpy())[0].min()))
        return energy_t(V64, verts, case["w"], case["w"], FIT_RHO).sum()

    for _ in range(FIT_STEPS):
        opt.zero_grad()
        evaluate().backward()
        opt.step()
    with torch.no_grad():
        evaluate()
    return np.array(depth)
