"""Oracles of the bound points (smplpp_skin_points, smplpp_unskin_points and their vector-Jacobian products).

`forward` and `backward` restate rules 1 to 4 of include/smplpp_hip.h operation by operation in numpy (no FMA: numpy rounds every
product and sum on its own), in the dtype asked for: float32 is what the kernels must reproduce bit for bit, float64 the same closed
forms without rounding to speak of.  `definition` and `definition_torch` are what they are measured against: the blend as matrices,
einsum for skinning and a linear solve for its inverse, and torch autograd for the gradients (float64 is the yardstick, float32 what a
plain evaluation of the definition gets wrong)."""
import numpy as np
import torch

import sum_rules

TILE = 32       # SMPLPP_VERTEX_OFFSETS_TILE
MIN_DET = 1e-4  # SMPLPP_UNSKIN_MIN_DET
NJ = 24
f32 = np.float32


def omega_of(W, faces, face=None, bary=None, weights=None, dtype=f32):
    """(omega [B,K,24], ok [B,K]) of a binding: the weights as given, or by the face rule
    (bary0 W[v0][j] + bary1 W[v1][j]) + bary2 W[v2][j] with W the model's weights (every non-zero one is kept).  ok is False where
    the binding alone makes the point dead: a face id outside [0, F), a bary or a weight that is not finite."""
    if weights is not None:
        om = np.asarray(weights, dtype)
        om = om[None] if om.ndim == 2 else om
        return om, np.isfinite(om).all(-1)
    face, b = np.asarray(face, np.int64), np.asarray(bary, dtype)
    face, b = (face[None] if face.ndim == 1 else face), (b[None] if b.ndim == 2 else b)
    W, faces = np.asarray(W, dtype), np.asarray(faces, np.int64)
    inside = (face >= 0) & (face < len(faces))
    tri = faces[np.where(inside, face, 0)]  # [B,K,3]
    with np.errstate(invalid="ignore", over="ignore"):
        om = (b[..., 0:1] * W[tri[..., 0]] + b[..., 1:2] * W[tri[..., 1]]) + b[..., 2:3] * W[tri[..., 2]]
    return om, inside & np.isfinite(b).all(-1)


def relative_translations(world, joints):
    """c [n,24,3]: c_j[a] = p_j[a] - ((A_j[a][0] J_j[0] + A_j[a][1] J_j[1]) + A_j[a][2] J_j[2]), in the arrays' dtype."""
    A, p, J = world[..., :3], world[..., 3], joints[:, :, None, :]
    return p - ((A[..., 0] * J[..., 0] + A[..., 1] * J[..., 1]) + A[..., 2] * J[..., 2])


def forward(world, joints, points, omega, ok, unskin=False, dtype=f32):
    """Rules 1 and 2.  world [n,24,3,4], joints [n,24,3], points [P,K,3], omega [B,K,24], ok [B,K] (P, B in {1, n}).  Returns a dict:
    out [n,K,3], blend [n,K,3,4], valid [n,K] uint8, and what the backward needs (s, M, t, c, x, C, det, live)."""
    world, joints, x = np.asarray(world, dtype), np.asarray(joints, dtype), np.asarray(points, dtype)
    x = x[None] if x.ndim == 2 else x
    n, K = world.shape[0], x.shape[1]
    A, c = world[..., :3], relative_translations(world, joints)
    x = np.broadcast_to(x, (n, K, 3))
    omega, ok = np.broadcast_to(omega, (n, K, NJ)), np.broadcast_to(ok, (n, K))
    s, M, t = np.zeros((n, K), dtype), np.zeros((n, K, 3, 3), dtype), np.zeros((n, K, 3), dtype)
    with np.errstate(all="ignore"):
        for j in range(NJ):
            w = omega[..., j]
            on = w != 0
            if not on.any():
                continue
            s = np.where(on, s + w, s)
            M = np.where(on[..., None, None], M + w[..., None, None] * A[:, None, j], M)
            t = np.where(on[..., None], t + w[..., None] * c[:, None, j], t)
        live = ok & np.isfinite(x).all(-1) & (s > 0)
        C = det = None
        if not unskin:
            h = ((M[..., 0] * x[..., None, 0] + M[..., 1] * x[..., None, 1]) + M[..., 2] * x[..., None, 2]) + t
            out = h / s[..., None]
        else:
            q = s[..., None] * x - t
            C = np.empty_like(M)
            for a in range(3):
                for b in range(3):
                    a1, a2, b1, b2 = (a + 1) % 3, (a + 2) % 3, (b + 1) % 3, (b + 2) % 3
                    C[..., a, b] = M[..., a1, b1] * M[..., a2, b2] - M[..., a1, b2] * M[..., a2, b1]
            det = (M[..., 0, 0] * C[..., 0, 0] + M[..., 0, 1] * C[..., 0, 1]) + M[..., 0, 2] * C[..., 0, 2]
            live = live & (np.abs(det) > ((dtype(MIN_DET) * s) * s) * s)
            out = ((C[..., 0, :] * q[..., 0:1] + C[..., 1, :] * q[..., 1:2]) + C[..., 2, :] * q[..., 2:3]) / det[..., None]
        blend = np.concatenate([M / s[..., None, None], (t / s[..., None])[..., None]], -1)
    zero = dtype(0)
    return dict(out=np.where(live[..., None], out, zero), blend=np.where(live[..., None, None], blend, zero), valid=live.astype(np.uint8),
                s=s, M=M, t=t, c=c, x=x, C=C, det=det, live=live, omega=omega)


def tree_sum(t):
    """[n,...] -> [...]: tiles of TILE consecutive frames, each summed in ascending frame from its first term; the tile sums added in
    ascending tile from the first (the rule of smplpp_vertex_offsets_vjp)."""
    total = None
    for f0 in range(0, t.shape[0], TILE):
        s = t[f0].copy()
        for f in range(f0 + 1, min(f0 + TILE, t.shape[0])):
            s = s + t[f]
        total = s if total is None else total + s
    return total


def backward(world, joints, points, omega, ok, grad_out, unskin=False, dtype=f32, want_weights=False):
    """Rules 3 and 4: a dict of points [P,K,3], world [n,24,3,4], joints [n,24,3] and, with want_weights, weights [B,K,24]; P and B
    are those of `points` and `omega` (1: the frames' sum by `tree_sum`).  "forward" holds the recomputed forward."""
    fw = forward(world, joints, points, omega, ok, unskin, dtype)
    world, joints, g = np.asarray(world, dtype), np.asarray(joints, dtype), np.asarray(grad_out, dtype)
    n, K = g.shape[0], g.shape[1]
    P = 1 if np.ndim(points) == 2 else np.shape(points)[0]
    B = omega.shape[0]
    A, c, s, M, live, om = world[..., :3], fw["c"], fw["s"], fw["M"], fw["live"], fw["omega"]
    zero = dtype(0)
    with np.errstate(all="ignore"):
        if not unskin:
            gt = g / s[..., None]
            u = gt
            gp = (M[..., 0, :] * gt[..., 0:1] + M[..., 1, :] * gt[..., 1:2]) + M[..., 2, :] * gt[..., 2:3]
            xr = fw["x"]
        else:
            C, det = fw["C"], fw["det"]
            u = ((C[..., 0] * g[..., None, 0] + C[..., 1] * g[..., None, 1]) + C[..., 2] * g[..., None, 2]) / det[..., None]
            gt = -u
            gp = s[..., None] * u
            xr = fw["out"]
        gp = np.where(live[..., None], gp, zero)
        res = dict(forward=fw, points=tree_sum(gp)[None] if P == 1 and n > 1 else gp)
        # the sums over the points, per (frame, joint): a point that is dead or has no weight on the joint adds +0
        dc, dR = np.zeros((n, NJ, 3), dtype), np.zeros((n, NJ, 3, 3), dtype)
        for f in range(n):
            inc = live[f][:, None] & (om[f] != 0)                               # [K,24]
            wg = np.where(inc[..., None], om[f][..., None] * gt[f][:, None, :], zero)  # [K,24,3]
            wgx = np.where(inc[..., None, None], wg[..., None] * xr[f][:, None, None, :], zero)  # [K,24,3,3]
            dc[f] = sum_rules.sum1024(wg, axis=0)
            dR[f] = sum_rules.sum1024(wgx, axis=0)
        J = joints
        gw = np.empty((n, NJ, 3, 4), dtype)
        gw[..., :3] = dR - dc[..., None] * J[:, :, None, :]
        gw[..., 3] = dc
        res["world"] = gw
        res["joints"] = -((A[..., 0, :] * dc[..., 0:1] + A[..., 1, :] * dc[..., 1:2]) + A[..., 2, :] * dc[..., 2:3])
        if want_weights:
            # r_j = A_j xr + c_j for every joint: [n,K,24,3]
            r = ((A[:, None, :, :, 0] * xr[:, :, None, None, 0] + A[:, None, :, :, 1] * xr[:, :, None, None, 1])
                 + A[:, None, :, :, 2] * xr[:, :, None, None, 2]) + c[:, None]
            d = (fw["x"][:, :, None, :] - r) if unskin else (r - fw["out"][:, :, None, :])
            gwt = (u[:, :, None, 0] * d[..., 0] + u[:, :, None, 1] * d[..., 1]) + u[:, :, None, 2] * d[..., 2]
            gwt = np.where(live[..., None], gwt, zero)
            res["weights"] = tree_sum(gwt)[None] if B == 1 and n > 1 else gwt
    return res


# ------------------------------------------------------------------------------------------------ the definitions
def transforms_torch(world, joints, omega):
    """T [n,K,3,4]: the normalised blend of the relative transforms [A_j | p_j - A_j J_j] (torch tensors of one dtype; omega [B,K,24])."""
    A = world[..., :3]
    c = world[..., 3] - torch.einsum("njab,njb->nja", A, joints)
    G = torch.cat([A, c[..., None]], -1)
    w = omega / omega.sum(-1, keepdim=True)
    return torch.einsum("nkj,njab->nkab", w.expand(world.shape[0], -1, -1), G)


def definition_torch(world, joints, points, omega, unskin=False):
    """skin: T [x; 1]; unskin: the solution x of T [x; 1] = y.  Differentiable in all four."""
    T = transforms_torch(world, joints, omega)
    p = points.expand(world.shape[0], -1, -1) if points.dim() == 3 else points.expand(world.shape[0], *points.shape)
    if not unskin:
        return (T[..., :3] @ p[..., None])[..., 0] + T[..., 3]
    return torch.linalg.solve(T[..., :3], (p - T[..., 3])[..., None])[..., 0]


def definition(world, joints, points, omega, unskin=False):
    """The same in numpy float64: einsum for skinning, np.linalg.solve for its inverse.  Returns (out [n,K,3], T [n,K,3,4], det of
    the normalised blend [n,K])."""
    world, joints, x, om = (np.asarray(a, np.float64) for a in (world, joints, points, omega))
    n = world.shape[0]
    A = world[..., :3]
    G = np.concatenate([A, (world[..., 3] - np.einsum("njab,njb->nja", A, joints))[..., None]], -1)
    w = np.broadcast_to(om / om.sum(-1, keepdims=True), (n,) + om.shape[1:])
    T = np.einsum("nkj,njab->nkab", w, G)
    x = np.broadcast_to(x if x.ndim == 3 else x[None], (n, om.shape[1], 3))
    det = np.linalg.det(T[..., :3])
    if not unskin:
        return np.einsum("nkab,nkb->nka", T[..., :3], x) + T[..., 3], T, det
    return np.linalg.solve(T[..., :3], (x - T[..., 3])[..., None])[..., 0], T, det


def definition_vjp(world, joints, points, omega, grad_out, unskin=False, dtype=torch.float64):
    """dict(world, joints, points, weights): dL/d(each) of L = <definition, grad_out> by autograd in `dtype`, shaped like the inputs,
    as float64 numpy."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dtype)
    leaves = [t(a).clone().requires_grad_(True) for a in (world, joints, points, omega)]
    (definition_torch(*leaves, unskin=unskin) * t(grad_out)).sum().backward()
    return {k: v.grad.double().numpy() for k, v in zip(("world", "joints", "points", "weights"), leaves)}


def collapsed_pair():
    """(world [1,24,3,4], joints [1,24,3], weights [1,24]): every joint the identity but joint 1, a rotation by pi about z, and a point
    bound half and half to joints 0 and 1: M = diag(0, 0, 1), det 0."""
    world = np.zeros((1, NJ, 3, 4), f32)
    world[:, :, :, :3] = np.eye(3, dtype=f32)
    world[0, 1, :, :3] = np.diag([-1.0, -1.0, 1.0]).astype(f32)
    w = np.zeros((1, NJ), f32)
    w[0, 0] = w[0, 1] = 0.5
    return world, np.zeros((1, NJ, 3), f32), w
