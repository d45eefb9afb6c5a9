"""Oracles of the forward mode of FK (smplpp_fk_jvp / smplpp_fk_rotmat_jvp), in three parts:

1. `tangent` / `tangent_rotmat`: torch.func.jvp over the torch restatements of the forward (fk_vjp_oracle.fk, fk_rotmat_oracle.fk,
   skeleton_oracle.skeleton / chain) in a chosen dtype.  In float64 it is the oracle; in float32 it measures what a plain fp32
   forward mode of the same graph gets wrong.
2. `closed_form` / `closed_form_theta`: the rule include/smplpp_hip.h states, in numpy float64, without autograd.
3. `lm_fit`: the Levenberg-Marquardt loop on dense Jacobians the application tests run, over any (forward, jacobian) pair.

Outputs carry the tangent axis the ABI has: verts [n,T,V,3], joints [n,T,24,3] (the rest joints), world [n,T,24,3,4]."""
import numpy as np
import torch

import fk_rotmat_oracle as RO
import fk_vjp_oracle as O
import skeleton_oracle as SO

model_tensors = O.model_tensors
cast = RO.cast


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype)


def _per_frame(a, n, shared, tail, dtype):
    """A tangent array as [n,T,...] in `dtype` (shared: [T,...] repeated over the frames); None stays None."""
    if a is None:
        return None
    a = _t(a, dtype)
    if shared:
        a = a[None].expand((n,) + tuple(a.shape)).contiguous()
    assert tuple(a.shape[2:]) == tail and a.shape[0] == n, (a.shape, n, tail)
    return a


def _columns(x, T):
    """[n,...] -> [n*T,...]: every frame once per tangent (the frames of the restatements are independent)."""
    return x[:, None].expand((x.shape[0], T) + tuple(x.shape[1:])).reshape((-1,) + tuple(x.shape[1:])).contiguous()


def _run(f, primals, tangents, n, T):
    """One torch.func.jvp over the n*T columns; a tangent of None is zero.  numpy float64 [n,T,...] per output."""
    prim = tuple(_columns(x, T) for x in primals)
    tans = tuple(torch.zeros_like(x) if d is None else d.reshape(x.shape) for x, d in zip(prim, tangents))
    _, out = torch.func.jvp(f, prim, tans)
    return {k: v.reshape((n, T) + tuple(v.shape[1:])).numpy().astype(np.float64) for k, v in zip(("verts", "joints", "world"), out)}


def tangent(m, beta, theta, dbeta=None, dtheta=None, shared=False, dtype=torch.float64, rest=None):
    """dict(verts, joints, world) by torch.func.jvp of fk_vjp_oracle.fk and skeleton_oracle.skeleton in `dtype` (one call over the n*T
    columns).  `rest` [n,V,3]: fk's rest_value (the numbers the skinning reads; the derivative runs through the graph's own rest)."""
    mm = cast(m, dtype)
    b, th = _t(beta, dtype), _t(theta, dtype)
    n = th.shape[0]
    db, dth = _per_frame(dbeta, n, shared, (10,), dtype), _per_frame(dtheta, n, shared, (25, 3), dtype)
    T = (db if db is not None else dth).shape[1]
    rv = None if rest is None else _columns(_t(rest, dtype), T)

    def f(b_, th_):
        o, s = O.fk(mm, b_, th_, rv), SO.skeleton(mm, b_, th_)
        return o["verts"], o["joints"], s["world"]

    return _run(f, (b, th), (db, dth), n, T)


def tangent_rotmat(m, beta, trans, R, dbeta=None, dtrans=None, dR=None, shared=False, dtype=torch.float64, offsets=None):
    """The rotation-matrix entry: torch.func.jvp of fk_rotmat_oracle.fk and skeleton_oracle.chain.  offsets [n,V,3] or [V,3]: the
    SMPL+D displacement, a constant of the body."""
    mm = cast(m, dtype)
    r = _t(R, dtype)
    n = r.shape[0]
    b = torch.zeros(n, 10, dtype=dtype) if beta is None else _t(beta, dtype)
    tr = torch.zeros(n, 3, dtype=dtype) if trans is None else _t(trans, dtype)
    db, dtr = _per_frame(dbeta, n, shared, (10,), dtype), _per_frame(dtrans, n, shared, (3,), dtype)
    dr = _per_frame(dR, n, shared, (24, 3, 3), dtype)
    T = next(a for a in (db, dtr, dr) if a is not None).shape[1]
    off = _t(offsets, dtype)
    if off is not None and off.dim() == 3:
        off = _columns(off, T)

    def f(b_, t_, r_):
        o, s = RO.fk(mm, b_, t_, r_, off), SO.chain(mm, b_, t_, r_)
        return o["verts"], o["joints"], s["world"]

    return _run(f, (b, tr, r), (db, dtr, dr), n, T)


def rodrigues_tangent(theta, dtheta):
    """dR [...,3,3] = sum_m dtheta_m dRodrigues(theta)/dtheta_m in float64, by forward mode of the reference's formula."""
    th, d = _t(theta, torch.float64), _t(dtheta, torch.float64)
    return torch.func.jvp(O.rodrigues, (th,), (d,))[1].numpy()


def closed_form(m, beta, trans, R, dbeta=None, dtrans=None, dR=None, rest=None):
    """The rule of include/smplpp_hip.h in numpy float64 for ONE tangent per frame (dbeta [n,10], dtrans [n,3], dR [n,24,3,3]; None =
    zero): dict(verts [n,V,3], joints [n,24,3], world [n,24,3,4], rest [n,V,3]) of tangents.  `rest`: the rest shape the skinning
    reads (None: the body's own)."""
    f64 = lambda a: np.asarray(a, np.float64)
    R = f64(R)
    n = R.shape[0]
    zeros = lambda *s: np.zeros((n,) + s)
    beta = zeros(10) if beta is None else f64(beta)
    dbeta = zeros(10) if dbeta is None else f64(dbeta)
    dtrans = zeros(3) if dtrans is None else f64(dtrans)
    dR = zeros(24, 3, 3) if dR is None else f64(dR)
    Jreg, T, S, P, W = (m[k].double().numpy() for k in ("Jreg", "T", "S", "P", "W"))
    parent = [int(p) for p in m["parent"]]
    J0, JS = Jreg @ T, np.einsum("jv,vxk->jxk", Jreg, S)
    J = J0 + np.einsum("jxk,nk->njx", JS, beta)
    dJ = np.einsum("jxk,nk->njx", JS, dbeta)
    if rest is None:
        rest = T + np.einsum("vxk,nk->nvx", S, beta) + np.einsum("vxk,nk->nvx", P, (R[:, 1:] - np.eye(3)).reshape(n, -1))
    drest = np.einsum("vxk,nk->nvx", S, dbeta) + np.einsum("vxk,nk->nvx", P, dR[:, 1:].reshape(n, -1))
    A, g, dA, dg = zeros(24, 3, 3), zeros(24, 3), zeros(24, 3, 3), zeros(24, 3)
    A[:, 0], g[:, 0], dA[:, 0], dg[:, 0] = R[:, 0], J[:, 0], dR[:, 0], dJ[:, 0]
    mv = lambda M, v: np.einsum("nab,nb->na", M, v)
    for lv in SO.levels(parent)[1:]:
        for j in lv:
            p = parent[j]
            A[:, j] = A[:, p] @ R[:, j]
            g[:, j] = mv(A[:, p], J[:, j] - J[:, p]) + g[:, p]
            dA[:, j] = dA[:, p] @ R[:, j] + A[:, p] @ dR[:, j]
            dg[:, j] = mv(dA[:, p], J[:, j] - J[:, p]) + mv(A[:, p], dJ[:, j] - dJ[:, p]) + dg[:, p]
    dt = dg - np.einsum("njab,njb->nja", dA, J) - np.einsum("njab,njb->nja", A, dJ)
    wsum = W.sum(1)
    bl = lambda X: np.einsum("vj,nj...->nv...", W, X)
    dverts = (np.einsum("nvab,nvb->nva", bl(dA), f64(rest)) + bl(dt) + np.einsum("nvab,nvb->nva", bl(A), drest)) / wsum[None, :, None]
    dverts = dverts + dtrans[:, None, :]
    dworld = np.concatenate([dA, (dg + dtrans[:, None, :])[..., None]], -1)
    return dict(verts=dverts, joints=dJ, world=dworld, rest=drest)


def closed_form_theta(m, beta, theta, dbeta=None, dtheta=None, rest=None):
    """The axis-angle entry: `closed_form` at the float64 Rodrigues matrices with dR = `rodrigues_tangent`, dtrans = dtheta[:, 0]."""
    theta = np.asarray(theta, np.float64)
    dtheta = np.zeros_like(theta) if dtheta is None else np.asarray(dtheta, np.float64)
    return closed_form(m, beta, theta[:, 0], RO.rodrigues_np(theta[:, 1:]), dbeta, dtheta[:, 0], rodrigues_tangent(theta[:, 1:], dtheta[:, 1:]),
                       rest)


# ------------------------------------------------------------------------------------------------ Levenberg-Marquardt
LM_N, LM_ITERS, LM_LAMBDA0 = 2, 12, 1e-3


def lm_target():
    """theta* = 0.3 default_rng(5).standard_normal((2,25,3)) as float32; beta = 0."""
    return (0.3 * np.random.default_rng(5).standard_normal((LM_N, 25, 3))).astype(np.float32)


def lm_fit(forward, jacobian, dtype=np.float32):
    """Levenberg-Marquardt on dense Jacobians from theta = 0 towards forward(lm_target()): forward(theta [2,25,3]) -> verts [2,V,3],
    jacobian(theta) -> [2,75,V,3] (the tangent axis of SMPL.jacobian(wrt=("theta",))), both handed `dtype` arrays.  Per frame, with
    r = verts - verts*, J [3V,75], H = J^T J: step = solve(H + lambda diag(H) + 1e-9 I, -J^T r), lambda_0 = 1e-3; a step is kept when
    the frame's energy sum(r^2) falls, then lambda /= 3, else lambda *= 5; 12 iterations.  The normal equations are formed and solved
    in float64 from whatever the two callables return.  Returns (first, last) summed energy."""
    f64 = lambda a: np.asarray(a, np.float64)
    target = f64(forward(lm_target().astype(dtype)))
    theta = np.zeros((LM_N, 25, 3), np.float64)
    lam = np.full(LM_N, LM_LAMBDA0)
    energy = lambda v: ((f64(v) - target) ** 2).reshape(LM_N, -1).sum(1)
    e = energy(forward(theta.astype(dtype)))
    first = float(e.sum())
    for _ in range(LM_ITERS):
        r = (f64(forward(theta.astype(dtype))) - target).reshape(LM_N, -1)
        J = f64(jacobian(theta.astype(dtype))).reshape(LM_N, 75, -1)
        trial = theta.copy()
        for f in range(LM_N):
            H = J[f] @ J[f].T
            step = np.linalg.solve(H + lam[f] * np.diag(np.diag(H)) + 1e-9 * np.eye(75), -J[f] @ r[f])
            trial[f] += step.reshape(25, 3)
        et = energy(forward(trial.astype(dtype)))
        for f in range(LM_N):
            if et[f] < e[f]:
                theta[f], e[f], lam[f] = trial[f], et[f], lam[f] / 3
            else:
                lam[f] *= 5
    return first, float(e.sum())


def lm_passes(first, last, last64):
    return first / last >= 1e3 and last <= 2 * last64


def oracle_lm(m, dtype):
    """(forward, jacobian) of `lm_fit` from the torch restatement in `dtype`, beta = 0."""
    mm = cast(m, dtype)
    beta = torch.zeros(LM_N, 10, dtype=dtype)
    f = lambda th: O.fk(mm, beta, th)["verts"]
    basis = torch.eye(75, dtype=dtype).reshape(1, 75, 25, 3).expand(LM_N, 75, 25, 3).reshape(LM_N * 75, 25, 3).contiguous()
    fc = lambda th: O.fk(mm, torch.zeros(LM_N * 75, 10, dtype=dtype), th)["verts"]

    def forward(theta):
        with torch.no_grad():
            return f(torch.as_tensor(theta, dtype=dtype)).numpy()

    def jacobian(theta):
        th = _columns(torch.as_tensor(theta, dtype=dtype), 75)
        return torch.func.jvp(fc, (th,), (basis,))[1].reshape(LM_N, 75, -1, 3).numpy()

    return forward, jacobian
