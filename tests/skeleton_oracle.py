"""The skeleton of the torch restatement of SMPL::launch (tests/fk_vjp_oracle.py, tests/fk_rotmat_oracle.py): joint regression and
the kinematic chain alone, with the world orientations A, the chain positions g, posed = g + trans and the rest joints J as outputs.
In float64 it is the oracle of smplpp_skeleton / smplpp_skeleton_rotmat and, by autograd, of their vector-Jacobian products; in
float32 it measures what plain fp32 gets wrong.  `closed_form` is a second float64 implementation of the backward: the recurrence
include/smplpp_hip.h states, in numpy, without autograd."""
import numpy as np
import torch

import fk_rotmat_oracle as RO
import fk_vjp_oracle as O

model_tensors = O.model_tensors
rodrigues = O.rodrigues
contract_rodrigues = RO.contract_rodrigues
cast = RO.cast


def chain(m, beta, trans, R):
    """beta [n,10], trans [n,3], R [n,24,3,3] (any matrices, used as given) -> dict(A [n,24,3,3], g [n,24,3], posed [n,24,3],
    J [n,24,3], world [n,24,3,4] = [A | posed]).  The lines of fk_rotmat_oracle.fk, up to the relative transforms."""
    shaped = m["T"] + torch.einsum("vxk,nk->nvx", m["S"], beta)
    J = torch.einsum("jv,nvx->njx", m["Jreg"], shaped)
    A, g = [R[:, 0]], [J[:, 0]]
    for i in range(1, 24):
        p = int(m["parent"][i])
        A.append(A[p] @ R[:, i])
        g.append((A[p] @ (J[:, i] - J[:, p])[..., None])[..., 0] + g[p])
    A, g = torch.stack(A, 1), torch.stack(g, 1)
    posed = g + trans[:, None, :]
    return dict(A=A, g=g, posed=posed, J=J, world=torch.cat([A, posed[..., None]], -1))


def skeleton(m, beta, theta):
    """The axis-angle entry: theta [n,25,3], row 0 the translation."""
    return chain(m, beta, theta[:, 0], rodrigues(theta[:, 1:]))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def forward(m, beta, theta, dtype=torch.float64):
    """`skeleton` on numpy inputs in `dtype`, numpy float64 out."""
    with torch.no_grad():
        out = skeleton(cast(m, dtype), _t(beta, dtype), _t(theta, dtype))
    return {k: v.numpy().astype(np.float64) for k, v in out.items()}


def forward_rotmat(m, beta, trans, R, dtype=torch.float64):
    with torch.no_grad():
        out = chain(cast(m, dtype), _t(beta, dtype), _t(trans, dtype), _t(R, dtype))
    return {k: v.numpy().astype(np.float64) for k, v in out.items()}


def _loss(out, gw, gp, gj, dtype):
    loss = 0
    for key, g in (("world", gw), ("posed", gp), ("J", gj)):
        if g is not None:
            loss = loss + (out[key] * _t(g, dtype)).sum()
    return loss


def _grads(loss, leaves):
    gs = torch.autograd.grad(loss, leaves, allow_unused=True)
    return tuple((torch.zeros_like(x) if g is None else g).detach().numpy().astype(np.float64) for g, x in zip(gs, leaves))


def vjp(m, beta, theta, grad_world=None, grad_posed=None, grad_joints=None, dtype=torch.float64):
    """(dL/dbeta [n,10], dL/dtheta [n,25,3]) by autograd of `skeleton` in `dtype`, L = <world, gw> + <posed, gp> + <J, gj>."""
    leaves = tuple(_t(a, dtype).clone().requires_grad_(True) for a in (beta, theta))
    return _grads(_loss(skeleton(cast(m, dtype), *leaves), grad_world, grad_posed, grad_joints, dtype), leaves)


def vjp_rotmat(m, beta, trans, R, grad_world=None, grad_posed=None, grad_joints=None, dtype=torch.float64):
    """(dL/dbeta [n,10], dL/dtrans [n,3], dL/dR [n,24,3,3]) by autograd of `chain` in `dtype`."""
    leaves = tuple(_t(a, dtype).clone().requires_grad_(True) for a in (beta, trans, R))
    return _grads(_loss(chain(cast(m, dtype), *leaves), grad_world, grad_posed, grad_joints, dtype), leaves)


def levels(parent):
    """The joints by depth, ascending inside a level (model_tables.h, joint_levels / chain_tables)."""
    depth = np.zeros(24, np.int64)
    for i in range(1, 24):
        depth[i] = depth[int(parent[i])] + 1
    return [[i for i in range(24) if depth[i] == L] for L in range(int(depth.max()) + 1)]


def closed_form(m, beta, trans, R, grad_world=None, grad_posed=None, grad_joints=None):
    """(dL/dbeta, dL/dtrans, dL/dR) in float64 numpy by the recurrence of include/smplpp_hip.h: seeds, the levels from the deepest to
    level 1, the parent gathering its children in ascending joint order, the root, then the folded regressor."""
    f64 = lambda a: np.asarray(a, np.float64)
    beta, trans, R = f64(beta), f64(trans), f64(R)
    n = R.shape[0]
    zeros = lambda *s: np.zeros((n,) + s)
    gw = zeros(24, 3, 4) if grad_world is None else f64(grad_world)
    gp = zeros(24, 3) if grad_posed is None else f64(grad_posed)
    gj = zeros(24, 3) if grad_joints is None else f64(grad_joints)
    Jreg, T, S = (m[k].double().numpy() for k in ("Jreg", "T", "S"))
    parent = [int(p) for p in m["parent"]]
    J0, JS = Jreg @ T, np.einsum("jv,vxk->jxk", Jreg, S)
    J = J0 + np.einsum("jxk,nk->njx", JS, beta)
    A, g = np.zeros((n, 24, 3, 3)), np.zeros((n, 24, 3))
    A[:, 0], g[:, 0] = R[:, 0], J[:, 0]
    for i in range(1, 24):
        p = parent[i]
        A[:, i] = A[:, p] @ R[:, i]
        g[:, i] = np.einsum("nab,nb->na", A[:, p], J[:, i] - J[:, p]) + g[:, p]
    dA, dg, dJ = gw[..., :3].copy(), gw[..., 3] + gp, gj.copy()
    dtrans = dg.sum(1)
    dR, cA, cJ = zeros(24, 3, 3), zeros(24, 3, 3), zeros(24, 3)
    lv = levels(parent)
    for L in range(len(lv) - 1, 0, -1):
        for j in lv[L]:
            p = parent[j]
            ApT = A[:, p].transpose(0, 2, 1)
            dR[:, j] = ApT @ dA[:, j]
            cA[:, j] = dA[:, j] @ R[:, j].transpose(0, 2, 1) + dg[:, j, :, None] * (J[:, j] - J[:, p])[:, None, :]
            cJ[:, j] = np.einsum("nab,nb->na", ApT, dg[:, j])
            dJ[:, j] += cJ[:, j]
        for p in lv[L - 1]:
            for i in lv[L]:
                if parent[i] == p:
                    dA[:, p] += cA[:, i]
                    dg[:, p] += dg[:, i]
                    dJ[:, p] -= cJ[:, i]
    dR[:, 0] = dA[:, 0]
    dJ[:, 0] += dg[:, 0]
    dbeta = np.einsum("jxk,njx->nk", JS, dJ)
    return dbeta, dtrans, dR


def closed_form_theta(m, beta, theta, grad_world=None, grad_posed=None, grad_joints=None):
    """(dL/dbeta, dL/dtheta [n,25,3]) of the axis-angle entry: `closed_form` at the float64 Rodrigues matrices, dL/dR contracted
    with the Rodrigues derivative; row 0 is dL/dtrans."""
    theta = np.asarray(theta, np.float64)
    R = RO.rodrigues_np(theta[:, 1:])
    db, dt, dR = closed_form(m, beta, theta[:, 0], R, grad_world, grad_posed, grad_joints)
    return db, np.concatenate([dt[:, None, :], contract_rodrigues(theta[:, 1:], dR)], 1)
