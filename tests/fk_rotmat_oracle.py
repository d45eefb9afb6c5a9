"""The torch restatement of SMPL::launch (tests/fk_vjp_oracle.py) with the 24 rotation matrices as the leaf instead of the
axis-angles: fk_vjp_oracle.fk from the line after its Rodrigues call, the matrices used as given.  In float64 it is the oracle of
smplpp_fk_rotmat and (by autograd) of smplpp_fk_rotmat_vjp; in float32 it measures what plain fp32 gets wrong.  Also the float64
Rodrigues derivative that ties dL/dR to dL/dtheta, and the 6-D Gram-Schmidt restated in float64."""
import numpy as np
import torch

import fk_vjp_oracle as O

model_tensors = O.model_tensors
rodrigues = O.rodrigues


def fk(m, beta, trans, R, offsets=None):
    """beta [n,10], trans [n,3], R [n,24,3,3] -> dict(verts [n,V,3], joints [n,24,3], rest [n,V,3], xforms [n,24,4,4]).  offsets
    [V,3] or [n,V,3] (SMPL+D): added to the rest shape in front of the skinning; `rest` and the joints stay those of the body."""
    n = R.shape[0]
    dt = R.dtype
    eye = torch.eye(3, dtype=dt)
    c = (R[:, 1:] - eye).reshape(n, -1)  # [n,207]
    shaped = m["T"] + torch.einsum("vxk,nk->nvx", m["S"], beta)
    rest = shaped + torch.einsum("vxk,nk->nvx", m["P"], c)
    J = torch.einsum("jv,nvx->njx", m["Jreg"], shaped)
    A, g = [R[:, 0]], [J[:, 0]]
    for i in range(1, 24):
        p = int(m["parent"][i])
        A.append(A[p] @ R[:, i])
        g.append((A[p] @ (J[:, i] - J[:, p])[..., None])[..., 0] + g[p])
    A, g = torch.stack(A, 1), torch.stack(g, 1)
    t = g - (A @ J[..., None])[..., 0]
    top = torch.cat([A, t[..., None]], -1)
    bottom = torch.zeros(n, 24, 1, 4, dtype=dt)
    bottom[..., 3] = 1
    X = torch.cat([top, bottom], 2)
    M = torch.einsum("vj,njab->nvab", m["W"], X)
    skinned = rest if offsets is None else rest + offsets
    h = (M @ torch.cat([skinned, torch.ones(n, rest.shape[1], 1, dtype=dt)], -1)[..., None])[..., 0]
    verts = h[..., :3] / h[..., 3:4] + trans[:, None, :]
    return dict(verts=verts, joints=J, rest=rest, xforms=X)


def cast(m, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in m.items()}


def forward(m, beta, trans, R, dtype=torch.float64):
    """`fk` on numpy inputs in `dtype`, numpy float64 out."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    with torch.no_grad():
        out = fk(cast(m, dtype), t(beta), t(trans), t(R))
    return {k: v.numpy().astype(np.float64) for k, v in out.items()}


def vjp(m, beta, trans, R, grad_verts=None, grad_joints=None, dtype=torch.float64, offsets=None):
    """(dL/dbeta [n,10], dL/dtrans [n,3], dL/dR [n,24,3,3]) by autograd of `fk` in `dtype`; with `offsets` also dL/doffsets."""
    mm = cast(m, dtype)
    leaf = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype).clone().requires_grad_(True)
    b, t, r = leaf(beta), leaf(trans), leaf(R)
    leaves = (b, t, r) if offsets is None else (b, t, r, leaf(offsets))
    out = fk(mm, *leaves)
    loss = 0
    if grad_verts is not None:
        loss = loss + (out["verts"] * torch.as_tensor(np.asarray(grad_verts), dtype=dtype)).sum()
    if grad_joints is not None:
        loss = loss + (out["joints"] * torch.as_tensor(np.asarray(grad_joints), dtype=dtype)).sum()
    gs = torch.autograd.grad(loss, leaves, allow_unused=True)
    return tuple((torch.zeros_like(x) if g is None else g).detach().numpy().astype(np.float64) for g, x in zip(gs, leaves))


def rodrigues_np(theta):
    """float64 [..., 3] -> [..., 3, 3] by the reference's formula (eps 1e-8 per component)."""
    return rodrigues(torch.as_tensor(np.asarray(theta, np.float64))).numpy()


def contract_rodrigues(theta, grad_R):
    """dL/dtheta [..., 3] = sum_q dL/dR[q] dR[q]/dtheta in float64, by autograd of `rodrigues`."""
    th = torch.as_tensor(np.asarray(theta, np.float64)).clone().requires_grad_(True)
    (g,) = torch.autograd.grad((rodrigues(th) * torch.as_tensor(np.asarray(grad_R, np.float64))).sum(), (th,))
    return g.numpy()


def rot6d_to_rotmat(x):
    """The 6-D representation's Gram-Schmidt (columns a1 = x[..., 0::2], a2 = x[..., 1::2]) in the dtype of x."""
    m = x.reshape(*x.shape[:-1], 3, 2)
    a1, a2 = m[..., 0], m[..., 1]
    b1 = a1 / a1.norm(dim=-1, keepdim=True)
    u = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
    b2 = u / u.norm(dim=-1, keepdim=True)
    return torch.stack([b1, b2, torch.linalg.cross(b1, b2)], -1)
