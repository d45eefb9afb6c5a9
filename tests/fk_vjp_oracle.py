"""A short torch restatement of SMPL::launch (src/SMPL.cpp:671-737) for the backward-pass tests: blend shapes, joint regression,
the chain with the reference's Rodrigues (||theta + 1e-8||, src/BlendShape.cpp:803-844), relative transforms and linear blend
skinning with the homogeneous divide and the root translation.  In float64 it is the oracle of smplpp_fk_vjp (autograd); in
float32 it measures what a plain fp32 autograd of the same graph gets wrong."""
import numpy as np
import torch


def model_tensors(model, dtype=torch.float64):
    t = lambda k: torch.as_tensor(np.asarray(model[k], np.float64), dtype=dtype)
    parent = np.asarray(model["kinematic_tree"], np.int64)[0].copy()
    parent[0] = -1
    return dict(T=t("vertices_template"), S=t("shape_blend_shapes"), P=t("pose_blend_shapes"), Jreg=t("joint_regressor"),
                W=t("weights"), parent=parent)


def rodrigues(th):
    """[..., 3] -> [..., 3, 3]: R = I + sin(a) K + (1 - cos a) K.K, K = skew(theta / a), a = ||theta + 1e-8||."""
    a = torch.sqrt(((th + 1e-8) ** 2).sum(-1, keepdim=True))
    k = th / a
    z = torch.zeros_like(k[..., 0])
    K = torch.stack([z, -k[..., 2], k[..., 1], k[..., 2], z, -k[..., 0], -k[..., 1], k[..., 0], z], -1).reshape(*k.shape[:-1], 3, 3)
    eye = torch.eye(3, dtype=th.dtype).expand_as(K)
    s, c = torch.sin(a)[..., None], torch.cos(a)[..., None]
    return eye + s * K + (1 - c) * (K @ K)


def fk(m, beta, theta, rest_value=None):
    """beta [n,10], theta [n,25,3] -> dict(verts [n,V,3], joints [n,24,3], rest [n,V,3], xforms [n,24,4,4]).  rest_value [n,V,3]:
    the skinning reads these numbers as its rest shape, while the derivative still runs through the graph's own rest (what
    smplpp_fk_vjp does with the `rest` it is handed or recomputes)."""
    n = beta.shape[0]
    R = rodrigues(theta[:, 1:, :])  # [n,24,3,3]
    eye = torch.eye(3, dtype=beta.dtype)
    c = (R[:, 1:] - eye).reshape(n, -1)  # [n,207]
    shaped = m["T"] + torch.einsum("vxk,nk->nvx", m["S"], beta)
    rest = shaped + torch.einsum("vxk,nk->nvx", m["P"], c)
    if rest_value is not None:
        rest = rest + (rest_value - rest).detach()
    J = torch.einsum("jv,nvx->njx", m["Jreg"], shaped)
    A, g = [R[:, 0]], [J[:, 0]]
    for i in range(1, 24):
        p = int(m["parent"][i])
        A.append(A[p] @ R[:, i])
        g.append((A[p] @ (J[:, i] - J[:, p])[..., None])[..., 0] + g[p])
    A, g = torch.stack(A, 1), torch.stack(g, 1)  # [n,24,3,3], [n,24,3]
    t = g - (A @ J[..., None])[..., 0]
    top = torch.cat([A, t[..., None]], -1)  # [n,24,3,4]
    bottom = torch.zeros(n, 24, 1, 4, dtype=beta.dtype)
    bottom[..., 3] = 1
    X = torch.cat([top, bottom], 2)  # [n,24,4,4]
    M = torch.einsum("vj,njab->nvab", m["W"], X)
    h = (M @ torch.cat([rest, torch.ones(n, rest.shape[1], 1, dtype=beta.dtype)], -1)[..., None])[..., 0]
    verts = h[..., :3] / h[..., 3:4] + theta[:, 0:1, :]
    return dict(verts=verts, joints=J, rest=rest, xforms=X)


def vjp(m, beta, theta, grad_verts=None, grad_joints=None, dtype=torch.float64, rest=None):
    """(dL/dbeta [n,10], dL/dtheta [n,25,3]) by autograd of `fk` in `dtype`; `rest`: fk's rest_value."""
    mm = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in m.items()}
    b = torch.as_tensor(np.asarray(beta), dtype=dtype).clone().requires_grad_(True)
    th = torch.as_tensor(np.asarray(theta), dtype=dtype).clone().requires_grad_(True)
    out = fk(mm, b, th, None if rest is None else torch.as_tensor(np.asarray(rest), dtype=dtype))
    loss = 0
    if grad_verts is not None:
        loss = loss + (out["verts"] * torch.as_tensor(np.asarray(grad_verts), dtype=dtype)).sum()
    if grad_joints is not None:
        loss = loss + (out["joints"] * torch.as_tensor(np.asarray(grad_joints), dtype=dtype)).sum()
    gb, gt = torch.autograd.grad(loss, (b, th), allow_unused=True)
    gb = torch.zeros_like(b) if gb is None else gb
    gt = torch.zeros_like(th) if gt is None else gt
    return gb.detach().numpy().astype(np.float64), gt.detach().numpy().astype(np.float64)
