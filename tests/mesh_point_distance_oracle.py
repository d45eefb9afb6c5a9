"""Restatements of smplpp_mesh_point_distance (the nearest cloud point of every posed vertex) for the tests.

`forward` is the exact rule in numpy float32, so the kernel's index and sqdist must match it bit for bit:
  - d = ((dx*dx + dy*dy) + dz*dz) with d = v - p, every operation rounded to fp32 on its own (numpy ufuncs never contract);
  - the smallest d wins, the lowest point index among equal ones;
  - a non-finite d (NaN, inf, overflow) is never chosen; a vertex with no eligible point gets (-1, 0).
It is chunked over K so that a large cloud never builds a [V, K] matrix.

`sqdist` is a float64 (or any dtype) torch restatement of the distance at a GIVEN index, so torch autograd through it is the
reference gradient in the vertices and the points; `closed_form` is the product the kernel computes:
grad_verts[v] = 2 g_v r_v, grad_points[k] = sum over v with index_v == k of -2 g_v r_v, r = v - p[index].
"""
import numpy as np
import torch

CHUNK = 1024


def forward_frame(v, p):
    """index [V] int64 and sqdist [V] float32 for one frame: v [V,3], p [K,3] float32."""
    v = np.ascontiguousarray(v, np.float32)
    p = np.ascontiguousarray(p, np.float32)
    V, K = len(v), len(p)
    best_d = np.full(V, np.inf, np.float32)
    best_k = np.full(V, -1, np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for k0 in range(0, K, CHUNK):
            q = p[k0:k0 + CHUNK]
            dx = v[:, None, 0] - q[None, :, 0]
            dy = v[:, None, 1] - q[None, :, 1]
            dz = v[:, None, 2] - q[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            d[~np.isfinite(d)] = np.inf
            j = np.argmin(d, 1)  # first occurrence: the lowest index among equal minima of the chunk
            dj = d[np.arange(V), j]
            take = dj < best_d  # strict: an earlier chunk keeps a tie
            best_d[take] = dj[take]
            best_k[take] = k0 + j[take]
    best_d[best_k < 0] = 0.0
    return best_k, best_d


def forward(verts, points):
    """index [n,V] int64, sqdist [n,V] float32 for verts [n,V,3] and points [n,K,3]."""
    out = [forward_frame(verts[f], points[f]) for f in range(len(verts))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def sqdist(verts, points, index):
    """|v - p[index]|^2 [n,V] in the dtype of verts (torch); 0 where index = -1."""
    index = torch.as_tensor(index, dtype=torch.int64, device=verts.device)
    valid = index >= 0
    p = points.gather(1, index.clamp(min=0)[..., None].expand(*index.shape, 3))
    r = torch.where(valid[..., None], verts - p, torch.zeros((), dtype=verts.dtype, device=verts.device))  # (masked before squaring: no NaN in the gradient)
    return (r * r).sum(-1)


def closed_form(verts, points, index, grad_sqdist):
    """(grad_verts [n,V,3], grad_points [n,K,3]) from the closed form (no autograd), in the dtype of verts."""
    with torch.no_grad():
        index = torch.as_tensor(index, dtype=torch.int64, device=verts.device)
        g = torch.as_tensor(grad_sqdist, dtype=verts.dtype, device=verts.device)
        valid = (index >= 0) & (g != 0)
        p = points.gather(1, index.clamp(min=0)[..., None].expand(*index.shape, 3))
        r = torch.where(valid[..., None], verts - p, torch.zeros((), dtype=verts.dtype, device=verts.device))
        gv = 2 * g[..., None] * r
        gp = torch.zeros_like(points)
        gp.scatter_add_(1, index.clamp(min=0)[..., None].expand(*index.shape, 3), -2 * g[..., None] * r)
        return gv, gp


def vjp(verts, points, index, grad_sqdist):
    """(grad_verts, grad_points) by torch autograd through `sqdist`, in the dtype of verts."""
    v = verts.detach().clone().requires_grad_(True)
    p = points.detach().clone().requires_grad_(True)
    d = sqdist(v, p, index)
    g = torch.as_tensor(grad_sqdist, dtype=d.dtype, device=d.device)
    gv, gp = torch.autograd.grad((d * g).sum(), (v, p), allow_unused=True)
    return gv, (gp if gp is not None else torch.zeros_like(p))
