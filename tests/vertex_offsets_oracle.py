"""Oracles of the SMPL+D layer (smplpp_vertex_offsets, smplpp_vertex_offsets_vjp, smplpp_mesh_laplacian).

float32 restatements of the three rules of include/smplpp_hip.h, operation by operation, in numpy (no FMA: numpy rounds every
product and sum on its own); and the definitions they are measured against: LBS(rest + D, G') + root in torch (float64 is the
yardstick, float32 what a plain evaluation of the definition gets wrong), its autograd, and the graph Laplacian."""
import numpy as np
import torch

TILE = 32  # SMPLPP_VERTEX_OFFSETS_TILE
f32 = np.float32


def smooth_field(template, scale=0.015):
    """A smooth displacement field [V,3] of about `scale` metres on the template's vertices."""
    t = np.asarray(template, np.float64)
    d = np.stack([np.sin(4.0 * t[:, 1] + 0.3), np.cos(3.0 * t[:, 0] - 0.2), np.sin(5.0 * t[:, 0] + 2.0 * t[:, 1])], 1)
    return (scale * d).astype(np.float32)


def w_sum(W):
    """The model's wSum: sum_j W[v,j] in ascending j, fp32."""
    W = np.asarray(W, f32)
    s = np.zeros(W.shape[0], f32)
    for j in range(W.shape[1]):
        s = s + W[:, j]
    return s


def blend_rotations(W, xforms):
    """M [n,V,3,3]: over the joints with a non-zero weight in ascending j, from +0, M = M + w * R' (fp32)."""
    W, R = np.asarray(W, f32), np.asarray(xforms, f32)[:, :, :3, :3]
    M = np.zeros((R.shape[0], W.shape[0], 3, 3), f32)
    for j in range(W.shape[1]):
        w = W[:, j]
        live = w != 0
        if live.any():
            M[:, live] = M[:, live] + w[live][None, :, None, None] * R[:, j][:, None]
    return M


def forward(W, verts, xforms, offsets, rest=None):
    """verts_out [n,V,3] (and rest_displaced when rest is given); offsets [1,V,3] or [n,V,3]."""
    verts, d = np.asarray(verts, f32), np.asarray(offsets, f32)
    M, ws = blend_rotations(W, xforms), w_sum(W)
    d = np.broadcast_to(d, verts.shape)
    delta = ((M[..., 0] * d[..., None, 0] + M[..., 1] * d[..., None, 1]) + M[..., 2] * d[..., None, 2]) / ws[None, :, None]
    out = verts + delta
    if rest is None:
        return out
    return out, np.asarray(rest, f32) + d


def backward_terms(W, xforms, grad_verts):
    """t [n,V,3] = M^T (g / wSum)."""
    g = np.asarray(grad_verts, f32)
    M, ws = blend_rotations(W, xforms), w_sum(W)
    gt = g / ws[None, :, None]
    return (M[:, :, 0, :] * gt[..., 0:1] + M[:, :, 1, :] * gt[..., 1:2]) + M[:, :, 2, :] * gt[..., 2:3]


def tree_sum(t):
    """[n,...] -> [...]: tiles of TILE consecutive frames, each summed in ascending frame from its first term; the tile sums added
    in ascending tile from the first."""
    t = np.asarray(t, f32)
    total = None
    for f0 in range(0, t.shape[0], TILE):
        s = t[f0].copy()
        for f in range(f0 + 1, min(f0 + TILE, t.shape[0])):
            s = s + t[f]
        total = s if total is None else total + s
    return total


def backward(W, xforms, grad_verts, shared):
    """grad_offsets [n,V,3], or [1,V,3] when one field is shared by all frames."""
    t = backward_terms(W, xforms, grad_verts)
    return tree_sum(t)[None] if shared else t


def incidences(faces, V):
    """(v, a, b) of every (face, corner) sorted by (v, face, corner), and each one's rank among its vertex's."""
    faces = np.asarray(faces, np.int64)
    v = faces.reshape(-1)
    a = np.roll(faces, -1, axis=1).reshape(-1)
    b = np.roll(faces, -2, axis=1).reshape(-1)
    order = np.argsort(v, kind="stable")  # the flat order is (face, corner) already
    v, a, b = v[order], a[order], b[order]
    start = np.searchsorted(v, np.arange(V))
    return v, a, b, np.arange(len(v)) - start[v]


def laplacian(faces, x):
    """(L x) [n,V,C] in fp32: per vertex from +0, its faces in ascending id, s = s + ((x_v - x_a) + (x_v - x_b))."""
    x = np.asarray(x, f32)
    v, a, b, rank = incidences(faces, x.shape[1])
    out = np.zeros_like(x)
    for r in range(int(rank.max()) + 1 if len(rank) else 0):
        k = rank == r
        vv = v[k]
        out[:, vv] = out[:, vv] + ((x[:, vv] - x[:, a[k]]) + (x[:, vv] - x[:, b[k]]))
    return out


# ------------------------------------------------------------------------------------------------ the definitions
def lbs(W, rest, xforms, root=None):
    """LinearBlendSkinning on torch tensors of one dtype: (sum_j w_vj G'_j [rest; 1]) with the homogeneous divide, + root."""
    n, V = rest.shape[0], rest.shape[1]
    M = torch.einsum("vj,njab->nvab", W, xforms)
    h = (M @ torch.cat([rest, torch.ones(n, V, 1, dtype=rest.dtype)], -1)[..., None])[..., 0]
    out = h[..., :3] / h[..., 3:4]
    return out if root is None else out + root[:, None, :]


def definition(W, rest, xforms, offsets, root=None, dtype=torch.float64):
    """LBS(rest + D, G', root) evaluated in `dtype`, as float64 numpy."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dtype)
    return lbs(t(W), t(rest) + t(offsets), t(xforms), None if root is None else t(root)).double().numpy()


def definition_vjp(W, rest, xforms, offsets, grad_verts, dtype=torch.float64):
    """dL/dD of the definition by autograd in `dtype`, D shaped like `offsets` ([1,V,3]: shared), as float64 numpy."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dtype)
    D = t(offsets).clone().requires_grad_(True)
    (lbs(t(W), t(rest) + D, t(xforms)) * t(grad_verts)).sum().backward()
    return D.grad.double().numpy()


def graph_laplacian_dense(faces, V):
    """deg - adjacency of the mesh's edge graph, [V,V] float64."""
    faces = np.asarray(faces, np.int64)
    A = np.zeros((V, V), np.float64)
    for i, j in ((0, 1), (1, 2), (2, 0)):
        A[faces[:, i], faces[:, j]] = 1.0
        A[faces[:, j], faces[:, i]] = 1.0
    return np.diag(A.sum(1)) - A


def laplacian_torch(faces, x):
    """The definition of L on a torch tensor [n,V,C] (differentiable; any dtype)."""
    f = torch.as_tensor(np.asarray(faces, np.int64))
    out = torch.zeros_like(x)
    for c in range(3):
        v, a, b = f[:, c], f[:, (c + 1) % 3], f[:, (c + 2) % 3]
        out = out.index_add(1, v, 2 * x[:, v] - x[:, a] - x[:, b])
    return out
