"""Float64 torch restatement of the mesh normals the reference differentiates with libtorch autograd: SMPL::calcNormal and
SMPL::calcVertexNormal (src/SMPL.cpp:518-535: cross product, torch's normalize x / max(|x|, 1e-12), adjacent faces weighted
1/deg and summed in ascending face id) and the IkTask surface (src/IkTask.cpp:58-86).  The oracle of the normals' VJP tests."""
import numpy as np
import torch

EPS = 1e-12


def normalize(x):
    return torch.nn.functional.normalize(x, dim=-1, eps=EPS)


class Mesh:
    """Faces [F,3] (0-based) and the per-vertex adjacency as a padded table [V, maxdeg] in ascending face id (one entry per
    (vertex, face), as the reference's emplace keeps)."""

    def __init__(self, faces0, V):
        self.faces = torch.as_tensor(np.asarray(faces0, np.int64))
        self.V = V
        adj = [[] for _ in range(V)]
        for f, tri in enumerate(np.asarray(faces0, np.int64)):
            for u in tri:
                if not adj[u] or adj[u][-1] != f:
                    adj[u].append(f)
        self.deg = torch.tensor([len(a) for a in adj], dtype=torch.int64)
        D = max(1, int(self.deg.max()))
        tab = np.zeros((V, D), np.int64)
        mask = np.zeros((V, D), bool)
        for u, a in enumerate(adj):
            tab[u, :len(a)] = a
            mask[u, :len(a)] = True
        self.adj = torch.as_tensor(tab)
        self.mask = torch.as_tensor(mask)


def face_normals(mesh, verts, ids=None):
    """verts [n,V,3] -> unit normals [n,count,3] of faces `ids` (None: all faces)."""
    f = mesh.faces if ids is None else mesh.faces[torch.as_tensor(np.asarray(ids, np.int64))]
    v0, v1, v2 = verts[:, f[:, 0]], verts[:, f[:, 1]], verts[:, f[:, 2]]
    return normalize(torch.cross(v1 - v0, v2 - v0, dim=-1))


def vertex_normals(mesh, verts, ids=None):
    """verts [n,V,3] -> vertex normals [n,count,3] of vertices `ids` (None: every vertex)."""
    ids = torch.arange(mesh.V) if ids is None else torch.as_tensor(np.asarray(ids, np.int64))
    fn = face_normals(mesh, verts)  # [n,F,3]
    deg = mesh.deg[ids].to(verts.dtype)
    w = torch.where(deg > 0, 1.0 / torch.clamp(deg, min=1.0), torch.zeros_like(deg))[None, :, None]
    acc = torch.zeros(verts.shape[0], len(ids), 3, dtype=verts.dtype)
    for q in range(mesh.adj.shape[1]):  # ascending face id, one term at a time
        m = mesh.mask[ids, q].to(verts.dtype)[None, :, None]
        acc = acc + m * (w * fn[:, mesh.adj[ids, q]])
    return normalize(acc)


def task_surface(mesh, verts, face_idx, vertex_weights, normal_offset):
    """IkTask::calcActualPos / calcActualNormal for face_idx [n,K], vertex_weights [n,K,3], normal_offset [n,K]."""
    n = verts.shape[0]
    fi = torch.as_tensor(np.asarray(face_idx, np.int64)).reshape(n, -1)
    K = fi.shape[1]
    fv = mesh.faces[fi]  # [n,K,3]
    vn = vertex_normals(mesh, verts)  # [n,V,3]
    b = torch.arange(n)[:, None, None]
    pts, nrm = verts[b, fv], vn[b, fv]  # [n,K,3,3]
    w = vertex_weights
    acc = w[..., 0:1] * nrm[:, :, 0]
    acc = acc + w[..., 1:2] * nrm[:, :, 1]
    acc = acc + w[..., 2:3] * nrm[:, :, 2]
    normal = normalize(acc)
    pos = (pts * w[..., None]).sum(dim=2)
    off = torch.as_tensor(np.asarray(normal_offset, np.float64), dtype=verts.dtype).reshape(n, K)
    off = torch.where(off > 0, off, torch.zeros_like(off))
    return pos + off[..., None] * normal, normal


def triangle_vertex_weights(pos, tri):
    """calcTriangleVertexWeights (include/smplpp/toolbox/GeometryUtils.h:42-52) in torch: pos [...,3], tri [...,3,3] ->
    weights [...,3], w_i = |(t_{i+1} - p) x (t_{i+2} - p)| normalised to sum 1."""
    d = tri - pos[..., None, :]
    w = torch.stack([torch.linalg.norm(torch.cross(d[..., (i + 1) % 3, :], d[..., (i + 2) % 3, :], dim=-1), dim=-1) for i in range(3)], dim=-1)
    return w / ((w[..., 0] + w[..., 1]) + w[..., 2])[..., None]


def vjp(fn, verts, grad, dtype=torch.float64):
    """dL/dverts of <fn(verts), grad> by autograd in `dtype`."""
    v = torch.as_tensor(np.asarray(verts), dtype=dtype).clone().requires_grad_(True)
    out = fn(v)
    (g,) = torch.autograd.grad(out, v, torch.as_tensor(np.asarray(grad), dtype=dtype))
    return g.detach().numpy()
