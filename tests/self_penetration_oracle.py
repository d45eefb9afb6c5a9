"""Oracles of smplpp_self_intersections / smplpp_self_penetration / smplpp_self_penetration_vjp.

- intersections(v, faces, dtype): the detection rule of the C header with every operation in `dtype`.  In float32 it restates the
  kernel's arithmetic (numpy rounds each elementwise operation on its own, no FMA), so the pair list must match bit for bit; in
  float64 it is the reference the fp32 rule approaches.  A sort and sweep on x generates the candidates; the AABB test is exact.
- brute_force(v, faces, dtype): the same rule over all pairs (small meshes).
- near_degenerate(v, faces, margin): the pairs whose smallest relative |orient| (over the orients the rule evaluates) is below
  margin, where the fp32 and fp64 decisions may differ.
- pair_energy / vjp: the energy of the C header in torch (float64 or float32), its vector-Jacobian product by autograd.
- icosphere, two_spheres: closed, outward-oriented test meshes."""
import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------- detection
def orient(a, b, c, d):
    u, v, w = b - a, c - a, d - a
    cx = u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1]
    cy = u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2]
    cz = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
    return (cx * w[..., 0] + cy * w[..., 1]) + cz * w[..., 2]


def _edge_crosses(op, oq, p, q, a, b, c):
    s = (op > 0) & (oq < 0) | (op < 0) & (oq > 0)
    s0, s1, s2 = orient(p, q, a, b), orient(p, q, b, c), orient(p, q, c, a)
    return s & (((s0 > 0) & (s1 > 0) & (s2 > 0)) | ((s0 < 0) & (s1 < 0) & (s2 < 0)))


def edges_cross(X, Y):
    """[P] whether some edge (x0 x1, x1 x2, x2 x0) of triangles X [P,3,3] crosses triangles Y [P,3,3]."""
    a, b, c = Y[:, 0], Y[:, 1], Y[:, 2]
    o = [orient(a, b, c, X[:, j]) for j in range(3)]
    hit = np.zeros(len(X), bool)
    for j in range(3):
        k = (j + 1) % 3
        hit |= _edge_crosses(o[j], o[k], X[:, j], X[:, k], a, b, c)
    return hit


def _boxes(v, faces):
    T = v[faces]  # [F,3,3]
    ok = np.isfinite(T).all(axis=(1, 2))
    return T, T.min(axis=1), T.max(axis=1), ok


def _decide(T, faces, P):
    """Of candidate pairs P [k,2] (AABBs overlapping), those that share no vertex and cross."""
    f, g = P[:, 0], P[:, 1]
    share = (faces[f][:, :, None] == faces[g][:, None, :]).any(axis=(1, 2))
    P = P[~share]
    if len(P) == 0:
        return P
    X, Y = T[P[:, 0]], T[P[:, 1]]
    return P[edges_cross(X, Y) | edges_cross(Y, X)]


def _sorted_pairs(P):
    P = np.sort(np.asarray(P, np.int64).reshape(-1, 2), axis=1)
    return P[np.lexsort((P[:, 1], P[:, 0]))] if len(P) else P.reshape(0, 2)


def candidates(v, faces):
    """Pairs (f < g) of valid faces whose closed AABBs overlap: a sweep on x."""
    T, lo, hi, ok = _boxes(v, faces)
    ids = np.nonzero(ok)[0]
    order = ids[np.argsort(lo[ids, 0], kind="stable")]
    slo = lo[order, 0]
    end = np.searchsorted(slo, hi[order, 0], side="right")
    start = np.arange(len(order)) + 1
    cnt = np.maximum(end - start, 0)
    i = np.repeat(np.arange(len(order)), cnt)
    j = np.concatenate([np.arange(s, e) for s, e in zip(start, end) if e > s]) if cnt.sum() else np.zeros(0, np.int64)
    f, g = order[i], order[j]
    keep = ((lo[f] <= hi[g]) & (lo[g] <= hi[f])).all(axis=1)
    return T, _sorted_pairs(np.stack([f[keep], g[keep]], axis=1))


def intersections(v, faces, dtype=np.float32):
    """[P,2] int64 pairs (f < g) of one frame's mesh v [V,3], ascending (f, g), computed in `dtype`."""
    v = np.asarray(v, dtype)
    faces = np.asarray(faces, np.int64)
    T, P = candidates(v, faces)
    return _sorted_pairs(_decide(T, faces, P))


def brute_force(v, faces, dtype=np.float32):
    v = np.asarray(v, dtype)
    faces = np.asarray(faces, np.int64)
    T, lo, hi, ok = _boxes(v, faces)
    f, g = np.triu_indices(len(faces), 1)
    keep = ok[f] & ok[g] & ((lo[f] <= hi[g]) & (lo[g] <= hi[f])).all(axis=1)
    return _sorted_pairs(_decide(T, faces, np.stack([f[keep], g[keep]], axis=1)))


def _rel_orient(a, b, c, d):
    s = np.linalg.norm(b - a, axis=-1) * np.linalg.norm(c - a, axis=-1) * np.linalg.norm(d - a, axis=-1)
    return np.abs(orient(a, b, c, d)) / np.where(s > 0, s, 1.0)


def near_degenerate(v, faces, margin):
    """Set of pairs (f, g) sharing no vertex, AABBs overlapping, whose smallest relative |orient| (in float64) is below margin."""
    v = np.asarray(v, np.float64)
    faces = np.asarray(faces, np.int64)
    T, P = candidates(v, faces)
    share = (faces[P[:, 0]][:, :, None] == faces[P[:, 1]][:, None, :]).any(axis=(1, 2))
    P = P[~share]
    X, Y = T[P[:, 0]], T[P[:, 1]]
    m = np.full(len(P), np.inf)
    for A, B in ((X, Y), (Y, X)):
        a, b, c = B[:, 0], B[:, 1], B[:, 2]
        for j in range(3):
            p, q = A[:, j], A[:, (j + 1) % 3]
            for val in (_rel_orient(a, b, c, p), _rel_orient(p, q, a, b), _rel_orient(p, q, b, c), _rel_orient(p, q, c, a)):
                m = np.minimum(m, val)
    return {tuple(x) for x in P[m < margin].tolist()}


# ---------------------------------------------------------------------------------------------------- energy
def _receiver(a, b, c, x, s2):
    o = (a + b + c) / 3
    m = torch.cross(b - a, c - a, dim=-1)
    ln = torch.linalg.norm(m, dim=-1, keepdim=True)
    area = ln[..., 0] > 0
    n = m / torch.where(ln > 0, ln, torch.ones_like(ln))
    r2 = ((a - o).pow(2).sum(-1) + (b - o).pow(2).sum(-1) + (c - o).pow(2).sum(-1)) / 3
    d = x - o
    h = (d * n).sum(-1)
    q2 = d.pow(2).sum(-1) - h * h
    phi = torch.clamp(1 - q2 / (s2 * torch.where(area, r2, torch.ones_like(r2))), min=0)
    return torch.where(area & (h < 0), phi * phi * (h * h), torch.zeros_like(h))


def pair_energy(v, faces, pairs, sigma):
    """[P] energies of pairs [P,2] (f, g) of one frame's vertices v [V,3] (a torch tensor of any float dtype)."""
    faces = torch.as_tensor(np.asarray(faces, np.int64))
    pairs = torch.as_tensor(np.asarray(pairs, np.int64).reshape(-1, 2))
    F, G = v[faces[pairs[:, 0]]], v[faces[pairs[:, 1]]]  # [P,3,3]
    s2 = sigma * sigma
    e = torch.zeros(len(pairs), dtype=v.dtype)
    for j in range(3):
        e = e + _receiver(F[:, 0], F[:, 1], F[:, 2], G[:, j], s2)
    for j in range(3):
        e = e + _receiver(G[:, 0], G[:, 1], G[:, 2], F[:, j], s2)
    return e


def vjp(v, faces, pairs, grad, sigma):
    """dL/dv [V,3] for L = sum(grad * pair_energy) in v's dtype."""
    v = v.detach().clone().requires_grad_(True)
    (pair_energy(v, faces, pairs, sigma) * torch.as_tensor(grad, dtype=v.dtype)).sum().backward()
    return v.grad


# ---------------------------------------------------------------------------------------------------- meshes
def icosphere(level, radius=1.0, center=(0.0, 0.0, 0.0)):
    """(verts [V,3] float64, faces [F,3] int64), outward-oriented, 20 * 4^level faces."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(center, float), np.array(f, np.int64)


def spheres(level, centers, radius=0.5):
    """Several icospheres in one mesh: (verts, faces)."""
    vs, fs, off = [], [], 0
    for c in centers:
        v, f = icosphere(level, radius, c)
        vs.append(v)
        fs.append(f + off)
        off += len(v)
    return np.concatenate(vs), np.concatenate(fs)
