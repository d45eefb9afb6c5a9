"""Float64 torch restatement of the point-triangle evaluation behind smplpp_point_mesh_distance for a GIVEN face (Ericson, Real-Time
Collision Detection 5.1.5; closest_on_triangle_t in smplpp_amd/csrc/mesh_device.h): the same region tests in the same order, and the
closest point built from the region's parameters, so torch autograd through `sqdist` is the reference gradient of the squared
distance in the vertices and the points.

Regions (REGIONS order) and the vertex weights of the closest point:
  vertex a / b / c   one-hot
  edge ab            (1 - v, v, 0),  v = d1 / (d1 - d3)
  edge ac            (1 - w, 0, w),  w = d2 / (d2 - d6)
  edge bc            (0, 1 - w, w),  w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
  interior           (1 - v - w, v, w),  v = vb / (va + vb + vc), w = vc / (va + vb + vc)
Closed form (envelope theorem, every region): with r = p - c, d|r|^2/dp = 2 r and d|r|^2/dv_j = -2 w_j r.
"""
import torch

REGIONS = ("vertex_a", "vertex_b", "vertex_c", "edge_ab", "edge_ac", "edge_bc", "interior")


def _dot(x, y):
    return (x * y).sum(-1)


def region(p, a, b, c):
    """Region index [...] (REGIONS) of points p against triangles abc, all [..., 3], with the kernel's tests and order."""
    with torch.no_grad():
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        # Ericson's order: a, b, ab, c, ac, bc, interior
        order = [0, 1, 3, 2, 4, 5]
        reg = torch.full(p.shape[:-1], 6, dtype=torch.int64, device=p.device)
        done = torch.zeros(p.shape[:-1], dtype=torch.bool, device=p.device)
        for cond, r in zip(conds, order):
            take = cond & ~done
            reg = torch.where(take, torch.full_like(reg, r), reg)
            done = done | take
    return reg


def weights(p, a, b, c, reg=None):
    """Vertex weights [..., 3] of the closest point (differentiable inside a region; denominators of other regions are masked so
    that no NaN reaches the gradient)."""
    if reg is None:
        reg = region(p, a, b, c)
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    one = torch.ones_like(d1)
    zero = torch.zeros_like(d1)
    v_ab = d1 / torch.where(reg == 3, d1 - d3, one)
    w_ac = d2 / torch.where(reg == 4, d2 - d6, one)
    w_bc = (d4 - d3) / torch.where(reg == 5, (d4 - d3) + (d5 - d6), one)
    va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
    den = torch.where(reg == 6, va + vb + vc, one)
    v_in, w_in = vb / den, vc / den
    table = [
        (one, zero, zero),
        (zero, one, zero),
        (zero, zero, one),
        (1 - v_ab, v_ab, zero),
        (1 - w_ac, zero, w_ac),
        (zero, 1 - w_bc, w_bc),
        (1 - v_in - w_in, v_in, w_in),
    ]
    out = torch.zeros(p.shape, dtype=p.dtype, device=p.device)
    for r, (w0, w1, w2) in enumerate(table):
        out = torch.where((reg == r)[..., None], torch.stack([w0, w1, w2], -1), out)
    return out


def closest(p, a, b, c, reg=None):
    """(closest point [..., 3], weights [..., 3])."""
    w = weights(p, a, b, c, reg)
    return w[..., 0:1] * a + w[..., 1:2] * b + w[..., 2:3] * c, w


def sqdist(verts, faces, points, face):
    """Squared distances [n, K] of points [n, K, 3] to the faces `face` [n, K] of verts [n, V, 3] (faces [F, 3] 0-based)."""
    faces = torch.as_tensor(faces, dtype=torch.int64, device=verts.device)
    face = torch.as_tensor(face, dtype=torch.int64, device=verts.device)
    n, K = face.shape
    fv = faces[face]  # [n, K, 3]
    tri = verts.gather(1, fv.reshape(n, K * 3, 1).expand(n, K * 3, 3)).reshape(n, K, 3, 3)
    c, _ = closest(points, tri[:, :, 0], tri[:, :, 1], tri[:, :, 2])
    r = points - c
    return (r * r).sum(-1)


def closed_form(verts, faces, points, face, grad_sqdist):
    """(grad_verts [n, V, 3], grad_points [n, K, 3]) from the closed form, float64 (no autograd)."""
    with torch.no_grad():
        faces = torch.as_tensor(faces, dtype=torch.int64, device=verts.device)
        face = torch.as_tensor(face, dtype=torch.int64, device=verts.device)
        n, K = face.shape
        fv = faces[face]
        tri = verts.gather(1, fv.reshape(n, K * 3, 1).expand(n, K * 3, 3)).reshape(n, K, 3, 3)
        c, w = closest(points, tri[:, :, 0], tri[:, :, 1], tri[:, :, 2])
        r = points - c
        g = torch.as_tensor(grad_sqdist, dtype=verts.dtype, device=verts.device)
        gp = 2 * g[..., None] * r
        gv = torch.zeros_like(verts)
        contrib = (-2 * g[..., None, None] * w[..., None] * r[:, :, None, :]).reshape(n, K * 3, 3)
        gv.scatter_add_(1, fv.reshape(n, K * 3, 1).expand(n, K * 3, 3), contrib)
        return gv, gp


def vjp(verts, faces, points, face, grad_sqdist):
    """(grad_verts, grad_points) by torch autograd through `sqdist`, in the dtype of verts."""
    v = verts.detach().clone().requires_grad_(True)
    p = points.detach().clone().requires_grad_(True)
    d = sqdist(v, faces, p, face)
    gv, gp = torch.autograd.grad((d * torch.as_tensor(grad_sqdist, dtype=d.dtype, device=d.device)).sum(), (v, p), allow_unused=True)
    return gv, gp
