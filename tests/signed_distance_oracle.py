"""Float64 restatements behind the signed point-to-mesh distance: the generalized winding number as a plain numpy sum over the faces
(igl::winding_number's published definition, the formula oracle.cpu.OracleModel.winding_numbers evaluates in C), and the signed
squared distance sigma d^2, sigma = -1 inside (w > 0.5), +1 outside, through the point-to-mesh oracle so that torch autograd gives
the reference gradient (sigma is piecewise constant: the gradient is sigma times the distance's)."""
import numpy as np
import torch

import point_distance_oracle as PO


def winding64(verts, faces, points, chunk=512):
    """w [K] of the mesh (verts [V,3], faces [F,3] 0-based) at points [K,3], float64: sum_f atan2(det, den) / (2 pi)."""
    v = np.asarray(verts, np.float64)
    tri = v[np.asarray(faces, np.int64)]  # [F, 3, 3]
    p = np.asarray(points, np.float64).reshape(-1, 3)
    out = np.empty(len(p))
    for s in range(0, len(p), chunk):
        d = tri[None] - p[s:s + chunk, None, None, :]  # [k, F, 3, 3]
        a, b, c = d[:, :, 0], d[:, :, 1], d[:, :, 2]
        la, lb, lc = (np.sqrt((x * x).sum(-1)) for x in (a, b, c))
        det = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[s:s + chunk] = np.arctan2(det, den).sum(-1) / (2 * np.pi)
    return out


def signed_sqdist(verts, faces, points, face, inside):
    """sigma d^2 [n, K] at the faces `face` [n, K]; inside [n, K] bool."""
    sigma = 1.0 - 2.0 * torch.as_tensor(np.asarray(inside), dtype=verts.dtype, device=verts.device)
    return sigma * PO.sqdist(verts, faces, points, face)


def vjp(verts, faces, points, face, inside, grad):
    """(grad_verts, grad_points) by torch autograd through `signed_sqdist`, in the dtype of verts."""
    v = verts.detach().clone().requires_grad_(True)
    p = points.detach().clone().requires_grad_(True)
    d = signed_sqdist(v, faces, p, face, inside)
    return torch.autograd.grad((d * torch.as_tensor(grad, dtype=d.dtype, device=d.device)).sum(), (v, p))
