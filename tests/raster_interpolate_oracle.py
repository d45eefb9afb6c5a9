"""The raster attribute interpolation (include/smplpp_hip.h, smplpp_raster_interpolate) restated: the forward in numpy, operation by
operation in float32, so that every output bit of the library can be reproduced; the function the backward pass differentiates,
sum_i beta_i(verts) A_i with the rasteriser's own beta formula (depth_raster_oracle.ray_plane), in torch of any dtype (float64
autograd is the oracle of the backward pass, float32 measures what a plain fp32 evaluation gets wrong); and the closed-form backward
of the header in numpy."""
import numpy as np
import torch

import depth_raster_oracle as DR

f32 = np.float32


def interpolate(attr, faces, face_img, bary, dtype=f32):
    """One frame: attr [V,C], faces [F,3], face_img [H,W], bary [H,W,3] -> image [H,W,C] with
    (beta_a A_a + beta_b A_b) + beta_c A_c at a covered pixel and +0 elsewhere (ids outside [0, F) included)."""
    A = np.asarray(attr, dtype)
    faces = np.asarray(faces, np.int64)
    fi = np.asarray(face_img, np.int64)
    b = np.asarray(bary, dtype)
    out = np.zeros(fi.shape + (A.shape[1],), dtype)
    hit = (fi >= 0) & (fi < len(faces))
    tri = faces[fi[hit]]
    bh = b[hit]
    with np.errstate(all="ignore"):
        out[hit] = (bh[:, 0:1] * A[tri[:, 0]] + bh[:, 1:2] * A[tri[:, 1]]) + bh[:, 2:3] * A[tri[:, 2]]
    return out


def interpolate_batch(attr, faces, face_img, bary):
    return np.stack([interpolate(attr[i], faces, face_img[i], bary[i]) for i in range(len(attr))])


def interpolate_torch(attr, verts, faces, cam, face_img):
    """attr [V,C], verts [V,3] torch tensors of one dtype (either may require grad) -> (pix [K] flat indices of the covered pixels,
    values [K,C]) with values = sum_i beta_i(verts) attr_i and beta the barycentrics of the pixel centre's ray on the face's plane."""
    pix, _, beta = DR.ray_plane(verts, faces, cam, face_img)
    fi = torch.as_tensor(np.asarray(face_img, np.int64)).reshape(-1)
    tri = torch.as_tensor(np.asarray(faces, np.int64))[fi[pix]]
    return pix, (beta[:, :, None] * attr[tri]).sum(1)


def _live(face_img, grad_image, nfaces):
    """The face image with every pixel whose cotangent is all zero, or whose id is out of range, turned to background."""
    g = np.asarray(grad_image)
    fi = np.asarray(face_img, np.int64)
    return np.where((g != 0).any(-1) & (fi < nfaces), fi, -1)


def vjp_autograd(attr, verts, faces, cam, face_img, grad_image, dtype=torch.float64):
    """(dL/dattr [V,C], dL/dverts [V,3]) for dL/dimage = grad_image [H,W,C] by autograd of interpolate_torch in `dtype`; pixels whose
    cotangent is all zero are left out of the graph (they contribute nothing, whatever their data)."""
    a = torch.tensor(np.asarray(attr, np.float64), dtype=dtype, requires_grad=True)
    v = torch.tensor(np.asarray(verts, np.float64), dtype=dtype, requires_grad=True)
    g = torch.tensor(np.asarray(grad_image, np.float64), dtype=dtype)
    pix, val = interpolate_torch(a, v, faces, cam, _live(face_img, grad_image, len(faces)))
    if len(pix) == 0:
        return np.zeros(a.shape), np.zeros(v.shape)
    (val * g.reshape(-1, g.shape[-1])[pix]).sum().backward()
    return a.grad.double().numpy(), v.grad.double().numpy()


def vjp(attr, verts, faces, cam, face_img, grad_image, dtype=np.float64):
    """The backward rule of the header.  grad_attr: corner i of a pixel's face receives beta_i g.  grad_verts: with gamma_i = g . A_i,
    q = ((gamma_b - gamma_a) cross(e2, n) + (gamma_c - gamma_a) cross(n, e1)) / nn and h = n (q.d) / (n.d) - q, camera-space corner i
    receives beta_i h; R^T applied.  (dL/dattr [V,C], dL/dverts [V,3]) in `dtype`."""
    faces = np.asarray(faces, np.int64)
    cam = np.asarray(cam, dtype)
    A, X = np.asarray(attr, dtype), np.asarray(verts, dtype)
    R = cam[:9].reshape(3, 3)
    g = np.asarray(grad_image, dtype)
    g = g.reshape(-1, g.shape[-1])
    W = np.shape(face_img)[1]
    p = np.nonzero(_live(face_img, grad_image, len(faces)).reshape(-1) >= 0)[0]
    tri = faces[np.asarray(face_img, np.int64).reshape(-1)[p]]
    a, b, c = (X[tri[:, e]] @ R.T + cam[9:12] for e in range(3))
    d = DR._ray(p % W, p // W, cam, np.dtype(dtype).type)
    _, beta = DR._hit(a, b, c, d)
    e1, e2 = b - a, c - a
    n = DR._cross(e1, e2)
    gam = [(g[p] * A[tri[:, e]]).sum(1) for e in range(3)]
    q = ((gam[1] - gam[0])[:, None] * DR._cross(e2, n) + (gam[2] - gam[0])[:, None] * DR._cross(n, e1)) / DR._dot(n, n)[:, None]
    h = n * (DR._dot(q, d) / DR._dot(n, d))[:, None] - q
    ga, gv = np.zeros(A.shape, dtype), np.zeros(X.shape, dtype)
    for e in range(3):
        np.add.at(ga, tri[:, e], beta[:, e:e + 1] * g[p])
        np.add.at(gv, tri[:, e], (beta[:, e:e + 1] * h) @ R)
    return ga, gv
