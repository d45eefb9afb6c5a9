"""The silhouette term's rule (include/smplpp_hip.h: smplpp_mask_distance_transform, smplpp_silhouette, smplpp_silhouette_vjp) restated
in numpy so that every output bit of the library can be reproduced: the feature transform by brute force over all set pixels with the
key rule, the same transform in its separable two-pass form, an independent brute force to pin both against, the two residual sets in
float32 with each operation rounded on its own (projection, coverage and barycentrics from depth_raster_oracle), and the
fixed-correspondence loss in torch (float64 autograd is the oracle of the backward pass)."""
import numpy as np
import torch

import depth_raster_oracle as DR

f32 = np.float32


def feature_transform(mask, chunk=1 << 22):
    """One frame mask [H,W] (nonzero = set) -> (nearest [H,W] int64, sqdist [H,W] int32): the minimum over all set pixels of the key
    d2 << 32 | linear index; -1 and 0 without a set pixel."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    q = np.nonzero(mask.ravel())[0].astype(np.int64)
    if len(q) == 0:
        return np.full((H, W), -1, np.int64), np.zeros((H, W), np.int32)
    qj, qi = q // W, q % W
    best = np.empty(H * W, np.uint64)
    step = max(1, chunk // len(q))
    for p0 in range(0, H * W, step):
        p = np.arange(p0, min(H * W, p0 + step), dtype=np.int64)
        d2 = (p[:, None] % W - qi[None]) ** 2 + (p[:, None] // W - qj[None]) ** 2
        best[p0:p0 + len(p)] = ((d2.astype(np.uint64) << np.uint64(32)) | q[None].astype(np.uint64)).min(1)
    return (best & np.uint64(0xFFFFFFFF)).astype(np.int64).reshape(H, W), (best >> np.uint64(32)).astype(np.int32).reshape(H, W)


def feature_transform_loops(mask):
    """The same by plain loops, written independently of the key: the smallest distance, then the first set pixel in row-major order
    that attains it."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    nearest, sqdist = np.full((H, W), -1, np.int64), np.zeros((H, W), np.int32)
    pts = [(j, i) for j in range(H) for i in range(W) if mask[j, i]]
    for j in range(H):
        for i in range(W):
            found = None
            for (jj, ii) in pts:
                d = (i - ii) * (i - ii) + (j - jj) * (j - jj)
                if found is None or d < found[0]:
                    found = (d, jj * W + ii)
            if found is not None:
                sqdist[j, i], nearest[j, i] = found
    return nearest, sqdist


def column_pass(mask):
    """Pass 1 of the separable form: col [H,W] = the row of the nearest set pixel of the same column (the upper one on a tie), -1 for
    an empty column."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    rows = np.arange(H)[:, None]
    up = np.maximum.accumulate(np.where(mask, rows, -1), 0)
    dn = np.minimum.accumulate(np.where(mask, rows, H + H)[::-1], 0)[::-1]
    take_dn = (dn < H + H) & ((up < 0) | (dn - rows < rows - up))
    return np.where(take_dn, dn, up)


def feature_transform_separable(mask):
    """The two passes: per pixel the minimum key over its row's column candidates."""
    col = column_pass(mask)
    H, W = col.shape
    i = np.arange(W)
    nearest, sqdist = np.full((H, W), -1, np.int64), np.zeros((H, W), np.int32)
    for j in range(H):
        ok = col[j] >= 0
        if not ok.any():
            continue
        d2 = (i[:, None] - i[None, ok]) ** 2 + ((j - col[j, ok]) ** 2)[None]
        key = (d2.astype(np.uint64) << np.uint64(32)) | (col[j, ok] * W + i[ok]).astype(np.uint64)[None]
        best = key.min(1)
        nearest[j], sqdist[j] = (best & np.uint64(0xFFFFFFFF)).astype(np.int64), (best >> np.uint64(32)).astype(np.int32)
    return nearest, sqdist


def transform_batch(masks):
    out = [feature_transform(m) for m in masks]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def project(verts, cam, near, dtype=f32):
    """The rasteriser's vertex rule without the snap's cast: (u, v, accepted).  dtype float64 projects the same points in double (the
    refusal still read off the float32 rule)."""
    xc = DR.camera_vertices(verts, cam)
    _, _, ok = DR.snap(xc, cam, near)
    cam32 = np.asarray(cam, f32)
    if dtype == f32:
        with np.errstate(all="ignore"):
            u = (cam32[12] * xc[:, 0]) / xc[:, 2] + cam32[14]
            v = (cam32[13] * xc[:, 1]) / xc[:, 2] + cam32[15]
        return u, v, ok
    c = cam32.astype(np.float64)
    x = np.asarray(verts, np.float64) @ c[:9].reshape(3, 3).T + c[9:12]
    with np.errstate(all="ignore"):
        return c[12] * x[:, 0] / x[:, 2] + c[14], c[13] * x[:, 1] / x[:, 2] + c[15], ok


def vertex_pixels(u, v, H, W):
    """(column, row) of the pixel under a projection: floor, clamped into the image."""
    with np.errstate(all="ignore"):
        i = np.clip(np.floor(np.where(np.isfinite(u), u, 0)), 0, W - 1).astype(np.int64)
        j = np.clip(np.floor(np.where(np.isfinite(v), v, 0)), 0, H - 1).astype(np.int64)
    return i, j


def silhouette(verts, cam, H, W, face, mask, near=0.05):
    """One frame: dict(vert_target [V] int64, vert_sq [V] f32, pix_source [H,W] int64, pix_sq [H,W] f32) under the exact rule."""
    mask = np.asarray(mask) != 0
    face = np.asarray(face, np.int64)
    u, v, ok = project(verts, cam, near)
    i, j = vertex_pixels(u, v, H, W)
    nm, _ = feature_transform(mask)
    t = nm[j, i]
    live = ok & ~mask[j, i] & (t >= 0)
    it, jt = t % W, t // W
    with np.errstate(all="ignore"):
        rx = u - (it.astype(f32) + f32(0.5))
        ry = v - (jt.astype(f32) + f32(0.5))
        sq = rx * rx + ry * ry
    vert_target = np.where(live, t, -1)
    vert_sq = np.where(live, sq, f32(0)).astype(f32)
    nc, dc = feature_transform(face >= 0)
    want = mask & (face < 0) & (nc >= 0)
    return dict(vert_target=vert_target, vert_sq=vert_sq, pix_source=np.where(want, nc, -1), pix_sq=np.where(want, dc.astype(f32), f32(0)).astype(f32))


def silhouette_batch(verts, cams, H, W, face, mask, near=0.05):
    out = [silhouette(verts[k], cams[k], H, W, face[k], mask[k], near) for k in range(len(verts))]
    return {key: np.stack([o[key] for o in out]) for key in out[0]}


# ---- the fixed-correspondence loss in torch: the function the backward pass differentiates
def _pi(x, cam):
    return torch.stack([cam[12] * x[:, 0] / x[:, 2] + cam[14], cam[13] * x[:, 1] / x[:, 2] + cam[15]], 1)


def loss(verts, faces, cam, H, W, face_img, vert_target, pix_source, grad_vert_sq, grad_pix_sq, at=None):
    """sum_v g_v |pi(x_v) - c_t|^2 + sum_q g_q |pi(sum_i beta_i x_i) - c_q|^2 for one frame, verts a torch tensor [V,3] of any float
    dtype: targets t and sources s fixed, beta the barycentrics of pixel s's ray on its face (the rasteriser's ray-plane rule in
    verts' dtype) evaluated at `at` (default: verts itself, detached).  Entries with a zero cotangent or an id of -1 are left out of the graph."""
    dt = verts.dtype
    c = torch.as_tensor(np.asarray(cam, np.float64), dtype=dt)
    xc = verts @ c[:9].reshape(3, 3).T + c[9:12]
    total = torch.zeros((), dtype=dt)
    if grad_vert_sq is not None:
        g = np.asarray(grad_vert_sq, np.float64).reshape(-1)
        t = np.asarray(vert_target, np.int64).reshape(-1)
        k = np.nonzero((t >= 0) & (g != 0))[0]
        if len(k):
            ctr = torch.as_tensor(np.stack([t[k] % W + 0.5, t[k] // W + 0.5], 1), dtype=dt)
            total = total + (torch.as_tensor(g[k], dtype=dt) * ((_pi(xc[k], c) - ctr) ** 2).sum(1)).sum()
    if grad_pix_sq is not None:
        g = np.asarray(grad_pix_sq, np.float64).reshape(-1)
        s = np.asarray(pix_source, np.int64).reshape(-1)
        fi = np.asarray(face_img, np.int64).reshape(-1)
        q = np.nonzero((s >= 0) & (g != 0))[0]
        q = q[fi[s[q]] >= 0]
        if len(q):
            src = np.full(H * W, -1, np.int64)
            src[s[q]] = fi[s[q]]
            pix, _, beta = DR.ray_plane(verts.detach() if at is None else torch.as_tensor(at, dtype=dt), faces, cam, src.reshape(H, W))
            where = np.full(H * W, -1, np.int64)
            where[pix.numpy()] = np.arange(len(pix))
            b = beta[where[s[q]]]
            tri = torch.as_tensor(np.asarray(faces, np.int64))[fi[s[q]]]
            y = (b[:, :, None] * xc[tri]).sum(1)
            ctr = torch.as_tensor(np.stack([q % W + 0.5, q // W + 0.5], 1), dtype=dt)
            total = total + (torch.as_tensor(g[q], dtype=dt) * ((_pi(y, c) - ctr) ** 2).sum(1)).sum()
    return total


def vjp_autograd(verts, faces, cam, H, W, face_img, vert_target, pix_source, grad_vert_sq, grad_pix_sq, dtype=torch.float64):
    """dL/dverts [V,3] (float64 numpy) of `loss` by autograd in `dtype`."""
    v = torch.tensor(np.asarray(verts, np.float64), dtype=dtype, requires_grad=True)
    out = loss(v, faces, cam, H, W, face_img, vert_target, pix_source, grad_vert_sq, grad_pix_sq)
    if not out.requires_grad:
        return np.zeros(v.shape)
    out.backward()
    return v.grad.double().numpy()
