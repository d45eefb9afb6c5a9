"""The depth rasteriser's rule (include/smplpp_hip.h, smplpp_depth_raster) restated in numpy, operation by operation in float32, so
that every output bit of the library can be reproduced; an unsnapped float64 rasterisation of the same scene to pin the rule
against; the ray-plane depth and its 3-D barycentrics in torch (any dtype: float64 autograd is the oracle of the backward pass,
float32 measures what a plain fp32 evaluation gets wrong); and the backward formula g * beta_i * n / (n.d), R^T applied."""
import numpy as np
import torch

f32 = np.float32
SUB = 256                  # snapped units per pixel
GUARD = f32(2.0 ** 23)     # guard band in snapped units: 32768 px
MAX_SIDE = 8192            # largest H or W


def pinhole(R, t, fx, fy, cx, cy):
    """One camera as the 16 floats of the ABI: R row-major (world -> camera), t, fx, fy, cx, cy."""
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3), [fx, fy, cx, cy]]).astype(f32)


def look_at_camera(centre, distance, yaw, H, W, f=1.1):
    """A camera `distance` from `centre`, turned by `yaw` about the vertical, y down, focal length f * H, principal point at the
    image centre."""
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0, s], [0, -1, 0], [s, 0, -c]])
    t = -R @ np.asarray(centre, np.float64) + np.array([0, 0, distance])
    return pinhole(R, t, f * H, f * H, W / 2, H / 2)


def camera_vertices(verts, cam):
    """xc = R x + t in float32, ((r0 x + r1 y) + r2 z) + t per row: [V,3]."""
    X = np.asarray(verts, f32)
    cam = np.asarray(cam, f32)
    with np.errstate(all="ignore"):
        return np.stack([((cam[3 * k] * X[:, 0] + cam[3 * k + 1] * X[:, 1]) + cam[3 * k + 2] * X[:, 2]) + cam[9 + k] for k in range(3)], 1)


def snap(xc, cam, near):
    """Snapped projections (int64) and the vertices the rule accepts."""
    cam = np.asarray(cam, f32)
    with np.errstate(all="ignore"):
        u = (cam[12] * xc[:, 0]) / xc[:, 2] + cam[14]
        v = (cam[13] * xc[:, 1]) / xc[:, 2] + cam[15]
        su, sv = np.rint(u * f32(SUB)), np.rint(v * f32(SUB))
        ok = np.isfinite(xc).all(1) & (xc[:, 2] > f32(near)) & (np.abs(su) <= GUARD) & (np.abs(sv) <= GUARD)
    sx = np.where(ok, su, 0).astype(np.int64)
    sy = np.where(ok, sv, 0).astype(np.int64)
    return sx, sy, ok


def _candidates(fid, i0, i1, j0, j1, chunk=1 << 21):
    """(face, column, row) of every pixel of the boxes [i0, i1] x [j0, j1], in chunks of about `chunk` candidates."""
    w, h = i1 - i0 + 1, j1 - j0 + 1
    area = w * h
    start = 0
    while start < len(fid):
        tot = np.cumsum(area[start:])
        stop = start + max(1, int(np.searchsorted(tot, chunk, side="right")))
        a = area[start:stop]
        k = np.repeat(np.arange(start, stop), a)
        r = np.arange(int(a.sum())) - np.repeat(np.cumsum(a) - a, a)
        yield k, i0[k] + r % w[k], j0[k] + r // w[k]
        start = stop


def _cross(p, q):
    return np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1)


def _dot(p, q):
    return (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]) + p[:, 2] * q[:, 2]


def _ray(i, j, cam, dtype):
    cam = np.asarray(cam, dtype)
    half = dtype(0.5)
    dx = ((i.astype(dtype) + half) - cam[14]) / cam[12]
    dy = ((j.astype(dtype) + half) - cam[15]) / cam[13]
    return np.stack([dx, dy, np.ones_like(dx)], 1)


def _hit(a, b, c, d):
    """depth = (n.a) / (n.d) and the barycentrics of depth * d in (a, b, c); arrays [K,3] of one dtype, every operation on its own."""
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        n = _cross(e1, e2)
        depth = _dot(n, a) / _dot(n, d)
        w = depth[:, None] * d - a
        nn = _dot(n, n)
        bb = _dot(_cross(w, e2), n) / nn
        bc = _dot(_cross(e1, w), n) / nn
        one = a.dtype.type(1)
        return depth, np.stack([(one - bb) - bc, bb, bc], 1)


def raster(verts, faces, cam, H, W, near=0.05):
    """One frame under the exact rule: dict(face [H,W] int64, depth [H,W] f32, bary [H,W,3] f32, visible [V] uint8, culled int)."""
    faces = np.asarray(faces, np.int64)
    cam = np.asarray(cam, f32)
    xc = camera_vertices(verts, cam)
    sx, sy, ok = snap(xc, cam, near)
    fok = ok[faces].all(1)
    culled = int((~fok).sum())
    x, y = sx[faces], sy[faces]
    A2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    i0 = np.maximum(0, (x.min(1) + 127) >> 8)
    i1 = np.minimum(W - 1, (x.max(1) - 128) >> 8)
    j0 = np.maximum(0, (y.min(1) + 127) >> 8)
    j1 = np.minimum(H - 1, (y.max(1) - 128) >> 8)
    live = np.nonzero(fok & (A2 != 0) & (i0 <= i1) & (j0 <= j1))[0]
    key = np.full(H * W, np.uint64(0xFFFFFFFFFFFFFFFF))
    sgn = np.sign(A2)
    for k, i, j in _candidates(live, i0[live], i1[live], j0[live], j1[live]):
        f = live[k]
        px, py = i * SUB + SUB // 2, j * SUB + SUB // 2
        inside = np.ones(len(f), bool)
        for e in range(3):
            p, q = (e + 1) % 3, (e + 2) % 3
            ex, ey = sgn[f] * (x[f, q] - x[f, p]), sgn[f] * (y[f, q] - y[f, p])
            E = ex * (py - y[f, p]) - ey * (px - x[f, p])
            inside &= (E > 0) | ((E == 0) & ((ey < 0) | ((ey == 0) & (ex > 0))))
        f, i, j = f[inside], i[inside], j[inside]
        a, b, c = (xc[faces[f, e]] for e in range(3))
        depth, _ = _hit(a, b, c, _ray(i, j, cam, f32))
        with np.errstate(all="ignore"):
            keep = (depth > f32(near)) & (depth < f32(np.inf))
        f, i, j, depth = f[keep], i[keep], j[keep], depth[keep]
        cand = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | f.astype(np.uint64)
        np.minimum.at(key, j * W + i, cand)
    hit = key != np.uint64(0xFFFFFFFFFFFFFFFF)
    face = np.where(hit, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    depth = np.where(hit, (key >> np.uint64(32)).astype(np.uint32).view(f32), f32(0))
    bary = np.zeros((H * W, 3), f32)
    p = np.nonzero(hit)[0]
    fp = face[p]
    a, b, c = (xc[faces[fp, e]] for e in range(3))
    d = _ray(p % W, p // W, cam, f32)
    with np.errstate(all="ignore"):
        w = depth[p][:, None] * d - a
        e1, e2 = b - a, c - a
        n = _cross(e1, e2)
        nn = _dot(n, n)
        bb = _dot(_cross(w, e2), n) / nn
        bc = _dot(_cross(e1, w), n) / nn
    bary[p] = np.stack([(f32(1) - bb) - bc, bb, bc], 1)
    visible = np.zeros(len(xc), np.uint8)
    visible[faces[fp].ravel()] = 1
    return dict(face=face.reshape(H, W), depth=depth.reshape(H, W), bary=bary.reshape(H, W, 3), visible=visible, culled=culled)


def raster_batch(verts, faces, cams, H, W, near=0.05):
    out = [raster(verts[i], faces, cams[i], H, W, near) for i in range(len(verts))]
    r = {k: np.stack([o[k] for o in out]) for k in ("face", "depth", "bary", "visible")}
    r["culled"] = np.array([o["culled"] for o in out], np.int64)
    return r


def raster64(verts, faces, cam, H, W, near=0.05):
    """The same scene without the snap, everything in float64: float64 projection, float64 edge functions at the pixel centres (the
    same top-left rule), float64 ray-plane depth.  dict(face, depth, bary)."""
    faces = np.asarray(faces, np.int64)
    cam = np.asarray(cam, np.float64)
    X = np.asarray(verts, np.float64)
    xc = X @ cam[:9].reshape(3, 3).T + cam[9:12]
    with np.errstate(all="ignore"):
        u = cam[12] * xc[:, 0] / xc[:, 2] + cam[14]
        v = cam[13] * xc[:, 1] / xc[:, 2] + cam[15]
    ok = np.isfinite(xc).all(1) & (xc[:, 2] > near) & (np.abs(u) <= 32768) & (np.abs(v) <= 32768)
    fok = ok[faces].all(1)
    x, y = np.where(ok, u, 0)[faces], np.where(ok, v, 0)[faces]
    A2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    i0 = np.maximum(0, np.ceil(x.min(1) - 0.5)).astype(np.int64)
    i1 = np.minimum(W - 1, np.floor(x.max(1) - 0.5)).astype(np.int64)
    j0 = np.maximum(0, np.ceil(y.min(1) - 0.5)).astype(np.int64)
    j1 = np.minimum(H - 1, np.floor(y.max(1) - 0.5)).astype(np.int64)
    live = np.nonzero(fok & (A2 != 0) & (i0 <= i1) & (j0 <= j1))[0]
    best = np.full(H * W, np.inf)
    face = np.full(H * W, -1, np.int64)
    sgn = np.sign(A2)
    for k, i, j in _candidates(live, i0[live], i1[live], j0[live], j1[live]):
        f = live[k]
        px, py = i + 0.5, j + 0.5
        inside = np.ones(len(f), bool)
        for e in range(3):
            p, q = (e + 1) % 3, (e + 2) % 3
            ex, ey = sgn[f] * (x[f, q] - x[f, p]), sgn[f] * (y[f, q] - y[f, p])
            E = ex * (py - y[f, p]) - ey * (px - x[f, p])
            inside &= (E > 0) | ((E == 0) & ((ey < 0) | ((ey == 0) & (ex > 0))))
        f, i, j = f[inside], i[inside], j[inside]
        a, b, c = (xc[faces[f, e]] for e in range(3))
        depth, _ = _hit(a, b, c, _ray(i, j, cam, np.float64))
        keep = np.isfinite(depth) & (depth > near)
        f, depth, pix = f[keep], depth[keep], (j * W + i)[keep]
        order = np.lexsort((-f, -depth))  # the last write per pixel wins: smallest depth, then lowest face id
        f, depth, pix = f[order], depth[order], pix[order]
        better = depth <= best[pix]
        best[pix[better]], face[pix[better]] = depth[better], f[better]
    hit = face >= 0
    bary = np.zeros((H * W, 3))
    p = np.nonzero(hit)[0]
    a, b, c = (xc[faces[face[p], e]] for e in range(3))
    depth, bary[p] = _hit(a, b, c, _ray(p % W, p // W, cam, np.float64))
    out = np.zeros(H * W)
    out[p] = depth
    return dict(face=face.reshape(H, W), depth=out.reshape(H, W), bary=bary.reshape(H, W, 3))


# ---- the ray-plane depth in torch: the function the backward pass differentiates
def ray_plane(verts, faces, cam, face_img):
    """verts [V,3] (world, any float dtype, may require grad), cam [16], face_img [H,W] ids -> (pix [K] flat indices of the covered
    pixels, depth [K], bary [K,3]) with depth = (n.a) / (n.d) in camera space and the 3-D barycentrics of depth * d."""
    dt = verts.dtype
    cam = torch.as_tensor(np.asarray(cam, np.float64), dtype=dt)
    fi = torch.as_tensor(np.asarray(face_img, np.int64))
    H, W = fi.shape
    pix = torch.nonzero(fi.reshape(-1) >= 0)[:, 0]
    tri = torch.as_tensor(np.asarray(faces, np.int64))[fi.reshape(-1)[pix]]
    xc = verts @ cam[:9].reshape(3, 3).T + cam[9:12]
    a, b, c = xc[tri[:, 0]], xc[tri[:, 1]], xc[tri[:, 2]]
    i, j = (pix % W).to(dt), torch.div(pix, W, rounding_mode="floor").to(dt)
    d = torch.stack([(i + 0.5 - cam[14]) / cam[12], (j + 0.5 - cam[15]) / cam[13], torch.ones_like(i)], 1)
    e1, e2 = b - a, c - a
    n = torch.linalg.cross(e1, e2)
    depth = (n * a).sum(1) / (n * d).sum(1)
    w = depth[:, None] * d - a
    nn = (n * n).sum(1)
    bb = (torch.linalg.cross(w, e2) * n).sum(1) / nn
    bc = (torch.linalg.cross(e1, w) * n).sum(1) / nn
    return pix, depth, torch.stack([1 - bb - bc, bb, bc], 1)


def vjp_autograd(verts, faces, cam, face_img, grad_depth, dtype=torch.float64):
    """dL/dverts [V,3] for dL/ddepth = grad_depth [H,W] by autograd of ray_plane in `dtype`; pixels with a zero cotangent are left
    out of the graph (they contribute nothing, whatever their data)."""
    g = np.asarray(grad_depth, np.float64).reshape(-1)
    fi = np.where(g.reshape(np.shape(face_img)) != 0, np.asarray(face_img), -1)
    v = torch.tensor(np.asarray(verts, np.float64), dtype=dtype)
    v.requires_grad_(True)
    pix, depth, _ = ray_plane(v, faces, cam, fi)
    if len(pix) == 0:
        return np.zeros(v.shape)
    (depth * torch.tensor(g, dtype=dtype)[pix]).sum().backward()
    return v.grad.double().numpy()


def vjp(verts, faces, cam, face_img, grad_depth, dtype=np.float64):
    """The backward rule of the header: per covered pixel with a nonzero cotangent g, corner i of its face receives
    R^T (g * beta_i * n / (n.d)).  dL/dverts [V,3] in `dtype`."""
    faces = np.asarray(faces, np.int64)
    cam = np.asarray(cam, dtype)
    X = np.asarray(verts, dtype)
    R = cam[:9].reshape(3, 3)
    g = np.asarray(grad_depth, dtype).reshape(-1)
    fi = np.asarray(face_img, np.int64).reshape(-1)
    W = np.shape(face_img)[1]
    p = np.nonzero((fi >= 0) & (fi < len(faces)) & (g != 0))[0]
    tri = faces[fi[p]]
    a, b, c = (X[tri[:, e]] @ R.T + cam[9:12] for e in range(3))
    d = _ray(p % W, p // W, cam, np.dtype(dtype).type)
    _, beta = _hit(a, b, c, d)
    n = _cross(b - a, c - a)
    coef = g[p] / _dot(n, d)
    out = np.zeros(X.shape, dtype)
    for e in range(3):
        np.add.at(out, tri[:, e], ((beta[:, e] * coef)[:, None] * n) @ R)
    return out


def icosphere(level, radius=0.5, centre=(0.0, 0.0, 0.0)):
    """A subdivided icosahedron, outward-facing: (verts [V,3] float64, faces [F,3] int64)."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, g = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v) * radius + np.asarray(centre, np.float64), np.array(f, np.int64)


def two_spheres(level, c0, c1, radius=0.5):
    v0, f0 = icosphere(level, radius, c0)
    v1, f1 = icosphere(level, radius, c1)
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)])


def holes(covered):
    """Background pixels whose four 4-neighbours are covered."""
    c = covered
    h = np.zeros_like(c)
    h[1:-1, 1:-1] = (~c[1:-1, 1:-1]) & c[:-2, 1:-1] & c[2:, 1:-1] & c[1:-1, :-2] & c[1:-1, 2:]
    return h
