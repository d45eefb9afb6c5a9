"""smplpp_ray_cast and smplpp_ray_cast_vjp restated in numpy (include/smplpp_hip.h states the rule; smplpp_amd/csrc/ray_cast_device.h
is its device form).  With dtype float32 every operation below is one rounded fp32 operation in the header's order, so the outputs
are the library's to the bit; with float64 the same rule is the yardstick.  The edge signs are exact in the float32 form: the two
products of fp32 numbers are formed in float64, where they are exact.  The closed-form backward pass is here too, in both dtypes,
with the fixed orders of its sums."""
import numpy as np

f32, f64 = np.float32, np.float64
TILE = 32  # SMPLPP_VERTEX_OFFSETS_TILE: frames per tile of a shared input's sum
EDGES = ((0, 1), (1, 2), (2, 0))


def _err():
    return np.errstate(all="ignore")


def ray_setup(origin, direction, dtype=f32):
    """Per ray [K,3]: dict(o, d, kz, dead, Sx, Sy, dsign); a dead ray has Sx = Sy = NaN."""
    o, d = np.asarray(origin, dtype), np.asarray(direction, dtype)
    ad = np.abs(d)
    kz = np.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, np.where(ad[:, 1] >= ad[:, 2], 1, 2))
    idx = np.arange(len(o))
    dz = d[idx, kz]
    dead = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1)) | (dz == 0)
    with _err():
        Sx = np.where(dead, dtype(np.nan), d[idx, (kz + 1) % 3] / dz).astype(dtype)
        Sy = np.where(dead, dtype(np.nan), d[idx, (kz + 2) % 3] / dz).astype(dtype)
    return dict(o=o, d=d, kz=kz, dead=dead, Sx=Sx, Sy=Sy, dsign=np.sign(dz))


def edge_sign(Xp, Yp, Xq, Yq):
    """The sign of the edge function of p -> q at the ray, ties broken by the symbolic shift (eps, eps^2) of the ray in its sheared
    plane: the exact sign of Xp Yq - Yp Xq, else that of Yp - Yq, else that of Xq - Xp.  NaN where a product is NaN."""
    with _err():
        p1, p2 = Xp.astype(f64) * Yq.astype(f64), Yp.astype(f64) * Xq.astype(f64)
        s = (p1 > p2).astype(f64) - (p1 < p2)
        tie = p1 == p2
        s = np.where(tie, (Yp > Yq).astype(f64) - (Yp < Yq), s)
        tie2 = tie & (Yp == Yq)
        s = np.where(tie2, (Xq > Xp).astype(f64) - (Xq < Xp), s)
        bad = ~((p1 > p2) | (p1 < p2) | tie)
    return np.where(bad, np.nan, s)


def plane(tri, o, d, dtype=f32):
    """Range of rays (o, d) [M,3] on the planes of tri [M,3,3]: dict(A, e1, e2, n, na, nd, t) in the header's order of operations."""
    with _err():
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        A, e1, e2 = a - o, b - a, c - a
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(dtype)
        na = (n[:, 0] * A[:, 0] + n[:, 1] * A[:, 1]) + n[:, 2] * A[:, 2]
        nd = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
        t = na / nd
    return dict(A=A, e1=e1, e2=e2, n=n, na=na, nd=nd, t=t)


def bary_of(p, t, d):
    """(beta_a, beta_b, beta_c) [M,3] of the hit points t d on plane() records p, as the rasteriser forms them."""
    with _err():
        n, e1, e2 = p["n"], p["e1"], p["e2"]
        w = t[:, None] * d - p["A"]
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        px, py, pz = w[:, 1] * e2[:, 2] - w[:, 2] * e2[:, 1], w[:, 2] * e2[:, 0] - w[:, 0] * e2[:, 2], w[:, 0] * e2[:, 1] - w[:, 1] * e2[:, 0]
        qx, qy, qz = e1[:, 1] * w[:, 2] - e1[:, 2] * w[:, 1], e1[:, 2] * w[:, 0] - e1[:, 0] * w[:, 2], e1[:, 0] * w[:, 1] - e1[:, 1] * w[:, 0]
        bb = ((px * n[:, 0] + py * n[:, 1]) + pz * n[:, 2]) / nn
        bc = ((qx * n[:, 0] + qy * n[:, 1]) + qz * n[:, 2]) / nn
        ba = (n.dtype.type(1) - bb) - bc
    return np.stack([ba, bb, bc], 1)


def coverage(verts, faces, origin, direction, dtype=f32, chunk=256):
    """The covered (ray, face) pairs of one frame, before `facing` and the range test: (ray [M], face [M], s [M] in {+1, -1},
    front [M] bool), in ascending (ray, face)."""
    v = np.asarray(verts, dtype)
    faces = np.asarray(faces, np.int64)
    r = ray_setup(origin, direction, dtype)
    okface = np.isfinite(v).all(1)[faces].all(1)
    rays, ids, sg = [], [], []
    for k0 in range(0, len(r["o"]), chunk):
        sl = slice(k0, k0 + chunk)
        kz = r["kz"][sl]
        with _err():
            P = v[None, :, :] - r["o"][sl, None, :]  # [k,V,3]
            take = lambda ax: np.take_along_axis(P, np.broadcast_to(ax[:, None, None], P.shape[:2] + (1,)), 2)[..., 0]  # noqa: E731
            Pz, Px, Py = take(kz), take((kz + 1) % 3), take((kz + 2) % 3)
            X = (Px - r["Sx"][sl, None] * Pz).astype(dtype)
            Y = (Py - r["Sy"][sl, None] * Pz).astype(dtype)
        # the pairs no edge rules out (every product pair ordered one way, ties included), then the full edge rule on those few
        Xc, Yc = [X[:, faces[:, i]].astype(f64) for i in range(3)], [Y[:, faces[:, i]].astype(f64) for i in range(3)]
        ge, le = okface[None, :].copy(), okface[None, :].copy()
        with _err():
            for p, q in EDGES:
                p1, p2 = Xc[p] * Yc[q], Yc[p] * Xc[q]
                ge, le = ge & (p1 >= p2), le & (p1 <= p2)
        kk, ff = np.nonzero(ge | le)
        cx, cy = X[kk[:, None], faces[ff]], Y[kk[:, None], faces[ff]]  # [M,3]
        e = [edge_sign(cx[:, p], cy[:, p], cx[:, q], cy[:, q]) for p, q in EDGES]
        cov = (e[0] == e[1]) & (e[1] == e[2]) & (e[0] != 0)  # (NaN == NaN is false)
        rays.append(kk[cov] + k0), ids.append(ff[cov]), sg.append(e[0][cov].astype(np.int64))
    rays, ids, sg = np.concatenate(rays), np.concatenate(ids), np.concatenate(sg)
    order = np.lexsort((ids, rays))
    rays, ids, sg = rays[order], ids[order], sg[order]
    return rays, ids, sg, sg * r["dsign"][rays] < 0


def ray_cast_frame(verts, faces, origin, direction, t_min=0.0, t_max=np.inf, facing=3, dtype=f32, chunk=256):
    """One frame: dict(face [K] int64, t [K], bary [K,3], hits [K,2] int32, cover [K] the signed number of covering faces before
    `facing` and the range test (0 for a closed mesh), plus the accepted candidates cand = (ray, face, t, front))."""
    v, o, d = np.asarray(verts, dtype), np.asarray(origin, dtype), np.asarray(direction, dtype)
    faces = np.asarray(faces, np.int64)
    K = len(o)
    rays, ids, sg, front = coverage(v, faces, o, d, dtype, chunk)
    cover = np.zeros(K, np.int64)
    np.add.at(cover, rays, sg)
    p = plane(v[faces[ids]], o[rays], d[rays], dtype)
    t = p["t"]
    with _err():
        keep = np.isfinite(t) & (t > dtype(t_min)) & (t <= dtype(t_max)) & (np.where(front, 1, 2) & facing).astype(bool)
    rays, ids, t, front = rays[keep], ids[keep], t[keep], front[keep]
    hits = np.zeros((K, 2), np.int32)
    np.add.at(hits, (rays, np.where(front, 0, 1)), 1)
    face, tt = np.full(K, -1, np.int64), np.zeros(K, dtype)
    order = np.lexsort((ids, t, rays))  # per ray the smallest t, then the lowest face: first of its run
    first = np.ones(len(order), bool)
    first[1:] = rays[order][1:] != rays[order][:-1]
    w = order[first]
    face[rays[w]], tt[rays[w]] = ids[w], t[w]
    bary = np.zeros((K, 3), dtype)
    hit = face >= 0
    if hit.any():
        ph = plane(v[faces[face[hit]]], o[hit], d[hit], dtype)
        bary[hit] = bary_of(ph, tt[hit], d[hit])
    return dict(face=face, t=tt, bary=bary, hits=hits, cover=cover, cand=(rays, ids, t, front))


def ray_cast(verts, faces, origin, direction, t_min=0.0, t_max=np.inf, facing=3, dtype=f32):
    """n frames verts [n,V,3] against rays [1 or n,K,3]: dict(face [n,K], t, bary [n,K,3], hits [n,K,2], cover [n,K])."""
    n = len(verts)
    per = [ray_cast_frame(verts[f], faces, origin[f % len(origin)], direction[f % len(direction)], t_min, t_max, facing, dtype) for f in range(n)]
    return {k: np.stack([p[k] for p in per]) for k in ("face", "t", "bary", "hits", "cover")}


def tile_sum(terms):
    """Sum over axis 0 in the two-level order of smplpp_vertex_offsets_vjp: tiles of TILE frames, ascending within a tile from its
    first term, then across the tiles from the first tile's sum."""
    tot = None
    for f0 in range(0, len(terms), TILE):
        tile = terms[f0].copy()
        for f in range(f0 + 1, min(f0 + TILE, len(terms))):
            tile = tile + terms[f]
        tot = tile if tot is None else tot + tile
    return tot


def ray_cast_vjp(verts, faces, origin, direction, face, grad_t, dtype=f32):
    """The closed-form backward pass at the faces `face` [n,K] held fixed: dict(verts [n,V,3], origin, dir [ray_frames,K,3]).  A ray
    with face outside [0, F), a dead ray or a zero cotangent contributes nothing; grad_verts is one sum per vertex in ascending ray,
    then corner; shared rays are summed over the frames by tile_sum."""
    v, o, d = np.asarray(verts, dtype), np.asarray(origin, dtype), np.asarray(direction, dtype)
    faces, face, g = np.asarray(faces, np.int64), np.asarray(face, np.int64), np.asarray(grad_t, dtype)
    n, K, rf = len(v), o.shape[1], len(o)
    gv, go, gd = np.zeros_like(v), np.zeros((n, K, 3), dtype), np.zeros((n, K, 3), dtype)
    for f in range(n):
        of, df = o[f % rf], d[f % rf]
        live = (face[f] >= 0) & (face[f] < len(faces)) & ~ray_setup(of, df, dtype)["dead"] & (g[f] != 0)
        ks = np.nonzero(live)[0]
        if not len(ks):
            continue
        ids = faces[face[f, ks]]
        p = plane(v[f][ids], of[ks], df[ks], dtype)
        beta = bary_of(p, p["t"], df[ks])
        with _err():
            vec = (g[f, ks] / p["nd"])[:, None] * p["n"]
            go[f, ks], gd[f, ks] = -vec, -(p["t"][:, None] * vec)
            share = beta[:, :, None] * vec[:, None, :]  # [M,3 corners,3]
            for i in range(len(ks)):
                for c in range(3):
                    gv[f, ids[i, c]] = gv[f, ids[i, c]] + share[i, c]
    if rf == 1 and n > 1:
        go, gd = tile_sum(go)[None], tile_sum(gd)[None]
    elif rf == 1:
        go, gd = go[:1], gd[:1]
    return dict(verts=gv, origin=go, dir=gd)


def moller_trumbore(tri, o, d, dtype=f32):
    """Plain Moller-Trumbore on tri [M,3,3]: (t, u, v), for the error a textbook fp32 intersection makes on the same hit."""
    tri, o, d = np.asarray(tri, dtype), np.asarray(o, dtype), np.asarray(d, dtype)
    with _err():
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        pv = np.cross(d, e2).astype(dtype)
        det = (e1 * pv).sum(1, dtype=dtype)
        tv = o - tri[:, 0]
        u = (tv * pv).sum(1, dtype=dtype) / det
        qv = np.cross(tv, e1).astype(dtype)
        return (e2 * qv).sum(1, dtype=dtype) / det, u, (d * qv).sum(1, dtype=dtype) / det


def camera_rays(camera, H, W, dtype=f64):
    """The rasteriser's pixel-centre rays of camera rows [n,16] in world space: (origin [n,H*W,3], dir [n,H*W,3]) = (-R^T t,
    R^T ((i + 0.5 - cx) / fx, (j + 0.5 - cy) / fy, 1)) for pixel (row j, column i); the range along them is the depth."""
    cam = np.asarray(camera, dtype).reshape(-1, 16)
    R, t = cam[:, :9].reshape(-1, 3, 3), cam[:, 9:12]
    j, i = np.meshgrid(np.arange(H, dtype=dtype), np.arange(W, dtype=dtype), indexing="ij")
    dx = ((i.reshape(-1)[None] + dtype(0.5)) - cam[:, 14:15]) / cam[:, 12:13]
    dy = ((j.reshape(-1)[None] + dtype(0.5)) - cam[:, 15:16]) / cam[:, 13:14]
    dc = np.stack([dx, dy, np.ones_like(dx)], 2)
    return np.broadcast_to(-np.einsum("nji,nj->ni", R, t)[:, None], dc.shape).copy(), np.einsum("nji,nkj->nki", R, dc)
