"""smplpp_measure and smplpp_measure_vjp restated in numpy (include/smplpp_hip.h states the rule; smplpp_amd/csrc/measure.hip is its
device form).  With dtype float32 every operation below is one rounded fp32 operation in the header's order and every sum is the
header's fixed-order sum, so the outputs are the library's to the bit; with float64 the same rule is the yardstick.  The closed-form
backward pass is here too, in both dtypes, with the fixed orders of its sums; `measure_torch` is the same definition in torch (any
dtype) for autograd; `tables` restates the host table builder of smplpp_amd/csrc/measure_tables.h."""
import numpy as np

from ray_cast_oracle import tile_sum
from sum_rules import sum1024

f32, f64 = np.float32, np.float64


def _err():
    return np.errstate(all="ignore")


# ------------------------------------------------------------------------------------------------ the tables
def tables(F, regions, sections):
    """The builder's tables as a dict of int32 arrays, or the refusal's text.  `regions`: lists of face ids; `sections`: region ids."""
    R, S = len(regions), len(sections)
    if not 1 <= R <= 256:
        return "R must be in [1, 256]"
    if not 0 <= S <= 256:
        return "S must be in [0, 256]"
    flat = [int(f) for r in regions for f in r]
    if any(f < 0 or f >= F for f in flat):
        return "a face id is outside [0, F)"
    if any(s < 0 or s >= R for s in sections):
        return "a section_region is outside [0, R)"
    if any(len(set(int(f) for f in r)) != len(r) for r in regions):
        return "a face is listed twice in a region"
    pairs = [[] for _ in range(F)]
    for r, lst in enumerate(regions):
        for k, f in enumerate(lst):
            pairs[int(f)].append((r, k))
    secs = [[s for s in range(S) if sections[s] == r] for r in range(R)]
    i32 = lambda a: np.asarray(a, np.int32).reshape(-1)  # noqa: E731
    return dict(dims=np.array([R, len(flat), S, F], np.int64), regionPtr=i32(np.cumsum([0] + [len(r) for r in regions])), regionFace=i32(flat),
                facePtr=i32(np.cumsum([0] + [len(p) for p in pairs])), faceRegion=i32([r for p in pairs for r, _ in p]),
                faceSlot=i32([k for p in pairs for _, k in p]), secPtr=i32(np.cumsum([0] + [len(s) for s in secs])),
                secId=i32([s for ss in secs for s in ss]), secRegion=i32(list(sections)))


# ------------------------------------------------------------------------------------------------ one face
def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def face_terms(vf, c, dtype):
    """vf [K,3,3] raw corners, c [3]: dict(live [K], p [K,3,3], a, b, cr [K,3], nrm, area, vol [K])."""
    with _err():
        p = vf - c
        a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        cr = cross(a, b)
        nrm = np.sqrt(dot3(cr, cr))
        area = dtype(0.5) * nrm
        vol = dot3(p[:, 0], cross(p[:, 1], p[:, 2])) / dtype(6)
    return dict(live=np.isfinite(vf).all((1, 2)), p=p, a=a, b=b, cr=cr, nrm=nrm, area=area, vol=vol)


def plane_live(pl):
    return bool(np.isfinite(pl).all() and (pl[:3] != 0).any())


def segment(vf, pl):
    """The segments the plane pl [4] cuts from the faces vf [K,3,3]: dict(crossed [K], L [K], Labove [K], len [K], d [K,3], and per
    edge j = 1, 2 the dicts e[j] = (sa, sb, den, t [K], a, b, ba [K,3]))."""
    K = len(vf)
    with _err():
        s = ((pl[0] * vf[:, :, 0] + pl[1] * vf[:, :, 1]) + pl[2] * vf[:, :, 2]) - pl[3]
        ab = s >= 0
        cnt = ab.sum(1)
        crossed = (cnt == 1) | (cnt == 2)
        Labove = cnt == 1
        L = np.argmax(ab == Labove[:, None], 1)
        ij = (L[:, None] + np.arange(3)) % 3
        x, sx = np.take_along_axis(vf, ij[:, :, None], 1), np.take_along_axis(s, ij, 1)
        e, q = {}, {}
        for j in (1, 2):
            sa, sb = np.where(Labove, sx[:, j], sx[:, 0]), np.where(Labove, sx[:, 0], sx[:, j])
            a, b = np.where(Labove[:, None], x[:, j], x[:, 0]), np.where(Labove[:, None], x[:, 0], x[:, j])
            den = sa - sb
            t = sa / den
            ba = b - a
            q[j] = a + t[:, None] * ba
            e[j] = dict(sa=sa, sb=sb, den=den, t=t, a=a, b=b, ba=ba)
        d = q[2] - q[1]
        ln = np.sqrt(dot3(d, d))
    assert ln.shape == (K,)
    return dict(crossed=crossed, L=L, Labove=Labove, len=ln, d=d, e=e)


def segment_grad(sg, pl, g, dtype):
    """g d len per face: (G [K,3 corners of the face,3], P [K,4])."""
    K = len(sg["len"])
    with _err():
        gu = g * (sg["d"] / sg["len"][:, None])
        cl, co, pn = {}, {}, {}
        for j in (1, 2):
            e = sg["e"][j]
            gq = -gu if j == 1 else gu
            gt = dot3(gq, e["ba"])
            r = gt / e["den"]
            gsa, gsb, omt = -(r * (e["sb"] / e["den"])), r * e["t"], dtype(1) - e["t"]
            ca = omt[:, None] * gq + gsa[:, None] * pl[:3]
            cb = e["t"][:, None] * gq + gsb[:, None] * pl[:3]
            la = sg["Labove"][:, None]
            cl[j], co[j] = np.where(la, cb, ca), np.where(la, ca, cb)
            pn[j] = np.concatenate([gsa[:, None] * e["a"] + gsb[:, None] * e["b"], ((-gsa) - gsb)[:, None]], 1)
        rot = np.stack([cl[1] + cl[2], co[1], co[2]], 1)  # corners L, M, N
        P = pn[1] + pn[2]
    G = np.zeros((K, 3, 3), dtype)
    ij = (sg["L"][:, None] + np.arange(3)) % 3
    np.put_along_axis(G, np.broadcast_to(ij[:, :, None], G.shape), rot.astype(dtype), 1)
    return G, P.astype(dtype)


# ------------------------------------------------------------------------------------------------ the two calls
def _frame(verts, planes, center, f, dtype):
    c = np.zeros(3, dtype) if center is None else np.asarray(center, dtype)[f]
    pl = None if planes is None else np.asarray(planes, dtype)[f % len(planes)]
    return np.asarray(verts, dtype)[f], pl, c


def measure(verts, faces, regions, sections, planes=None, center=None, dtype=f32):
    """dict(area [n,R], volume [n,R], section [n,S], crossings [n,S] int32)."""
    faces = np.asarray(faces, np.int64)
    n, R, S = len(verts), len(regions), len(sections)
    out = dict(area=np.zeros((n, R), dtype), volume=np.zeros((n, R), dtype), section=np.zeros((n, S), dtype), crossings=np.zeros((n, S), np.int32))
    for f in range(n):
        v, pl, c = _frame(verts, planes, center, f, dtype)
        for r, lst in enumerate(regions):
            vf = v[faces[np.asarray(lst, np.int64)]].reshape(-1, 3, 3)
            ft = face_terms(vf, c, dtype)
            out["area"][f, r] = sum1024(np.where(ft["live"], ft["area"], dtype(0)))
            out["volume"][f, r] = sum1024(np.where(ft["live"], ft["vol"], dtype(0)))
            for s in range(S):
                if sections[s] != r or not plane_live(pl[s]):
                    continue
                sg = segment(vf, pl[s])
                on = sg["crossed"] & ft["live"]
                out["section"][f, s] = sum1024(np.where(on, sg["len"], dtype(0)))
                out["crossings"][f, s] = on.sum()
    return out


def measure_vjp(verts, faces, regions, sections, planes=None, center=None, grad_area=None, grad_volume=None, grad_section=None, dtype=f32):
    """The closed-form backward pass: dict(verts [n,V,3], planes [plane_frames,S,4]) in the header's orders."""
    faces = np.asarray(faces, np.int64)
    n, V, R, S = len(verts), np.shape(verts)[1], len(regions), len(sections)
    gv, gp = np.zeros((n, V, 3), dtype), np.zeros((n, S, 4), dtype)
    get = lambda g, f, k: dtype(0) if g is None else np.asarray(g, dtype)[f, k]  # noqa: E731
    for f in range(n):
        v, pl, c = _frame(verts, planes, center, f, dtype)
        vert, key, val = [], [], []  # the terms that exist: (vertex, order key, value [3])

        def emit(ids, lst, exists, G, r, slot):
            for cn in range(3):
                m = np.nonzero(exists)[0]
                vert.append(ids[m, cn])
                key.append(np.stack([ids[m, cn], lst[m], np.full(len(m), cn), np.full(len(m), r), np.full(len(m), slot)], 1))
                val.append(G[m, cn])

        for r, lst in enumerate(regions):
            lst = np.asarray(lst, np.int64)
            ids = faces[lst].reshape(-1, 3)
            vf = v[ids]
            ft = face_terms(vf, c, dtype)
            g = get(grad_area, f, r)
            if g != 0:
                with _err():
                    k = (g * dtype(0.5)) / ft["nrm"]
                    gc = k[:, None] * ft["cr"]
                    ga, gb = cross(ft["b"], gc), cross(gc, ft["a"])
                    G = np.stack([-(ga + gb), ga, gb], 1)
                emit(ids, lst, ft["live"] & (ft["nrm"] != 0), G, r, 0)
            g = get(grad_volume, f, r)
            if g != 0:
                with _err():
                    k, p = g / dtype(6), ft["p"]
                    G = k * np.stack([cross(p[:, 1], p[:, 2]), cross(p[:, 2], p[:, 0]), cross(p[:, 0], p[:, 1])], 1)
                emit(ids, lst, ft["live"], G, r, 1)
            for s in range(S):
                g = get(grad_section, f, s)
                if sections[s] != r or g == 0 or not plane_live(pl[s]):
                    continue
                sg = segment(vf, pl[s])
                on = sg["crossed"] & ft["live"] & (sg["len"] != 0)
                G, P = segment_grad(sg, pl[s], g, dtype)
                emit(ids, lst, on, G, r, 2 + s)
                gp[f, s] = sum1024(np.where(on[:, None], P, dtype(0)), axis=0)
        if vert:
            vert, key, val = np.concatenate(vert), np.concatenate(key), np.concatenate(val)
            order = np.lexsort(key.T[::-1])
            vert, val = vert[order], val[order]
            start = np.r_[0, np.nonzero(np.diff(vert))[0] + 1]
            rank = np.arange(len(vert)) - np.repeat(start, np.diff(np.r_[start, len(vert)]))
            for j in range(rank.max() + 1 if len(rank) else 0):
                m = rank == j
                gv[f, vert[m]] = gv[f, vert[m]] + val[m]
    if planes is not None and len(planes) == 1:
        gp = tile_sum(gp)[None] if n > 1 else gp[:1]
    return dict(verts=gv, planes=gp)


# ------------------------------------------------------------------------------------------------ the definition in torch
def measure_torch(verts, faces, regions, sections, planes=None, center=None):
    """(area [n,R], volume [n,R], section [n,S]) of torch tensors in their dtype, differentiable in verts and planes; plain sums."""
    import torch

    n = verts.shape[0]
    faces = torch.as_tensor(np.asarray(faces, np.int64))
    c = torch.zeros(n, 3, dtype=verts.dtype) if center is None else center.detach()
    zero = torch.zeros((), dtype=verts.dtype)
    area, volume, section = [], [], [None] * len(sections)
    for r, lst in enumerate(regions):
        tri = verts[:, faces[torch.as_tensor(np.asarray(lst, np.int64))].reshape(-1, 3)]  # [n,K,3,3]
        live = torch.isfinite(tri.detach()).all(-1).all(-1)
        p = tri - c[:, None, None, :]
        cr = torch.linalg.cross(p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 0])
        n2 = (cr * cr).sum(-1)
        ok = live & (n2.detach() > 0)
        area.append(torch.where(ok, 0.5 * torch.sqrt(torch.where(ok, n2, torch.ones_like(n2))), zero).sum(1))
        vol = (p[:, :, 0] * torch.linalg.cross(p[:, :, 1], p[:, :, 2])).sum(-1) / 6
        volume.append(torch.where(live, vol, zero).sum(1))
        for s in range(len(sections)):
            if sections[s] != r:
                continue
            pl = planes[:, s]  # [n or 1,4]
            pd = pl.detach()
            alive = torch.isfinite(pd).all(-1) & (pd[:, :3] != 0).any(-1)
            sv = (tri * pl[:, None, None, :3]).sum(-1) - pl[:, None, None, 3]  # [n,K,3]
            ab = sv.detach() >= 0
            cnt = ab.sum(-1)
            on = ((cnt == 1) | (cnt == 2)) & live & alive[:, None]
            la = cnt == 1
            L = torch.argmax((ab == la[..., None]).to(torch.int64), -1)
            q = []
            for j in (1, 2):
                o = (L + j) % 3
                ia, ib = torch.where(la, o, L), torch.where(la, L, o)
                xa = torch.gather(tri, 2, ia[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
                xb = torch.gather(tri, 2, ib[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
                sa, sb = torch.gather(sv, 2, ia[..., None])[..., 0], torch.gather(sv, 2, ib[..., None])[..., 0]
                t = sa / torch.where(on, sa - sb, torch.ones_like(sa))
                q.append(xa + t[..., None] * (xb - xa))
            d2 = ((q[1] - q[0]) ** 2).sum(-1)
            on = on & (d2.detach() > 0)
            section[s] = torch.where(on, torch.sqrt(torch.where(on, d2, torch.ones_like(d2))), zero).sum(1)
    sec = torch.stack(section, 1) if sections else verts.new_zeros((n, 0))
    return torch.stack(area, 1), torch.stack(volume, 1), sec
