"""Restatements of the normal-compatible, distance-capped correspondences (smplpp_point_mesh_distance_compatible,
smplpp_mesh_point_distance_compatible; include/smplpp_hip.h states the rule) for the tests.

The float32 rule, in numpy (every ufunc rounds on its own, numpy never contracts to FMA), so the kernels must match it bit for bit:
  - compatible(m, q, cos_min):  s = (m.x q.x + m.y q.y) + m.z q.z, mm and qq the same way;  s >= 0 and mm*qq > 0 and
    s*s >= (cos_min*cos_min)*(mm*qq).  A NaN fails a comparison.
  - face_normals(verts, faces): m = (b - a) x (c - a), each component (e1y*e2z) - (e1z*e2y) and so on.
  - candidates(...): the [K, F] compatibility matrix of a frame's queries, with non-finite rows unmatched.
  - mesh_point_forward(...): mesh_point_distance_oracle.forward_frame's loop over the cloud with the eligibility mask applied
    before the minimum (with no mask it is that function, which test_scan_compat_cpu.py pins).
compatible_f64 is the float64 angle test cos(angle) >= cos_min the fp32 rule is checked against.
"""
import numpy as np

import closest_ref as cr
import mesh_point_distance_oracle as MO

CHUNK = MO.CHUNK


def _f32(x):
    return np.ascontiguousarray(x, np.float32)


def dot3(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z in float32, broadcasting over leading axes."""
    a, b = _f32(a), _f32(b)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def compatible(m, q, cos_min):
    """The fp32 rule on normals m, q [..., 3] (broadcast)."""
    m, q = _f32(m), _f32(q)
    c2 = np.float32(cos_min) * np.float32(cos_min)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        s = dot3(m, q)
        l = dot3(m, m) * dot3(q, q)
        return (s >= 0) & (l > 0) & (s * s >= c2 * l)


def compatible_f64(m, q, cos_min):
    """(cos(angle) >= cos_min, cos(angle)) in float64; a zero normal is incompatible (cos = nan)."""
    m, q = np.asarray(m, np.float64), np.asarray(q, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (m * q).sum(-1) / (np.linalg.norm(m, axis=-1) * np.linalg.norm(q, axis=-1))
    return c >= cos_min, c


def face_normals(verts, faces):
    """Unfused fp32 face normals [F, 3] of one frame verts [V, 3]."""
    v = _f32(verts)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    with np.errstate(over="ignore", invalid="ignore"):
        e1, e2 = b - a, c - a
        return np.stack([(e1[:, 1] * e2[:, 2]) - (e1[:, 2] * e2[:, 1]), (e1[:, 2] * e2[:, 0]) - (e1[:, 0] * e2[:, 2]),
                         (e1[:, 0] * e2[:, 1]) - (e1[:, 1] * e2[:, 0])], 1)


def finite_rows(x):
    return np.isfinite(np.asarray(x)).all(-1)


def candidates(verts, faces, points, normals, cos_min):
    """[K, F] bool for one frame: face f is compatible with query k (normals None: every face), False on a query with a non-finite
    coordinate or normal.  The distance cap is not part of it (it needs the kernel's fp32 distances)."""
    P = _f32(points)
    ok = finite_rows(P)
    if normals is None:
        return np.broadcast_to(ok[:, None], (len(P), len(faces))).copy()
    N = _f32(normals)
    ok &= finite_rows(N)
    return compatible(face_normals(verts, faces)[None, :, :], N[:, None, :], cos_min) & ok[:, None]


def masked_choice_check(verts, faces, points, cand, face):
    """For one frame: None if every matched query's face passes closest_ref.check_choice on the float64 distances of
    closest_ref.mesh_sqdist restricted to the query's candidates (the sub-mesh keeps ascending face ids), else a message."""
    ec = cr.eps_c(verts, faces, points)
    for k in range(len(points)):
        ids = np.nonzero(cand[k])[0]
        if face[k] < 0:
            if len(ids):
                return "query %d unmatched with %d candidates" % (k, len(ids))
            continue
        if not cand[k, face[k]]:
            return "query %d: face %d is not a candidate" % (k, face[k])
        loc = int(np.searchsorted(ids, face[k]))
        D = cr.mesh_sqdist(verts, faces[ids], points[k:k + 1], also=[loc])[0]
        msg = cr.check_choice(D, ec[k, ids], loc)
        if msg is not None:
            return "query %d: %s" % (k, msg)
    return None


def mesh_point_forward_frame(v, vn, p, pn, cos_min, max_sqdist):
    """index [V] int64 and sqdist [V] float32 for one frame: the nearest eligible point of every vertex.  vn / pn None: no normal
    test.  A vertex with a non-finite normal is unmatched; a point with one is never chosen."""
    v, p = _f32(v), _f32(p)
    V, K = len(v), len(p)
    normals = vn is not None and pn is not None
    if normals:
        vn, pn = _f32(vn), _f32(pn)
        vok, pok = finite_rows(vn), finite_rows(pn)
    best_d = np.full(V, np.inf, np.float32)
    best_k = np.full(V, -1, np.int64)
    cap = np.float32(max_sqdist)
    with np.errstate(over="ignore", invalid="ignore"):
        for k0 in range(0, K, CHUNK):
            q = p[k0:k0 + CHUNK]
            dx = v[:, None, 0] - q[None, :, 0]
            dy = v[:, None, 1] - q[None, :, 1]
            dz = v[:, None, 2] - q[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            bad = ~np.isfinite(d) | ~(d <= cap)
            if normals:
                bad |= ~(compatible(vn[:, None, :], pn[None, k0:k0 + CHUNK, :], cos_min) & vok[:, None] & pok[None, k0:k0 + CHUNK])
            d[bad] = np.inf
            j = np.argmin(d, 1)
            dj = d[np.arange(V), j]
            take = dj < best_d
            best_d[take] = dj[take]
            best_k[take] = k0 + j[take]
    best_d[best_k < 0] = 0.0
    return best_k, best_d


def mesh_point_forward(verts, vert_normals, points, point_normals, cos_min, max_sqdist):
    out = [mesh_point_forward_frame(verts[f], None if vert_normals is None else vert_normals[f], points[f],
                                    None if point_normals is None else point_normals[f], cos_min, max_sqdist) for f in range(len(verts))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
