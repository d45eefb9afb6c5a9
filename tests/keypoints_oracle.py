"""The keypoint rules (include/smplpp_hip.h: smplpp_landmarks, smplpp_landmarks_vjp, smplpp_project_points, smplpp_project_points_vjp)
restated twice: in numpy float32, operation for operation with the partial and tree orders, so that every output bit of the library
can be reproduced; and in torch (any dtype) as the plain definitions, whose float64 autograd is the oracle of the backward passes and
whose float32 autograd measures what a plain fp32 evaluation gets wrong.  Also the two regressors the tests and the benchmark share."""
import numpy as np
import torch

from sum_rules import TREE64, meet

f32 = np.float32
SUB = f32(256.0)        # snapped units per pixel (the rasteriser's vertex rule)
GUARD = f32(2.0 ** 23)  # its guard band in snapped units
NJ = 24


# ------------------------------------------------------------------------------------------------ regressors (CSR: row_ptr, col, val)
def csr(rows):
    """rows: a list of lists of (column, weight) -> (row_ptr int64 [L+1], col int64 [nnz], val float32 [nnz])."""
    row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    col = np.array([c for r in rows for c, _ in r], np.int64)
    val = np.array([w for r in rows for _, w in r], f32)
    return row_ptr, col, val


def regressor_11(V, seed=3):
    """The 11 rows of the bit tests over V + 24 sources: empty, a vertex pick, a joint pick, rows of 7, 8 and 9 entries (the partial
    boundary), every source once, a repeated column, negative weights, a second empty row and a row of one joint and one vertex."""
    rng = np.random.default_rng(seed)
    S = V + NJ
    w = lambda k: rng.uniform(0.05, 1.0, k).astype(f32)  # noqa: E731
    pick = lambda k: rng.choice(S, k, replace=False)  # noqa: E731
    rows = [[], [(V // 2, 1.0)], [(V + 5, 1.0)]]
    rows += [list(zip(pick(k), w(k))) for k in (7, 8, 9)]
    rows.append(list(zip(rng.permutation(S), w(S))))
    rows.append([(4, 0.25), (9, 0.5), (4, 0.125), (V + 2, 0.3), (4, 0.7), (9, -0.1)])
    rows.append(list(zip(pick(10), -w(10))))
    rows += [[], [(V + 23, 0.5), (V - 1, 0.5)]]
    return csr(rows)


def regressor_53(model):
    """53 rows on a model: the 24 joints as picks, the 24 rows of the model's own joint_regressor (their non-zeros, ascending vertex),
    and 5 vertex picks."""
    J = np.asarray(model["joint_regressor"], f32)
    V = J.shape[1]
    rows = [[(V + j, 1.0)] for j in range(NJ)]
    rows += [[(int(c), J[j, c]) for c in np.nonzero(J[j])[0]] for j in range(NJ)]
    rows += [[(int(v), 1.0)] for v in (0, V // 5, V // 3, V // 2, V - 1)]
    return csr(rows)


def dense(reg, S):
    """The regressor as a dense [L, S] float64 matrix (repeated columns summed)."""
    row_ptr, col, val = reg
    A = np.zeros((len(row_ptr) - 1, S))
    np.add.at(A, (np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr)), col), val.astype(np.float64))
    return A


# ------------------------------------------------------------------------------------------------ numpy float32, operation for operation
def landmarks(reg, verts, joints):
    """points [n,L,3]: per row eight partials over the entries' ranks mod 8, then ((s0+s4)+(s2+s6)) + ((s1+s5)+(s3+s7))."""
    row_ptr, col, val = reg
    X = np.concatenate([np.asarray(verts, f32), np.asarray(joints, f32)], axis=1)
    n, L = X.shape[0], len(row_ptr) - 1
    out = np.empty((n, L, 3), f32)
    with np.errstate(all="ignore"):
        for l in range(L):
            s = np.zeros((8, n, 3), f32)
            for e in range(row_ptr[l], row_ptr[l + 1]):
                p = (e - row_ptr[l]) % 8
                s[p] = s[p] + val[e] * X[:, col[e]]
            out[:, l] = ((s[0] + s[4]) + (s[2] + s[6])) + ((s[1] + s[5]) + (s[3] + s[7]))
    return out


def landmarks_vjp(reg, grad_points, V, base_verts=None, base_joints=None):
    """(grad_verts [n,V,3], grad_joints [n,24,3]): per source one sequential sum over its entries in ascending e from +0; a base is
    what accumulate = 1 adds the finished sums to."""
    row_ptr, col, val = reg
    g = np.asarray(grad_points, f32)
    G = np.zeros((g.shape[0], V + NJ, 3), f32)
    with np.errstate(all="ignore"):
        for l in range(len(row_ptr) - 1):
            for e in range(row_ptr[l], row_ptr[l + 1]):
                G[:, col[e]] = G[:, col[e]] + val[e] * g[:, l]
        gv, gj = G[:, :V], G[:, V:]
        if base_verts is not None:
            gv = np.asarray(base_verts, f32) + gv
        if base_joints is not None:
            gj = np.asarray(base_joints, f32) + gj
    return np.ascontiguousarray(gv), np.ascontiguousarray(gj)


def _project(points, camera, near):
    """The rasteriser's vertex rule on [n,K,3] points with [n,16] cameras: xc [n,K,3], u, v [n,K], ok [n,K]."""
    X, cam = np.asarray(points, f32), np.asarray(camera, f32)[:, None, :]
    with np.errstate(all="ignore"):
        xc = np.stack([((cam[..., 3 * k] * X[..., 0] + cam[..., 3 * k + 1] * X[..., 1]) + cam[..., 3 * k + 2] * X[..., 2]) + cam[..., 9 + k]
                       for k in range(3)], -1)
        u = (cam[..., 12] * xc[..., 0]) / xc[..., 2] + cam[..., 14]
        v = (cam[..., 13] * xc[..., 1]) / xc[..., 2] + cam[..., 15]
        su, sv = np.rint(u * SUB), np.rint(v * SUB)
        ok = np.isfinite(xc).all(-1) & (xc[..., 2] > f32(near)) & (np.abs(su) <= GUARD) & (np.abs(sv) <= GUARD)
    return xc, u, v, ok


def _energy(u, v, target, rho):
    """(has a term [n,K], energy, r.x, r.y, w = d energy / d q) of the projections against target rows (tu, tv, c)."""
    t = np.asarray(target, f32)
    c = t[..., 2]
    has = c != 0
    with np.errstate(all="ignore"):
        rx, ry = u - t[..., 0], v - t[..., 1]
        q, cc = rx * rx + ry * ry, c * c
        if rho == 0:
            w, e = cc, cc * q
        else:
            r2 = f32(rho) * f32(rho)
            den = r2 + q
            d = r2 / den
            w, e = cc * (d * d), cc * ((r2 * q) / den)
    return has, e, rx, ry, np.broadcast_to(w, e.shape)


def project(points, camera, near=0.05, target=None, rho=0.0):
    """(uv [n,K,2], energy [n,K] or None, valid [n,K] uint8)."""
    _, u, v, ok = _project(points, camera, near)
    uv = np.where(ok[..., None], np.stack([u, v], -1), f32(0)).astype(f32)
    energy = None
    if target is not None:
        has, e, _, _, _ = _energy(u, v, target, rho)
        energy = np.where(ok & has, e, f32(0)).astype(f32)
    return uv, energy, ok.astype(np.uint8)


def project_vjp(points, camera, near=0.05, target=None, rho=0.0, grad_uv=None, grad_energy=None, base_points=None, base_camera=None):
    """(grad_points [n,K,3], grad_camera [n,16]): the cotangent k on (u, v), the pull through the projection, and per frame the 16
    camera sums over 64 partials (point k to partial k mod 64, ascending k) met by the xor tree of sum_rules.sum64."""
    X, cam = np.asarray(points, f32), np.asarray(camera, f32)
    n, K = X.shape[:2]
    xc, u, v, ok = _project(X, cam, near)
    z = f32(0)
    with np.errstate(all="ignore"):
        kx = np.zeros((n, K), f32) if grad_uv is None else np.asarray(grad_uv, f32)[..., 0].copy()
        ky = np.zeros((n, K), f32) if grad_uv is None else np.asarray(grad_uv, f32)[..., 1].copy()
        if grad_energy is not None:
            g = np.asarray(grad_energy, f32)
            has, _, rx, ry, w = _energy(u, v, target, rho)
            term = has & (g != 0)
            gw = (f32(2) * g) * w
            kx = np.where(term, kx + gw * rx, kx)
            ky = np.where(term, ky + gw * ry, ky)
        c = cam[:, None, :]
        jx = (c[..., 12] * kx) / xc[..., 2]
        jy = (c[..., 13] * ky) / xc[..., 2]
        jz = -((jx * xc[..., 0] + jy * xc[..., 1]) / xc[..., 2])
        j = np.stack([jx, jy, jz], -1)
        gp = np.stack([(c[..., a] * jx + c[..., 3 + a] * jy) + c[..., 6 + a] * jz for a in range(3)], -1)
        gp = np.where(ok[..., None], gp, z).astype(f32)
        if base_points is not None:
            gp = np.asarray(base_points, f32) + gp
        # the 16 contributions of every point, in the layout of the camera row
        contrib = np.concatenate([(j[..., :, None] * X[..., None, :]).reshape(n, K, 9), j,
                                  (kx * (xc[..., 0] / xc[..., 2]))[..., None], (ky * (xc[..., 1] / xc[..., 2]))[..., None],
                                  kx[..., None], ky[..., None]], -1).astype(f32)
        part = np.zeros((n, 64, 16), f32)
        for k0 in range(0, K, 64):
            m = min(64, K - k0)
            live = ok[:, k0:k0 + m, None]
            part[:, :m] = np.where(live, part[:, :m] + contrib[:, k0:k0 + m], part[:, :m])
        gc = meet(part, TREE64, axis=1)
        if base_camera is not None:
            gc = np.asarray(base_camera, f32) + gc
    return np.ascontiguousarray(gp), np.ascontiguousarray(gc)


# ------------------------------------------------------------------------------------------------ torch: the definitions, any dtype
def landmarks_t(A, verts, joints):
    """A [L, V+24] dense (torch) times [verts; joints]."""
    return torch.einsum("ls,nsx->nlx", A, torch.cat([verts, joints], 1))


def project_t(points, camera, near=0.05):
    """(uv [n,K,2], valid [n,K] bool) by the definition: xc = R x + t, u = fx xc.x / xc.z + cx, v likewise."""
    R, t = camera[:, :9].reshape(-1, 3, 3), camera[:, 9:12]
    xc = torch.einsum("nab,nkb->nka", R, points) + t[:, None, :]
    uv = camera[:, None, 12:14] * xc[..., :2] / xc[..., 2:3] + camera[:, None, 14:16]
    with torch.no_grad():
        valid = torch.isfinite(xc).all(-1) & (xc[..., 2] > near) & (uv.abs() * 256 <= 2.0 ** 23 + 0.5).all(-1)
    return uv, valid


def energy_t(uv, valid, target, rho=0.0):
    """[n,K]: c^2 q (rho = 0) or c^2 rho^2 q / (rho^2 + q), q the squared pixel distance; 0 for a refused point or c = 0."""
    c = target[..., 2]
    live = valid & (c != 0)
    r = torch.where(live[..., None], uv - target[..., :2], torch.zeros_like(uv))
    q = (r * r).sum(-1)
    e = c * c * q if rho == 0 else c * c * (rho * rho * q / (rho * rho + q))
    return torch.where(live, e, torch.zeros_like(e))


# ------------------------------------------------------------------------------------------------ scenes the tests share
def scene(n, K, seed, bad=2):
    """Points about 2.5 m in front of n cameras (frame 0: R = diag(1, -1, -1) exactly, so xc.z = -z bit for bit; the others turned a
    little), targets a few pixels off the true projections with confidences in (0.2, 1), a tenth of them 0 and a tenth far outliers,
    and cotangents.  bad >= 1 (K > 8): point 0 behind the camera; bad = 2: point 1 of frame 0 exactly at near = 0.05, point 2 NaN,
    a NaN target row under confidence 0 at point 3, a NaN target row under a zero grad_energy at point 4.
    Returns dict(points, camera, target, grad_uv, grad_energy)."""
    rng = np.random.default_rng(seed)
    P = np.concatenate([rng.normal(0, 0.4, (n, K, 2)), rng.normal(-2.5, 0.3, (n, K, 1))], -1).astype(f32)
    cam = np.empty((n, 16), f32)
    for f in range(n):
        a = 0.0 if f == 0 else rng.normal(0, 0.2)
        c, s = np.cos(a), np.sin(a)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([1.0, -1.0, -1.0])
        t = np.array([0.0, 0.0, 0.0]) if f == 0 else rng.normal(0, 0.05, 3)
        cam[f] = np.concatenate([R.reshape(9), t, [500.0 + 10 * f, 480.0 - 5 * f, 320.0 + f, 240.0 - f]])
    if bad >= 1 and K > 8:
        P[:, 0, 2] = 1.0
    uv, _, _ = project(P, cam)
    T = np.empty((n, K, 3), f32)
    T[..., :2] = uv + rng.normal(0, 5.0, (n, K, 2))
    T[..., 2] = rng.uniform(0.2, 1.0, (n, K))
    kind = rng.random((n, K))
    T[..., 2][kind < 0.1] = 0.0
    T[..., :2][kind > 0.9] += f32(300.0)
    guv = rng.normal(size=(n, K, 2)).astype(f32)
    ge = rng.normal(size=(n, K)).astype(f32)
    if bad >= 2 and K > 8:
        P[0, 1] = (0.1, 0.1, -0.05)
        P[:, 2, 1] = np.nan
        T[:, 3] = (np.nan, np.nan, 0.0)
        T[:, 4, :2] = np.nan
        T[:, 4, 2] = 0.5
        ge[:, 4] = 0.0
    return dict(points=P, camera=cam, target=T, grad_uv=guv, grad_energy=ge)
