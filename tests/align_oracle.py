"""Rigid and similarity alignment of point sets (smplpp_align, smplpp_align_vjp) restated in numpy, operation by operation
and with the dtype as a parameter: in float32 it is the rule whose bits the kernels must give, in float64 it is compared with the
definition.  The sums are sum_rules.sum1024, the Jacobi is a plain loop (over the frames at once: a pair that is skipped keeps its
values).  Then the closed-form backward, and the definition in torch: weighted Kabsch / Umeyama by torch.linalg.svd with the determinant
correction."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sum_rules import sum1024  # noqa: E402

SWEEPS = 7                      # ALN_SWEEPS of align.hip
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
MIN_GAP = 1e-3


def _rows(a, n):
    """[1 or n, ...] -> [n, ...]"""
    return np.broadcast_to(a, (n,) + a.shape[1:])


def _inputs(source, target, weight, dtype):
    x = np.asarray(source, dtype)
    n, K = x.shape[:2]
    y = np.asarray(target, dtype)
    y = _rows(y.reshape((-1, K, 3)), n)
    w = np.ones((1, K), dtype) if weight is None else np.asarray(weight, dtype).reshape(-1, K)
    w = _rows(w, n)
    moved = np.isfinite(x).all(-1)
    live = np.isfinite(w) & (w > 0) & moved & np.isfinite(y).all(-1)
    return x, y, w, live, moved


def jacobi(A, sweeps=SWEEPS):
    """Cyclic Jacobi on symmetric A [n,4,4]: (eigenvalues [n,4], V [n,4,4] with the eigenvectors in its columns)."""
    T = A.dtype.type
    A = A.copy()
    V = np.broadcast_to(np.eye(4, dtype=A.dtype), A.shape).copy()
    one, two = T(1), T(2)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                apq = A[:, p, q].copy()
                on = apq != 0
                theta = (A[:, q, q] - A[:, p, p]) / (two * apq)
                t = np.where(theta < 0, -one, one) / (np.abs(theta) + np.sqrt(theta * theta + one))
                c = one / np.sqrt(t * t + one)
                s = t * c
                h = t * apq
                N = A.copy()
                N[:, p, p], N[:, q, q] = A[:, p, p] - h, A[:, q, q] + h
                N[:, p, q] = N[:, q, p] = 0
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[:, r, p], A[:, r, q]
                        N[:, r, p] = N[:, p, r] = c * arp - s * arq
                        N[:, r, q] = N[:, q, r] = s * arp + c * arq
                U = V.copy()
                U[:, :, p], U[:, :, q] = c[:, None] * V[:, :, p] - s[:, None] * V[:, :, q], s[:, None] * V[:, :, p] + c[:, None] * V[:, :, q]
                A = np.where(on[:, None, None], N, A)
                V = np.where(on[:, None, None], U, V)
    return A[:, np.arange(4), np.arange(4)].copy(), V


def _rot(R, x):
    """R [n,9] row-major on x [n,...,3]"""
    R = R.reshape((-1,) + (1,) * (x.ndim - 2) + (3, 3))
    return (R[..., 0] * x[..., None, 0] + R[..., 1] * x[..., None, 1]) + R[..., 2] * x[..., None, 2]


def _rot_t(R, g):
    """R^T on g [n,...,3]"""
    R = R.reshape((-1,) + (1,) * (g.ndim - 2) + (3, 3))
    return (R[..., 0, :] * g[..., 0, None] + R[..., 1, :] * g[..., 1, None]) + R[..., 2, :] * g[..., 2, None]


def frame(source, target, weight=None, with_scale=False, min_gap=MIN_GAP, dtype=np.float32, sweeps=SWEEPS):
    """Steps 1 to 7 and 9 of the forward rule: a dict of everything a frame's threads hold after the solve."""
    T = np.dtype(dtype).type
    x, y, w, live, moved = _inputs(source, target, weight, dtype)
    n, K = x.shape[:2]
    zero, one, two = T(0), T(1), T(2)
    L = live[..., None]
    with np.errstate(all="ignore"):
        W = sum1024(np.where(live, w, zero))
        cx = sum1024(np.where(L, w[..., None] * x, zero), axis=1) / W[:, None]
        cy = sum1024(np.where(L, w[..., None] * y, zero), axis=1) / W[:, None]
        xt, yt = x - cx[:, None], y - cy[:, None]
        S = sum1024(np.where(L[..., None], (w[..., None] * xt)[..., :, None] * yt[..., None, :], zero), axis=1)  # [n,3,3]
        vx = sum1024(np.where(live, w * ((xt[..., 0] * xt[..., 0] + xt[..., 1] * xt[..., 1]) + xt[..., 2] * xt[..., 2]), zero))
        Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = (S[:, i, j] for i in range(3) for j in range(3))
        A = np.zeros((n, 4, 4), dtype)
        A[:, 0, 0], A[:, 1, 1], A[:, 2, 2], A[:, 3, 3] = (Sxx + Syy) + Szz, (Sxx - Syy) - Szz, ((-Sxx) + Syy) - Szz, ((-Sxx) - Syy) + Szz
        A[:, 0, 1] = A[:, 1, 0] = Syz - Szy
        A[:, 0, 2] = A[:, 2, 0] = Szx - Sxz
        A[:, 0, 3] = A[:, 3, 0] = Sxy - Syx
        A[:, 1, 2] = A[:, 2, 1] = Sxy + Syx
        A[:, 1, 3] = A[:, 3, 1] = Szx + Sxz
        A[:, 2, 3] = A[:, 3, 2] = Syz + Szy
        bit0 = ~((W > 0) & np.isfinite(W))
        A[bit0] = 0
        lam, V = jacobi(A, sweeps)
        top = np.zeros(n, np.int64)
        l1, l4 = lam[:, 0].copy(), lam[:, 0].copy()
        for i in range(1, 4):
            up = lam[:, i] > l1
            l1, top = np.where(up, lam[:, i], l1), np.where(up, i, top)
            l4 = np.where(lam[:, i] < l4, lam[:, i], l4)
        l2 = np.full(n, -np.inf, dtype)
        for i in range(4):
            l2 = np.where((top != i) & (lam[:, i] > l2), lam[:, i], l2)
        spread = l1 - l4
        gap = np.where(spread > 0, (l1 - l2) / spread, zero).astype(dtype)
        status = np.where(vx == 0, 2, 0) | np.where(gap <= T(min_gap), 4, 0)
        e = V[np.arange(n), :, top]
        length = np.sqrt(((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) + e[:, 3] * e[:, 3])
        q = e / length[:, None]
        qw, qx, qy, qz = q.T
        ww, xx, yy, zz, xy, xz, yz, wx, wy, wz = qw * qw, qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qw * qx, qw * qy, qw * qz
        R = np.stack([((ww + xx) - yy) - zz, two * (xy - wz), two * (xz + wy),
                      two * (xy + wz), ((ww - xx) + yy) - zz, two * (yz - wx),
                      two * (xz - wy), two * (yz + wx), ((ww - xx) - yy) + zz], -1).astype(dtype)
        eye = np.eye(3, dtype=dtype).reshape(9)
        flat = vx == 0
        R = np.where(flat[:, None], eye, R)
        St = S.transpose(0, 2, 1).reshape(n, 9)
        acc = R[:, 0] * St[:, 0]
        for i in range(1, 9):
            acc = acc + R[:, i] * St[:, i]
        s = np.where(flat | (not with_scale), one, acc / vx).astype(dtype)
        t = cy - s[:, None] * _rot(R, cx)
        # bit 0: the identity, and nothing else
        R = np.where(bit0[:, None], eye, R)
        s = np.where(bit0, one, s)
        t = np.where(bit0[:, None], zero, t)
        gap = np.where(bit0, zero, gap)
        status = np.where(bit0, 1, status).astype(np.int32)
        q = np.where(bit0[:, None], np.array([1, 0, 0, 0], dtype), q)
    return dict(x=x, y=y, w=w, live=live, moved=moved, W=W, cx=cx, cy=cy, S=S, vx=vx, lam=lam, V=V, top=top, q=q, R=R, t=t, s=s, gap=gap,
                status=status, with_scale=bool(with_scale))


def _apply(F, x):
    return F["s"][:, None, None] * _rot(F["R"], x) + F["t"][:, None]


def align(source, target, weight=None, with_scale=False, min_gap=MIN_GAP, dtype=np.float32, sweeps=SWEEPS):
    """smplpp_align: (transform [n,13], aligned [n,K,3], energy [n], point_error [n,K], gap [n], status [n] int32)."""
    F = frame(source, target, weight, with_scale, min_gap, dtype, sweeps)
    T = np.dtype(dtype).type
    live, w, y = F["live"], F["w"], F["y"]
    with np.errstate(all="ignore"):
        al = _apply(F, F["x"])
        d = al - y
        pe = np.where(live, (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], T(0))
        energy = sum1024(np.where(live, w * pe, T(0)))
    energy = np.where(F["status"] & 1, T(0), energy)
    transform = np.concatenate([F["R"], F["t"], F["s"][:, None]], 1)
    return tuple(np.ascontiguousarray(a, dtype) for a in (transform, al, energy, pe, F["gap"])) + (F["status"],)


def align_vjp(source, target, weight=None, with_scale=False, min_gap=MIN_GAP, grad_transform=None, grad_aligned=None, grad_energy=None,
              grad_source=None, grad_target=None, accumulate=0, dtype=np.float32, sweeps=SWEEPS):
    """smplpp_align_vjp: (grad_source, grad_target), each [n,K,3]; stored into (accumulate = 0) or added to the arrays given, which may be
    None (then that output is not asked for and None comes back)."""
    F = frame(source, target, weight, with_scale, min_gap, dtype, sweeps)
    T = np.dtype(dtype).type
    x, y, w, live, moved = (F[k] for k in ("x", "y", "w", "live", "moved"))
    n, K = x.shape[:2]
    zero, two = T(0), T(2)
    R, s, cx, cy, S, vx, V, lam, q, top = (F[k] for k in ("R", "s", "cx", "cy", "S", "vx", "V", "lam", "q", "top"))
    gal = np.zeros((n, K, 3), dtype) if grad_aligned is None else np.asarray(grad_aligned, dtype)
    ge = np.zeros(n, dtype) if grad_energy is None else np.asarray(grad_energy, dtype)
    gtr = np.zeros((n, 13), dtype) if grad_transform is None else np.asarray(grad_transform, dtype)
    L, M = live[..., None], moved[..., None]
    with np.errstate(all="ignore"):
        d = _apply(F, x) - y
        c2 = ((two * ge)[:, None] * w)[..., None]
        ga = gal + np.where(L, c2 * d, zero)
        sg = sum1024(np.where(M, ga, zero), axis=1)                                                   # [n,3]
        P = sum1024(np.where(M[..., None], ga[..., :, None] * x[..., None, :], zero), axis=1).reshape(n, 9)
        Gt = gtr[:, 9:12] + sg
        rc = _rot(R, cx)
        rp = R[:, 0] * P[:, 0]
        for i in range(1, 9):
            rp = rp + R[:, i] * P[:, i]
        Gs = (gtr[:, 12] + rp) - ((Gt[:, 0] * rc[:, 0] + Gt[:, 1] * rc[:, 1]) + Gt[:, 2] * rc[:, 2])
        if not F["with_scale"]:
            Gs = np.zeros(n, dtype)
        St = S.transpose(0, 2, 1).reshape(n, 9)
        GR = ((gtr[:, :9] + s[:, None] * P) - ((s[:, None] * Gt)[:, :, None] * cx[:, None, :]).reshape(n, 9)) + (Gs[:, None] * St) / vx[:, None]
        g2 = two * ((-(Gs * s)) / vx)
        qw, qx, qy, qz = q.T
        d0, d1 = (GR[:, 0] + GR[:, 4]) + GR[:, 8], (GR[:, 0] - GR[:, 4]) - GR[:, 8]
        d2, d3 = ((-GR[:, 0]) + GR[:, 4]) - GR[:, 8], ((-GR[:, 0]) - GR[:, 4]) + GR[:, 8]
        a01, a02, a03 = GR[:, 7] - GR[:, 5], GR[:, 2] - GR[:, 6], GR[:, 3] - GR[:, 1]
        a12, a13, a23 = GR[:, 1] + GR[:, 3], GR[:, 2] + GR[:, 6], GR[:, 5] + GR[:, 7]
        gq = np.stack([two * (((d0 * qw + a01 * qx) + a02 * qy) + a03 * qz), two * (((a01 * qw + d1 * qx) + a12 * qy) + a13 * qz),
                       two * (((a02 * qw + a12 * qx) + d2 * qy) + a23 * qz), two * (((a03 * qw + a13 * qx) + a23 * qy) + d3 * qz)], -1)
        l1 = lam[np.arange(n), top]
        co = []
        for i in range(4):
            dot = ((V[:, 0, i] * gq[:, 0] + V[:, 1, i] * gq[:, 1]) + V[:, 2, i] * gq[:, 2]) + V[:, 3, i] * gq[:, 3]
            co.append(np.where(top == i, zero, dot / (l1 - lam[:, i])))
        u = [((V[:, r, 0] * co[0] + V[:, r, 1] * co[1]) + V[:, r, 2] * co[2]) + V[:, r, 3] * co[3] for r in range(4)]
        qq = [qw, qx, qy, qz]
        D = [u[i] * qq[i] for i in range(4)]
        H = {(i, j): u[i] * qq[j] + u[j] * qq[i] for i in range(4) for j in range(i + 1, 4)}
        GS = np.zeros((n, 9), dtype)
        GS[:, 0], GS[:, 4], GS[:, 8] = ((D[0] + D[1]) - D[2]) - D[3], ((D[0] - D[1]) + D[2]) - D[3], ((D[0] - D[1]) - D[2]) + D[3]
        GS[:, 5], GS[:, 7] = H[2, 3] + H[0, 1], H[2, 3] - H[0, 1]
        GS[:, 6], GS[:, 2] = H[1, 3] + H[0, 2], H[1, 3] - H[0, 2]
        GS[:, 1], GS[:, 3] = H[1, 2] + H[0, 3], H[1, 2] - H[0, 3]
        GM = (Gs[:, None] * R) / vx[:, None] + GS.reshape(n, 3, 3).transpose(0, 2, 1).reshape(n, 9)
        cs = -(s[:, None] * _rot_t(R, Gt))
        # the last pass
        gx = s[:, None, None] * _rot_t(R, ga)
        gy = np.where(L, zero - c2 * d, zero)
        xt, yt = x - cx[:, None], y - cy[:, None]
        share = (w / F["W"][:, None])[..., None]
        my = _rot_t(GM, yt)
        mx = _rot(GM, xt)
        wx = w[..., None]
        full_x = (gx + wx * (my + g2[:, None, None] * xt)) + share * cs[:, None]
        full_y = (gy + wx * mx) + share * Gt[:, None]
        whole = ((F["status"] == 0)[:, None] & live)[..., None]
        gx = np.where(whole, full_x, gx).astype(dtype)
        gy = np.where(whole, full_y, gy).astype(dtype)
        out = []
        for g, into in ((gx, grad_source), (gy, grad_target)):
            if into is None:
                out.append(None)
            else:
                into = np.asarray(into, dtype)
                out.append(np.ascontiguousarray(into + g if accumulate else g, dtype))
    return tuple(out)


def apply(transform, points):
    """s (R x) + t in the arithmetic of `points`' dtype, by the order of the rule."""
    tr = np.asarray(transform, points.dtype)
    return tr[:, None, 12:13] * _rot(np.ascontiguousarray(tr[:, :9]), points) + tr[:, None, 9:12]


# ---------------------------------------------------------------------------------------------------- the definition
def definition_t(source, target, weight=None, with_scale=False):
    """Weighted Kabsch / Umeyama in torch (differentiable): (R [n,3,3], t [n,3], s [n], aligned [n,K,3], energy [n]).  A weight of 0
    leaves a point out of the fit; every point is moved."""
    import torch

    n, K = source.shape[:2]
    y = target.expand(n, K, 3) if target.dim() == 3 else target.expand(n, K, 3)
    w = torch.ones(n, K, dtype=source.dtype) if weight is None else torch.as_tensor(weight, dtype=source.dtype).reshape(-1, K).expand(n, K)
    W = w.sum(1)
    cx = (w[..., None] * source).sum(1) / W[:, None]
    cy = (w[..., None] * y).sum(1) / W[:, None]
    xt, yt = source - cx[:, None], y - cy[:, None]
    C = torch.einsum("nk,nka,nkb->nab", w, yt, xt)  # sum w y~ x~^T
    U, sig, Vh = torch.linalg.svd(C)
    det = torch.det(U @ Vh)
    fix = torch.ones(n, 3, dtype=source.dtype)
    fix[:, 2] = torch.where(det < 0, -1.0, 1.0).to(source.dtype)
    R = U @ torch.diag_embed(fix) @ Vh
    if with_scale:
        s = (sig * fix).sum(1) / (w * (xt * xt).sum(-1)).sum(1)
    else:
        s = torch.ones(n, dtype=source.dtype)
    t = cy - s[:, None] * torch.einsum("nab,nb->na", R, cx)
    aligned = s[:, None, None] * torch.einsum("nab,nkb->nka", R, source) + t[:, None]
    energy = (w * ((aligned - y) ** 2).sum(-1)).sum(1)
    return R, t, s, aligned, energy


def float64_gap(source, target, weight=None):
    """The gap of every frame in float64 (the tests assert it, so that no frame near a degenerate rotation is compared)."""
    return frame(source, target, weight, False, 0.0, np.float64)["gap"]


# ---------------------------------------------------------------------------------------------------- cases
def random_case(n, K, seed, mirrored=False, coplanar=False, noise=0.05, scale=1.0, dtype=np.float32, shared=False):
    """source [n,K,3] and target = scale Q source + move + noise, Q a random rotation (a reflection when `mirrored`).  `shared`: the two
    change roles and every frame starts from the same set, so that the target's first frame serves all of them."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 0.4, (n, K, 3)) * np.array([1.0, 0.6, 0.3]) + rng.normal(0, 0.5, (n, 1, 3))
    if shared:
        x[:] = x[0]
    if coplanar:
        x[..., 2] = 0.3
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    Q = Q * np.sign(np.linalg.det(Q))[:, None, None]
    if mirrored:
        Q[:, :, 0] = -Q[:, :, 0]
    y = scale * np.einsum("nab,nkb->nka", Q, x) + rng.normal(0, 0.5, (n, 1, 3)) + rng.normal(0, noise, (n, K, 3))
    return (y.astype(dtype), x.astype(dtype)) if shared else (x.astype(dtype), y.astype(dtype))


def special_points(x, y, w, seed):
    """Points that are not live, spread over the case in place (w [Wn,K] may be None: then only coordinates are spoilt): a NaN and an
    infinite coordinate on either side, and weights that are 0, negative, NaN and infinite.  Needs K >= 16."""
    n, K = x.shape[:2]
    at = (np.arange(8) * 5 + seed) % K
    f = seed % n
    x[f, at[0], seed % 3] = np.nan
    y[f % y.shape[0], at[1], (seed + 1) % 3] = np.inf
    x[-1, at[2], 0] = -np.inf
    y[-1, at[3], 2] = np.nan
    if w is not None:
        w[0, at[4]], w[-1, at[5]], w[0, at[6]], w[-1, at[7]] = 0.0, -1.0, np.nan, np.inf
        w[:, 2::9] = 0.0


# ---------------------------------------------------------------------------------------------------- the chain and the fit
def chain_case(model):
    """theta, beta -> FK -> the 53 landmarks -> similarity alignment onto fixed noisy targets -> energy, n = 2."""
    import image_oracle as IM

    rng = np.random.default_rng(77)
    n = 2
    beta = rng.normal(0, 1, (n, 10)).astype(np.float32)
    theta = np.zeros((n, 25, 3), np.float32)
    theta[:, 1:] = rng.normal(0, 0.2, (n, 24, 3))
    reg, dense = IM.regressor(model)
    beta0, theta0 = beta + rng.normal(0, 0.3, beta.shape), theta.copy()
    theta0[:, 1:] += rng.normal(0, 0.1, (n, 24, 3))
    import torch
    with torch.no_grad():
        lm = IM.landmarks64(model, dense, beta0.astype(np.float32), theta0.astype(np.float32)).numpy()
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    Q = Q * np.sign(np.linalg.det(Q))[:, None, None]
    target = 1.2 * np.einsum("nab,nkb->nka", Q, lm) + rng.normal(0, 0.3, (n, 1, 3)) + rng.normal(0, 0.01, lm.shape)
    weight = rng.uniform(0.5, 2.0, (n, lm.shape[1])).astype(np.float32)
    return dict(beta=beta, theta=theta, reg=reg, dense=dense, target=target.astype(np.float32), weight=weight)


ICP_STEPS, ICP_POINTS, ICP_NOISE, ICP_ANGLE, ICP_MOVE = 10, 2000, 0.002, 25.0, 0.2


def icp_case(verts):
    """verts [n,V,3] float64 posed vertices -> the cloud [n,2000,3] float32: 2000 of them with 2 mm Gaussian noise, turned by 25 degrees
    about a fixed axis through the body's centroid and moved 0.2 m."""
    rng = np.random.default_rng(91)
    n, V = verts.shape[:2]
    pick = np.stack([rng.choice(V, ICP_POINTS, replace=False) for _ in range(n)])
    cloud = verts[np.arange(n)[:, None], pick] + rng.normal(0, ICP_NOISE, (n, ICP_POINTS, 3))
    axis = np.array([0.3, 0.9, 0.316])
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(ICP_ANGLE)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rm = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    c = verts.mean(1, keepdims=True)
    move = ICP_MOVE * np.array([0.6, 0.0, 0.8])
    return ((cloud - c) @ Rm.T + c + move).astype(np.float32)


def nearest(verts, cloud):
    """For each vertex the nearest cloud point: (index [n,V], sqdist [n,V]), the lowest index on ties, in the arrays' dtype."""
    idx, sq = [], []
    for v, p in zip(verts, cloud):
        i = np.empty(len(v), np.int64)
        s = np.empty(len(v), v.dtype)
        for lo in range(0, len(v), 512):
            d = v[lo:lo + 512, None] - p[None]
            dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            i[lo:lo + 512] = dd.argmin(1)
            s[lo:lo + 512] = dd.min(1)
        idx.append(i), sq.append(s)
    return np.stack(idx), np.stack(sq)


def icp_float64(verts, cloud):
    """The ICP schedule in float64: RMS [n, ICP_STEPS + 1] of the vertex-to-cloud distance before each step and after the last."""
    cloud = cloud.astype(np.float64)
    n = len(verts)
    rms = []
    for _ in range(ICP_STEPS):
        idx, sq = nearest(verts, cloud)
        rms.append(np.sqrt(sq.mean(1)))
        tr = align(cloud[np.arange(n)[:, None], idx], verts, None, False, dtype=np.float64)[0]
        cloud = apply(tr, cloud)
    rms.append(np.sqrt(nearest(verts, cloud)[1].mean(1)))
    return np.stack(rms, 1)
