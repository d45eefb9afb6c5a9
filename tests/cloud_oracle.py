"""The scan-preparation rules of include/smplpp_hip.h (smplpp_cloud_knn, smplpp_cloud_normals, smplpp_cloud_farthest_points) restated in
numpy float32, operation by operation: every product, sum, quotient and square root below is one float32 operation on float32 arrays, in
the order the header writes them, so the GPU tests compare bits.  Also the definitions the CPU tests hold the restatement to (float64
brute force, a plain Python loop, float64 eigh), and the clouds both test files use."""
import numpy as np

f32 = np.float32
INF = f32(np.inf)
SWEEPS = 4


def sqdist(a, b):
    """((dx dx + dy dy) + dz dz) of float32 arrays [...,3], broadcast."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    with np.errstate(all="ignore"):
        dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
        return (dx * dx + dy * dy) + dz * dz


# ---------------------------------------------------------------------------------------------------- k nearest neighbours
def knn(points, k, queries=None, max_sqdist=np.inf):
    """(index [n,Q,k] int32, sqdist [n,Q,k] float32, count [n,Q] int32) by the rule."""
    points = np.asarray(points, f32)
    self_query = queries is None
    queries = points if self_query else np.asarray(queries, f32)
    n, K, Q = points.shape[0], points.shape[1], queries.shape[1]
    index = np.full((n, Q, k), -1, np.int32)
    dist = np.zeros((n, Q, k), f32)
    count = np.zeros((n, Q), np.int32)
    cap = f32(max_sqdist)
    for f in range(n):
        d = sqdist(queries[f][:, None, :], points[f][None, :, :]) if K else np.zeros((Q, 0), f32)
        with np.errstate(all="ignore"):
            listed = np.isfinite(d) & (d <= cap)
        if self_query:
            listed[np.arange(Q), np.arange(K)] = False
        key = np.where(listed, d, INF)
        order = np.argsort(key, axis=1, kind="stable")[:, :k]  # stable: equal distances stay in ascending index, the order (d, j)
        got = np.take_along_axis(listed, order, 1)
        kk = order.shape[1]
        index[f, :, :kk] = np.where(got, order, -1)
        dist[f, :, :kk] = np.where(got, np.take_along_axis(d, order, 1), f32(0))
        count[f] = got.sum(1)
    return index, dist, count


def knn_definition(points, k, queries=None):
    """Float64 brute force: for every query the candidates in a stable argsort of the float64 distances.  Returns (index [n,Q,kk] int64,
    sorted float64 distances [n,Q,K or K-1]) with kk = min(k, candidates)."""
    p = np.asarray(points, np.float64)
    q = p if queries is None else np.asarray(queries, np.float64)
    out_i, out_d = [], []
    for f in range(p.shape[0]):
        d = ((q[f][:, None, :] - p[f][None, :, :]) ** 2).sum(-1)
        if queries is None:
            d[np.arange(d.shape[0]), np.arange(d.shape[0])] = np.inf
        order = np.argsort(d, axis=1, kind="stable")
        cand = d.shape[1] - (1 if queries is None else 0)
        out_i.append(order[:, :min(k, cand)])
        out_d.append(np.take_along_axis(d, order, 1)[:, :cand])
    return np.stack(out_i), np.stack(out_d)


# ---------------------------------------------------------------------------------------------------- normals
def _rotate(A, V, p, q, live):
    """One Jacobi rotation on the pair (p, q) of every matrix of A [m,3,3] (kept whole), accumulated into V; `live` rows only."""
    one = f32(1)
    apq = A[:, p, q].copy()
    do = live & (apq != 0)
    safe = np.where(do, apq, one)
    tau = (A[:, q, q] - A[:, p, p]) / (f32(2) * safe)
    t = np.where(tau < 0, f32(-1), one) / (np.abs(tau) + np.sqrt(tau * tau + one))
    c = one / np.sqrt(t * t + one)
    s = t * c
    h = t * safe
    N = A.copy()
    N[:, p, p] = A[:, p, p] - h
    N[:, q, q] = A[:, q, q] + h
    N[:, p, q] = N[:, q, p] = f32(0)
    r = 3 - p - q
    arp, arq = A[:, r, p], A[:, r, q]
    N[:, r, p] = N[:, p, r] = c * arp - s * arq
    N[:, r, q] = N[:, q, r] = s * arp + c * arq
    W = V.copy()
    W[:, :, p] = c[:, None] * V[:, :, p] - s[:, None] * V[:, :, q]
    W[:, :, q] = s[:, None] * V[:, :, p] + c[:, None] * V[:, :, q]
    A[do], V[do] = N[do], W[do]


def eigen3(C, sweeps=SWEEPS):
    """The rule's steps 3 and 4 on C [m,3,3] float32: (lam [m,3] ascending by (value, column), col [m,3] their columns, V [m,3,3])."""
    A, m = np.array(C, f32), len(C)
    V = np.broadcast_to(np.eye(3, dtype=f32), (m, 3, 3)).copy()
    live = np.ones(m, bool)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                _rotate(A, V, p, q, live)
        lam = np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], 1)
        col = np.broadcast_to(np.arange(3), (m, 3)).copy()
        for a, b in ((0, 1), (1, 2), (0, 1)):
            sw = lam[:, b] < lam[:, a]
            lam[sw, a], lam[sw, b] = lam[sw, b], lam[sw, a]
            col[sw, a], col[sw, b] = col[sw, b], col[sw, a]
    return lam, col, V


def covariance(points, index):
    """Steps 1 and 2 for one frame: (C [K,3,3] float32, m [K])."""
    K, k = index.shape
    s = np.zeros((K, 3), f32)
    T = np.zeros((K, 3, 3), f32)
    m = np.ones(K, np.int64)
    with np.errstate(all="ignore"):
        for r in range(k):
            j = index[:, r]
            ok = (j >= 0) & (j < K)
            e = points[np.where(ok, j, 0)] - points
            ok &= np.isfinite(e).all(1)
            m += ok
            for a in range(3):
                s[:, a] = np.where(ok, s[:, a] + e[:, a], s[:, a])
                for b in range(a, 3):
                    T[:, a, b] = np.where(ok, T[:, a, b] + e[:, a] * e[:, b], T[:, a, b])
        mf = m.astype(f32)
        mean = s / mf[:, None]
        C = np.zeros((K, 3, 3), f32)
        for a in range(3):
            for b in range(a, 3):
                C[:, a, b] = C[:, b, a] = T[:, a, b] - mf * (mean[:, a] * mean[:, b])
    return C, m


def normals(points, index, viewpoint=None, min_gap=0.0, sweeps=SWEEPS):
    """(normal [n,K,3], curvature [n,K] float32, status [n,K] int32) by the rule; viewpoint None, [3], [1,3] or [n,3]."""
    points, index = np.asarray(points, f32), np.asarray(index)
    n, K, _ = points.shape
    vp = None if viewpoint is None else np.broadcast_to(np.asarray(viewpoint, f32).reshape(-1, 3), (n, 3))
    normal, curv, status = np.zeros((n, K, 3), f32), np.zeros((n, K), f32), np.zeros((n, K), np.int32)
    zero = f32(0)
    for f in range(n):
        P = points[f]
        C, m = covariance(P, index[f])
        lam, col, V = eigen3(C, sweeps)
        with np.errstate(all="ignore"):
            v = np.take_along_axis(V, col[:, None, :1].repeat(3, 1), 2)[:, :, 0]
            length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            nr = v / length[:, None]
            if vp is not None:
                c = vp[f]
                flip = ((nr[:, 0] * (c[0] - P[:, 0]) + nr[:, 1] * (c[1] - P[:, 1])) + nr[:, 2] * (c[2] - P[:, 2])) < 0
            else:
                big, mag = nr[:, 0].copy(), np.abs(nr[:, 0])
                for a in (1, 2):
                    more = np.abs(nr[:, a]) > mag
                    big, mag = np.where(more, nr[:, a], big), np.where(more, np.abs(nr[:, a]), mag)
                flip = big < 0
            nr = np.where(flip[:, None], -nr, nr)
            total = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
            cv = np.where(total > 0, lam[:, 0] / np.where(total > 0, total, f32(1)), zero)
            st = np.where((lam[:, 2] <= 0) | ((lam[:, 1] - lam[:, 0]) < f32(min_gap) * lam[:, 2]), 2, 0)
        dead = (m < 3) | ~np.isfinite(P).all(1)
        normal[f] = np.where(dead[:, None], zero, nr)
        curv[f] = np.where(dead, zero, cv)
        status[f] = np.where(dead, 1, st)
    return normal, curv, status


def normals_definition(points, index):
    """Float64 eigh of the mean-centred covariance of {p_i} + its listed neighbours, one frame: (normal [K,3], lam [K,3] ascending)."""
    P = np.asarray(points, np.float64)
    nb = np.concatenate([np.arange(len(P))[:, None], np.asarray(index, np.int64)], 1)
    X = P[nb]
    X = X - X.mean(1, keepdims=True)
    lam, vec = np.linalg.eigh(np.einsum("kma,kmb->kab", X, X))
    return vec[:, :, 0], lam


# ---------------------------------------------------------------------------------------------------- farthest points
def farthest_points(points, M, start=None, also=()):
    """(index [n,M] int32, radius_sq [n,M], min_sqdist [n,K] float32) by the rule.  With `also` (smaller M's) a dict {M: that triple}
    from the one run: the picks of a shorter run are a prefix, only min_sqdist differs."""
    points = np.asarray(points, f32)
    n, K, _ = points.shape
    index, radius = np.full((n, M), -1, np.int32), np.zeros((n, M), f32)
    cover = {m: np.zeros((n, K), f32) for m in tuple(also) + (M,)}
    for f in range(n):
        P = points[f]
        finite = np.isfinite(P).all(1)
        dmin = np.where(finite, INF, f32(-1))  # -1: not a candidate (chosen, or not finite)
        if not finite.any():
            continue
        s = 0 if start is None else int(start[f])
        cur = s if 0 <= s < K and finite[s] else int(np.argmax(finite))
        curd = INF
        for i in range(M):
            if cur >= 0:
                index[f, i], radius[f, i] = cur, curd
                d = sqdist(P, P[cur])
                with np.errstate(all="ignore"):
                    dmin = np.where((dmin >= 0) & (d < dmin), d, dmin)
                dmin[cur] = f32(-1)
                cur = int(np.argmax(dmin))  # the first of the largest: the lowest index on ties
                curd = dmin[cur]
                if curd < 0:
                    cur = -1
            if i + 1 in cover:
                cover[i + 1][f] = np.maximum(dmin, f32(0))
    if also:
        return {m: (index[:, :m], radius[:, :m], cover[m]) for m in cover}
    return index, radius, cover[M]


def farthest_points_loop(points, M, start=0):
    """One frame, a plain Python loop over float32 scalars: the definition the restatement is held to (finite points only)."""
    P = [tuple(f32(v) for v in p) for p in np.asarray(points, f32)]
    K = len(P)

    def dist(a, b):
        dx, dy, dz = a[0] - b[0], a[1] - b[1], a[2] - b[2]
        return f32(f32(f32(dx * dx) + f32(dy * dy)) + f32(dz * dz))

    dmin, chosen, picks, radii = [INF] * K, [False] * K, [], []
    cur, curd = start, INF
    for _ in range(M):
        picks.append(cur), radii.append(curd)
        chosen[cur] = True
        best, bestd = -1, f32(-1)
        for j in range(K):
            d = dist(P[j], P[cur])
            if d < dmin[j]:
                dmin[j] = d
            if not chosen[j] and dmin[j] > bestd:
                best, bestd = j, dmin[j]
        cur, curd = best, bestd
        if cur < 0:
            break
    picks += [-1] * (M - len(picks))
    radii += [f32(0)] * (M - len(radii))
    return np.array(picks, np.int32), np.array(radii, f32), np.array([f32(0) if chosen[j] else dmin[j] for j in range(K)], f32)


# ---------------------------------------------------------------------------------------------------- clouds
def random_cloud(n, K, seed, scale=1.0):
    return (np.random.default_rng(seed).normal(size=(n, K, 3)) * scale).astype(f32)


def lattice_cloud(n, K, seed):
    """Integer coordinates in 0..7: every float32 distance is exact, equal distances and duplicated points abound."""
    return np.random.default_rng(seed).integers(0, 8, (n, K, 3)).astype(f32)


def surface_samples(model, K, seed, noise=0.0, verts=None):
    """K area-weighted samples of the model's template surface (or of `verts` [V,3]): (points [K,3] float32, face [K], face normals [K,3]
    float64), with isotropic Gaussian noise of `noise` metres."""
    rng = np.random.default_rng(seed)
    v = np.asarray(model["vertices_template"] if verts is None else verts, np.float64)
    F = np.asarray(model["face_indices"], np.int64) - 1  # the model file is 1-based
    a, b, c = v[F[:, 0]], v[F[:, 1]], v[F[:, 2]]
    cr = np.cross(b - a, c - a)
    area = np.linalg.norm(cr, axis=1)
    face = rng.choice(len(F), K, p=area / area.sum())
    u, w = rng.random(K), rng.random(K)
    fl = u + w > 1
    u, w = np.where(fl, 1 - u, u), np.where(fl, 1 - w, w)
    pts = a[face] + u[:, None] * (b[face] - a[face]) + w[:, None] * (c[face] - a[face]) + rng.normal(size=(K, 3)) * noise
    return pts.astype(f32), face, cr[face] / np.maximum(area[face], 1e-300)[:, None]


def sphere_cloud(K, seed, radius=1.0):
    x = np.random.default_rng(seed).normal(size=(K, 3))
    return (radius * x / np.linalg.norm(x, axis=1, keepdims=True)).astype(f32)


def degenerate_neighbourhoods():
    """(points [1,10,3], index [1,10,3], {min_gap: status list}): collinear neighbourhoods (0, 1), lists too short (2, 3), planes of three
    points (4, 5, and 6 whose list names the NaN point 7, which is skipped), the NaN point itself, and a point whose neighbours all
    coincide with it (8: the covariance is zero, l2 = 0), next to a point without a list (9)."""
    p = np.zeros((1, 10, 3), f32)
    p[0, :5, 0] = np.arange(5)
    p[0, 5:8] = [[0, 1, 0], [0, 2, 1], [np.nan, 0, 0]]
    index = np.array([[[1, 2, 3], [0, 2, -1], [1, -1, -1], [-1, -1, -1], [0, 5, 6], [4, 6, 0], [7, 0, 5], [0, 1, 2], [0, 9, -1], [-1, -1, -1]]],
                     np.int32)
    return p, index, {0.0: [0, 0, 1, 1, 0, 0, 0, 1, 2, 1], 0.01: [2, 2, 1, 1, 0, 0, 0, 1, 2, 1], 10.0: [2, 2, 1, 1, 2, 2, 2, 1, 2, 1]}


def single_view_scan(model, verts, camera, K, seed, noise=0.003, cos_incidence=0.26):
    """A depth sensor's view of one posed body, without normals: K surface samples of verts [V,3] on faces that look at `camera` [3] at
    no more than 75 degrees of incidence (cos > 0.26: a sensor returns nothing at grazing angles), with isotropic noise.  Returns (points
    [K,3] float32, the sampled faces' unit normals [K,3] float64)."""
    p, _, nrm = surface_samples(model, 4 * K, seed, noise, verts=verts)
    view = np.asarray(camera, np.float64) - p
    view /= np.linalg.norm(view, axis=1, keepdims=True)
    front = np.nonzero((nrm * view).sum(1) > cos_incidence)[0][:K]
    assert len(front) == K
    return np.ascontiguousarray(p[front]), nrm[front]
