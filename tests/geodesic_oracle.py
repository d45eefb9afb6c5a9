"""The rules of smplpp_mesh_geodesic and of the self-contact handle and search (include/smplpp_hip.h, smplpp_amd/csrc/edge_tables.h)
restated in numpy float32 for the tests: the edge table, the edge lengths, the distance field twice over (a Dijkstra with fp32 adds and
a synchronous pull relaxation, which must agree to the bit), the far mask by the min-index rule, and the masked search.  numpy's
float32 operations round one at a time, as the rule asks; nothing here is fused.  Also the small meshes the tests run on."""
from __future__ import annotations

import heapq

import numpy as np

F32 = np.float32
INF = F32(np.inf)


# ---------------------------------------------------------------- meshes: (verts [V,3] float32, faces [F,3] int64, 0-based)
def icosphere(level, radius=1.0, center=(0.0, 0.0, 0.0)):
    """V = 12, 42, 162, 642 at levels 0..3."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.asarray(v) * radius + np.asarray(center)).astype(F32), np.asarray(f, np.int64)


def torus(a, b, R=1.0, r=0.35):
    """A triangulated a x b torus grid: V = a b, F = 2 a b."""
    i, j = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    u, w = 2 * np.pi * i / a, 2 * np.pi * j / b
    verts = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], -1).reshape(-1, 3)
    idx = lambda p, q: (p % a) * b + (q % b)  # noqa: E731
    faces = []
    for p in range(a):
        for q in range(b):
            faces += [(idx(p, q), idx(p + 1, q), idx(p + 1, q + 1)), (idx(p, q), idx(p + 1, q + 1), idx(p, q + 1))]
    return verts.astype(F32), np.asarray(faces, np.int64)


def two_spheres(level=1):
    """Two disjoint icospheres: no path from one to the other."""
    v0, f0 = icosphere(level)
    v1, f1 = icosphere(level, 0.5, (3.0, 0.0, 0.0))
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)])


def fan(k=5):
    """k triangles around one shared edge (0, 1): non-manifold."""
    ang = 2 * np.pi * np.arange(k) / k
    verts = np.concatenate([[[0, 0, 0], [0, 0, 1]], np.stack([np.cos(ang), np.sin(ang), 0.5 + 0 * ang], -1)])
    return verts.astype(F32), np.asarray([(0, 1, 2 + i) for i in range(k)], np.int64)


def model_faces(faces0):
    """faces as tiny_model(V, faces=...) takes them: 1-based."""
    return np.asarray(faces0, np.int64) + 1


# ---------------------------------------------------------------- edge table
def edge_table(V, faces0):
    """(off [V+1] int32, adj [nnz] int32): the undirected edges as a per-vertex CSR, neighbours ascending, each once, no self-edges."""
    f = np.asarray(faces0, np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    b = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    keep = a != b
    a, b = a[keep], b[keep]
    pairs = np.unique(np.stack([np.concatenate([a, b]), np.concatenate([b, a])], 1), axis=0) if len(a) else np.zeros((0, 2), np.int64)
    off = np.zeros(V + 1, np.int64)
    np.add.at(off, pairs[:, 0] + 1, 1)
    return np.cumsum(off).astype(np.int32), pairs[:, 1].astype(np.int32)


def edge_rows(off):
    return np.repeat(np.arange(len(off) - 1), np.diff(off)).astype(np.int64)


def edge_weights(verts, off, adj):
    """The length of every directed edge of one frame verts [V,3], float32: sqrt((dx dx + dy dy) + dz dz), d = x_hi - x_lo; a length
    that is not finite is +inf (the edge does not exist)."""
    x = np.asarray(verts, F32)
    u, v = edge_rows(off), adj.astype(np.int64)
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    with np.errstate(all="ignore"):
        d = x[hi] - x[lo]
        w = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert w.dtype == F32
    return np.where(np.isfinite(w), w, INF).astype(F32)


# ---------------------------------------------------------------- the field, twice
def threshold(dist, max_dist):
    return dist if max_dist is None else np.where(dist > F32(max_dist), INF, dist).astype(F32)


def dijkstra(V, off, adj, w, sources, max_dist=None, dtype=F32):
    """Label-setting with `dtype` adds (valid because fl(a + w) is monotone in a and never below a).  Returns (dist [V], hops [V]):
    hops is the edge count of the path that set the value (-1: unreachable)."""
    dist = np.full(V, np.inf, dtype)
    hops = np.full(V, -1, np.int64)
    heap = []
    for s in sources:
        if 0 <= s < V and dist[s] != 0:
            dist[s], hops[s] = 0, 0
            heap.append((0.0, int(s)))
    heapq.heapify(heap)
    wl, al, ol = [float(x) for x in w], adj.tolist(), off.tolist()
    done = np.zeros(V, bool)
    while heap:
        d, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        for e in range(ol[u], ol[u + 1]):
            # (the float64 sum of two float32 rounded to float32 is the float32 sum: double rounding is innocuous for +)
            nd = float(dtype(d + wl[e]))
            v = al[e]
            if nd < dist[v]:
                dist[v], hops[v] = nd, hops[u] + 1
                heapq.heappush(heap, (nd, v))
    return threshold(dist, max_dist) if dtype is F32 else dist, hops


def padded(off, adj, w):
    """(nbr [V,D], wt [V,D]): the CSR as a rectangle; a missing slot is the vertex itself at +inf."""
    V = len(off) - 1
    deg = np.diff(off)
    D = max(int(deg.max()) if V else 0, 1)
    nbr = np.repeat(np.arange(V)[:, None], D, 1)
    wt = np.full((V, D), INF, F32)
    rows = edge_rows(off)
    slot = np.arange(len(adj)) - off[:-1].astype(np.int64)[rows]
    nbr[rows, slot] = adj
    wt[rows, slot] = w
    return nbr, wt


def relax(V, off, adj, w, source_sets, max_dist=None):
    """Synchronous pull relaxation of all the sets at once: dist [S,V] and the number of sweeps that changed a value, plus one."""
    nbr, wt = padded(off, adj, w)
    D = np.full((len(source_sets), V), INF, F32)
    for s, srcs in enumerate(source_sets):
        for q in srcs:
            if 0 <= q < V:
                D[s, q] = 0
    sweeps = 0
    while True:
        sweeps += 1
        with np.errstate(invalid="ignore"):
            cand = (D[:, nbr] + wt[None]).min(axis=2)
        new = np.minimum(D, cand)
        if np.array_equal(new, D):
            break
        D = new
    return threshold(D, max_dist), sweeps


# ---------------------------------------------------------------- the far mask
def words(V):
    return (V + 31) // 32


def pack_bits(far):
    """bool [R,V] -> uint32 [R,W]: bit (u & 31) of word (u >> 5)."""
    R, V = far.shape
    pad = np.zeros((R, words(V) * 32), np.uint8)
    pad[:, :V] = far
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint32).reshape(R, words(V))


def unpack_bits(mask, V):
    m = np.ascontiguousarray(mask, np.uint32)
    return np.unpackbits(m.view(np.uint8), axis=1, bitorder="little")[:, :V].astype(bool)


def single_source_fields(rest, faces0, sources=None, batch=256):
    """dist [len(sources), V]: the field of every listed single source (None: every vertex) on the mesh `rest`."""
    V = len(rest)
    off, adj = edge_table(V, faces0)
    w = edge_weights(rest, off, adj)
    src = np.arange(V) if sources is None else np.asarray(sources, np.int64)
    return np.concatenate([relax(V, off, adj, w, [[int(s)] for s in src[b0:b0 + batch]])[0] for b0 in range(0, len(src), batch)])


def far_matrix(rest, faces0, geo_min, sources=None, fields=None):
    """far [V,V] bool by the min-index rule: far(v, u) = far(u, v) = field of source min(v, u) read at max(v, u) > geo_min, far(v, v) =
    0.  With `sources` (ascending ids) only the entries whose min(v, u) is a listed source are meaningful; returns (far, known).
    `fields`: single_source_fields of the same arguments, computed before."""
    V = len(rest)
    src = np.arange(V) if sources is None else np.asarray(sources, np.int64)
    D = single_source_fields(rest, faces0, sources) if fields is None else fields
    far = np.zeros((V, V), bool)
    known = np.zeros((V, V), bool)
    for r, s in enumerate(src):
        up = np.arange(V) > s
        far[s, up] = D[r, up] > F32(geo_min)
        far[up, s] = far[s, up]
        known[s, up] = known[up, s] = True
    return far, known


def far_mask(rest, faces0, geo_min):
    """(mask [V,W] uint32, far_pairs)."""
    far, _ = far_matrix(rest, faces0, geo_min)
    return pack_bits(far), int(far.sum()) // 2


# ---------------------------------------------------------------- the search, the mask an input
def compat_dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def search(verts, mask, normals=None, cos_min=0.0, max_sq=np.inf, block=512):
    """One frame: (index [V] int64, sqdist [V] float32).  Candidate u of v: far(v, u), d = ((dx dx + dy dy) + dz dz) finite and <=
    max_sq, and with normals  s <= 0 && mm qq > 0 && s s >= (cos_min cos_min)(mm qq).  The smallest d, then the lowest u."""
    x = np.asarray(verts, F32)
    V = len(x)
    far = unpack_bits(mask, V)
    index = np.full(V, -1, np.int64)
    sq = np.zeros(V, F32)
    c2 = F32(cos_min) * F32(cos_min)
    if normals is not None:
        nn = np.asarray(normals, F32).copy()
        nn[~np.isfinite(nn).all(1)] = np.nan
        with np.errstate(all="ignore"):
            nl = compat_dot(nn, nn)
    with np.errstate(all="ignore"):
        for b0 in range(0, V, block):
            q = x[b0:b0 + block, None, :]
            dx, dy, dz = q[..., 0] - x[None, :, 0], q[..., 1] - x[None, :, 1], q[..., 2] - x[None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            ok = far[b0:b0 + block] & np.isfinite(d) & (d <= F32(max_sq))
            if normals is not None:
                m = nn[b0:b0 + block, None, :]
                s = (m[..., 0] * nn[None, :, 0] + m[..., 1] * nn[None, :, 1]) + m[..., 2] * nn[None, :, 2]
                l = nl[b0:b0 + block, None] * nl[None, :]
                ok &= (s <= 0) & (l > 0) & (s * s >= c2 * l)
            dm = np.where(ok, d, INF)
            k = dm.argmin(1)  # (the first minimum: the lowest u)
            hit = ok[np.arange(len(k)), k]
            index[b0:b0 + block] = np.where(hit, k, -1)
            sq[b0:b0 + block] = np.where(hit, dm[np.arange(len(k)), k], F32(0))
    return index, sq
