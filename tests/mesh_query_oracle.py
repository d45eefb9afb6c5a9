"""Plain numpy statements of the forward mesh queries (smplpp_amd/csrc/mesh.hip, mesh_device.h): face normals, vertex normals with
uniform 1/deg weights over the ascending adjacent faces, their condition numbers, and the sweep grid's extents.  No torch, no GPU.
float64 is the reference; float32 is "the same graph in fp32", the yardstick of the bar."""
import numpy as np

EPS32 = 2.0 ** -24
GRID_SCALE = np.float32(0.025)


def adjacency(faces, V):
    """CSR adjacency of faces [F,3] (0-based): (off [V+1], face [3F] ascending per vertex, weight [3F] = float32(1)/float32(deg))."""
    faces = np.asarray(faces, np.int64)
    F = len(faces)
    vert = faces.reshape(-1)
    fid = np.repeat(np.arange(F, dtype=np.int64), 3)
    order = np.lexsort((fid, vert))
    deg = np.bincount(vert, minlength=V)
    off = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    w = np.float32(1) / np.repeat(deg, deg).astype(np.float32)
    return off, fid[order], w.astype(np.float32)


def _normalize(x, dtype):
    nrm = np.sqrt((x * x).sum(-1, keepdims=True, dtype=dtype))
    return x / np.maximum(nrm, dtype(1e-12))


def _edges(verts, faces, dtype):
    v = np.asarray(verts, dtype)
    tri = v[..., np.asarray(faces, np.int64), :]  # [..., F, 3, 3]
    return tri[..., 1, :] - tri[..., 0, :], tri[..., 2, :] - tri[..., 0, :]


def face_normals(verts, faces, ids=None, dtype=np.float64):
    """verts [..., V, 3], faces [F,3] 0-based -> normalize(cross(v1 - v0, v2 - v0)) at `ids` (all faces when None),
    normalize = x / max(||x||, 1e-12)."""
    f = np.asarray(faces, np.int64)
    if ids is not None:
        f = f[np.asarray(ids, np.int64)]
    a, b = _edges(verts, f, dtype)
    out = _normalize(np.cross(a, b), dtype)
    assert out.dtype == dtype
    return out


def _star_sum(adj, per_face, dtype):
    """per_face [..., F, k] -> [..., V, k]: for every vertex the sum over its adjacent faces, one term at a time in ascending face
    id (np.add.at adds unbuffered, in order, in `dtype`), as the kernel's loop does."""
    off, fid, _ = adj
    V = len(off) - 1
    row = np.repeat(np.arange(V), np.diff(off))
    lead = per_face.shape[:-2]
    x = per_face.reshape((-1,) + per_face.shape[-2:])
    out = np.zeros((len(x), V, x.shape[-1]), dtype)
    for b in range(len(x)):
        np.add.at(out[b], row, x[b][fid])
    return out.reshape(lead + out.shape[1:])


def vertex_normals(verts, faces, adj, ids=None, dtype=np.float64):
    """normalize(sum over the adjacent faces of (1/deg).n_f) at vertex `ids` (all when None); a vertex in no face gives zeros."""
    off = adj[0]
    fn = face_normals(verts, faces, None, dtype)  # [..., F, 3]
    deg = np.diff(off)
    w = dtype(1) / np.maximum(deg, 1).astype(dtype)  # per vertex
    # w * n_f per (vertex, adjacent face): scale the face normal by the weight of the vertex it is added to
    V = len(off) - 1
    row = np.repeat(np.arange(V), deg)
    lead = fn.shape[:-2]
    x = fn.reshape((-1,) + fn.shape[-2:])
    acc = np.zeros((len(x), V, 3), dtype)
    for b in range(len(x)):
        np.add.at(acc[b], row, w[row][:, None] * x[b][adj[1]])
    out = _normalize(acc.reshape(lead + (V, 3)), dtype)
    assert out.dtype == dtype
    return out if ids is None else out[..., np.asarray(ids, np.int64), :]


def face_condition(verts, faces):
    """kappa_f = ||a|| ||b|| / ||a x b|| per face, in float64 (inf for a degenerate face)."""
    a, b = _edges(verts, faces, np.float64)
    num = np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1)
    den = np.linalg.norm(np.cross(a, b), axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.inf)


def vertex_condition(verts, faces, adj):
    """kappa_v = (sum kappa_f / deg) / ||sum n_f / deg|| per vertex, in float64.  An exactly degenerate face adds 0 to the numerator:
    its normal is exactly 0 in every precision, so it carries no rounding error into the sum.  inf where the sum of normals is 0."""
    deg = np.maximum(np.diff(adj[0]), 1)
    kf = face_condition(verts, faces)
    kf = np.where(np.isfinite(kf), kf, 0.0)
    num = _star_sum(adj, kf[..., None], np.float64)[..., 0] / deg
    den = np.linalg.norm(_star_sum(adj, face_normals(verts, faces, None, np.float64), np.float64), axis=-1) / deg
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / den, np.inf)


def dead_faces(verts, faces):
    """[..., F] bool: the exactly degenerate faces.  Their normal is exactly (0,0,0) in every precision."""
    return ~np.isfinite(face_condition(verts, faces))


def dead_vertices(verts, faces, adj):
    """[..., V] bool: the vertices whose every adjacent face is exactly degenerate (or that sit in no face).  Their normal is
    exactly (0,0,0) in every precision."""
    live = (~dead_faces(verts, faces)).astype(np.float64)
    return _star_sum(adj, live[..., None], np.float64)[..., 0] == 0


def scaled_error(x, ref64, kappa, exact):
    """max_i |x_i - ref_i| / kappa_i over ALL elements; kappa [...] scales the three components of its row.  Every value is
    finite.  The rows of `exact` (dead_faces / dead_vertices) must EQUAL the reference; any other row of infinite kappa (a vertex
    whose live face normals cancel exactly in float64) has no definite direction and is held to nothing but finiteness."""
    x, ref64, kappa = np.asarray(x, np.float64), np.asarray(ref64, np.float64), np.asarray(kappa, np.float64)
    err = np.abs(x - ref64)
    assert np.isfinite(err).all(), "non-finite value"
    assert (err[exact] == 0).all(), "a degenerate row differs from its exact zero by %g" % err[exact].max()
    return float((err / kappa[..., None])[~exact].max())


def bar(e32, factor=4):
    return max(factor * e32, factor * EPS32)


def grid_extents(verts):
    """(grid_min [3], grid_num [3]) int32 of one frame's vertices [V,3], in float32 arithmetic: floor(min / float32(0.025)),
    ceil(max / float32(0.025)), count = hi - lo + 1."""
    v = np.asarray(verts, np.float32)
    lo = np.floor(v.min(axis=0) / GRID_SCALE).astype(np.int32)
    hi = np.ceil(v.max(axis=0) / GRID_SCALE).astype(np.int32)
    return lo, hi - lo + 1


# ---- models and cases of tests/test_mesh_queries_gpu.py (shared with tests/test_stage_oracle_cpu.py)
FANS = (18, 70, 128, 129)
LIST_LENGTHS = (1, 127, 128, 129)


def double_fan_model(N):
    """Closed double cone (the construction of tests/test_ik_gpu.py::_double_fan_model): apex 0 and bottom centre N + 1 each meet N
    faces (valence N), the N ring vertices 4; F = 2N."""
    from smplpp_amd import model_io

    top = [(0, 1 + i, 1 + (i + 1) % N) for i in range(N)]
    bottom = [(N + 1, 1 + (i + 1) % N, 1 + i) for i in range(N)]
    faces = np.array(top + bottom, np.int64) + 1
    md = model_io.tiny_model(N + 2, seed=3, faces=faces)
    ang = 2 * np.pi * np.arange(N) / N
    vt = md["vertices_template"].copy()
    vt[0] = (0, 0, 0.25)
    vt[1:N + 1] = np.stack([0.3 * np.cos(ang), 0.3 * np.sin(ang), 0.02 * np.cos(3 * ang)], axis=1)
    vt[N + 1] = (0, 0, -0.2)
    md["vertices_template"] = vt.astype(np.float32)
    return md


def faces0(model):
    return np.asarray(model["face_indices"], np.int64) - 1


def posed_inputs():
    """beta [3,10], theta [3,25,3] of every model's posed vertices: n = 3, theta scaled by 0.5 (frame 1 is the zero pose)."""
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(3, seed=9)
    theta[:, 1:] *= 0.5
    return beta, theta


CORNER_PAIRS = ((0, 1), (0, 2), (1, 2))  # (kept corner, moved corner) of the collapsed face: a = 0, b = 0, a = b


def collapse_face(verts, faces, f, pair):
    """verts [n,V,3] with corner pair[1] of face f moved onto corner pair[0] in every frame: face f (and whichever face shares
    that edge) is exactly degenerate."""
    v = np.array(verts, np.float32)
    v[:, faces[f, pair[1]]] = v[:, faces[f, pair[0]]]
    return v


def collapse_vertex_star(verts, faces, vertex):
    """verts [n,V,3] with every neighbour of `vertex` moved onto it: every face around it is exactly degenerate."""
    v = np.array(verts, np.float32)
    ring = np.unique(faces[(faces == vertex).any(axis=1)])
    v[:, ring] = v[:, vertex:vertex + 1]
    return v


def degenerate_targets(model_faces, V):
    """(face to collapse, vertex whose star collapses) for a model: a face and a vertex in the middle of the id range."""
    return len(model_faces) // 2, V // 2


def id_lists(count, seed):
    """The id lists of the normals tests over `count` ids: ALL ids shuffled with the first and last id repeated, and lists of
    length 1, 127, 128 and 129 (drawn with replacement, so any count serves)."""
    rng = np.random.default_rng(seed)
    lists = [np.concatenate([rng.permutation(count), [0, count - 1]]).astype(np.int64)]
    lists += [rng.integers(0, count, k).astype(np.int64) for k in LIST_LENGTHS]
    return lists


def bounds_vertices(V, variant):
    """Vertices [V,3] float32 for the bounds tests: interior everywhere, each axis' minimum at vertex V - 1 and maximum at vertex
    min(1024, V - 1): at V = 2500 the last vertex of the last pass and the first lane of the second pass of bounds_kernel's
    1024-thread loop.  For V <= 1025 those are one vertex, which cannot hold both extremes of an axis: the maximum then sits at
    vertex V - 2 (at V = 1025 the last lane of the first pass, the minimum in the first lane of the second).
    variant: 'plain', 'negative' (all coordinates < 0) or 'on_grid' (extremes exactly on k * float32(0.025))."""
    rng = np.random.default_rng(5000 + V)
    v = rng.uniform(-0.3, 0.3, (V, 3)).astype(np.float32)
    imin, imax = V - 1, min(1024, V - 1)
    lo, hi = np.float32(-0.4371), np.float32(0.4129)
    if variant == "on_grid":
        lo, hi = np.float32(-17) * GRID_SCALE, np.float32(16) * GRID_SCALE
    if imin == imax:
        imax = V - 2
    v[imin] = lo
    v[imax] = hi
    if variant == "negative":
        v = (v - np.float32(1.0)).astype(np.float32)
    return v
