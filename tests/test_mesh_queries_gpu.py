"""The forward mesh queries (smplpp_face_normals / _vertex_normals / _mesh_vertex_normals / _sweep_grid / _closest_points and the
adjacency getter; csrc/mesh.hip, mesh_device.h) against the float64 statement of each (tests/mesh_query_oracle.py), every element,
on six meshes: the synthetic body, a random 61-vertex model and closed double-cone fans whose apex has 18, 70, 128 and 129 faces.

Normals bar: each element's absolute error is divided by the condition number of its row (kappa_f = |a||b|/|a x b| of a face,
kappa_v = (sum kappa_f/deg)/|sum n_f/deg| of a vertex, both from float64), and
    max_i err_i/kappa_i (gpu) <= max(4 max_i err_i/kappa_i (fp32 oracle), 4 * 2^-24):
about a hundred times tighter than an absolute 2e-5 on a well-shaped face, and still following a sliver.  The fp32 oracle's own
figure on these meshes is printed by tests/test_stage_oracle_cpu.py (0.3 .. 2.3 x 2^-24); each test here prints both."""
import ctypes as C

import numpy as np
import pytest

import mesh_query_oracle as mq

pytestmark = pytest.mark.gpu

NUMERIC = 3  # SMPLPP_ERR_NUMERIC


class _Mesh:
    """One model on the GPU with its posed vertices [3,V,3] (launch at n = 3, theta scaled by 0.5) and its float64 / fp32 normals."""

    def __init__(self, name, md):
        from smplpp_amd.smpl import SMPL

        self.name, self.md = name, md
        self.s = SMPL()
        self.s.setDevice("cuda:0")
        self.s.init(md)
        self.faces, self.V = mq.faces0(md), md["vertices_template"].shape[0]
        self.F = len(self.faces)
        self.adj = mq.adjacency(self.faces, self.V)
        beta, theta = mq.posed_inputs()
        self.verts = self.s.launch(beta, theta)["verts"].copy()
        self.ref = _Reference(self, self.verts)


class _Reference:
    """float64 and fp32 normals of every face and vertex of `verts`, their condition numbers and exactly degenerate rows."""

    def __init__(self, m, verts):
        self.fn = {dt: mq.face_normals(verts, m.faces, None, dt) for dt in (np.float64, np.float32)}
        self.vn = {dt: mq.vertex_normals(verts, m.faces, m.adj, None, dt) for dt in (np.float64, np.float32)}
        self.kf, self.kv = mq.face_condition(verts, m.faces), mq.vertex_condition(verts, m.faces, m.adj)
        self.df, self.dv = mq.dead_faces(verts, m.faces), mq.dead_vertices(verts, m.faces, m.adj)

    def held(self, name, gpu, vertex, ids=None):
        """gpu [n,count,3] at `ids` (all when None) within the bar."""
        ref, kappa, dead = (self.vn, self.kv, self.dv) if vertex else (self.fn, self.kf, self.df)
        ix = slice(None) if ids is None else np.asarray(ids)
        assert gpu.dtype == np.float32 and gpu.shape == ref[np.float64][:, ix].shape
        e = mq.scaled_error(gpu, ref[np.float64][:, ix], kappa[:, ix], dead[:, ix])
        e32 = mq.scaled_error(ref[np.float32][:, ix], ref[np.float64][:, ix], kappa[:, ix], dead[:, ix])
        print("%-44s max err/kappa: gpu %.3g (%.2f x 2^-24)   fp32 oracle %.3g (%.2f x 2^-24)"
              % (name, e, e / mq.EPS32, e32, e32 / mq.EPS32))
        assert e <= mq.bar(e32), (name, e, e32)


_MODELS = ["synthetic", "tiny61"] + ["fan%d" % N for N in mq.FANS]
_cache = {}


def _mesh(name, synth_model=None):
    from smplpp_amd import model_io

    if name not in _cache:
        md = (synth_model if name == "synthetic" else model_io.tiny_model(61, seed=7) if name == "tiny61"
              else mq.double_fan_model(int(name[3:])))
        _cache[name] = _Mesh(name, md)
    return _cache[name]


@pytest.fixture(scope="module", params=_MODELS)
def mesh(request, synth_model):
    return _mesh(request.param, synth_model)


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _cache.clear()


def _lib():
    from smplpp_amd import _lib as lib

    return lib.load()


def _normals(m, verts, kind, ids=None):
    """smplpp_face_normals (kind 0) / _vertex_normals (1) / _mesh_vertex_normals (2) on explicit host vertices [n,V,3]."""
    from smplpp_amd._lib import HOST, check
    from smplpp_amd.smpl import _ptr

    verts = np.ascontiguousarray(verts, np.float32)
    n = len(verts)
    if kind == 2:
        out = np.full((n, m.V, 3), np.nan, np.float32)
        check(_lib().smplpp_mesh_vertex_normals(m.s.handle, n, _ptr(verts), _ptr(out), HOST, None))
        return out
    ids = np.ascontiguousarray(ids, np.int64)
    out = np.full((n, len(ids), 3), np.nan, np.float32)
    fn = _lib().smplpp_vertex_normals if kind == 1 else _lib().smplpp_face_normals
    check(fn(m.s.handle, n, _ptr(verts), len(ids), _ptr(ids), _ptr(out), HOST, None))
    return out


# ---- normals
def test_normals_on_id_lists(mesh):
    """ALL face ids and ALL vertex ids in a shuffled order with the first and last repeated, and lists of 1, 127, 128 and 129 ids
    (one 128-thread block, one short of it, one over): the bar on every element, a list's bits at the whole-mesh result's rows."""
    m = mesh
    whole = _normals(m, m.verts, 2)
    for vertex, count in ((False, m.F), (True, m.V)):
        ordered = _normals(m, m.verts, int(vertex), np.arange(count))
        for ids in mq.id_lists(count, seed=11 + int(vertex)):
            out = _normals(m, m.verts, int(vertex), ids)
            m.ref.held("%s %s list of %d" % (m.name, "vertex" if vertex else "face", len(ids)), out, vertex, ids)
            assert np.array_equal(out, ordered[:, ids])  # a permuted list gives permuted bits; a repeated id its bits again
            if vertex:
                assert np.array_equal(out, whole[:, ids])  # a list result equals the whole-mesh result at its ids


def test_whole_mesh_vertex_normals(mesh):
    """Every vertex of every frame; the mirror's calcMeshVertexNormals / calcVertexNormalBatch / calcNormalBatch carry the same bits."""
    m = mesh
    whole = m.s.calcMeshVertexNormals()
    m.ref.held("%s whole mesh" % m.name, whole, True)
    assert np.array_equal(whole, m.s.calcVertexNormalBatch(np.arange(m.V)))
    assert np.array_equal(whole, _normals(m, m.verts, 2))
    faces = m.s.calcNormalBatch(np.arange(m.F))
    m.ref.held("%s every face" % m.name, faces, False)
    assert np.array_equal(m.s.calcNormal(m.F - 1), faces[0, m.F - 1]) and np.array_equal(m.s.calcVertexNormal(m.V - 1), whole[0, m.V - 1])


def test_degenerate_faces(mesh):
    """Two corners of one face on the same point, for each pair of corners (edge a = 0, edge b = 0, a = b): the face's normal is
    EXACTLY (0,0,0) by the max(|x|, 1e-12) rule, in lists and through its vertices' normals, which stay finite and within the bar
    of the float64 definition.  Every face around one vertex collapsed: that vertex normal is exactly zero, not NaN."""
    m = mesh
    f, v = mq.degenerate_targets(m.faces, m.V)
    for pair in mq.CORNER_PAIRS:
        dv = mq.collapse_face(m.verts, m.faces, f, pair)
        ref = _Reference(m, dv)
        assert ref.df[:, f].all() and not ref.dv.all()
        out = _normals(m, dv, 0, np.arange(m.F))
        assert np.array_equal(out[:, f], np.zeros((3, 3), np.float32)), (pair, out[:, f])
        ref.held("%s face %d corners %s: faces" % (m.name, f, pair), out, False)  # (every exactly degenerate face must be exactly 0)
        ref.held("%s face %d corners %s: vertices" % (m.name, f, pair), _normals(m, dv, 2), True)
        ids = np.concatenate([m.faces[f], m.faces[f][::-1]])
        ref.held("%s face %d corners %s: its vertices" % (m.name, f, pair), _normals(m, dv, 1, ids), True, ids)
    dv = mq.collapse_vertex_star(m.verts, m.faces, v)
    ref = _Reference(m, dv)
    assert ref.dv[:, v].all()
    whole = _normals(m, dv, 2)
    assert np.array_equal(whole[:, v], np.zeros((3, 3), np.float32)), whole[:, v]
    assert np.array_equal(_normals(m, dv, 1, [v]), np.zeros((3, 1, 3), np.float32))
    ref.held("%s star of vertex %d: vertices" % (m.name, v), whole, True)
    ref.held("%s star of vertex %d: faces" % (m.name, v), _normals(m, dv, 0, np.arange(m.F)), False)


# ---- adjacency
@pytest.mark.parametrize("name", ["tiny61"] + ["fan%d" % N for N in mq.FANS])
def test_adjacency(name):
    """getAdjacentFaces of EVERY vertex: the face ids of adjacency(), weights float32(1)/float32(deg) at tolerance 0 (the 70-, 128-
    and 129-face apexes need more than the getter's first 64 entries).  Through the C ABI: a cap below the degree writes exactly
    cap entries and reports the full count; cap = 0 with null buffers reports the count."""
    from smplpp_amd._lib import check

    m = _mesh(name)
    off, fid, w = m.adj
    for v in range(m.V):
        got = m.s.getAdjacentFaces(v)
        want = fid[off[v]:off[v + 1]]
        assert list(got) == want.tolist(), v  # ascending face ids, all of them
        assert np.array_equal(np.array(list(got.values()), np.float32), w[off[v]:off[v + 1]]), v
        assert all(np.float32(x) == x for x in got.values())
    L = _lib()
    for v in (0, 1, m.V - 1):
        deg = int(off[v + 1] - off[v])
        cnt = C.c_int64(-1)
        check(L.smplpp_adjacent_faces(m.s.handle, v, 0, None, None, C.byref(cnt)))
        assert cnt.value == deg
        for cap in (1, deg - 1, deg, deg + 3):
            faces, wt = np.full(deg + 4, -7, np.int64), np.full(deg + 4, -7, np.float32)
            cnt = C.c_int64(-1)
            check(L.smplpp_adjacent_faces(m.s.handle, v, cap, faces.ctypes.data_as(C.POINTER(C.c_int64)),
                                          wt.ctypes.data_as(C.POINTER(C.c_float)), C.byref(cnt)))
            k = min(cap, deg)
            assert cnt.value == deg
            assert np.array_equal(faces[:k], fid[off[v]:off[v] + k]) and (faces[k:] == -7).all()
            assert np.array_equal(wt[:k], w[off[v]:off[v] + k]) and (wt[k:] == -7).all()


# ---- closest points: the three outputs are nullable
def test_closest_points_nullable_outputs(synth_model):
    from smplpp_amd._lib import HOST, check
    from smplpp_amd.smpl import _ptr

    m = _mesh("synthetic", synth_model)
    n, K = 3, 7
    rng = np.random.default_rng(3)
    pts = (m.verts[:, rng.integers(0, m.V, K)] + rng.normal(0, 0.01, (n, K, 3))).astype(np.float32)

    def call(want):
        out = dict(face=np.full((n, K), -7, np.int64), closest=np.full((n, K, 3), np.nan, np.float32), sqdist=np.full((n, K), np.nan, np.float32))
        check(_lib().smplpp_closest_points(m.s.handle, n, _ptr(m.verts), K, _ptr(pts), *[_ptr(out[k]) if k in want else None for k in out],
                                           HOST, None))
        return out

    full = call(("face", "closest", "sqdist"))
    assert (full["face"] >= 0).all() and np.isfinite(full["closest"]).all() and np.isfinite(full["sqdist"]).all()
    for k in full:
        assert np.array_equal(call((k,))[k], full[k]), k


# ---- sweep grid
def _sweep(m, verts, cap, winding=None, inside=None, device=False):
    """smplpp_sweep_grid on explicit vertices [V,3] in host or device space -> (grid_min, grid_num, cells); winding / inside are
    the caller's buffers (numpy in host space, torch in device space) or None."""
    import torch

    from smplpp_amd._lib import DEVICE, HOST, check
    from smplpp_amd.smpl import _ptr, _stream

    v = np.ascontiguousarray(verts, np.float32)
    assert v.shape == (m.V, 3)
    if device:
        v = torch.from_numpy(v).cuda()
    gmin, gnum, cells = np.full(3, -99, np.int32), np.full(3, -99, np.int32), C.c_int64(-1)
    check(_lib().smplpp_sweep_grid(m.s.handle, _ptr(v), _ptr(gmin), _ptr(gnum), cap, _ptr(winding), _ptr(inside), C.byref(cells),
                                   DEVICE if device else HOST, _stream() if device else None))
    if device:
        torch.cuda.synchronize()
    return gmin, gnum, cells.value


class _Bare:
    """A model of V vertices on the GPU, for the calls that only need its vertex count."""

    def __init__(self, V):
        from smplpp_amd import model_io
        from smplpp_amd.smpl import SMPL

        self.V = V
        self.s = SMPL()
        self.s.setDevice("cuda:0")
        self.s.init(model_io.tiny_model(V))


@pytest.fixture(scope="module", params=[61, 1024, 1025, 2500])
def bare(request):
    return _Bare(request.param)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_sweep_grid_bounds(bare, device):
    """bounds_kernel is one workgroup of 1024 threads strided over V: the extremes sit in the last vertex and at the seam of its
    first and second pass (mesh_query_oracle.bounds_vertices), once all negative and once exactly on cell boundaries;
    grid_min and grid_num equal the float32 floor/ceil statement exactly."""
    from smplpp_amd._lib import SmplppError

    for variant in ("plain", "negative", "on_grid"):
        v = mq.bounds_vertices(bare.V, variant)
        lo, num = mq.grid_extents(v)
        gmin, gnum, cells = _sweep(bare, v, 0, device=device)
        assert np.array_equal(gmin, lo) and np.array_equal(gnum, num), (variant, gmin, lo, gnum, num)
        assert cells == int(np.prod(num.astype(np.int64)))
    good = mq.bounds_vertices(bare.V, "plain")
    for value in (np.nan, 3e4, -3e4, np.inf):  # refused, whichever lane meets it; and the next in-range call is clean
        for at in (bare.V - 1, 0):
            bad = good.copy()
            bad[at, 1] = value
            with pytest.raises(SmplppError) as ei:
                _sweep(bare, bad, 0, device=device)
            assert ei.value.code == NUMERIC
        gmin, gnum, _ = _sweep(bare, good, 0, device=device)
        assert np.array_equal(gmin, mq.grid_extents(good)[0]) and np.array_equal(gnum, mq.grid_extents(good)[1])


@pytest.fixture(scope="module")
def fan129_grid():
    """The full sweep of the 129-fan's frame 0 in host space: (mesh, grid_min, grid_num, cells, winding, inside)."""
    m = _mesh("fan129")
    gmin, gnum, cells = _sweep(m, m.verts[0], 0)
    w, ins = np.full(cells, np.nan, np.float32), np.full(cells, 7, np.uint8)
    assert _sweep(m, m.verts[0], cells, w, ins)[2] == cells
    return m, gmin, gnum, cells, w, ins


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_sweep_grid_cap(fan129_grid, device):
    """cap = 0 returns the cell count only; cap = 1000 (no multiple of the 256-thread block) writes cells [0, 1000) with the bits
    of the full run and leaves a canary untouched in [1000, cells); winding alone and inside alone keep their bits."""
    import torch

    m, gmin, gnum, cells, w, ins = fan129_grid
    assert cells > 2000 and np.isfinite(w).all() and set(np.unique(ins)) <= {0, 1}
    cap = 1000

    def buffers():
        bw, bi = np.full(cells, -123.0, np.float32), np.full(cells, 7, np.uint8)
        return (torch.from_numpy(bw).cuda(), torch.from_numpy(bi).cuda()) if device else (bw, bi)

    host = (lambda a: a.cpu().numpy()) if device else (lambda a: a)
    bw, bi = buffers()
    g = _sweep(m, m.verts[0], 0, bw, bi, device=device)
    assert np.array_equal(g[0], gmin) and np.array_equal(g[1], gnum) and g[2] == cells
    assert (host(bw) == -123.0).all() and (host(bi) == 7).all()  # cap = 0 writes nothing
    for want_w, want_i in ((True, True), (True, False), (False, True)):
        bw, bi = buffers()
        g = _sweep(m, m.verts[0], cap, bw if want_w else None, bi if want_i else None, device=device)
        assert g[2] == cells  # the full count, whatever the cap
        hw, hi = host(bw), host(bi)
        assert np.array_equal(hw[:cap], w[:cap] if want_w else np.full(cap, -123.0, np.float32))
        assert np.array_equal(hi[:cap], ins[:cap] if want_i else np.full(cap, 7, np.uint8))
        assert (hw[cap:] == -123.0).all() and (hi[cap:] == 7).all()
    bw, bi = buffers()  # the full run keeps its bits in either space, and a cap beyond the count writes the count
    assert _sweep(m, m.verts[0], cells + 300, bw, bi, device=device)[2] == cells
    assert np.array_equal(host(bw), w) and np.array_equal(host(bi), ins)


@pytest.mark.parametrize("N", [18, 128, 129])
def test_sweep_grid_winding(N):
    """ALL cells of a closed fan (F = 36, 256 and 258: the winding loop's 256-face chunks with a short, a full and a 2-face last
    chunk) against the oracle's fp64 solid-angle sum: 2e-4 absolute, the same inside verdict wherever |w - 0.5| > 0.01, and
    inside == (winding > 0.5) everywhere."""
    from oracle import cpu

    m = _mesh("fan%d" % N)
    v = m.verts[0]
    gmin, gnum, cells = _sweep(m, v, 0)
    assert np.array_equal(gmin, mq.grid_extents(v)[0]) and np.array_equal(gnum, mq.grid_extents(v)[1])
    w, ins = np.full(cells, np.nan, np.float32), np.full(cells, 7, np.uint8)
    _sweep(m, v, cells, w, ins)
    ix, iy, iz = np.meshgrid(*[np.arange(gmin[a], gmin[a] + gnum[a], dtype=np.int32) for a in range(3)], indexing="ij")
    gidx = np.stack([ix.reshape(-1), iy.reshape(-1), iz.reshape(-1)], axis=1)  # x outermost, z innermost
    ref = cpu.OracleModel(m.md).winding_numbers(v, np.float32(0.025) * gidx.astype(np.float32))
    print("fan%d: %d cells, max |winding - oracle| = %.3g" % (N, cells, np.abs(w - ref).max()))
    assert np.abs(w - ref).max() < 2e-4
    clear = np.abs(ref - 0.5) > 0.01
    assert ((ref > 0.5) == (ins == 1))[clear].all()
    assert np.array_equal(ins, (w > np.float32(0.5)).astype(np.uint8))
    assert 0.02 < ins.mean() < 0.9  # a closed body: a solid share of its bounding grid
    g = m.s.calcSweepGrid(frame=0)  # the mirror's two-call form carries the same bits
    assert np.array_equal(g["winding"], w) and np.array_equal(g["inside"], ins.astype(bool)) and np.array_equal(g["grid_idx"], gidx)
