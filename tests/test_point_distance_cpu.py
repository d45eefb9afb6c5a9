"""The point-to-mesh distance without a GPU: the entry points are declared, exported and bound; the Python methods marshal their
calls as pinned here (a recording stub in place of the library, as test_binding_cpu.py does); and the float64 restatement the GPU
tests compare against (tests/point_distance_oracle.py) is pinned to the closed form, to finite differences, and to the tie property:
faces tied at a shared edge or vertex give the same gradient."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_ref as cr  # noqa: E402
import point_distance_oracle as O  # noqa: E402

SYMBOLS = {"smplpp_point_mesh_distance": 11, "smplpp_point_mesh_distance_vjp": 12}


def test_point_distance_declared_exported_bound():
    from smplpp_amd import _lib

    L = _lib.load()
    for name, nargs in SYMBOLS.items():
        assert name in _lib.declared_symbols()
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name


def test_point_distance_without_gpu_raises():
    from smplpp_amd import _lib

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _lib.load()
    v = np.zeros((1, 4, 3), np.float32)
    p = np.zeros((1, 2, 3), np.float32)
    face = np.zeros((1, 2), np.int64)
    sq = np.full((1, 2), 7.0, np.float32)
    gv = np.full((1, 4, 3), 7.0, np.float32)
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_point_mesh_distance(None, 1, v.ctypes.data, 2, p.ctypes.data, face.ctypes.data, None, None, sq.ctypes.data, 0,
                                                None))
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_point_mesh_distance_vjp(None, 1, v.ctypes.data, 2, p.ctypes.data, face.ctypes.data, sq.ctypes.data,
                                                    gv.ctypes.data, None, 0, 0, None))
    assert (sq == 7.0).all() and (gv == 7.0).all()


# ---------------------------------------------------------------------------------------------------- the float64 oracle
def _triangle(seed):
    """A generic triangle: the unit right triangle, sheared, rotated, scaled and moved; and the map applied to it."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    M = q @ np.diag([0.05, 0.04, 0.03]) @ np.array([[1.0, 0.2, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    t = rng.normal(0.0, 0.5, 3)
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]) @ M.T + t
    return tri, M, t


# a point of each region of the unit right triangle a = 0, b = e_x, c = e_y (lifted off its plane)
REGION_POINTS = {
    "vertex_a": (-0.3, -0.2, 0.1),
    "vertex_b": (1.3, -0.2, 0.1),
    "vertex_c": (-0.2, 1.3, -0.1),
    "edge_ab": (0.4, -0.3, 0.2),
    "edge_ac": (-0.3, 0.4, 0.2),
    "edge_bc": (0.7, 0.7, 0.3),
    "interior": (0.2, 0.3, 0.25),
}


@pytest.mark.parametrize("name", O.REGIONS)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_gradient_closed_form_and_fd(name, seed):
    tri, M, t = _triangle(seed)
    p = np.array(REGION_POINTS[name]) @ M.T + t
    verts = torch.tensor(tri[None], dtype=torch.float64)
    points = torch.tensor(p[None, None], dtype=torch.float64)
    faces = np.array([[0, 1, 2]])
    face = np.zeros((1, 1), np.int64)
    reg = O.region(points[0, 0], verts[0, 0], verts[0, 1], verts[0, 2])
    assert O.REGIONS[int(reg)] == name
    g = np.array([[0.7]])
    gv, gp = O.vjp(verts, faces, points, face, g)
    cv, cp = O.closed_form(verts, faces, points, face, g)
    np.testing.assert_allclose(gv.numpy(), cv.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(gp.numpy(), cp.numpy(), rtol=1e-12, atol=1e-15)
    # weights: non-negative, sum 1, one-hot at a vertex; sum_j w_j v_j is the exact closest point
    c, w = O.closest(points[0, 0], verts[0, 0], verts[0, 1], verts[0, 2])
    assert (w >= -1e-15).all() and abs(float(w.sum()) - 1.0) < 1e-14
    if name.startswith("vertex"):
        assert sorted(w.tolist()) == [0.0, 0.0, 1.0]
    D, C = cr.tri_sqdist(p, tri[0], tri[1], tri[2])
    np.testing.assert_allclose(c.numpy(), C, atol=1e-14)
    # central differences of the squared distance (the region does not change within h)
    h = 1e-6

    def f(v, q):
        return 0.7 * float(O.sqdist(torch.tensor(v[None]), faces, torch.tensor(q[None, None]), face)[0, 0])

    for j in range(3):
        for x in range(3):
            vp, vm = tri.copy(), tri.copy()
            vp[j, x] += h
            vm[j, x] -= h
            num = (f(vp, p) - f(vm, p)) / (2 * h)
            assert abs(num - float(gv[0, j, x])) <= 1e-7 * max(1.0, abs(num)), (j, x, num, float(gv[0, j, x]))
        pp, pm = p.copy(), p.copy()
        pp[j] += h
        pm[j] -= h
        num = (f(tri, pp) - f(tri, pm)) / (2 * h)
        assert abs(num - float(gp[0, 0, j])) <= 1e-7 * max(1.0, abs(num))


@pytest.mark.parametrize("cls", ["on_edge", "edge_region", "on_vertex", "vertex_region"])
def test_oracle_tied_faces_same_gradient(synth_model, cls):
    """Where two faces share the closest point (an edge or a vertex between them), either face gives the same gradient, so the tie
    rule does not move it."""
    from oracle import cpu
    from smplpp_amd import model_io

    faces = synth_model["face_indices"].astype(np.int64) - 1
    beta, theta = model_io.synthetic_inputs(1, seed=7)
    v32 = cpu.OracleModel(synth_model).fk(beta, theta)["verts"][0]
    rng = np.random.default_rng(11)
    P = cr.make_queries(v32, faces, cls, 40, rng)
    D = cr.mesh_sqdist(v32, faces, P)
    verts = torch.tensor(v32[None], dtype=torch.float64)
    pairs = 0
    for k in range(len(P)):
        mn = D[k].min()
        tied = np.nonzero(D[k] <= mn * (1 + 1e-9) + 1e-16)[0]
        if len(tied) < 2:
            continue
        pairs += 1
        pts = torch.tensor(P[k][None, None], dtype=torch.float64)
        ref = None
        for f in tied:
            gv, gp = O.vjp(verts, faces, pts, np.array([[f]]), np.array([[1.0]]))
            if ref is None:
                ref = (gv, gp)
                continue
            # 1 cm off the surface the gradients agree to rounding; a query ON the surface (fp32 rounding puts it ~1e-8 m to one
            # side) has |r| ~ 1e-8 and both gradients are that small: 2 |g| |r| bounds each, so they agree to 4 |r|
            tol = 1e-7 * float(ref[1].abs().max()) if cls.endswith("region") else 4.0 * np.sqrt(D[k, tied].max())
            assert float((gv - ref[0]).abs().max()) <= tol + 1e-13, (cls, k, tied)
            assert float((gp - ref[1]).abs().max()) <= tol + 1e-13, (cls, k, tied)
    assert pairs >= len(P) // 4, (cls, pairs)  # (above a concave edge, or near another part of the body, one face wins alone)


# ---------------------------------------------------------------------------------------------------- bindings (recording stub)
N, V = 2, 6890


class _Stub:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("smplpp_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if name in ("smplpp_model_create", "smplpp_device_count"):
                args[-1]._obj.value = 1
            return 0

        return fn

    def last(self, name):
        assert self.calls and self.calls[-1][0] == name, [c[0] for c in self.calls[-3:]]
        return self.calls[-1][1]


@pytest.fixture
def stub(monkeypatch):
    from smplpp_amd import _lib

    s = _Stub()
    monkeypatch.setattr(_lib, "_lib", s)
    return s


@pytest.fixture
def smpl(stub, synth_model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.init(synth_model)
    yield s
    s._h = None  # the stub's handle must never reach the real library's destroy


def _addr(a):
    return a.ctypes.data


def _refused(stub, fn, *args, **kw):
    from smplpp_amd._lib import SmplppError

    before = len(stub.calls)
    with pytest.raises(SmplppError) as e:
        fn(*args, **kw)
    assert e.value.code == 1
    assert len(stub.calls) == before, "refused input reached the ABI"


def test_point_mesh_distance_binding(stub, smpl):
    from smplpp_amd._lib import HOST

    verts = np.zeros((N, V, 3), np.float32)
    face, w, closest, sq = smpl.pointMeshDistance(verts, np.zeros((N, 5, 3)))
    h, n, v, K, pts, pf, pw, pc, ps, space, stream = stub.last("smplpp_point_mesh_distance")
    assert (n, K, space, stream) == (N, 5, HOST, None)
    assert v == _addr(verts) and isinstance(pts, int)
    assert face.shape == (N, 5) and face.dtype == np.int64
    assert w.shape == (N, 5, 3) and w.dtype == np.float32
    assert closest.shape == (N, 5, 3) and closest.dtype == np.float32
    assert sq.shape == (N, 5) and sq.dtype == np.float32
    assert (pf, pw, pc, ps) == (_addr(face), _addr(w), _addr(closest), _addr(sq))


def test_point_mesh_distance_backward_binding(stub, smpl):
    from smplpp_amd._lib import HOST

    verts, pts = np.zeros((N, V, 3), np.float32), np.zeros((N, 4, 3), np.float32)
    face, g = np.zeros((N, 4), np.int64), np.ones((N, 4), np.float32)
    gv, gp = smpl.pointMeshDistanceBackward(verts, pts, face, g)
    h, n, v, K, p, f, pg, pgv, pgp, acc, space, stream = stub.last("smplpp_point_mesh_distance_vjp")
    assert (n, K, acc, space, stream) == (N, 4, 0, HOST, None)
    assert v == _addr(verts) and p == _addr(pts) and isinstance(f, int) and pg == _addr(g)
    assert gv.shape == (N, V, 3) and gv.dtype == np.float32 and pgv == _addr(gv)
    assert gp.shape == (N, 4, 3) and gp.dtype == np.float32 and pgp == _addr(gp)

    out = np.zeros((N, V, 3), np.float32)
    gv, gp = smpl.pointMeshDistanceBackward(verts, pts, torch.zeros((N, 4), dtype=torch.int64), g, out=out)
    *_, pgv, pgp, acc, _, _ = stub.last("smplpp_point_mesh_distance_vjp")
    assert acc == 1 and gv is out and pgv == _addr(out)
    assert pgp == _addr(gp) and (gp == 0).all()  # the other output starts at zero when the call adds

    gpo = np.ones((N, 4, 3), np.float32)
    gv, gp = smpl.pointMeshDistanceBackward(verts, pts, face, g, grad_points=gpo)
    *_, pgv, pgp, acc, _, _ = stub.last("smplpp_point_mesh_distance_vjp")
    assert acc == 1 and gp is gpo and pgp == _addr(gpo) and pgv == _addr(gv) and (gv == 0).all()


def test_point_mesh_distance_refuses(stub, smpl):
    verts, pts = np.zeros((N, V, 3), np.float32), np.zeros((N, 4, 3), np.float32)
    face, g = np.zeros((N, 4), np.int64), np.ones((N, 4), np.float32)
    _refused(stub, smpl.pointMeshDistance, verts, pts[0])
    _refused(stub, smpl.pointMeshDistance, verts, pts[:1])
    _refused(stub, smpl.pointMeshDistance, verts, np.zeros((N, 0, 3), np.float32))
    _refused(stub, smpl.pointMeshDistance, verts[:, :-1], pts)
    _refused(stub, smpl.pointMeshDistance, verts, torch.from_numpy(pts))
    _refused(stub, smpl.pointMeshDistanceBackward, verts, pts, face[:, :3], g)
    _refused(stub, smpl.pointMeshDistanceBackward, verts, pts, face, g[:, :3])
    _refused(stub, smpl.pointMeshDistanceBackward, verts, pts, face, g, out=np.zeros((N, V, 3), np.float64))
    _refused(stub, smpl.pointMeshDistanceBackward, verts, pts, face, g, grad_points=np.zeros((N, 3, 3), np.float32))
    _refused(stub, smpl.pointMeshDistanceBackward, verts, pts, face, g, out=torch.zeros((N, V, 3)))
    _refused(stub, smpl.point_mesh_distance_differentiable, verts, pts)
