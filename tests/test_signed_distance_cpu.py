"""The winding numbers and the signed point-to-mesh distance without a GPU: the entry points are declared, exported and bound; the
Python methods marshal their calls as pinned here (a recording stub in place of the library, as test_mesh_point_distance_cpu.py
does) and refuse loudly without a GPU; the float64 restatements the GPU tests compare against (tests/signed_distance_oracle.py)
agree with the C oracle's winding numbers, and the backward's sign rule with finite differences of sigma d^2 away from the surface."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_distance_oracle as PO  # noqa: E402
import signed_distance_oracle as SO  # noqa: E402

SYMBOLS = {"smplpp_point_mesh_winding": 9, "smplpp_point_mesh_signed_distance": 13, "smplpp_point_mesh_signed_distance_vjp": 13}


def test_signed_distance_declared_exported_bound():
    from smplpp_amd import _lib

    L = _lib.load()
    for name, nargs in SYMBOLS.items():
        assert name in _lib.declared_symbols()
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name


def test_signed_distance_without_gpu_raises():
    from smplpp_amd import _lib

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _lib.load()
    v = np.zeros((1, 4, 3), np.float32)
    p = np.zeros((1, 2, 3), np.float32)
    face = np.zeros((1, 2), np.int64)
    ins = np.zeros((1, 2), np.uint8)
    w = np.full((1, 2), 7.0, np.float32)
    gv = np.full((1, 4, 3), 7.0, np.float32)
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_point_mesh_winding(None, 1, v.ctypes.data, 2, p.ctypes.data, w.ctypes.data, None, 0, None))
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_point_mesh_signed_distance(None, 1, v.ctypes.data, 2, p.ctypes.data, face.ctypes.data, None, None, None,
                                                       ins.ctypes.data, w.ctypes.data, 0, None))
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_point_mesh_signed_distance_vjp(None, 1, v.ctypes.data, 2, p.ctypes.data, face.ctypes.data, ins.ctypes.data,
                                                           w.ctypes.data, gv.ctypes.data, None, 0, 0, None))
    assert (w == 7.0).all() and (gv == 7.0).all()


# ---------------------------------------------------------------------------------------------------- the float64 restatements
def test_winding_restatement_matches_c_oracle(synth_model):
    from oracle import cpu
    from smplpp_amd import model_io

    o = cpu.OracleModel(synth_model)
    faces = synth_model["face_indices"].astype(np.int64) - 1
    beta, theta = model_io.synthetic_inputs(1, seed=4)
    for v in (synth_model["vertices_template"].astype(np.float32), o.fk(beta, theta)["verts"][0]):
        rng = np.random.default_rng(4)
        lo, hi = v.min(0), v.max(0)
        P = np.concatenate([rng.uniform(lo, hi, (150, 3)), v[rng.choice(len(v), 50)] + rng.normal(0, 0.005, (50, 3)),
                            rng.normal(0, 10.0, (10, 3))]).astype(np.float32)
        w = SO.winding64(v, faces, P)
        ref = o.winding_numbers(v, P)
        assert np.abs(w - ref).max() < 1e-9
    # the rest mesh is closed and outward-facing: 1 inside, 0 outside
    v = synth_model["vertices_template"].astype(np.float32)
    w = SO.winding64(v, faces, np.stack([v.mean(0), v.mean(0) + 20.0]))
    assert abs(w[0] - 1) < 1e-9 and abs(w[1]) < 1e-9


def _octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * 0.3
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)
    return v, f


def test_octahedron_winding_and_orientation():
    v, f = _octahedron()
    w = SO.winding64(v, f, np.array([[0.0, 0.0, 0.0], [0.05, -0.02, 0.1], [1.0, 0.0, 0.0], [0.2, 0.2, 0.2]]))
    np.testing.assert_allclose(w, [1, 1, 0, 0], atol=1e-12)


def test_signed_vjp_sign_rule_vs_finite_differences():
    """sigma d^2 with sigma from the winding number at the point itself: away from the surface (and from the closest point's region
    boundaries) its finite differences in the points and the vertices are the autograd product of signed_distance_oracle.vjp."""
    v, f = _octahedron()
    rng = np.random.default_rng(8)
    P = np.concatenate([rng.normal(0, 0.05, (6, 3)), rng.normal(0, 0.05, (6, 3)) + np.array([0.3, 0.3, 0.3])])

    def closest_face(vv, p):
        d = torch.stack([PO.sqdist(torch.tensor(vv[None]), f, torch.tensor(p[None]), torch.full((1, len(p)), j)) for j in range(len(f))])
        return d.argmin(0).numpy(), d.min(0).values.numpy()

    face, d2 = closest_face(v, P)
    inside = SO.winding64(v, f, P) > 0.5
    assert inside.any() and (~inside).any() and (d2 > 1e-3).all()

    def loss(vv, pp):
        fc, dd = closest_face(vv, pp)
        sig = np.where(SO.winding64(vv, f, pp) > 0.5, -1.0, 1.0)
        return float((sig * dd[0]).sum()), fc

    gv, gp = SO.vjp(torch.tensor(v[None]), f, torch.tensor(P[None]), face, inside, np.ones((1, len(P))))
    h = 1e-6
    for k in range(len(P)):
        for x in range(3):
            pp, pm = P.copy(), P.copy()
            pp[k, x] += h
            pm[k, x] -= h
            (lp, fp), (lm, fm) = loss(v, pp), loss(v, pm)
            assert (fp == face).all() and (fm == face).all()
            assert abs((lp - lm) / (2 * h) - float(gp[0, k, x])) < 1e-6
    for u in range(len(v)):
        vp, vm = v.copy(), v.copy()
        vp[u, 1] += h
        vm[u, 1] -= h
        assert abs((loss(vp, P)[0] - loss(vm, P)[0]) / (2 * h) - float(gv[0, u, 1])) < 1e-6
    # the inside points' gradient is the distance's with the sign flipped
    _, up = PO.vjp(torch.tensor(v[None]), f, torch.tensor(P[None]), face, np.ones((1, len(P))))
    np.testing.assert_allclose(gp[0].numpy(), np.where(inside[:, None], -1.0, 1.0) * up[0].numpy(), rtol=1e-12)


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


def test_point_mesh_winding_binding(stub, smpl):
    from smplpp_amd._lib import HOST

    verts = np.zeros((N, V, 3), np.float32)
    w, ins = smpl.pointMeshWinding(verts, np.zeros((N, 5, 3)))
    h, n, v, K, pts, pw, pi, space, stream = stub.last("smplpp_point_mesh_winding")
    assert (n, K, space, stream) == (N, 5, HOST, None)
    assert v == _addr(verts) and isinstance(pts, int) and isinstance(pw, int) and isinstance(pi, int)
    assert w.shape == (N, 5) and w.dtype == np.float32 and pw == _addr(w)
    assert ins.shape == (N, 5) and ins.dtype == bool


def test_point_mesh_signed_distance_binding(stub, smpl):
    from smplpp_amd._lib import HOST

    verts = np.zeros((N, V, 3), np.float32)
    face, w, closest, wn, ins, sq = smpl.pointMeshSignedDistance(verts, np.zeros((N, 5, 3)))
    h, n, v, K, pts, pf, pw, pc, pwn, pi, ps, space, stream = stub.last("smplpp_point_mesh_signed_distance")
    assert (n, K, space, stream) == (N, 5, HOST, None)
    assert v == _addr(verts) and isinstance(pts, int) and isinstance(pi, int)
    assert face.shape == (N, 5) and face.dtype == np.int64 and pf == _addr(face)
    assert w.shape == (N, 5, 3) and pw == _addr(w) and closest.shape == (N, 5, 3) and pc == _addr(closest)
    assert wn.shape == (N, 5) and wn.dtype == np.float32 and pwn == _addr(wn)
    assert ins.shape == (N, 5) and ins.dtype == bool
    assert sq.shape == (N, 5) and sq.dtype == np.float32 and ps == _addr(sq)


def test_point_mesh_signed_distance_backward_binding(stub, smpl):
    from smplpp_amd._lib import HOST

    verts, pts = np.zeros((N, V, 3), np.float32), np.zeros((N, 4, 3), np.float32)
    face, g = np.zeros((N, 4), np.int64), np.ones((N, 4), np.float32)
    ins = np.array([[True, False, True, False]] * N)
    gv, gp = smpl.pointMeshSignedDistanceBackward(verts, pts, face, ins, g)
    h, n, v, K, p, f, pi, pg, pgv, pgp, acc, space, stream = stub.last("smplpp_point_mesh_signed_distance_vjp")
    assert (n, K, acc, space, stream) == (N, 4, 0, HOST, None)
    assert v == _addr(verts) and p == _addr(pts) and isinstance(f, int) and isinstance(pi, int) and pg == _addr(g)
    assert gv.shape == (N, V, 3) and gv.dtype == np.float32 and pgv == _addr(gv)
    assert gp.shape == (N, 4, 3) and gp.dtype == np.float32 and pgp == _addr(gp)

    out = np.zeros((N, V, 3), np.float32)
    gv, gp = smpl.pointMeshSignedDistanceBackward(verts, pts, torch.zeros((N, 4), dtype=torch.int64), torch.from_numpy(ins), g, out=out)
    *_, pgv, pgp, acc, _, _ = stub.last("smplpp_point_mesh_signed_distance_vjp")
    assert acc == 1 and gv is out and pgv == _addr(out)
    assert pgp == _addr(gp) and (gp == 0).all()  # the other output starts at zero when the call adds

    gpo = np.ones((N, 4, 3), np.float32)
    gv, gp = smpl.pointMeshSignedDistanceBackward(verts, pts, face, ins.astype(np.uint8), g, grad_points=gpo)
    *_, pgv, pgp, acc, _, _ = stub.last("smplpp_point_mesh_signed_distance_vjp")
    assert acc == 1 and gp is gpo and pgp == _addr(gpo) and pgv == _addr(gv) and (gv == 0).all()


def test_signed_distance_refuses(stub, smpl):
    verts, pts = np.zeros((N, V, 3), np.float32), np.zeros((N, 4, 3), np.float32)
    face, g, ins = np.zeros((N, 4), np.int64), np.ones((N, 4), np.float32), np.zeros((N, 4), bool)
    for fn in (smpl.pointMeshWinding, smpl.pointMeshSignedDistance):
        _refused(stub, fn, verts, pts[0])
        _refused(stub, fn, verts, pts[:1])
        _refused(stub, fn, verts, np.zeros((N, 0, 3), np.float32))
        _refused(stub, fn, verts[:, :-1], pts)
        _refused(stub, fn, verts, torch.from_numpy(pts))
    _refused(stub, smpl.pointMeshSignedDistanceBackward, verts, pts, face[:, :3], ins, g)
    _refused(stub, smpl.pointMeshSignedDistanceBackward, verts, pts, face, ins[:, :3], g)
    _refused(stub, smpl.pointMeshSignedDistanceBackward, verts, pts, face, ins, g[:, :3])
    _refused(stub, smpl.pointMeshSignedDistanceBackward, verts, pts, face, ins, g, out=np.zeros((N, V, 3), np.float64))
    _refused(stub, smpl.pointMeshSignedDistanceBackward, verts, pts, face, ins, g, grad_points=np.zeros((N, 3, 3), np.float32))
    _refused(stub, smpl.point_mesh_signed_distance_differentiable, verts, pts)
