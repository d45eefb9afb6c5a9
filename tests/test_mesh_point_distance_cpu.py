"""The mesh-to-point distance without a GPU: the entry points are declared, exported and bound; the Python methods marshal their
calls as pinned here (a recording stub in place of the library, as test_point_distance_cpu.py does); and the restatements the GPU
tests compare against (tests/mesh_point_distance_oracle.py) are pinned on hand-built cases (ties, non-finite points, an all-NaN
frame) and to the closed form and finite differences of the gradient."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_point_distance_oracle as O  # noqa: E402

SYMBOLS = {"smplpp_mesh_point_distance": 9, "smplpp_mesh_point_distance_vjp": 12}


def test_mesh_point_distance_declared_exported_bound():
    from smplpp_amd import _lib

    L = _lib.load()
    for name, nargs in SYMBOLS.items():
        assert name in _lib.declared_symbols()
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name


def test_mesh_point_distance_without_gpu_raises():
    from smplpp_amd import _lib

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _lib.load()
    v = np.zeros((1, 4, 3), np.float32)
    p = np.zeros((1, 2, 3), np.float32)
    index = np.full((1, 4), 5, np.int64)
    sq = np.full((1, 4), 7.0, np.float32)
    gv = np.full((1, 4, 3), 7.0, np.float32)
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_mesh_point_distance(None, 1, v.ctypes.data, 2, p.ctypes.data, index.ctypes.data, sq.ctypes.data, 0, None))
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_mesh_point_distance_vjp(None, 1, v.ctypes.data, 2, p.ctypes.data, index.ctypes.data, sq.ctypes.data,
                                                    gv.ctypes.data, None, 0, 0, None))
    assert (sq == 7.0).all() and (gv == 7.0).all() and (index == 5).all()


# ---------------------------------------------------------------------------------------------------- the float32 rule
def _brute(v, p):
    """The rule written as plainly as possible: one pair at a time, float32 scalars."""
    out_k, out_d = [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for x in v.astype(np.float32):
            bk, bd = -1, np.float32(np.inf)
            for k, q in enumerate(p.astype(np.float32)):
                dx, dy, dz = x[0] - q[0], x[1] - q[1], x[2] - q[2]
                d = np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))
                if np.isfinite(d) and d < bd:
                    bk, bd = k, d
            out_k.append(bk)
            out_d.append(bd if bk >= 0 else np.float32(0))
    return np.array(out_k, np.int64), np.array(out_d, np.float32)


def test_oracle_duplicate_points_lowest_index():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.5, 0.5, 0.5]], np.float32)
    p = np.array([[3.0, 0, 0], [0.1, 0, 0], [0.1, 0, 0], [1.0, 1.0, 1.25], [1.0, 1.0, 0.75], [0.1, 0, 0]], np.float32)
    k, d = O.forward_frame(v, p)
    assert k.tolist()[:2] == [1, 3]  # duplicates 1, 2, 5: the lowest; 3 and 4 exactly equidistant from vertex 1: the lower
    assert d[0] == np.float32(0.1) * np.float32(0.1) and d[1] == np.float32(0.0625)
    bk, bd = _brute(v, p)
    assert (k == bk).all() and d.tobytes() == bd.tobytes()


def test_oracle_ties_across_chunks():
    """Equal minima in different chunks of the restatement: the lowest index still wins."""
    v = np.zeros((2, 3), np.float32)
    p = np.full((3 * O.CHUNK, 3), 5.0, np.float32)
    p[O.CHUNK + 7] = (0.25, 0, 0)
    p[2 * O.CHUNK + 1] = (0, 0.25, 0)
    p[2 * O.CHUNK + 3] = (0, 0, -0.25)
    k, d = O.forward_frame(v, p)
    assert (k == O.CHUNK + 7).all() and (d == np.float32(0.0625)).all()


def test_oracle_non_finite_points_skipped():
    v = np.array([[0.0, 0.0, 0.0], [1e30, 0.0, 0.0]], np.float32)
    p = np.array([[np.nan, 0, 0], [0, np.inf, 0], [3e38, 3e38, 3e38], [-np.inf, -np.inf, -np.inf], [2.0, 0, 0], [0, 0, np.nan]], np.float32)
    k, d = O.forward_frame(v, p)
    assert k[0] == 4 and d[0] == np.float32(4.0)
    # vertex 1: (1e30 - 2)^2 overflows fp32, and so does every other pair: no eligible point
    assert k[1] == -1 and d[1] == 0.0
    bk, bd = _brute(v, p)
    assert (k == bk).all() and d.tobytes() == bd.tobytes()


def test_oracle_all_nan_frame():
    rng = np.random.default_rng(0)
    v = rng.normal(size=(2, 50, 3)).astype(np.float32)
    p = rng.normal(size=(2, 30, 3)).astype(np.float32)
    p[1] = np.nan
    k, d = O.forward(v, p)
    assert (k[1] == -1).all() and (d[1] == 0).all()
    assert (k[0] >= 0).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_matches_brute_force(seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(0, 0.5, (40, 3)).astype(np.float32)
    p = rng.normal(0, 0.5, (O.CHUNK + 37, 3)).astype(np.float32)
    p[::97] = p[3]  # duplicates
    p[5::211] = np.nan
    k, d = O.forward_frame(v, p)
    bk, bd = _brute(v, p)
    assert (k == bk).all() and d.tobytes() == bd.tobytes()


def test_oracle_no_fma():
    """A case where a fused multiply-add would round differently: the restatement rounds every product."""
    v = np.array([[1067981117, 1068815661, 0]], np.int32).view(np.float32)  # (1.31327021..., 1.41275560..., 0)
    p = np.zeros((1, 3), np.float32)
    _, d = O.forward_frame(v, p)
    dx, dy = np.float64(v[0, 0]), np.float64(v[0, 1])
    want = np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(0))
    fused = np.float32(np.float32(dx * dx) + dy * dy)  # dy*dy unrounded, as an FMA would take it
    assert d[0] == want and want != fused


# ---------------------------------------------------------------------------------------------------- the float64 gradient
def test_oracle_gradient_closed_form_and_fd():
    rng = np.random.default_rng(3)
    n, V, K = 2, 30, 12
    v = rng.normal(0, 0.3, (n, V, 3))
    p = rng.normal(0, 0.3, (n, K, 3))
    p[1, 5] = np.nan
    index, _ = O.forward(v.astype(np.float32), p.astype(np.float32))
    index[0, 3] = -1  # no contribution
    g = rng.normal(size=(n, V))
    g[1, 7] = 0.0
    vt, pt = torch.tensor(v), torch.tensor(p)
    gv, gp = O.vjp(vt, pt, index, g)
    cv, cp = O.closed_form(vt, pt, index, g)
    assert torch.isfinite(gv).all() and torch.isfinite(gp).all()
    np.testing.assert_allclose(gv.numpy(), cv.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(gp.numpy(), cp.numpy(), rtol=1e-12, atol=1e-15)
    assert (gv[0, 3] == 0).all() and (gv[1, 7] == 0).all() and (gp[1, 5] == 0).all()
    h = 1e-6

    def f(vv, pp):
        return float((O.sqdist(torch.tensor(vv), torch.tensor(pp), index) * torch.tensor(g)).sum())

    for (a, b, x) in [(0, 0, 0), (0, 11, 2), (1, 29, 1), (1, 3, 0)]:
        vp, vm = v.copy(), v.copy()
        vp[a, b, x] += h
        vm[a, b, x] -= h
        num = (f(vp, p) - f(vm, p)) / (2 * h)
        assert abs(num - float(gv[a, b, x])) <= 1e-7 * max(1.0, abs(num)), (a, b, x)
    for (a, k, x) in [(0, int(index[0, 0]), 1), (1, int(index[1, 2]), 2)]:
        pp, pm = p.copy(), p.copy()
        pp[a, k, x] += h
        pm[a, k, x] -= h
        num = (f(v, pp) - f(v, pm)) / (2 * h)
        assert abs(num - float(gp[a, k, x])) <= 1e-7 * max(1.0, abs(num)), (a, k, x)


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


def test_mesh_point_distance_binding(stub, smpl):
    from smplpp_amd._lib import HOST

    verts = np.zeros((N, V, 3), np.float32)
    index, sq = smpl.meshPointDistance(verts, np.zeros((N, 5, 3)))
    h, n, v, K, pts, pi, ps, space, stream = stub.last("smplpp_mesh_point_distance")
    assert (n, K, space, stream) == (N, 5, HOST, None)
    assert v == _addr(verts) and isinstance(pts, int)
    assert index.shape == (N, V) and index.dtype == np.int64
    assert sq.shape == (N, V) and sq.dtype == np.float32
    assert (pi, ps) == (_addr(index), _addr(sq))


def test_mesh_point_distance_backward_binding(stub, smpl):
    from smplpp_amd._lib import HOST

    verts, pts = np.zeros((N, V, 3), np.float32), np.zeros((N, 4, 3), np.float32)
    index, g = np.zeros((N, V), np.int64), np.ones((N, V), np.float32)
    gv, gp = smpl.meshPointDistanceBackward(verts, pts, index, g)
    h, n, v, K, p, pi, pg, pgv, pgp, acc, space, stream = stub.last("smplpp_mesh_point_distance_vjp")
    assert (n, K, acc, space, stream) == (N, 4, 0, HOST, None)
    assert v == _addr(verts) and p == _addr(pts) and pi == _addr(index) and pg == _addr(g)
    assert gv.shape == (N, V, 3) and gv.dtype == np.float32 and pgv == _addr(gv)
    assert gp.shape == (N, 4, 3) and gp.dtype == np.float32 and pgp == _addr(gp)

    out = np.zeros((N, V, 3), np.float32)
    gv, gp = smpl.meshPointDistanceBackward(verts, pts, torch.zeros((N, V), dtype=torch.int64), g, out=out)
    *_, pgv, pgp, acc, _, _ = stub.last("smplpp_mesh_point_distance_vjp")
    assert acc == 1 and gv is out and pgv == _addr(out)
    assert pgp == _addr(gp) and (gp == 0).all()  # the other output starts at zero when the call adds

    gpo = np.ones((N, 4, 3), np.float32)
    gv, gp = smpl.meshPointDistanceBackward(verts, pts, index.astype(np.int32), g, grad_points=gpo)
    *_, pgv, pgp, acc, _, _ = stub.last("smplpp_mesh_point_distance_vjp")
    assert acc == 1 and gp is gpo and pgp == _addr(gpo) and pgv == _addr(gv) and (gv == 0).all()


def test_mesh_point_distance_refuses(stub, smpl):
    verts, pts = np.zeros((N, V, 3), np.float32), np.zeros((N, 4, 3), np.float32)
    index, g = np.zeros((N, V), np.int64), np.ones((N, V), np.float32)
    _refused(stub, smpl.meshPointDistance, verts, pts[0])
    _refused(stub, smpl.meshPointDistance, verts, pts[:1])
    _refused(stub, smpl.meshPointDistance, verts, np.zeros((N, 0, 3), np.float32))
    _refused(stub, smpl.meshPointDistance, verts, np.zeros((N, 4, 2), np.float32))
    _refused(stub, smpl.meshPointDistance, verts[:, :-1], pts)
    _refused(stub, smpl.meshPointDistance, verts, torch.from_numpy(pts))
    _refused(stub, smpl.meshPointDistanceBackward, verts, pts, index[:, :-1], g)
    _refused(stub, smpl.meshPointDistanceBackward, verts, pts, index, g[:, :-1])
    _refused(stub, smpl.meshPointDistanceBackward, verts, pts, index, g, out=np.zeros((N, V, 3), np.float64))
    _refused(stub, smpl.meshPointDistanceBackward, verts, pts, index, g, grad_points=np.zeros((N, 3, 3), np.float32))
    _refused(stub, smpl.meshPointDistanceBackward, verts, pts, index, g, out=torch.zeros((N, V, 3)))
    _refused(stub, smpl.mesh_point_distance_differentiable, verts, pts)
