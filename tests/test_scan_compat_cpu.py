"""The normal-compatible, distance-capped correspondences without a GPU: the entry points are declared, exported and bound; the fp32
compatibility rule of tests/scan_compat_oracle.py against the float64 angle test, with the threshold, zero-normal and NaN cases
asserted by hand; the oracle's unfused face normal and its masked mesh-to-point scan pinned to plainer statements; and the Python
methods' marshalling through a recording stub in place of the library."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_point_distance_oracle as MO  # noqa: E402
import scan_compat_oracle as O  # noqa: E402

SYMBOLS = {"smplpp_point_mesh_distance_compatible": 14, "smplpp_mesh_point_distance_compatible": 13}


def test_declared_exported_bound():
    from smplpp_amd import _lib

    L = _lib.load()
    for name, nargs in SYMBOLS.items():
        assert name in _lib.declared_symbols()
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name


def test_without_gpu_or_model_raises_and_leaves_outputs():
    from smplpp_amd import _lib

    L = _lib.load()
    v = np.zeros((1, 4, 3), np.float32)
    p = np.zeros((1, 2, 3), np.float32)
    ids = np.full((1, 4), 5, np.int64)
    sq = np.full((1, 4), 7.0, np.float32)
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_point_mesh_distance_compatible(None, 1, v.ctypes.data, 2, p.ctypes.data, None, 0.5, float("inf"), ids.ctypes.data,
                                                           None, None, sq.ctypes.data, 0, None))
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_mesh_point_distance_compatible(None, 1, v.ctypes.data, None, 2, p.ctypes.data, None, 0.5, float("inf"),
                                                           ids.ctypes.data, sq.ctypes.data, 0, None))
    assert (sq == 7.0).all() and (ids == 5).all()


# ---------------------------------------------------------------------------------------------------- the fp32 rule
def _pairs(seed, count=200000):
    """Random normal pairs of lengths in [1e-3, 1e3] (the library does not normalise), a tenth of them close to each other."""
    rng = np.random.default_rng(seed)
    m = rng.normal(size=(count, 3))
    q = rng.normal(size=(count, 3))
    near = rng.random(count) < 0.1
    q[near] = m[near] + 0.3 * rng.normal(size=(int(near.sum()), 3))
    m *= 10.0 ** rng.uniform(-3, 3, (count, 1)) / np.linalg.norm(m, axis=1, keepdims=True)
    q *= 10.0 ** rng.uniform(-3, 3, (count, 1)) / np.linalg.norm(q, axis=1, keepdims=True)
    return m.astype(np.float32), q.astype(np.float32)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("cos_min", [0.0, 0.5, 0.9])
def test_rule_agrees_with_float64_angle_test(seed, cos_min):
    m, q = _pairs(seed)
    got = O.compatible(m, q, cos_min)
    want, c = O.compatible_f64(m, q, cos_min)
    skip = np.abs(c - cos_min) < 1e-5
    assert skip.mean() <= 0.01, skip.mean()
    assert (got[~skip] == want[~skip]).all(), np.nonzero(got[~skip] != want[~skip])[0][:5]
    assert 0.02 < got.mean() < 0.98  # both outcomes are exercised


def test_rule_threshold_zero_and_nan_cases():
    one = np.float32(1)
    # exactly on the threshold: 60 degrees at cos_min = 0.5 (s = 1, mm = qq = 2: 1 >= 0.25 * 4), kept (>=)
    assert O.compatible([1, 1, 0], [1, 0, 1], 0.5)
    # ... and one ulp of q.z beyond it
    assert not O.compatible([1, 1, 0], [1, 0, np.nextafter(one, np.float32(2))], 0.5)
    assert O.compatible([1, 1, 0], [1, 0, np.nextafter(one, np.float32(0))], 0.5)
    # orthogonal normals at cos_min = 0 (s = 0 >= 0), and the first negative s
    assert O.compatible([1, 0, 0], [0, 1, 0], 0.0)
    assert not O.compatible([1, 0, 0], [-np.float32(1e-30), 1, 0], 0.0)
    # cos_min = 1: parallel normals of any length pass, s^2 = mm qq exactly
    assert O.compatible([3, 4, 0], [3, 4, 0], 1.0) and O.compatible([3, 4, 0], [6, 8, 0], 1.0)
    assert not O.compatible([3, 4, 0], [3, 4, 1], 1.0)
    # opposite normals never pass, whatever cos_min
    assert not O.compatible([0, 0, 1], [0, 0, -1], 0.0)
    # a zero normal on either side (mm qq = 0), at every cos_min
    for c in (0.0, 0.5, 1.0):
        assert not O.compatible([0, 0, 0], [0, 0, 1], c) and not O.compatible([0, 0, 1], [0, 0, 0], c)
        assert not O.compatible([0, 0, 0], [0, 0, 0], c)
    # a NaN anywhere
    for i in range(3):
        bad = np.array([0, 0, 1], np.float32)
        bad[i] = np.nan
        assert not O.compatible(bad, [0, 0, 1], 0.0) and not O.compatible([0, 0, 1], bad, 0.0)
    # broadcasting
    r = O.compatible(np.array([[0, 0, 1], [0, 0, -1]], np.float32)[:, None, :], np.array([[0, 0, 2], [0, 1, 0]], np.float32)[None], 0.5)
    assert r.tolist() == [[True, False], [False, False]]


def test_rule_is_unfused():
    """s must be ((m.x q.x + m.y q.y) + m.z q.z) with every product rounded: a pair for which an FMA gives another sign."""
    a = np.float32(1 + 2.0 ** -12)
    m = np.array([a, a, 0], np.float32)
    q = np.array([a, -a, 0], np.float32)
    assert O.dot3(m, q) == 0 and O.compatible(m, q, 0.0)  # the rounded products cancel exactly
    # (an fma(m.x, q.x, m.y q.y) would keep the product's low bits; the sign of s could then go either way)
    x = np.float32(np.float32(a * a))
    assert float(x) != float(a) * float(a)


def test_face_normals_unfused_and_degenerate():
    rng = np.random.default_rng(3)
    v = rng.normal(size=(30, 3)).astype(np.float32)
    faces = np.stack([rng.permutation(30)[:3] for _ in range(50)])
    faces[7] = (4, 4, 9)  # a degenerate face: m = 0
    v[12] = v[13]
    faces[8] = (12, 13, 2)  # coincident vertices
    m = O.face_normals(v, faces)
    for f in range(len(faces)):
        a, b, c = (v[i] for i in faces[f])
        e1, e2 = b - a, c - a
        want = [np.float32(e1[1] * e2[2]) - np.float32(e1[2] * e2[1]), np.float32(e1[2] * e2[0]) - np.float32(e1[0] * e2[2]),
                np.float32(e1[0] * e2[1]) - np.float32(e1[1] * e2[0])]
        assert m[f].tolist() == [float(x) for x in want]
    assert (m[7] == 0).all() and (m[8] == 0).all()
    assert not O.compatible(m[[7, 8]], [0, 0, 1], 0.0).any()
    ref = np.cross(v[faces[:, 1]].astype(np.float64) - v[faces[:, 0]], v[faces[:, 2]].astype(np.float64) - v[faces[:, 0]])
    assert np.abs(m - ref).max() <= 1e-5


def test_candidates_non_finite_rows():
    rng = np.random.default_rng(4)
    v = rng.normal(size=(20, 3)).astype(np.float32)
    faces = np.stack([rng.permutation(20)[:3] for _ in range(30)])
    P = rng.normal(size=(6, 3)).astype(np.float32)
    N = rng.normal(size=(6, 3)).astype(np.float32)
    P[1, 0] = np.nan
    N[2, 1] = np.inf
    P[3, 2] = -np.inf
    c = O.candidates(v, faces, P, N, 0.0)
    assert c.shape == (6, 30) and not c[[1, 2, 3]].any() and c[[0, 4, 5]].any(1).all()
    assert (c[0] == O.compatible(O.face_normals(v, faces), N[0], 0.0)).all()
    c = O.candidates(v, faces, P, None, 0.5)
    assert c[[0, 2, 4, 5]].all() and not c[[1, 3]].any()


def test_masked_mesh_point_scan():
    rng = np.random.default_rng(5)
    v = rng.normal(0, 0.3, (2, 300, 3)).astype(np.float32)
    p = rng.normal(0, 0.3, (2, 2500, 3)).astype(np.float32)  # several oracle chunks
    p[0, 7] = np.nan
    # no mask: the unfiltered oracle, bit for bit
    i0, s0 = MO.forward(v, p)
    i1, s1 = O.mesh_point_forward(v, None, p, None, 0.5, np.inf)
    assert (i0 == i1).all() and s0.tobytes() == s1.tobytes()
    # a cap on an attained distance keeps it; the next float below drops that vertex to its next choice or to -1
    cap = np.float32(np.sort(s0[0])[150])
    i2, s2 = O.mesh_point_forward(v, None, p, None, 0.5, cap)
    keep = s0 <= cap
    assert (i2[keep] == i0[keep]).all() and (i2[~keep] == -1).all() and (s2[~keep] == 0).all()
    i3, _ = O.mesh_point_forward(v, None, p, None, 0.5, np.nextafter(cap, np.float32(0)))
    assert (i3[0][s0[0] == cap] == -1).all() and (i3 >= 0).sum() < (i2 >= 0).sum()
    # normals: the plain statement, one pair at a time, on a small case
    vn = rng.normal(size=(2, 300, 3)).astype(np.float32)
    pn = rng.normal(size=(2, 2500, 3)).astype(np.float32)
    vn[1, 5] = np.nan
    pn[1, 9] = np.inf
    vn[0, 3] = 0
    i4, s4 = O.mesh_point_forward(v, vn, p, pn, 0.5, 0.05)
    assert (i4[1, 5] == -1) and (i4[0, 3] == -1) and not (i4[1] == 9).any()
    for f, u in [(0, 0), (0, 17), (1, 5), (1, 123), (1, 299)]:
        bk, bd = -1, np.float32(np.inf)
        for k in range(p.shape[1]):
            dx, dy, dz = v[f, u] - p[f, k]
            d = np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz)
            ok = np.isfinite(d) and d <= np.float32(0.05) and np.isfinite(vn[f, u]).all() and np.isfinite(pn[f, k]).all()
            if ok and O.compatible(vn[f, u], pn[f, k], 0.5) and d < bd:
                bk, bd = k, d
        assert i4[f, u] == bk and s4[f, u] == (bd if bk >= 0 else 0)


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


def test_point_mesh_binding(stub, smpl):
    from smplpp_amd._lib import HOST

    verts = np.zeros((N, V, 3), np.float32)
    pts, nrm = np.zeros((N, 5, 3), np.float32), np.ones((N, 5, 3), np.float32)
    face, w, closest, sq, matched = smpl.pointMeshDistanceCompatible(verts, pts, nrm, cos_min=0.25, max_dist=0.5)
    h, n, v, K, p, pn, cm, cap, pf, pw, pc, ps, space, stream = stub.last("smplpp_point_mesh_distance_compatible")
    assert (n, K, space, stream) == (N, 5, HOST, None) and (cm, cap) == (0.25, 0.25)
    assert (v, p, pn) == (_addr(verts), _addr(pts), _addr(nrm))
    assert (pf, pw, pc, ps) == (_addr(face), _addr(w), _addr(closest), _addr(sq))
    assert face.dtype == np.int64 and face.shape == (N, 5) and matched.dtype == bool and matched.shape == (N, 5)
    # the cap is the fp32 square of the fp32 distance; max_sqdist passes through; the defaults
    smpl.pointMeshDistanceCompatible(verts, pts, None, max_dist=0.05)
    *_, pn, cm, cap, _, _, _, _, _, _ = stub.last("smplpp_point_mesh_distance_compatible")
    assert pn is None and cm == 0.5 and cap == float(np.float32(0.05) * np.float32(0.05))
    smpl.pointMeshDistanceCompatible(verts, pts, nrm, max_sqdist=np.float32(0.3))
    assert stub.last("smplpp_point_mesh_distance_compatible")[7] == float(np.float32(0.3))
    smpl.pointMeshDistanceCompatible(verts, pts, nrm)
    assert stub.last("smplpp_point_mesh_distance_compatible")[7] == float("inf")


def test_point_mesh_backward_substitutes_unmatched(stub, smpl):
    verts, pts = np.zeros((N, V, 3), np.float32), np.zeros((N, 4, 3), np.float32)
    face = np.array([[3, -1, 5, -1], [-1, 0, 1, 2]], np.int64)
    g = np.arange(1, 9, dtype=np.float32).reshape(N, 4)
    seen = {}
    inner = smpl.pointMeshDistanceBackward

    def spy(verts, points, face, grad_sqdist, out=None, grad_points=None):
        seen["face"], seen["g"] = np.array(face), np.array(grad_sqdist)
        return inner(verts, points, face, grad_sqdist, out, grad_points)

    smpl.pointMeshDistanceBackward = spy
    gv, gp = smpl.pointMeshDistanceCompatibleBackward(verts, pts, face, g)
    assert stub.last("smplpp_point_mesh_distance_vjp")[1] == N and gv.shape == (N, V, 3) and gp.shape == (N, 4, 3)
    assert seen["face"].tolist() == [[3, 0, 5, 0], [0, 0, 1, 2]]
    assert seen["g"].tolist() == [[1, 0, 3, 0], [0, 6, 7, 8]] and seen["g"].dtype == np.float32
    assert face[0, 1] == -1 and g[0, 1] == 2  # the caller's arrays are left alone


def test_mesh_point_binding(stub, smpl):
    from smplpp_amd._lib import HOST

    verts = np.zeros((N, V, 3), np.float32)
    pts, nrm, vn = np.zeros((N, 5, 3), np.float32), np.ones((N, 5, 3), np.float32), np.ones((N, V, 3), np.float32)
    index, sq, matched = smpl.meshPointDistanceCompatible(verts, pts, nrm, vert_normals=vn, cos_min=0.0, max_dist=2.0)
    h, n, v, pvn, K, p, pn, cm, cap, pi, ps, space, stream = stub.last("smplpp_mesh_point_distance_compatible")
    assert (n, K, space, stream) == (N, 5, HOST, None) and (cm, cap) == (0.0, 4.0)
    assert (v, pvn, p, pn, pi, ps) == (_addr(verts), _addr(vn), _addr(pts), _addr(nrm), _addr(index), _addr(sq))
    assert index.shape == (N, V) and matched.shape == (N, V) and matched.dtype == bool
    # vert_normals None: the whole-mesh normals call first, its output passed on
    before = len(stub.calls)
    smpl.meshPointDistanceCompatible(verts, pts, nrm)
    names = [c[0] for c in stub.calls[before:]]
    assert names == ["smplpp_mesh_vertex_normals", "smplpp_mesh_point_distance_compatible"]
    assert stub.calls[-1][1][3] == stub.calls[-2][1][3] and stub.calls[-1][1][3] is not None
    # no point normals: no normal test, no normals call
    before = len(stub.calls)
    smpl.meshPointDistanceCompatible(verts, pts, None)
    assert [c[0] for c in stub.calls[before:]] == ["smplpp_mesh_point_distance_compatible"]
    assert stub.calls[-1][1][3] is None and stub.calls[-1][1][6] is None


def test_refuses(stub, smpl):
    verts, pts = np.zeros((N, V, 3), np.float32), np.zeros((N, 4, 3), np.float32)
    nrm = np.zeros((N, 4, 3), np.float32)
    _refused(stub, smpl.pointMeshDistanceCompatible, verts, pts, nrm[:, :-1])
    _refused(stub, smpl.pointMeshDistanceCompatible, verts, pts[0], nrm)
    _refused(stub, smpl.pointMeshDistanceCompatible, verts, pts, torch.from_numpy(nrm))
    _refused(stub, smpl.meshPointDistanceCompatible, verts, pts, nrm[:1])
    _refused(stub, smpl.meshPointDistanceCompatible, verts, pts, nrm, vert_normals=np.zeros((N, V - 1, 3), np.float32))
    _refused(stub, smpl.point_mesh_distance_compatible_differentiable, verts, pts, nrm)
    _refused(stub, smpl.mesh_point_distance_compatible_differentiable, verts, pts, nrm)
