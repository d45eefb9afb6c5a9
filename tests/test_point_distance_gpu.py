"""The point-to-mesh distance on the MI355X (smplpp_point_mesh_distance, smplpp_point_mesh_distance_vjp): the forward's bits against
smplpp_closest_points in every dispatch form, the weights, the backward against float64 autograd of tests/point_distance_oracle.py,
the tie property, determinism, call semantics, end-to-end gradients and a fit through forward_differentiable, and the C++ shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_ref as cr  # noqa: E402
import point_distance_oracle as O  # noqa: E402
from distance_cases import _rel, _same_bits, _surface_points, _verts  # noqa: E402

torch = O.torch
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("auto", "query", "tiled")


def _smpl(model, form="auto"):
    from smplpp_amd.smpl import SMPL

    old = os.environ.pop("SMPLPP_POINT_DISTANCE_FORM", None)
    try:
        if form != "auto":
            os.environ["SMPLPP_POINT_DISTANCE_FORM"] = form  # read once, at model creation
        s = SMPL()
        s.setDevice("cuda:0")
        s.init(model)
    finally:
        os.environ.pop("SMPLPP_POINT_DISTANCE_FORM", None)
        if old is not None:
            os.environ["SMPLPP_POINT_DISTANCE_FORM"] = old
    return s


@pytest.fixture(scope="module")
def forms(synth_model):
    return {f: _smpl(synth_model, f) for f in FORMS}


@pytest.fixture(scope="module")
def smpl(forms):
    return forms["auto"]


@pytest.fixture(scope="module")
def faces(synth_model):
    return synth_model["face_indices"].astype(np.int64) - 1


def _closest_points(s, verts, points):
    from smplpp_amd import _lib
    from smplpp_amd._lib import HOST, check
    from smplpp_amd.smpl import _ptr

    verts, points = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(points, np.float32)
    n, K = points.shape[:2]
    face, closest, sq = np.empty((n, K), np.int64), np.empty((n, K, 3), np.float32), np.empty((n, K), np.float32)
    check(_lib.load().smplpp_closest_points(s.handle, n, _ptr(verts), K, _ptr(points), _ptr(face), _ptr(closest), _ptr(sq), HOST, None))
    return face, closest, sq


def _assert_forward_bits(s, v, P):
    face, w, closest, sq = s.pointMeshDistance(v, P)
    rf, rc, rs = _closest_points(s, v, P)
    bad = np.nonzero((face != rf) | (sq.view(np.int32) != rs.view(np.int32)))
    assert len(bad[0]) == 0, (bad[0][:5], bad[1][:5], face[bad][:5], rf[bad][:5], sq[bad][:5], rs[bad][:5])
    assert _same_bits(face, rf) and _same_bits(closest, rc) and _same_bits(sq, rs)
    return face, w, closest, sq


# ---------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("form", FORMS)
def test_forward_bits_every_query_class(forms, faces, form):
    s = forms[form]
    v = _verts(s, 2, seed=3)
    rng = np.random.default_rng(5)
    edges = cr.shared_edges(faces)
    P = np.stack([np.concatenate([cr.make_queries(v[f], faces, c, 24, rng, edges) for c in cr.CLASSES]) for f in range(2)])
    face, w, closest, sq = _assert_forward_bits(s, v, P)
    # the choice passes the exhaustive rule
    for f in range(2):
        D = cr.mesh_sqdist(v[f], faces, P[f], also=face[f])
        ec = cr.eps_c(v[f], faces, P[f])
        for q in range(P.shape[1]):
            msg = cr.check_choice(D[q], ec[q], face[f, q])
            assert msg is None, (form, f, q, msg)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,K", [(3, 1), (2, 63), (5, 64), (2, 257), (1, 4096), (3, 4096)])
def test_forward_bits_sizes(forms, faces, form, n, K):
    s = forms[form]
    v = _verts(s, n, seed=K)
    rng = np.random.default_rng(n * 1000 + K)
    P = _surface_points(v, faces, K, rng)
    far = rng.random((n, K)) < 0.1  # some points 0.25 m off
    P[far] += np.float32(0.25) * rng.normal(size=(int(far.sum()), 3)).astype(np.float32)
    _assert_forward_bits(s, v, P)


def test_forward_nan_and_far_points_every_form(forms, faces):
    v = _verts(forms["auto"], 2, seed=9)
    rng = np.random.default_rng(9)
    P = _surface_points(v, faces, 80, rng)
    P[0, 3] = np.nan
    P[1, 70:] = np.nan
    P[1, 10] = (40.0, -3.0, 2.0)
    for s in forms.values():
        _assert_forward_bits(s, v, P)


def test_weights(smpl, faces):
    v = _verts(smpl, 2, seed=4)
    rng = np.random.default_rng(4)
    edges = cr.shared_edges(faces)
    for cls in cr.CLASSES:
        P = np.stack([cr.make_queries(v[f], faces, cls, 64, rng, edges) for f in range(2)])
        face, w, closest, sq = smpl.pointMeshDistance(v, P)
        # non-negative up to rounding: at a region boundary the branch's own parameter can round to a few ulps below 0
        assert (w >= -2e-6).all() and np.abs(w.sum(-1) - 1).max() <= 1e-6, (cls, w.min())
        tri = np.stack([v[f][faces[face[f]]] for f in range(2)]).astype(np.float64)  # [n,K,3,3]
        rec = np.einsum("nkj,nkjx->nkx", w.astype(np.float64), tri)
        scale = 1.0 + np.abs(tri).max()
        assert np.abs(rec - closest).max() <= 1e-6 * scale, cls
        # where the closest point is a vertex (the float64 region of the chosen face), the weights are exactly one-hot
        tt = torch.from_numpy(tri)
        reg = O.region(torch.from_numpy(P.astype(np.float64)), tt[:, :, 0], tt[:, :, 1], tt[:, :, 2]).numpy()
        at_vertex = reg <= 2
        onehot = (np.sort(w, -1) == np.array([0, 0, 1], np.float32)).all(-1)
        if at_vertex.sum():
            assert onehot[at_vertex].mean() >= 0.99, (cls, onehot[at_vertex].mean())
            assert (w[at_vertex][np.arange(at_vertex.sum()), reg[at_vertex]] >= 1 - 1e-6).mean() >= 0.99


# ---------------------------------------------------------------------------------------------------- backward
def _check_vjp(v, faces, P, face, g, gv, gp):
    """House tolerance: within 4x the error of an fp32 autograd of the same graph, or 1e-5 relative, per frame."""
    for f in range(len(v)):
        sl = slice(f, f + 1)
        args = (faces, face[sl], g[sl])
        rv, rp = O.vjp(torch.tensor(v[sl], dtype=torch.float64), faces, torch.tensor(P[sl], dtype=torch.float64), face[sl], g[sl])
        fv, fp = O.vjp(torch.tensor(v[sl]), args[0], torch.tensor(P[sl]), face[sl], torch.tensor(g[sl]))
        for got, ref, f32, name in ((gv[sl], rv.numpy(), fv.numpy(), "verts"), (gp[sl], rp.numpy(), fp.numpy(), "points")):
            assert np.isfinite(got).all()
            bar = max(4 * _rel(f32, ref), 1e-5)
            err = _rel(got, ref)
            assert err <= bar, (f, name, err, bar)


@pytest.mark.parametrize("form", ["query", "tiled"])
@pytest.mark.parametrize("n,K", [(1, 7), (3, 500), (2, 4096)])
def test_backward_vs_float64_autograd(forms, faces, form, n, K):
    s = forms[form]
    v = _verts(s, n, seed=K + 1)
    rng = np.random.default_rng(K)
    P = _surface_points(v, faces, K, rng)
    face, _, _, _ = s.pointMeshDistance(v, P)
    g = rng.normal(size=(n, K)).astype(np.float32)
    gv, gp = s.pointMeshDistanceBackward(v, P, face, g)
    _check_vjp(v, faces, P, face, g, gv, gp)


@pytest.mark.parametrize("cls", ["edge_region", "vertex_region"])
def test_tied_faces_give_the_same_gradient(smpl, faces, cls):
    """The tie rule does not move the gradient: where another face shares the chosen face's closest point (tied within 1e-6 in
    float64, the same float64 closest point to 1e-7 m), its product agrees with the chosen face's to fp32 rounding."""
    v = _verts(smpl, 1, seed=21)
    rng = np.random.default_rng(21)
    P = cr.make_queries(v[0], faces, cls, 256, rng)[None]
    face, _, _, _ = smpl.pointMeshDistance(v, P)
    D = cr.mesh_sqdist(v[0], faces, P[0], also=face[0])
    g = np.ones((1, P.shape[1]), np.float32)
    other = face.copy()
    vf = v[0].astype(np.float64)
    for k in range(P.shape[1]):
        tied = np.nonzero(D[k] <= D[k].min() * (1 + 1e-6))[0]
        _, C = cr.tri_sqdist(np.broadcast_to(P[0, k], (len(tied), 3)), vf[faces[tied, 0]], vf[faces[tied, 1]], vf[faces[tied, 2]])
        c0 = cr.tri_sqdist(P[0, k], *vf[faces[face[0, k]]])[1]
        alt = [f for f, c in zip(tied, C) if f != face[0, k] and np.abs(c - c0).max() <= 1e-7]
        if alt:
            other[0, k] = alt[0]
    changed = other != face
    assert changed.sum() >= 30, changed.sum()
    gv1, gp1 = smpl.pointMeshDistanceBackward(v, P, face, g)
    gv2, gp2 = smpl.pointMeshDistanceBackward(v, P, other, g)
    assert np.abs(gp1 - gp2).max() <= 1e-5 * np.abs(gp1).max()
    assert np.abs(gv1 - gv2).max() <= 1e-5 * np.abs(gv1).max()


# ---------------------------------------------------------------------------------------------------- determinism
def test_repeat_and_batch_independence(forms, faces):
    for form in ("query", "tiled"):
        s = forms[form]
        v = _verts(s, 4, seed=31)
        rng = np.random.default_rng(31)
        P = _surface_points(v, faces, 300, rng)
        g = rng.normal(size=(4, 300)).astype(np.float32)
        fw = s.pointMeshDistance(v, P)
        bw = s.pointMeshDistanceBackward(v, P, fw[0], g)
        fw2 = s.pointMeshDistance(v, P)
        bw2 = s.pointMeshDistanceBackward(v, P, fw[0], g)
        assert all(_same_bits(a, b) for a, b in zip(fw + bw, fw2 + bw2))
        # frame 2 alone, and frames (2, 0): the bits of frame 2 do not depend on n or on the slot
        for sel in ([2], [2, 0], [3, 1, 2]):
            i = sel.index(2)
            f1 = s.pointMeshDistance(v[sel], P[sel])
            b1 = s.pointMeshDistanceBackward(v[sel], P[sel], f1[0], g[sel])
            assert all(_same_bits(a[i], b[2]) for a, b in zip(f1 + b1, fw + bw)), (form, sel)


def test_hot_vertex(forms, faces):
    """4096 points around one vertex: every record of the batch lands on a handful of vertices."""
    s = forms["auto"]
    v = _verts(s, 2, seed=41)
    rng = np.random.default_rng(41)
    u = int(faces[100, 0])
    P = (v[:, u][:, None, :] + rng.normal(0, 1e-3, (2, 4096, 3))).astype(np.float32)
    for fs in forms.values():
        _assert_forward_bits(fs, v, P)
    face, _, _, _ = s.pointMeshDistance(v, P)
    g = rng.normal(size=(2, 4096)).astype(np.float32)
    gv, gp = s.pointMeshDistanceBackward(v, P, face, g)
    assert _same_bits(gv, s.pointMeshDistanceBackward(v, P, face, g)[0])
    _check_vjp(v, faces, P, face, g, gv, gp)


def _fp32_vjp(faces, P, face, closest, w, g, V):
    """The backward's fp32 arithmetic and order, from the forward's closest and weights: rr = p - closest, grad_points = (2 g) rr,
    corner j gets ((-2 g) w_j) rr; grad_verts a sum from +0 per vertex, in ascending query, then corner, over the g != 0."""
    n, K = face.shape
    f = np.arange(n)
    live = g != 0
    rr = P - closest
    gp = np.where(live[..., None], (2 * g)[..., None] * rr, np.float32(0))
    c = ((-2 * g)[..., None] * w)[..., None] * rr[:, :, None, :]
    corner = faces[face]
    gv = np.zeros((n, V, 3), np.float32)
    for k in range(K):
        m = live[:, k]
        for j in range(3):
            gv[f[m], corner[m, k, j]] += c[m, k, j]
    return gv, gp


@pytest.mark.parametrize("case", ["surface", "hot_vertex"])
def test_backward_bits_vs_fp32_restatement(forms, faces, case):
    """Every bit (tiled form): K > 1024 records (several LDS tiles), 6890 vertices (several target blocks), a hot vertex; zero g."""
    s = forms["tiled"]
    rng = np.random.default_rng(97)
    if case == "surface":
        v = _verts(s, 3, seed=97)
        P = _surface_points(v, faces, 3000, rng)
    else:
        v = _verts(s, 2, seed=41)
        P = (v[:, int(faces[100, 0])][:, None, :] + rng.normal(0, 1e-3, (2, 4096, 3))).astype(np.float32)
    face, w, closest, _ = s.pointMeshDistance(v, P)
    g = rng.normal(size=face.shape).astype(np.float32)
    g[rng.random(g.shape) < 0.1] = 0
    gv, gp = s.pointMeshDistanceBackward(v, P, face, g)
    rv, rp = _fp32_vjp(faces, P, face, closest, w, g, s.vertex_num)
    assert _same_bits(gp, rp)
    assert _same_bits(gv, rv), np.nonzero(gv != rv)[:2]


# ---------------------------------------------------------------------------------------------------- call semantics
def _raw_vjp(s, v, P, face, g, gv, gp, acc, space=0):
    from smplpp_amd import _lib
    from smplpp_amd.smpl import _ptr

    n, K = face.shape
    return _lib.load().smplpp_point_mesh_distance_vjp(s.handle, n, _ptr(v), K, _ptr(P), _ptr(face), _ptr(g), _ptr(gv), _ptr(gp), acc,
                                                      space, None)


def test_call_semantics(smpl, faces):
    from smplpp_amd import _lib

    v = _verts(smpl, 2, seed=51)
    rng = np.random.default_rng(51)
    K = 200
    P = _surface_points(v, faces, K, rng)
    face, _, _, _ = smpl.pointMeshDistance(v, P)
    g = rng.normal(size=(2, K)).astype(np.float32)
    gv, gp = smpl.pointMeshDistanceBackward(v, P, face, g)
    V = smpl.vertex_num
    # accumulate = 0 overwrites whatever is there (untouched vertices get 0)
    ov, op = np.full((2, V, 3), 7.0, np.float32), np.full((2, K, 3), 7.0, np.float32)
    assert _raw_vjp(smpl, v, P, face, g, ov, op, 0) == 0
    assert _same_bits(ov, gv) and _same_bits(op, gp)
    touched = np.zeros(V, bool)
    touched[faces[face].reshape(-1)] = True
    assert (gv[:, ~touched] == 0).all()
    # accumulate = 1 adds
    base_v, base_p = rng.normal(size=(2, V, 3)).astype(np.float32), rng.normal(size=(2, K, 3)).astype(np.float32)
    av, ap = smpl.pointMeshDistanceBackward(v, P, face, g, out=base_v.copy(), grad_points=base_p.copy())
    assert _same_bits(av, base_v + gv) and _same_bits(ap, base_p + gp)
    # either output NULL
    ov = np.full((2, V, 3), 7.0, np.float32)
    assert _raw_vjp(smpl, v, P, face, g, ov, None, 0) == 0 and _same_bits(ov, gv)
    op = np.full((2, K, 3), 7.0, np.float32)
    assert _raw_vjp(smpl, v, P, face, g, None, op, 0) == 0 and _same_bits(op, gp)
    # forward with weights / closest NULL: the same face and sqdist
    from smplpp_amd.smpl import _ptr

    f2, s2 = np.empty((2, K), np.int64), np.empty((2, K), np.float32)
    fw = smpl.pointMeshDistance(v, P)
    assert _lib.load().smplpp_point_mesh_distance(smpl.handle, 2, _ptr(v), K, _ptr(P), _ptr(f2), None, None, _ptr(s2), 0, None) == 0
    assert _same_bits(f2, fw[0]) and _same_bits(s2, fw[3])


def test_zero_cotangent_nan_rows(smpl, faces):
    """Ragged scans padded with NaN rows: a zero cotangent there contributes nothing, and the bits are those of the unpadded call."""
    v = _verts(smpl, 2, seed=61)
    rng = np.random.default_rng(61)
    K, pad = 150, 40
    P = _surface_points(v, faces, K, rng)
    Pp = np.concatenate([P, np.full((2, pad, 3), np.nan, np.float32)], 1)
    face, _, _, _ = smpl.pointMeshDistance(v, Pp)
    g = rng.normal(size=(2, K)).astype(np.float32)
    gpad = np.concatenate([g, np.zeros((2, pad), np.float32)], 1)
    gv, gp = smpl.pointMeshDistanceBackward(v, Pp, face, gpad)
    assert np.isfinite(gv).all() and np.isfinite(gp).all() and (gp[:, K:] == 0).all()
    gv0, gp0 = smpl.pointMeshDistanceBackward(v, P, face[:, :K], g)
    assert _same_bits(gv, gv0) and _same_bits(gp[:, :K], gp0)


def test_host_and_device_space(smpl, faces):
    v = _verts(smpl, 3, seed=71)
    rng = np.random.default_rng(71)
    P = _surface_points(v, faces, 333, rng)
    g = rng.normal(size=(3, 333)).astype(np.float32)
    hf = smpl.pointMeshDistance(v, P)
    hb = smpl.pointMeshDistanceBackward(v, P, hf[0], g)
    dv, dP, dg = (torch.from_numpy(x).cuda() for x in (v, P, g))
    df = smpl.pointMeshDistance(dv, dP)
    db = smpl.pointMeshDistanceBackward(dv, dP, df[0], dg)
    torch.cuda.synchronize()
    assert all(_same_bits(a, b.cpu().numpy()) for a, b in zip(hf + hb, df + db))
    # a device-space face id out of range contributes nothing
    bad = df[0].clone()
    bad[1, 5] = smpl.face_num
    g0 = dg.clone()
    g0[1, 5] = 0
    b1 = smpl.pointMeshDistanceBackward(dv, dP, bad, dg)
    b0 = smpl.pointMeshDistanceBackward(dv, dP, df[0], g0)
    torch.cuda.synchronize()
    assert _same_bits(b1[0].cpu().numpy(), b0[0].cpu().numpy())
    assert (b1[1][1, 5] == 0).all()


def test_invalid_arguments(smpl):
    from smplpp_amd import _lib
    from smplpp_amd._lib import SmplppError, check
    from smplpp_amd.smpl import _ptr

    L = _lib.load()
    V, F = smpl.vertex_num, smpl.face_num
    v = np.zeros((1, V, 3), np.float32)
    P = np.zeros((1, 4, 3), np.float32)
    face = np.zeros((1, 4), np.int64)
    sq, g = np.zeros((1, 4), np.float32), np.ones((1, 4), np.float32)
    gv = np.zeros((1, V, 3), np.float32)
    h = smpl.handle

    def fwd(*a):
        check(L.smplpp_point_mesh_distance(*a))

    def bwd(*a):
        check(L.smplpp_point_mesh_distance_vjp(*a))

    bad_calls = [
        (fwd, (None, 1, _ptr(v), 4, _ptr(P), _ptr(face), None, None, _ptr(sq), 0, None)),
        (fwd, (h, 0, _ptr(v), 4, _ptr(P), _ptr(face), None, None, _ptr(sq), 0, None)),
        (fwd, (h, 1, _ptr(v), 0, _ptr(P), _ptr(face), None, None, _ptr(sq), 0, None)),
        (fwd, (h, 1, _ptr(v), 4, _ptr(P), None, None, None, _ptr(sq), 0, None)),
        (fwd, (h, 1, _ptr(v), 4, _ptr(P), _ptr(face), None, None, None, 0, None)),
        (fwd, (h, 1, _ptr(v), 4, _ptr(P), _ptr(face), None, None, _ptr(sq), 5, None)),
        (fwd, (h, 1 << 16, _ptr(v), 1 << 16, _ptr(P), _ptr(face), None, None, _ptr(sq), 0, None)),  # n K beyond int32
        (bwd, (h, 1, _ptr(v), 4, _ptr(P), _ptr(face), _ptr(g), None, None, 0, 0, None)),  # both outputs NULL
        (bwd, (h, 1, _ptr(v), 4, _ptr(P), _ptr(face), _ptr(g), _ptr(gv), None, 2, 0, None)),
        (bwd, (h, 1, _ptr(v), 4, _ptr(P), None, _ptr(g), _ptr(gv), None, 0, 0, None)),
        (bwd, (h, 1 << 16, _ptr(v), 1 << 16, _ptr(P), _ptr(face), _ptr(g), _ptr(gv), None, 0, 0, None)),
    ]
    for fn, args in bad_calls:
        with pytest.raises(SmplppError):
            fn(*args)
    for f in (-1, F):
        face[0, 2] = f
        gv[:] = 7.0
        with pytest.raises(SmplppError):
            bwd(h, 1, _ptr(v), 4, _ptr(P), _ptr(face), _ptr(g), _ptr(gv), None, 0, 0, None)
        assert (gv == 7.0).all()


# ---------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_beta_theta_gradient(smpl, synth_model, faces):
    import fk_vjp_oracle as FK
    from smplpp_amd import model_io

    dev = torch.device("cuda")
    beta, theta = model_io.synthetic_inputs(2, seed=81)
    rng = np.random.default_rng(81)
    vt = _verts(smpl, 2, seed=82)
    P = _surface_points(vt, faces, 1000, rng)
    b = torch.from_numpy(beta).to(dev).requires_grad_(True)
    t = torch.from_numpy(theta).to(dev).requires_grad_(True)
    Pd = torch.from_numpy(P).to(dev)
    verts, _ = smpl.forward_differentiable(b, t)
    face, w, sq = smpl.point_mesh_distance_differentiable(verts, Pd)
    assert not face.requires_grad and not w.requires_grad and sq.requires_grad
    sq.mean().backward()
    face = face.cpu().numpy()

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        bb = torch.tensor(beta, dtype=dtype, requires_grad=True)
        tt = torch.tensor(theta, dtype=dtype, requires_grad=True)
        vv = FK.fk(m, bb, tt)["verts"]
        O.sqdist(vv, faces, torch.tensor(P, dtype=dtype), face).mean().backward()
        return bb.grad.double().numpy(), tt.grad.double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for got, want, f32, name in ((b.grad, r64[0], r32[0], "beta"), (t.grad, r64[1], r32[1], "theta")):
        got = got.cpu().numpy()
        bar = max(4 * _rel(f32, want), 1e-5)
        assert _rel(got, want) <= bar, (name, _rel(got, want), bar)


def test_adam_fit_to_point_cloud(smpl, faces):
    """θ fitted to 4096 points sampled from a target pose's surface, with the mean squared point-to-mesh distance alone."""
    dev = torch.device("cuda")
    rng = np.random.default_rng(91)
    theta_t = np.zeros((1, 25, 3), np.float32)
    theta_t[0, 1:] = rng.normal(0, 0.2, (24, 3))
    beta = torch.zeros(1, 10, device=dev)
    with torch.no_grad():
        vt, _ = smpl.forward_differentiable(beta, torch.from_numpy(theta_t).to(dev))
    P = torch.from_numpy(_surface_points(vt.cpu().numpy(), faces, 4096, rng, off=0.0)).to(dev)
    th = torch.zeros(1, 25, 3, device=dev)
    th[0, 0] = torch.from_numpy(theta_t[0, 0]).to(dev)
    th.requires_grad_(True)
    opt = torch.optim.Adam([th], lr=0.02)
    losses = []
    for it in range(400):
        opt.zero_grad()
        v, _ = smpl.forward_differentiable(beta, th)
        _, _, sq = smpl.point_mesh_distance_differentiable(v, P)
        loss = sq.mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] * 100 <= losses[0], (losses[0], losses[-1])


def test_point_distance_cpp_shim(tmp_path):
    from smplpp_amd import model_io

    exe = str(tmp_path / "point_distance_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "point_distance_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    # the program's inputs, restated
    n, K, V = 2, 24, 40
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    P = ((np.arange(n * K * 3, dtype=np.float32).reshape(n, K, 3) % 17) - 8) * np.float32(0.03)
    g = ((np.arange(n * K, dtype=np.float32).reshape(n, K) % 5) - 2) * np.float32(0.25)
    s = _smpl(model)
    v = s.launch(beta, theta, want=("verts",))["verts"]
    face, w, closest, sq = s.pointMeshDistance(v, P)
    gv, gp = s.pointMeshDistanceBackward(v, P, face, g)
    want = b"".join(np.ascontiguousarray(x).tobytes() for x in (face, w, closest, sq, gv, gp))
    assert len(raw) == len(want) and raw == want
