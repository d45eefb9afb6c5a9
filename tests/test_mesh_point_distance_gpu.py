"""The mesh-to-point distance on the MI355X (smplpp_mesh_point_distance, smplpp_mesh_point_distance_vjp): the forward's bits against
the float32 restatement of tests/mesh_point_distance_oracle.py at every size class (one tile, a partial tile, split and unsplit K),
ties and non-finite points, independence of batch, slot and split, host and device space, a model without faces; the backward
against float64 autograd, a hot point, call semantics; end-to-end gradients and a two-sided fit through forward_differentiable; and
the C++ shim."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_point_distance_oracle as O  # noqa: E402
from distance_cases import _rel, _same_bits, _surface_points, _verts  # noqa: E402

torch = O.torch
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def smpl(synth_model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    return s


@pytest.fixture(scope="module")
def faces(synth_model):
    return synth_model["face_indices"].astype(np.int64) - 1


def _assert_oracle_bits(index, sq, v, P):
    ri, rs = O.forward(v, P)
    bad = np.nonzero((index != ri) | (sq.view(np.int32) != rs.view(np.int32)))
    assert len(bad[0]) == 0, (len(bad[0]), bad[0][:5], bad[1][:5], index[bad][:5], ri[bad][:5], sq[bad][:5], rs[bad][:5])
    assert _same_bits(index, ri) and _same_bits(sq, rs)


# ---------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("n,K", [(3, 1), (2, 1000), (1, 16384), (16, 4096), (64, 1024)])
def test_forward_bits_sizes(smpl, faces, n, K):
    v = _verts(smpl, n, seed=K)
    rng = np.random.default_rng(n * 1000 + K)
    P = _surface_points(v, faces, K, rng)
    far = rng.random((n, K)) < 0.1  # some points 0.25 m off
    P[far] += np.float32(0.25) * rng.normal(size=(int(far.sum()), 3)).astype(np.float32)
    index, sq = smpl.meshPointDistance(v, P)
    assert index.dtype == np.int64 and index.shape == (n, smpl.vertex_num) and sq.shape == (n, smpl.vertex_num)
    _assert_oracle_bits(index, sq, v, P)


@pytest.mark.parametrize("K", [40, 3000])  # one chunk; a split call (single frame, K >= 512)
def test_ties_and_non_finite_points(smpl, faces, K):
    v = _verts(smpl, 3, seed=11)
    rng = np.random.default_rng(K)
    P = _surface_points(v, faces, K, rng)
    V = smpl.vertex_num
    # exact ties: points ON vertices (d = 0), each placed twice; and duplicates of ordinary points, late in the cloud
    for f in range(2):
        u = rng.integers(0, V, 6)
        P[f, 1:7] = v[f, u]
        P[f, K - 6:] = v[f, u]
        P[f, K // 2:K // 2 + 5] = P[f, 10:15]
    # non-finite and overflowing points, which are never chosen
    P[0, 20] = np.nan
    P[0, 21] = (np.inf, 0, 0)
    P[0, 22] = (3e38, -3e38, 3e38)
    P[1, 23] = (-np.inf, -np.inf, -np.inf)
    P[1, 24] = (np.nan, 1.0, 1.0)
    P[2] = np.nan  # a frame of padding: (-1, 0) everywhere
    index, sq = smpl.meshPointDistance(v, P)
    _assert_oracle_bits(index, sq, v, P)
    assert not np.isin(index[0], [20, 21, 22]).any() and not np.isin(index[1], [23, 24]).any()
    for f in range(2):
        u = np.nonzero(sq[f] == 0)[0]
        assert len(u) >= 6 and (index[f, u] <= 6).all()  # the first copy of a tied point
    assert (index[2] == -1).all() and (sq[2] == 0).all() and not np.signbit(sq[2]).any()


def test_split_and_batch_independence_and_repeat(smpl, faces):
    """A frame alone and inside a batch gives the same bits, forward and backward.  Under the split rule (K chunks chosen from n
    and K) K = 4096 alone is cut into 16 chunks, in a batch of 64 into 5; K = 512 alone into 2, in a batch of 300 not at all."""
    for K, nb, slot in ((4096, 64, 37), (512, 300, 201)):
        v = _verts(smpl, nb, seed=K + 7)
        rng = np.random.default_rng(K)
        P = _surface_points(v, faces, K, rng)
        g = rng.normal(size=(nb, smpl.vertex_num)).astype(np.float32)
        dv, dP, dg = (torch.from_numpy(x).cuda() for x in (v, P, g))
        bi, bs = smpl.meshPointDistance(dv, dP)
        bgv, bgp = smpl.meshPointDistanceBackward(dv, dP, bi, dg)
        runs = []
        for _ in range(3):
            ai, asq = smpl.meshPointDistance(dv[slot:slot + 1].contiguous(), dP[slot:slot + 1].contiguous())
            agv, agp = smpl.meshPointDistanceBackward(dv[slot:slot + 1].contiguous(), dP[slot:slot + 1].contiguous(), ai,
                                                      dg[slot:slot + 1].contiguous())
            runs.append([x.cpu().numpy() for x in (ai, asq, agv, agp)])
        torch.cuda.synchronize()
        batch = [x.cpu().numpy()[slot:slot + 1] for x in (bi, bs, bgv, bgp)]
        for r in runs:
            assert all(_same_bits(a, b) for a, b in zip(r, batch)), K
        _assert_oracle_bits(runs[0][0], runs[0][1], v[slot:slot + 1], P[slot:slot + 1])


def test_host_and_device_space(smpl, faces):
    v = _verts(smpl, 3, seed=71)
    rng = np.random.default_rng(71)
    P = _surface_points(v, faces, 777, rng)
    P[1, 5] = np.nan
    g = rng.normal(size=(3, smpl.vertex_num)).astype(np.float32)
    hf = smpl.meshPointDistance(v, P)
    hb = smpl.meshPointDistanceBackward(v, P, hf[0], g)
    dv, dP, dg = (torch.from_numpy(x).cuda() for x in (v, P, g))
    df = smpl.meshPointDistance(dv, dP)
    db = smpl.meshPointDistanceBackward(dv, dP, df[0], dg)
    torch.cuda.synchronize()
    assert all(_same_bits(a, b.cpu().numpy()) for a, b in zip(hf + hb, df + db))


def test_model_without_faces(synth_model):
    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import _ptr

    m = model_io._normalise(synth_model)
    L = _lib.load()
    V = m["vertices_template"].shape[0]
    h = C.c_void_p()
    _lib.check(L.smplpp_model_create(V, 0, _ptr(m["vertices_template"]), _ptr(m["shape_blend_shapes"]), _ptr(m["pose_blend_shapes"]),
                                     _ptr(m["joint_regressor"]), _ptr(m["weights"]), _ptr(m["kinematic_tree"]), None, 0, C.byref(h)))
    try:
        rng = np.random.default_rng(5)
        v = rng.normal(0, 0.4, (2, V, 3)).astype(np.float32)
        P = rng.normal(0, 0.4, (2, 600, 3)).astype(np.float32)
        index, sq = np.empty((2, V), np.int64), np.empty((2, V), np.float32)
        _lib.check(L.smplpp_mesh_point_distance(h, 2, _ptr(v), 600, _ptr(P), _ptr(index), _ptr(sq), _lib.HOST, None))
        _assert_oracle_bits(index, sq, v, P)
        g = rng.normal(size=(2, V)).astype(np.float32)
        gv, gp = np.empty((2, V, 3), np.float32), np.empty((2, 600, 3), np.float32)
        _lib.check(L.smplpp_mesh_point_distance_vjp(h, 2, _ptr(v), 600, _ptr(P), _ptr(index), _ptr(g), _ptr(gv), _ptr(gp), 0, _lib.HOST,
                                                    None))
        cv, cp = O.closed_form(torch.tensor(v, dtype=torch.float64), torch.tensor(P, dtype=torch.float64), index, g)
        assert np.abs(gv - cv.numpy()).max() <= 1e-5 * np.abs(cv.numpy()).max()
        assert np.abs(gp - cp.numpy()).max() <= 1e-5 * np.abs(cp.numpy()).max()
    finally:
        L.smplpp_model_destroy(h)


# ---------------------------------------------------------------------------------------------------- backward
def _check_vjp(v, P, index, g, gv, gp):
    """House tolerance: within 4x the error of an fp32 autograd of the same graph, or 1e-5 relative, per frame."""
    for f in range(len(v)):
        sl = slice(f, f + 1)
        rv, rp = O.vjp(torch.tensor(v[sl], dtype=torch.float64), torch.tensor(P[sl], dtype=torch.float64), index[sl], g[sl])
        fv, fp = O.vjp(torch.tensor(v[sl]), torch.tensor(P[sl]), index[sl], torch.tensor(g[sl]))
        for got, ref, f32, name in ((gv[sl], rv.numpy(), fv.numpy(), "verts"), (gp[sl], rp.numpy(), fp.numpy(), "points")):
            assert np.isfinite(got).all()
            bar = max(4 * _rel(f32, ref), 1e-5)
            err = _rel(got, ref)
            assert err <= bar, (f, name, err, bar)


@pytest.mark.parametrize("n,K", [(1, 7), (3, 500), (2, 4096)])
def test_backward_vs_float64_autograd(smpl, faces, n, K):
    v = _verts(smpl, n, seed=K + 1)
    rng = np.random.default_rng(K)
    P = _surface_points(v, faces, K, rng)
    index, _ = smpl.meshPointDistance(v, P)
    g = rng.normal(size=(n, smpl.vertex_num)).astype(np.float32)
    gv, gp = smpl.meshPointDistanceBackward(v, P, index, g)
    _check_vjp(v, P, index, g, gv, gp)
    assert _same_bits(gv, (2 * g[..., None]) * (v - P[np.arange(n)[:, None], index]))


def test_hot_point(smpl, faces):
    """A cloud of one finite point among NaN rows: every vertex of the frame maps to it, and its gradient is one sum of 6890 terms
    in ascending vertex, the same bits on every call."""
    v = _verts(smpl, 2, seed=41)
    K = 64
    P = np.full((2, K, 3), np.nan, np.float32)
    P[0, 17] = (0.05, 0.3, 0.1)
    P[1, 63] = (-0.2, 0.0, 0.4)
    index, sq = smpl.meshPointDistance(v, P)
    assert (index[0] == 17).all() and (index[1] == 63).all()
    _assert_oracle_bits(index, sq, v, P)
    rng = np.random.default_rng(41)
    g = rng.normal(size=(2, smpl.vertex_num)).astype(np.float32)
    gv, gp = smpl.meshPointDistanceBackward(v, P, index, g)
    for _ in range(2):
        gv2, gp2 = smpl.meshPointDistanceBackward(v, P, index, g)
        assert _same_bits(gv, gv2) and _same_bits(gp, gp2)
    assert (gp[0, np.arange(K) != 17] == 0).all() and (gp[1, :63] == 0).all()
    _check_vjp(v, P, index, g, gv, gp)


def _fp32_vjp(v, P, index, g):
    """The backward's fp32 arithmetic and order: r = v - p[index], grad_verts = (2 g) r; grad_points a sum from +0 per point, in
    ascending vertex, of (-2 g) r over the vertices with g != 0 and an index in [0, K)."""
    n, V = index.shape
    f = np.arange(n)
    live = (g != 0) & (index >= 0) & (index < P.shape[1])
    r = v - P[f[:, None], np.where(live, index, 0)]
    gv = np.where(live[..., None], (2 * g)[..., None] * r, np.float32(0))
    c = (-2 * g)[..., None] * r
    gp = np.zeros(P.shape, np.float32)
    for u in range(V):
        m = live[:, u]
        gp[f[m], index[m, u]] += c[m, u]
    return gv, gp


@pytest.mark.parametrize("case", ["surface", "hot_point"])
def test_backward_bits_vs_fp32_restatement(smpl, faces, case):
    """Every bit: 6890 records (several LDS tiles), 3000 points (several target blocks), a hot point; zero g and index -1."""
    rng = np.random.default_rng(97)
    if case == "surface":
        v = _verts(smpl, 3, seed=97)
        P = _surface_points(v, faces, 3000, rng)
    else:
        v = _verts(smpl, 2, seed=41)
        P = np.full((2, 64, 3), np.nan, np.float32)
        P[0, 17] = (0.05, 0.3, 0.1)
        P[1, 63] = (-0.2, 0.0, 0.4)
    index, _ = smpl.meshPointDistance(v, P)
    g = rng.normal(size=index.shape).astype(np.float32)
    g[rng.random(g.shape) < 0.1] = 0
    index[rng.random(index.shape) < 0.05] = -1
    gv, gp = smpl.meshPointDistanceBackward(v, P, index, g)
    rv, rp = _fp32_vjp(v, P, index, g)
    assert _same_bits(gv, rv)
    assert _same_bits(gp, rp), np.nonzero(gp != rp)[:2]


# ---------------------------------------------------------------------------------------------------- call semantics
def _raw_vjp(s, v, P, index, g, gv, gp, acc, space=0):
    from smplpp_amd import _lib
    from smplpp_amd.smpl import _ptr

    n, K = P.shape[:2]
    return _lib.load().smplpp_mesh_point_distance_vjp(s.handle, n, _ptr(v), K, _ptr(P), _ptr(index), _ptr(g), _ptr(gv), _ptr(gp), acc,
                                                      space, None)


def test_call_semantics(smpl, faces):
    v = _verts(smpl, 2, seed=51)
    rng = np.random.default_rng(51)
    K, V = 200, smpl.vertex_num
    P = _surface_points(v, faces, K, rng)
    P[:, K - 10:] += np.float32(5.0)  # 5 m off: no vertex chooses these
    index, _ = smpl.meshPointDistance(v, P)
    g = rng.normal(size=(2, V)).astype(np.float32)
    gv, gp = smpl.meshPointDistanceBackward(v, P, index, g)
    # accumulate = 0 overwrites whatever is there (points no vertex chose get 0)
    ov, op = np.full((2, V, 3), 7.0, np.float32), np.full((2, K, 3), 7.0, np.float32)
    assert _raw_vjp(smpl, v, P, index, g, ov, op, 0) == 0
    assert _same_bits(ov, gv) and _same_bits(op, gp)
    for f in range(2):
        unused = np.setdiff1d(np.arange(K), index[f])
        assert len(unused) and (gp[f, unused] == 0).all()
    # accumulate = 1 adds
    base_v, base_p = rng.normal(size=(2, V, 3)).astype(np.float32), rng.normal(size=(2, K, 3)).astype(np.float32)
    av, ap = smpl.meshPointDistanceBackward(v, P, index, g, out=base_v.copy(), grad_points=base_p.copy())
    assert _same_bits(av, base_v + gv) and _same_bits(ap, base_p + gp)
    # either output NULL
    ov = np.full((2, V, 3), 7.0, np.float32)
    assert _raw_vjp(smpl, v, P, index, g, ov, None, 0) == 0 and _same_bits(ov, gv)
    op = np.full((2, K, 3), 7.0, np.float32)
    assert _raw_vjp(smpl, v, P, index, g, None, op, 0) == 0 and _same_bits(op, gp)
    # zero cotangents and index = -1 contribute nothing: the same bits as the product without those vertices' terms
    mask = rng.random((2, V)) < 0.3
    g0, i0 = g.copy(), index.copy()
    g0[mask] = 0
    i0[~mask & (rng.random((2, V)) < 0.2)] = -1
    drop = (g0 == 0) | (i0 < 0)
    gvz, gpz = smpl.meshPointDistanceBackward(v, P, i0, g0)
    assert (gvz[drop] == 0).all() and _same_bits(gvz[~drop], gv[~drop])
    cv, cp = O.closed_form(torch.tensor(v, dtype=torch.float64), torch.tensor(P, dtype=torch.float64), i0, g0)
    assert np.abs(gpz - cp.numpy()).max() <= 1e-5 * np.abs(cp.numpy()).max()
    gd = np.where(drop, 0, g).astype(np.float32)
    assert _same_bits(gpz, smpl.meshPointDistanceBackward(v, P, index, gd)[1])


def test_index_out_of_range(smpl, faces):
    from smplpp_amd import _lib
    from smplpp_amd._lib import SmplppError, check

    v = _verts(smpl, 2, seed=61)
    rng = np.random.default_rng(61)
    K, V = 150, smpl.vertex_num
    P = _surface_points(v, faces, K, rng)
    index, _ = smpl.meshPointDistance(v, P)
    g = rng.normal(size=(2, V)).astype(np.float32)
    # host space: refused, outputs untouched
    for bad in (-2, K):
        bi = index.copy()
        bi[1, 100] = bad
        gv, gp = np.full((2, V, 3), 7.0, np.float32), np.full((2, K, 3), 7.0, np.float32)
        with pytest.raises(SmplppError):
            check(_raw_vjp(smpl, v, P, bi, g, gv, gp, 1))
        assert (gv == 7.0).all() and (gp == 7.0).all()
    # device space: contributes nothing
    dv, dP, dg, di = (torch.from_numpy(x).cuda() for x in (v, P, g, index))
    bad = di.clone()
    bad[1, 100] = K
    bad[0, 5] = -7
    g0 = dg.clone()
    g0[1, 100] = 0
    g0[0, 5] = 0
    b1 = smpl.meshPointDistanceBackward(dv, dP, bad, dg)
    b0 = smpl.meshPointDistanceBackward(dv, dP, di, g0)
    torch.cuda.synchronize()
    assert _same_bits(b1[0].cpu().numpy(), b0[0].cpu().numpy()) and _same_bits(b1[1].cpu().numpy(), b0[1].cpu().numpy())
    # invalid arguments
    L = _lib.load()
    from smplpp_amd.smpl import _ptr

    h = smpl.handle
    sq = np.zeros((2, V), np.float32)
    gv = np.zeros((2, V, 3), np.float32)
    bad_calls = [
        (L.smplpp_mesh_point_distance, (None, 2, _ptr(v), K, _ptr(P), _ptr(index), _ptr(sq), 0, None)),
        (L.smplpp_mesh_point_distance, (h, 0, _ptr(v), K, _ptr(P), _ptr(index), _ptr(sq), 0, None)),
        (L.smplpp_mesh_point_distance, (h, 2, _ptr(v), 0, _ptr(P), _ptr(index), _ptr(sq), 0, None)),
        (L.smplpp_mesh_point_distance, (h, 2, _ptr(v), K, _ptr(P), None, _ptr(sq), 0, None)),
        (L.smplpp_mesh_point_distance, (h, 2, _ptr(v), K, _ptr(P), _ptr(index), None, 0, None)),
        (L.smplpp_mesh_point_distance, (h, 2, _ptr(v), K, _ptr(P), _ptr(index), _ptr(sq), 5, None)),
        (L.smplpp_mesh_point_distance, (h, 1 << 16, _ptr(v), 1 << 16, _ptr(P), _ptr(index), _ptr(sq), 0, None)),  # n K beyond int32
        (L.smplpp_mesh_point_distance, (h, 1 << 19, _ptr(v), 1, _ptr(P), _ptr(index), _ptr(sq), 0, None)),  # n V beyond int32
        (L.smplpp_mesh_point_distance_vjp, (h, 2, _ptr(v), K, _ptr(P), _ptr(index), _ptr(g), None, None, 0, 0, None)),
        (L.smplpp_mesh_point_distance_vjp, (h, 2, _ptr(v), K, _ptr(P), _ptr(index), _ptr(g), _ptr(gv), None, 2, 0, None)),
        (L.smplpp_mesh_point_distance_vjp, (h, 2, _ptr(v), K, _ptr(P), None, _ptr(g), _ptr(gv), None, 0, 0, None)),
        (L.smplpp_mesh_point_distance_vjp, (h, 1 << 19, _ptr(v), 1, _ptr(P), _ptr(index), _ptr(g), _ptr(gv), None, 0, 0, None)),
    ]
    for fn, args in bad_calls:
        with pytest.raises(SmplppError):
            check(fn(*args))


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
    index, sq = smpl.mesh_point_distance_differentiable(verts, Pd)
    assert not index.requires_grad and sq.requires_grad
    sq.mean().backward()
    index = index.cpu().numpy()

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        bb = torch.tensor(beta, dtype=dtype, requires_grad=True)
        tt = torch.tensor(theta, dtype=dtype, requires_grad=True)
        vv = FK.fk(m, bb, tt)["verts"]
        O.sqdist(vv, torch.tensor(P, dtype=dtype), index).mean().backward()
        return bb.grad.double().numpy(), tt.grad.double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for got, want, f32, name in ((b.grad, r64[0], r32[0], "beta"), (t.grad, r64[1], r32[1], "theta")):
        got = got.cpu().numpy()
        bar = max(4 * _rel(f32, want), 1e-5)
        assert _rel(got, want) <= bar, (name, _rel(got, want), bar)
    # points differentiable too
    Pg = Pd.clone().requires_grad_(True)
    _, sq2 = smpl.mesh_point_distance_differentiable(verts.detach(), Pg)
    sq2.sum().backward()
    _, cp = O.closed_form(verts.detach().double().cpu(), Pd.double().cpu(), index, np.ones(index.shape))
    assert np.abs(Pg.grad.cpu().numpy() - cp.numpy()).max() <= 1e-5 * np.abs(cp.numpy()).max()


def test_adam_fit_two_sided(smpl, faces):
    """β and θ fitted from zero to a target with a non-zero β, against a cloud of the target's posed vertices plus 4096 surface
    samples, shuffled, so that both terms vanish at the target.  Loss = mean point-to-mesh + mean mesh-to-point."""
    dev = torch.device("cuda")
    rng = np.random.default_rng(93)
    theta_t = np.zeros((1, 25, 3), np.float32)
    theta_t[0, 1:] = rng.normal(0, 0.2, (24, 3))
    beta_t = rng.normal(0, 0.5, (1, 10)).astype(np.float32)
    with torch.no_grad():
        vt, _ = smpl.forward_differentiable(torch.from_numpy(beta_t).to(dev), torch.from_numpy(theta_t).to(dev))
    vt = vt.cpu().numpy()
    cloud = np.concatenate([vt[0], _surface_points(vt, faces, 4096, rng, off=0.0)[0]])
    cloud = cloud[rng.permutation(len(cloud))][None]
    P = torch.from_numpy(np.ascontiguousarray(cloud)).to(dev)
    beta = torch.zeros(1, 10, device=dev, requires_grad=True)
    th = torch.zeros(1, 25, 3, device=dev)
    th[0, 0] = torch.from_numpy(theta_t[0, 0]).to(dev)
    th.requires_grad_(True)
    opt = torch.optim.Adam([th, beta], lr=0.02)
    losses = []
    for it in range(500):
        if it == 350:
            for grp in opt.param_groups:
                grp["lr"] = 0.005
        opt.zero_grad()
        v, _ = smpl.forward_differentiable(beta, th)
        _, _, s2m = smpl.point_mesh_distance_differentiable(v, P)
        _, m2s = smpl.mesh_point_distance_differentiable(v, P)
        loss = s2m.mean() + m2s.mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] * 100 <= losses[0], (losses[0], losses[-1])


def test_mesh_point_distance_cpp_shim(tmp_path):
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    exe = str(tmp_path / "mesh_point_distance_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mesh_point_distance_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    # the program's inputs, restated
    n, K = 2, 24
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    P = ((np.arange(n * K * 3, dtype=np.float32).reshape(n, K, 3) % 17) - 8) * np.float32(0.03)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    V = s.vertex_num
    g = ((np.arange(n * V, dtype=np.float32).reshape(n, V) % 5) - 2) * np.float32(0.25)
    v = s.launch(beta, theta, want=("verts",))["verts"]
    index, sq = s.meshPointDistance(v, P)
    gv, gp = s.meshPointDistanceBackward(v, P, index, g)
    want = b"".join(np.ascontiguousarray(x).tobytes() for x in (index, sq, gv, gp))
    assert len(raw) == len(want) and raw == want
