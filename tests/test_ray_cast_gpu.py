"""Ray casting on the MI355X (smplpp_ray_cast, smplpp_ray_cast_vjp): every output bit against the numpy restatement of
tests/ray_cast_oracle.py on meshes on both sides of the 256-face chunk, with dead rays and a NaN vertex in the batch; the exact-edge
and exact-vertex rays; independence of n, slot, space, outputs asked for and work split; the call rules; the chain from theta and
beta against float64 autograd; a range fit; the C++ shim."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import ray_cast_oracle as RC  # noqa: E402
import test_ray_cast_cpu as CPU  # noqa: E402  (closed_mesh, sphere_rays, the octahedron and its hand rays)
import vjp_blocks as VB  # noqa: E402
from distance_cases import _same_bits  # noqa: E402
from test_vertex_offsets_gpu import _dev, _smpl  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
NMAX, KMAX = 3, 257
FWD, BWD = ("face", "t", "bary", "hits"), ("verts", "origin", "dir")
DEAD = (1, 3, 5, 7, 9)  # rays made dead, one kind each, when K allows


def _host(a):
    return None if a is None else a.detach().cpu().numpy()


def _mesh_case(F):
    """A handle whose faces are a closed sphere mesh (F odd: and one free triangle), NMAX frames of its vertices, and KMAX rays per
    frame from a sphere of radius 3 aimed into the unit ball."""
    from smplpp_amd import model_io

    v, f = CPU.closed_mesh(F - F % 2, lone=bool(F % 2))
    assert len(f) == F
    rng = np.random.default_rng(F)
    verts = np.stack([(v.astype(f64) * (1 + 0.2 * i) + 0.02 * rng.standard_normal(v.shape)).astype(f32) for i in range(NMAX)])
    o = np.stack([CPU.sphere_rays(KMAX, 0.0, F + i, radius=3.0) for i in range(NMAX)])
    aim = rng.uniform(-0.9, 0.9, (NMAX, KMAX, 3))
    aim[:, ::4] = verts[0][rng.integers(0, len(v), (NMAX, len(aim[0, ::4])))]  # a quarter of them at fp32 vertices
    d = (aim - o).astype(f32) * f32(0.5)  # (t in units of |dir|: about 2 where the body is)
    return dict(s=_smpl(model_io.tiny_model(len(v), seed=3, faces=f + 1)), v=verts, f=f, o=o, d=d,
                g=rng.standard_normal((NMAX, KMAX)).astype(f32))


@pytest.fixture(scope="module")
def meshes():
    return {F: _mesh_case(F) for F in (8, 255, 257, 513)}


def _rays(c, n, K, shared, dead=True):
    o, d = (c["o"][:1, :K] if shared else c["o"][:n, :K]).copy(), (c["d"][:1, :K] if shared else c["d"][:n, :K]).copy()
    if dead and K >= 63:
        o[:, 1, 0], o[:, 3, 2], d[:, 5, 1], d[:, 7, 0], d[:, 9] = np.nan, np.inf, np.nan, -np.inf, 0.0
    return o, d


def _run(s, v, o, d, g, device=True, want=("bary", "hits"), want_bwd=BWD, **kw):
    """Every output of the forward and of the backward call at the forward's faces, as numpy."""
    conv = _dev if device else (lambda a: a)
    back = _host if device else (lambda a: a)
    fwd = s.rayCast(conv(v), conv(o), conv(d), want=want, **kw)
    res = {k: back(fwd[k]) for k in fwd}
    bwd = s.rayCastBackward(conv(v), conv(o), conv(d), fwd["face"], conv(g), want=want_bwd)
    res.update({"g" + k: back(a) for k, a in bwd.items()})
    return res


def _expect(c, v, o, d, g, **kw):
    ref = RC.ray_cast(v, c["f"], o, d, **kw)
    bwd = RC.ray_cast_vjp(v, c["f"], o, d, ref["face"], g)
    ref.update({"g" + k: a for k, a in bwd.items()})
    ref["hit"] = ref["face"] >= 0
    return ref


def _check(got, ref, what):
    for k in got:
        assert got[k].dtype == ref[k].dtype, (what, k, got[k].dtype)
        assert _same_bits(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()))


# ---------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("F", [8, 255, 257, 513])
def test_every_output_bit(meshes, F, shared):
    c = meshes[F]
    hits = 0
    for n in (1, 3):
        for K in (1, 63, 65, 257):
            o, d = _rays(c, n, K, shared)
            v, g = c["v"][:n], c["g"][:n, :K].copy()
            g[:, ::7] = 0.0  # a zero cotangent contributes nothing
            for kw in (dict(facing=1), dict(facing=2), dict(facing=3), dict(facing=3, t_max=2.0)):
                got, ref = _run(c["s"], v, o, d, g, **kw), _expect(c, v, o, d, g, **kw)
                _check(got, ref, (F, shared, n, K, kw))
                if K >= 63:
                    assert (ref["face"][:, DEAD] == -1).all() and (ref["hits"][:, DEAD] == 0).all()
                hits += int(ref["hit"].sum())
            if K == 257:  # the finite t_max cut hits that the open range had
                assert (RC.ray_cast(v, c["f"], o, d)["hits"].sum() > RC.ray_cast(v, c["f"], o, d, t_max=2.0)["hits"].sum())
    assert hits > 1000


def test_synthetic_model_bits(synth_model):
    from smplpp_amd import model_io

    s = _smpl(synth_model)
    beta, theta = model_io.synthetic_inputs(2, seed=5)
    v = s.launch(beta, theta)["verts"]
    f = synth_model["face_indices"].astype(np.int64) - 1
    rng = np.random.default_rng(9)
    K = 257
    o = np.stack([CPU.sphere_rays(K, v[i].mean(0), 30 + i) for i in range(2)])
    aim = np.stack([v[i][rng.integers(0, v.shape[1], K)] + rng.normal(0, 0.02, (K, 3)) for i in range(2)])
    aim[:, ::3] = v[0][rng.integers(0, v.shape[1], (2, len(aim[0, ::3])))]  # a third exactly at fp32 vertices of frame 0
    d = (aim - o).astype(f32)
    g = rng.standard_normal((2, K)).astype(f32)
    c = dict(f=f)
    for shared in (False, True):
        oo, dd = (o[:1], d[:1]) if shared else (o, d)
        ref = _expect(c, v, oo, dd, g)
        assert (ref["cover"] == 0).all() and ref["hit"].mean() > 0.5
        _check(_run(s, v, oo, dd, g), ref, ("synthetic", shared))


def test_a_nan_vertex_leaves_its_neighbours_alone(meshes):
    c = meshes[257]
    n, K = 3, 257
    o, d = _rays(c, n, K, False)
    v, g = c["v"].copy(), c["g"]
    clean = _run(c["s"], v, o, d, g)
    assert clean["face"][1, 0] >= 0
    bad_v = int(c["f"][clean["face"][1, 0]][0])  # a vertex of a face that frame 1 hits
    v[1, bad_v, 2] = np.nan
    got, ref = _run(c["s"], v, o, d, g), _expect(c, v, o, d, g)
    _check(got, ref, "nan vertex")
    touched = (c["f"] == bad_v).any(1)
    assert not touched[got["face"][1][got["face"][1] >= 0]].any() and got["face"][1, 0] != clean["face"][1, 0]
    for k in FWD:  # the other frames, and frame 1's rays that met none of the vertex's faces before, are as they were
        assert _same_bits(got[k][[0, 2]], clean[k][[0, 2]]), k
    away = ~touched[np.maximum(clean["face"][1], 0)] & (got["face"][1] == clean["face"][1])
    assert away.sum() > K // 2 and _same_bits(got["t"][1][away], clean["t"][1][away])


# ---------------------------------------------------------------------------------------------------- 2. ties
def test_exact_edge_and_vertex_rays(meshes):
    """The rays of the CPU cases that pass exactly through a vertex or an edge of the octahedron: the fp64 branch of the edge
    test and the tie rule on the device."""
    c = meshes[8]
    assert np.array_equal(c["f"], CPU.OCT_F)
    rays = [([0, 0, 5], [0, 0, -1]), ([5, 0, 0], [-1, 0, 0]), ([0, -3, 0], [0, 2, 0]), ([0.5, 0, 3], [-0.25, 0, -1]),
            ([0.5, 0.25, 3], [-0.25, -0.125, -1]), ([2, 0, 2], [-1, 0, -1]), ([0.25, 0.25, 4], [0, 0, -1]), ([2, 0, 1], [-1.5, 0, -0.5]),
            ([2, 0, 3], [-1, 0, -1]), ([3, 0.5, 0.5], [-1, 0, 0])]  # vertices, edge points, a face; then ALONG an edge and touching one
    o, d = np.array([r[0] for r in rays], f32)[None], np.array([r[1] for r in rays], f32)[None]
    v = CPU.OCT_V[None].copy()
    g = np.ones((1, len(rays)), f32)
    for facing in (1, 2, 3):
        got, ref = _run(c["s"], v, o, d, g, facing=facing), _expect(c, v, o, d, g, facing=facing)
        _check(got, ref, ("ties", facing))
    assert (got["hits"][0, :8] == 1).all() and got["t"][0, 0] == 4 and got["t"][0, 5] == 1.5
    # the same rays against a second frame too, the octahedron mirrored through the origin with x and y swapped: the same vertices
    # and edges are met from the other side and through other corners of the stored faces
    vv = np.stack([CPU.OCT_V, -CPU.OCT_V[:, [1, 0, 2]]])
    got, ref = _run(c["s"], vv, o, d, np.ones((2, len(rays)), f32)), _expect(c, vv, o, d, np.ones((2, len(rays)), f32))
    _check(got, ref, "ties, two frames")
    assert (ref["cover"] == 0).all()


# ---------------------------------------------------------------------------------------------------- 3. independence
def test_bits_do_not_depend_on_n_slot_space_or_outputs(meshes):
    c = meshes[513]
    n, K = 3, 257
    for shared in (False, True):
        o, d = _rays(c, n, K, shared)
        v, g = c["v"], c["g"]
        full = _run(c["s"], v, o, d, g)
        host = _run(c["s"], v, o, d, g, device=False)
        _check(host, full, ("host space", shared))
        for i in range(n):  # each frame alone
            oi, di = (o, d) if shared else (o[i:i + 1], d[i:i + 1])
            one = _run(c["s"], v[i:i + 1], oi, di, g[i:i + 1])
            for k in FWD + ("gverts",):
                assert _same_bits(one[k][0], full[k][i]), (shared, i, k)
            if not shared:
                assert _same_bits(one["gorigin"][0], full["gorigin"][i]) and _same_bits(one["gdir"][0], full["gdir"][i])
        bare = _run(c["s"], v, o, d, g, want=(), want_bwd=("dir",))
        assert set(bare) == {"face", "t", "hit", "gdir"}
        for k in ("face", "t", "gdir"):
            assert _same_bits(bare[k], full[k]), (shared, k)
        for want_bwd in (("verts",), ("origin",)):
            part = _run(c["s"], v, o, d, g, want=("hits",), want_bwd=want_bwd)
            assert _same_bits(part["hits"], full["hits"]) and _same_bits(part["g" + want_bwd[0]], full["g" + want_bwd[0]])


@pytest.mark.parametrize("slices", [1, 2, 3])
def test_bits_do_not_depend_on_the_slices(meshes, slices):
    from smplpp_amd import model_io

    c = meshes[513]  # three chunks of faces
    s = _smpl(model_io.tiny_model(c["v"].shape[1], seed=3, faces=c["f"] + 1), env={"SMPLPP_RAY_SLICES": str(slices)})
    for n, K in ((1, 65), (3, 257)):
        o, d = _rays(c, n, K, False)
        _check(_run(s, c["v"][:n], o, d, c["g"][:n, :K]), _run(c["s"], c["v"][:n], o, d, c["g"][:n, :K]), (slices, n, K))


# ---------------------------------------------------------------------------------------------------- 4. the call rules
def test_refusals_leave_the_outputs_untouched(meshes, synth_model):
    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import _ptr

    L = _lib.load()
    c = meshes[8]
    s, n, K = c["s"], 2, 5
    o, d = _rays(c, n, K, False)
    v, g = c["v"][:n], c["g"][:n, :K]
    face = RC.ray_cast(v, c["f"], o, d)["face"]
    assert (face >= 0).any()
    out = {k: np.full(sh, 7.0, f32) for k, sh in dict(t=(n, K), bary=(n, K, 3), gv=v.shape, go=(n, K, 3), gd=(n, K, 3)).items()}
    fo, ho = np.full((n, K), 7, np.int64), np.full((n, K, 2), 7, np.int32)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    base = dict(m=s.handle, n=n, v=v, rf=n, K=K, o=o, d=d, t_min=0.0, t_max=np.inf, facing=3, face=face, g=g, space=0)

    def fwd(fo_=fo, t="t", **kw):
        k = dict(base, **kw)
        return L.smplpp_ray_cast(k["m"], k["n"], p(k["v"]), k["rf"], k["K"], p(k["o"]), p(k["d"]), k["t_min"], k["t_max"], k["facing"], p(fo_),
                                 p(out[t]) if t else None, p(out["bary"]), p(ho), k["space"], None)

    def vjp(gv="gv", go="go", gd="gd", acc=0, **kw):
        k = dict(base, **kw)
        q = lambda key: p(out[key]) if key else None  # noqa: E731
        return L.smplpp_ray_cast_vjp(k["m"], k["n"], p(k["v"]), k["rf"], k["K"], p(k["o"]), p(k["d"]), p(k["face"]), p(k["g"]), q(gv), q(go), q(gd),
                                     acc, k["space"], None)

    m = model_io._normalise(synth_model)
    faceless = C.c_void_p()
    _lib.check(L.smplpp_model_create(m["vertices_template"].shape[0], 0, _ptr(m["vertices_template"]), _ptr(m["shape_blend_shapes"]),
                                     _ptr(m["pose_blend_shapes"]), _ptr(m["joint_regressor"]), _ptr(m["weights"]), _ptr(m["kinematic_tree"]), None,
                                     0, C.byref(faceless)))
    common = [dict(m=None), dict(m=faceless), dict(n=0), dict(n=-1), dict(K=0), dict(K=-3), dict(v=None), dict(o=None), dict(d=None), dict(rf=0),
              dict(rf=3), dict(rf=-1), dict(space=2), dict(n=2 ** 20, rf=2 ** 20, K=2 ** 11), dict(n=2 ** 30, rf=1, K=1)]
    for kw in common + [dict(t_min=-1.0), dict(t_min=np.nan), dict(t_min=np.inf), dict(t_max=np.nan), dict(t_max=0.0), dict(t_min=1.0, t_max=1.0),
                        dict(t_min=2.0, t_max=1.0), dict(facing=0), dict(facing=4), dict(facing=-1), dict(fo_=None), dict(t=None)]:
        assert fwd(**kw) == 1 and L.smplpp_last_error(), list(kw)
    high, low = face.copy(), face.copy()
    high[1, 2], low[0, 0] = len(c["f"]), -2
    for kw in common + [dict(face=None), dict(g=None), dict(gv=None, go=None, gd=None), dict(acc=2), dict(acc=-1), dict(face=high), dict(face=low)]:
        assert vjp(**kw) == 1 and L.smplpp_last_error(), list(kw)
    assert "int32" in (fwd(n=2 ** 20, rf=2 ** 20, K=2 ** 11), L.smplpp_last_error().decode())[1]
    assert all((a == 7).all() for a in out.values()) and (fo == 7).all() and (ho == 7).all()
    assert fwd() == 0 and fwd(t_max=np.inf, t_min=0.0) == 0 and vjp() == 0  # the base calls are good ones (+inf is allowed)
    assert np.array_equal(fo, face)
    # a device-space id out of range contributes nothing
    got = s.rayCastBackward(_dev(v), _dev(o), _dev(d), _dev(high), _dev(g))
    gm = g.copy()
    gm[1, 2] = 0.0
    ref = RC.ray_cast_vjp(v, c["f"], o, d, face, gm)
    for k in BWD:
        assert _same_bits(_host(got[k]), ref[k]), k
    # the binding words its own refusals
    for bad in (dict(origin=o[:, :, :2]), dict(dir=d[:, :3]), dict(origin=o[:1]), dict(verts=v[:, :5])):
        kw = dict(verts=v, origin=o, dir=d)
        kw.update(bad)
        with pytest.raises(_lib.SmplppError):
            s.rayCast(**kw)
    with pytest.raises(_lib.SmplppError):
        s.rayCastBackward(v, o, d, face, g, want=())
    _lib.check(L.smplpp_model_destroy(faceless))


def test_accumulate_adds_exactly_once(meshes):
    c = meshes[257]
    s = c["s"]
    for n, K, shared in ((3, 65, True), (3, 63, False)):
        o, d = _rays(c, n, K, shared)
        v, g = c["v"][:n], c["g"][:n, :K]
        face = s.rayCast(v, o, d)["face"]
        plain = s.rayCastBackward(v, o, d, face, g)
        for device in (False, True):
            conv = _dev if device else (lambda a: a)
            acc = {k: conv(np.full(a.shape, 1.5, f32)) for k, a in plain.items()}
            res = s.rayCastBackward(conv(v), conv(o), conv(d), conv(face), conv(g), out=acc)
            assert set(res) == set(plain)
            for k, a in plain.items():
                got = _host(acc[k]) if device else acc[k]
                assert _same_bits(got, f32(1.5) + a), (n, K, k, device)


# ---------------------------------------------------------------------------------------------------- 5. the chain
def _range(verts, faces, face, o, d):
    """t = n . (a - o) / n . d on the faces `face` [n,K] in torch (any dtype), 0 where face < 0."""
    n = verts.shape[0]
    ids = torch.as_tensor(faces[np.maximum(face, 0)])
    tri = verts[torch.arange(n)[:, None, None], ids]
    a, b, c = tri[:, :, 0], tri[:, :, 1], tri[:, :, 2]
    nrm = torch.linalg.cross(b - a, c - a)
    t = (nrm * (a - o)).sum(-1) / (nrm * d).sum(-1)
    return torch.where(torch.as_tensor(face >= 0), t, torch.zeros_like(t))


def test_chain_from_theta_and_beta(synth_model):
    from smplpp_amd import model_io

    s = _smpl(synth_model)
    faces = synth_model["face_indices"].astype(np.int64) - 1
    n, K = 2, 600
    beta, theta = model_io.synthetic_inputs(n, seed=81)
    v0 = s.launch(beta, theta)["verts"]
    rng = np.random.default_rng(82)
    o = np.stack([CPU.sphere_rays(K, v0[i].mean(0), 83 + i) for i in range(n)])
    aim = np.stack([v0[i][rng.integers(0, v0.shape[1], K)] for i in range(n)]) + rng.normal(0, 0.03, (n, K, 3))
    d = (aim - o).astype(f32)
    w = rng.uniform(0.5, 1.5, (n, K)).astype(f32)
    dev = torch.device("cuda")
    b, t, od, dd = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (beta, theta, o, d))
    verts, _ = s.forward_differentiable(b, t)
    r = s.ray_cast_differentiable(verts, od, dd)
    assert r["t"].requires_grad and not any(r[k].requires_grad for k in ("face", "bary", "hits", "hit"))
    (r["t"] * torch.from_numpy(w).to(dev)).sum().backward()
    face = _host(r["face"])
    assert (face >= 0).mean() > 0.8

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        args = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in (beta, theta, o, d)]
        vv = FK.fk(m, args[0], args[1])["verts"]
        (_range(vv, faces, face, args[2], args[3]) * torch.tensor(w, dtype=dtype)).sum().backward()
        return [a.grad.double().numpy() for a in args]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for got, want, low, name, axes in ((b.grad, r64[0], r32[0], "beta", (1,)), (t.grad, r64[1], r32[1], "theta", VB.THETA),
                                       (od.grad, r64[2], r32[2], "origin", (2,)), (dd.grad, r64[3], r32[3], "dir", (2,))):
        e, e32 = VB.block_error(_host(got), want, axes), VB.block_error(low, want, axes)
        print("chain %s: %.3g per block (fp32 autograd %.3g)" % (name, e, e32))
        assert e <= max(4 * e32, 1e-5), (name, e, e32)


# ---------------------------------------------------------------------------------------------------- 6. a range fit
def test_range_fit():
    """512 fixed beams, their ranges recorded from a target pose; Adam on the root translation and theta from a perturbed start, 60
    steps, on the device in fp32 and the same loop in float64 on the CPU oracle.  Both must cut the loss tenfold.  Where a loop
    "ends" is only defined up to what its own last steps still move: Adam changes every coordinate by about lr a step whatever the
    size of its gradient, so the weakly determined directions of the 75 parameters wander (the two end poses differed by up to 0.022
    rad, two steps, in a first run, at losses of 2.3e-3 and 1.6e-3 from 0.26) while the loss does not.  The bar is therefore on the
    loss, and it is the float64 loop's own spread over its last 10 steps: the device ends no further from the float64 end than
    the float64 loop was itself moving."""
    from smplpp_amd import model_io

    v, f = CPU.closed_mesh(512)
    model = model_io.tiny_model(len(v), seed=3, faces=f + 1)
    model["vertices_template"] = (0.4 * v).astype(model["vertices_template"].dtype)
    s = _smpl(model)
    K, steps, lr = 512, 60, 0.01
    rng = np.random.default_rng(7)
    o = CPU.sphere_rays(K, 0.0, 8, radius=3.0)[None]
    d = (rng.uniform(-0.2, 0.2, (1, K, 3)) - o).astype(f32)
    beta = np.zeros((1, 10), f32)
    target = np.zeros((1, 25, 3), f32)
    target[0, 1:] = rng.normal(0, 0.2, (24, 3))
    start = target + rng.normal(0, 0.05, target.shape).astype(f32)
    start[0, 0] += f32([0.05, -0.04, 0.03])
    measured = s.rayCast(s.launch(beta, target)["verts"], o, d)
    seen = measured["hit"]
    assert seen.mean() > 0.9

    def fit(theta, loss_of):
        opt = torch.optim.Adam([theta], lr=lr)
        hist = []
        for _ in range(steps):
            opt.zero_grad()
            loss = loss_of(theta)
            loss.backward()
            opt.step()
            hist.append(float(loss.detach()))
        return hist

    dev = torch.device("cuda")
    th = torch.from_numpy(start).to(dev).requires_grad_(True)
    bd, od, dd = (torch.from_numpy(a).to(dev) for a in (beta, o, d))
    tm, sm = torch.from_numpy(measured["t"]).to(dev), torch.from_numpy(seen).to(dev)

    def loss_dev(theta):
        r = s.ray_cast_differentiable(s.forward_differentiable(bd, theta)[0], od, dd)
        return (((r["t"] - tm) ** 2)[sm & r["hit"]]).sum()

    hist = fit(th, loss_dev)
    m64 = FK.model_tensors(model, torch.float64)
    th64 = torch.tensor(start, dtype=torch.float64, requires_grad=True)
    o64, d64, t64, b64 = (torch.tensor(a, dtype=torch.float64) for a in (o, d, measured["t"], beta))

    def loss_cpu(theta):
        vv = FK.fk(m64, b64, theta)["verts"]
        face = RC.ray_cast(vv.detach().numpy(), f, o.astype(f64), d.astype(f64), dtype=f64)["face"]
        return (((_range(vv, f, face, o64, d64) - t64) ** 2)[torch.as_tensor(seen & (face >= 0))]).sum()

    hist64 = fit(th64, loss_cpu)
    end, end64 = _host(th).astype(f64), th64.detach().numpy()
    print("range fit: loss %.6g -> %.6g on the device, %.6g -> %.6g in float64; the ends differ by at most %.3g"
          % (hist[0], hist[-1], hist64[0], hist64[-1], np.abs(end - end64).max()))
    assert hist64[-1] < 0.1 * hist64[0] and hist[-1] < 0.1 * hist[0]
    spread = max(hist64[-10:]) - min(hist64[-10:])
    print("range fit: the float64 loss over its last 10 steps spans %.6g; the two ends are %.6g apart" % (spread, abs(hist[-1] - hist64[-1])))
    assert abs(hist[-1] - hist64[-1]) <= spread


# ---------------------------------------------------------------------------------------------------- 7. C++ shim
def test_ray_cast_cpp_shim(tmp_path):
    from smplpp_amd import model_io

    exe = str(tmp_path / "ray_cast_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ray_cast_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    v, f = CPU.closed_mesh(64)
    model = model_io.tiny_model(len(v), seed=9, faces=f + 1)
    model["vertices_template"] = (0.5 * v).astype(model["vertices_template"].dtype)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    n, K = 3, 70
    beta = (np.arange(n * 10, dtype=f32).reshape(n, 10) % 7 - 3) * f32(0.1)
    theta = ((np.arange(n * 75, dtype=f32).reshape(n, 25, 3) % 11) - 5) * f32(0.05)
    s = _smpl(model)
    verts = s.launch(beta, theta)["verts"]
    g = ((np.arange(n * K, dtype=f32).reshape(n, K) % 5) - 2) * f32(0.25)
    parts, hits = [], 0
    for rf in (1, n):
        i = np.arange(rf * K)
        o = np.stack([(i % 5 - 2) * 1.5, (i % 3 - 1) * 3.0, (i % 7 - 3) * 1.0], 1).astype(f32)
        p = np.stack([(i % 4 - 2) * 0.125, (i % 9 - 4) * 0.0625, (i % 6 - 3) * 0.125], 1).astype(f32)
        o, d = o.reshape(rf, K, 3), (p - o).reshape(rf, K, 3)
        kw = {} if rf == 1 else dict(t_max=1.25, facing=1)
        fw = s.rayCast(verts, o, d, **kw)
        bw = s.rayCastBackward(verts, o, d, fw["face"], g)
        hits += int(fw["hit"].sum())
        parts += [fw["face"], fw["t"], fw["bary"], fw["hits"].astype(np.int64), bw["verts"], bw["origin"], bw["dir"]]
    assert hits > 50
    want = b"".join(np.ascontiguousarray(a).tobytes() for a in parts)
    assert len(raw) == len(want) and raw == want
