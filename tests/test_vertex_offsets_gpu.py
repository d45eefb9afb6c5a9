"""SMPL+D on the MI355X (smplpp_vertex_offsets, smplpp_vertex_offsets_vjp, smplpp_mesh_laplacian): every bit against the numpy
restatements of tests/vertex_offsets_oracle.py on models that keep 4, 8 and 24 skinning weights per vertex; independence of batch,
slot, space and in-place use; the forward against the float64 definition beside smplpp_stage_skinning; the chain to beta, theta and
the offsets against float64 autograd; the Laplacian; the call rules; a registration of a known displacement field; the C++ shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import vertex_offsets_oracle as VO  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NMAX = 65
TINY_V = 61  # not a multiple of 32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _smpl(model, env=None):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        s.init(model)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    return s


def _eight_weight_model():
    """tiny_model with 5 to 8 weights per vertex, and vertices of all three skinning classes (joints 0..15 only, both, 16..23 only)."""
    from smplpp_amd import model_io

    m = model_io.tiny_model(TINY_V, seed=12)
    rng = np.random.default_rng(13)
    w = m["weights"].astype(np.float64)
    for v in range(TINY_V):
        pool = (np.arange(16), np.arange(24), np.arange(16, 24))[v % 3]
        keep = rng.choice(pool, size=int(rng.integers(5, 9)), replace=False)
        row = np.zeros(24)
        row[keep] = w[v, keep]
        w[v] = row / row.sum()
    m["weights"] = w.astype(np.float32)
    assert set(model_io.skinning_classes(m["weights"]).tolist()) == {0, 1, 2}
    return m


@pytest.fixture(scope="module")
def cases(synth_model):
    """Per weight width: the handle, the model, and one launch of NMAX frames (verts, xforms, rest) with offsets and cotangents."""
    from smplpp_amd import model_io

    out = {}
    for name, model, width in (("synth", synth_model, 4), ("eight", _eight_weight_model(), 8),
                               ("dense", model_io.tiny_model(TINY_V, seed=7), 24)):
        s = _smpl(model)
        assert s.info()["weights_per_vertex"] == width
        beta, theta = model_io.synthetic_inputs(NMAX, seed=31)
        fk = s.launch(beta, theta, want=("verts", "xforms", "rest"))
        rng = np.random.default_rng(width)
        V = s.vertex_num
        each = rng.normal(0, 0.01, (NMAX, V, 3)).astype(np.float32)
        each[:, 5] = 0.0  # a zero offsets row
        g = rng.normal(size=(NMAX, V, 3)).astype(np.float32)
        g[:, 3] = 0.0  # a vertex without cotangent
        out[name] = dict(s=s, W=model["weights"].astype(np.float32), theta=theta, verts=fk["verts"], xforms=fk["xforms"], rest=fk["rest"],
                         each=each, g=g)
    return out


@pytest.fixture(scope="module")
def smpl(cases):
    return cases["synth"]["s"]


@pytest.fixture(scope="module")
def faces(synth_model):
    return synth_model["face_indices"].astype(np.int64) - 1


# ---------------------------------------------------------------------------------------------------- 1. forward bits
@pytest.mark.parametrize("n", [1, 3, 33])
@pytest.mark.parametrize("name", ["synth", "eight", "dense"])
def test_forward_bits(cases, name, n):
    c = cases[name]
    s, W = c["s"], c["W"]
    v, xf, rest = c["verts"][:n], c["xforms"][:n], c["rest"][:n]
    for kind, D in (("each", c["each"][:n]), ("shared", c["each"][7:8])):
        want, want_rest = VO.forward(W, v, xf, D, rest=rest)
        got, got_rest = s.vertexOffsets(v, xf, D, rest=rest)
        assert got.dtype == np.float32 and _same_bits(got, want), (kind, int((got != want).sum()))
        assert _same_bits(got_rest, want_rest) and _same_bits(got_rest, rest + D)
        assert np.abs(got - v).max() > 1e-3
        assert _same_bits(s.vertexOffsets(v, xf, D), got)  # without rest
        # in place, on the host and on the device; device space out of place
        vh = v.copy()
        assert s.vertexOffsets(vh, xf, D, out=vh) is vh and _same_bits(vh, got)
        dv, dx, dd, dr = _dev(v), _dev(xf), _dev(D), _dev(rest)
        o, r = s.vertexOffsets(dv, dx, dd, rest=dr)
        assert _same_bits(o.cpu().numpy(), got) and _same_bits(r.cpu().numpy(), got_rest)
        assert _same_bits(dv.cpu().numpy(), v)
        s.vertexOffsets(dv, dx, dd, out=dv)
        assert _same_bits(dv.cpu().numpy(), got)
        # a frame alone has the bits it has inside the batch
        k = n - 1
        alone = s.vertexOffsets(v[k:k + 1], xf[k:k + 1], D[k:k + 1] if kind == "each" else D)
        assert _same_bits(alone[0], got[k])
    # zero offsets return the input
    zero = np.zeros((1, s.vertex_num, 3), np.float32)
    assert (s.vertexOffsets(v, xf, zero) == v).all() and (s.vertexOffsets(v, xf, -zero) == v).all()
    assert (s.vertexOffsets(v, xf, c["each"][:n])[:, 5] == v[:, 5]).all()
    # [V,3] is the shared field
    assert _same_bits(s.vertexOffsets(v, xf, c["each"][7]), s.vertexOffsets(v, xf, c["each"][7:8]))


@pytest.mark.parametrize("form", ["h", "b", "v"])
def test_forward_rule_on_every_form(synth_model, cases, form):
    """The rule is stated on the verts and xforms smplpp_fk returned, whichever form computed them."""
    from smplpp_amd import model_io

    s = _smpl(synth_model, {"SMPLPP_SKIN": form})
    beta, theta = model_io.synthetic_inputs(3, seed=32)
    fk = s.launch(beta, theta, want=("verts", "xforms", "rest"))
    D = cases["synth"]["each"][:3]
    got, rd = s.vertexOffsets(fk["verts"], fk["xforms"], D, rest=fk["rest"])
    want, want_rest = VO.forward(cases["synth"]["W"], fk["verts"], fk["xforms"], D, rest=fk["rest"])
    assert _same_bits(got, want) and _same_bits(rd, want_rest)


# ---------------------------------------------------------------------------------------------------- 2. forward against the definition
def test_forward_vs_definition(cases):
    from smplpp_amd.smpl import stage_skinning

    c = cases["synth"]
    s, W, n = c["s"], c["W"], 3
    v, xf, rest, root = c["verts"][:n], c["xforms"][:n], c["rest"][:n], c["theta"][:n, 0]
    for kind, D in (("each", c["each"][:n]), ("shared", VO.smooth_field(rest[0])[None])):
        want = VO.definition(W, rest, xf, D, root)
        got = s.vertexOffsets(v, xf, D)
        stage = stage_skinning(W, rest + D, xf, root_pos=root)
        e_new, e_stage = _rel(got, want), _rel(stage, want)
        print("forward vs definition (%s): new call rel %.3g, smplpp_stage_skinning rel %.3g" % (kind, e_new, e_stage))
        assert e_new <= max(4 * e_stage, 1e-5), (e_new, e_stage)
        base = VO.definition(W, rest, xf, np.zeros_like(rest), root)
        print("  correction alone: rel %.3g" % _rel(got.astype(np.float64) - v, want - base))


# ---------------------------------------------------------------------------------------------------- 3. backward bits
@pytest.mark.parametrize("n", [1, 3, 31, 32, 33, 65])
@pytest.mark.parametrize("name", ["synth", "eight", "dense"])
def test_backward_bits(cases, name, n):
    c = cases[name]
    s, W = c["s"], c["W"]
    xf, g = c["xforms"][:n], c["g"][:n]
    modes = [False] * (n in (1, 3, 33)) + [True] * (n in (1, 31, 32, 33, 65))
    for shared in modes:
        want = VO.backward(W, xf, g, shared)
        got = s.vertexOffsetsBackward(xf, g, shared=shared)
        assert got.dtype == np.float32 and got.shape == want.shape and _same_bits(got, want), (shared, int((got != want).sum()))
        assert np.abs(got).max() > 0 and (got[:, 3] == 0).all()  # the vertex without cotangent
        assert _same_bits(s.vertexOffsetsBackward(xf, g, shared=shared), got)  # twice
        base = np.random.default_rng(n).normal(size=got.shape).astype(np.float32)
        acc = base.copy()
        assert s.vertexOffsetsBackward(xf, g, shared=shared, out=acc) is acc and _same_bits(acc, base + got)
        dx, dg = _dev(xf), _dev(g)
        assert _same_bits(s.vertexOffsetsBackward(dx, dg, shared=shared).cpu().numpy(), got)
        dacc = _dev(base)
        s.vertexOffsetsBackward(dx, dg, shared=shared, out=dacc)
        assert _same_bits(dacc.cpu().numpy(), base + got)
        if not shared:  # a frame alone has the bits it has inside the batch
            assert _same_bits(s.vertexOffsetsBackward(xf[n - 1:], g[n - 1:])[0], got[n - 1])


# ---------------------------------------------------------------------------------------------------- 3b. tile sizes
@pytest.mark.parametrize("name", ["synth", "eight", "dense"])
def test_tile_size_changes_no_bit(cases, synth_model, name):
    """The frames a workgroup takes shape the launch only.  SMPLPP_VERTEX_OFFSETS_FRAMES fixes them: 1, 5 (a tile shorter than a
    batch of loads), 12 and 32 (several batches, the last one partial), at n = 3, 33 and 45 (a full tile and a short last one of 1
    or 13 frames), the forward out of place with rest and in place, the per-frame backward stored and accumulated: the oracle's
    bits every time, so the bits at one frame per workgroup too."""
    from smplpp_amd import model_io

    c = cases[name]
    model = {"synth": lambda: synth_model, "eight": _eight_weight_model, "dense": lambda: model_io.tiny_model(TINY_V, seed=7)}[name]()
    W = c["W"]
    want = {}
    for n in (3, 33, 45):
        v, xf, rest, D, g = c["verts"][:n], c["xforms"][:n], c["rest"][:n], c["each"][:n], c["g"][:n]
        want[n] = (VO.forward(W, v, xf, D, rest=rest), VO.forward(W, v, xf, c["each"][7:8]), VO.backward(W, xf, g, False))
    for ft in (1, 5, 12, 32):
        s = _smpl(model, {"SMPLPP_VERTEX_OFFSETS_FRAMES": str(ft)})
        for n in (3, 33, 45):
            v, xf, rest, D, g = c["verts"][:n], c["xforms"][:n], c["rest"][:n], c["each"][:n], c["g"][:n]
            (wv, wr), wshared, wg = want[n]
            got, got_rest = s.vertexOffsets(v, xf, D, rest=rest)
            assert _same_bits(got, wv) and _same_bits(got_rest, wr), (ft, n)
            assert _same_bits(s.vertexOffsets(v, xf, c["each"][7:8]), wshared), (ft, n)
            dv = _dev(v)
            s.vertexOffsets(dv, _dev(xf), _dev(D), out=dv)  # in place on the device
            assert _same_bits(dv.cpu().numpy(), wv), (ft, n)
            assert _same_bits(s.vertexOffsetsBackward(xf, g), wg), (ft, n)
            base = np.random.default_rng(ft * 100 + n).normal(size=wg.shape).astype(np.float32)
            dacc = _dev(base)
            s.vertexOffsetsBackward(_dev(xf), _dev(g), out=dacc)
            assert _same_bits(dacc.cpu().numpy(), base + wg), (ft, n)
            assert _same_bits(s.vertexOffsetsBackward(xf, g, shared=True), VO.backward(W, xf, g, True))  # the shared tile is the rule's


# ---------------------------------------------------------------------------------------------------- 4. chain
@pytest.mark.parametrize("shared", [True, False])
def test_chain(smpl, synth_model, shared):
    from smplpp_amd import model_io

    n, V = 3, smpl.vertex_num
    dev = torch.device("cuda")
    beta, theta = model_io.synthetic_inputs(n, seed=41)
    rng = np.random.default_rng(42)
    D = VO.smooth_field(synth_model["vertices_template"])
    D = D if shared else (D[None] + rng.normal(0, 0.004, (n, V, 3))).astype(np.float32)
    cv, cj = rng.normal(size=(n, V, 3)).astype(np.float32), rng.normal(size=(n, 24, 3)).astype(np.float32)
    b, t, d = (torch.from_numpy(x).to(dev).requires_grad_(True) for x in (beta, theta, D))
    verts, joints = smpl.forward_displaced_differentiable(b, t, d)
    ((verts * _dev(cv)).sum() + (joints * _dev(cj)).sum()).backward()
    assert d.grad.shape == d.shape

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        bb, th, dd = (torch.tensor(x, dtype=dtype, requires_grad=True) for x in (beta, theta, D))
        out = FK.fk(m, bb, th)
        vv = VO.lbs(m["W"], out["rest"] + dd, out["xforms"], th[:, 0])
        ((vv * torch.tensor(cv, dtype=dtype)).sum() + (out["joints"] * torch.tensor(cj, dtype=dtype)).sum()).backward()
        return vv.detach().double().numpy(), [x.grad.double().numpy() for x in (bb, th, dd)]

    (v64, r64), (_, r32) = ref(torch.float64), ref(torch.float32)
    assert _rel(verts.detach().cpu().numpy(), v64) < 1e-5
    for got, want, w32, name in zip((b.grad, t.grad, d.grad), r64, r32, ("beta", "theta", "offsets")):
        err, bar = _rel(got.cpu().numpy(), want), max(4 * _rel(w32, want), 1e-5)
        print("chain %s %s: rel %.3g, fp32 autograd %.3g" % ("shared" if shared else "per-frame", name, err, _rel(w32, want)))
        assert np.abs(want).max() > 0 and err <= bar, (name, err, bar)


def test_chain_zero_offsets_is_forward_differentiable(smpl):
    from smplpp_amd import model_io

    n, V = 3, smpl.vertex_num
    dev = torch.device("cuda")
    beta, theta = model_io.synthetic_inputs(n, seed=43)
    rng = np.random.default_rng(44)
    cv, cj = _dev(rng.normal(size=(n, V, 3)).astype(np.float32)), _dev(rng.normal(size=(n, 24, 3)).astype(np.float32))
    grads = []
    for displaced in (False, True):
        b, t = (torch.from_numpy(x).to(dev).requires_grad_(True) for x in (beta, theta))
        if displaced:
            verts, joints = smpl.forward_displaced_differentiable(b, t, torch.zeros(V, 3, device=dev))
        else:
            verts, joints = smpl.forward_differentiable(b, t)
        ((verts * cv).sum() + (joints * cj).sum()).backward()
        grads.append((verts.detach().cpu().numpy(), b.grad.cpu().numpy(), t.grad.cpu().numpy()))
    assert (grads[0][0] == grads[1][0]).all()
    assert _same_bits(grads[0][1], grads[1][1]) and _same_bits(grads[0][2], grads[1][2])


# ---------------------------------------------------------------------------------------------------- 5. Laplacian
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("C", [1, 3, 4, 32])
def test_laplacian_bits(smpl, faces, C, n):
    rng = np.random.default_rng(10 * C + n)
    x = rng.normal(size=(n, smpl.vertex_num, C)).astype(np.float32)
    want = VO.laplacian(faces, x)
    got = smpl.meshLaplacian(x)
    assert got.dtype == np.float32 and _same_bits(got, want), int((got != want).sum())
    assert _same_bits(smpl.meshLaplacian(_dev(x)).cpu().numpy(), got)
    base = rng.normal(size=x.shape).astype(np.float32)
    acc = base.copy()
    assert smpl.meshLaplacian(x, out=acc) is acc and _same_bits(acc, base + got)
    const = np.ascontiguousarray(np.broadcast_to(rng.normal(size=(n, 1, C)).astype(np.float32), x.shape))
    assert (smpl.meshLaplacian(const) == 0).all()


def test_laplacian_on_a_tiny_mesh(cases):
    """Random faces (not a manifold), 61 vertices: the same rule."""
    from smplpp_amd import model_io

    s = cases["dense"]["s"]
    f = model_io.tiny_model(TINY_V, seed=7)["face_indices"].astype(np.int64) - 1
    x = np.random.default_rng(2).normal(size=(3, TINY_V, 5)).astype(np.float32)
    assert _same_bits(s.meshLaplacian(x), VO.laplacian(f, x))


def test_laplacian_differentiable(smpl, faces):
    rng = np.random.default_rng(6)
    x = rng.normal(size=(2, smpl.vertex_num, 3)).astype(np.float32)
    w = rng.normal(size=x.shape).astype(np.float32)
    xd = _dev(x).requires_grad_(True)
    y = smpl.mesh_laplacian_differentiable(xd)
    ((y * y).sum() + (y * _dev(w)).sum()).backward()  # |L x|^2: the gradient is 2 L (L x), two calls

    def ref(dtype):
        xx = torch.tensor(x, dtype=dtype, requires_grad=True)
        yy = VO.laplacian_torch(faces, xx)
        ((yy * yy).sum() + (yy * torch.tensor(w, dtype=dtype)).sum()).backward()
        return xx.grad.double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    err = _rel(xd.grad.cpu().numpy(), r64)
    print("laplacian autograd: rel %.3g, fp32 autograd %.3g" % (err, _rel(r32, r64)))
    assert np.abs(r64).max() > 0 and err <= max(4 * _rel(r32, r64), 1e-5)


# ---------------------------------------------------------------------------------------------------- 6. call rules
def test_call_rules(cases, synth_model):
    import ctypes as C

    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import _ptr

    L = _lib.load()
    c = cases["synth"]
    s, n = c["s"], 3
    V = s.vertex_num
    v, xf, rest, D, g = c["verts"][:n], c["xforms"][:n], c["rest"][:n], c["each"][:n], c["g"][:n]
    two = c["each"][:2]
    vo, rd, go = (np.full((n, V, 3), 7.0, np.float32) for _ in range(3))
    x = np.random.default_rng(1).normal(size=(n, V, 3)).astype(np.float32)
    lo = np.full((n, V, 3), 7.0, np.float32)

    def fwd(handle=None, n=n, vp=v, xp=xf, dp=D, frames=n, rp=rest, rdp=rd, op=vo, space=_lib.HOST):
        return L.smplpp_vertex_offsets(s.handle if handle is None else handle, n, _ptr(vp), _ptr(xp), _ptr(dp), frames, _ptr(rp), _ptr(rdp),
                                       _ptr(op), space, None)

    def bwd(handle=None, n=n, xp=xf, gp=g, frames=n, op=go, acc=0, space=_lib.HOST):
        return L.smplpp_vertex_offsets_vjp(s.handle if handle is None else handle, n, _ptr(xp), _ptr(gp), frames, _ptr(op), acc, space, None)

    def lap(handle=None, n=n, xp=x, ch=3, op=lo, acc=0, space=_lib.HOST):
        return L.smplpp_mesh_laplacian(s.handle if handle is None else handle, n, _ptr(xp), ch, _ptr(op), acc, space, None)

    names = {"fwd": "smplpp_vertex_offsets", "bwd": "smplpp_vertex_offsets_vjp", "lap": "smplpp_mesh_laplacian"}

    def refused(call, **kw):
        rc = call(**kw)
        msg = L.smplpp_last_error().decode()  # SMPLPP_ERR_INVALID with a message of this call's own
        assert rc == 1 and msg.startswith(names[call.__name__] + ": ") and len(msg) > len(names[call.__name__]) + 2, (kw, rc, msg)

    for kw in (dict(frames=2, dp=two), dict(frames=0), dict(frames=-1), dict(n=0), dict(n=-1), dict(n=1 << 40), dict(n=1 << 20), dict(vp=None),
               dict(xp=None), dict(dp=None), dict(op=None), dict(rp=None), dict(space=5)):
        refused(fwd, **kw)
    for kw in (dict(frames=2), dict(frames=0), dict(n=0), dict(n=-1), dict(n=1 << 40), dict(xp=None), dict(gp=None), dict(op=None),
               dict(op=g), dict(acc=2), dict(acc=-1), dict(space=5)):
        refused(bwd, **kw)
    for kw in (dict(ch=0), dict(ch=33), dict(ch=-1), dict(n=0), dict(n=-1), dict(n=1 << 40), dict(xp=None), dict(op=None), dict(op=x),
               dict(acc=2), dict(space=5)):
        refused(lap, **kw)
    # a model without faces has no Laplacian
    m = model_io._normalise(synth_model)
    h = C.c_void_p()
    _lib.check(L.smplpp_model_create(V, 0, _ptr(m["vertices_template"]), _ptr(m["shape_blend_shapes"]), _ptr(m["pose_blend_shapes"]),
                                     _ptr(m["joint_regressor"]), _ptr(m["weights"]), _ptr(m["kinematic_tree"]), None, 0, C.byref(h)))
    try:
        refused(lap, handle=h)
    finally:
        L.smplpp_model_destroy(h)
    assert all((a == 7.0).all() for a in (vo, rd, go, lo))  # refused calls leave the outputs alone
    with pytest.raises(_lib.SmplppError):
        s.vertexOffsets(v, xf, two)
    with pytest.raises(_lib.SmplppError):
        s.meshLaplacian(np.zeros((1, V, 33), np.float32))
    # rest without rest_displaced is ignored; the accepted calls write every element
    assert fwd(rdp=None) == 0 and fwd() == 0 and bwd() == 0 and lap() == 0
    assert _same_bits(vo, VO.forward(c["W"], v, xf, D)) and _same_bits(rd, rest + D)
    assert _same_bits(go, VO.backward(c["W"], xf, g, False)) and (lo != 7.0).all()


# ---------------------------------------------------------------------------------------------------- 7. a registration
def test_registration_of_a_displacement_field(smpl, synth_model):
    """The synthetic body at 4 poses carrying one smooth field of about 1.5 cm; a shared D fitted from zero by 10 plain gradient
    steps (size 0.25 V) on the mean squared vertex distance + lambda mean |L D|^2, lambda = 1e-3.  Asserted: the loss and the error
    of D both fell."""
    n, V, lam = 4, smpl.vertex_num, 1e-3
    dev = torch.device("cuda")
    rng = np.random.default_rng(51)
    theta = np.zeros((n, 25, 3), np.float32)
    theta[:, 1:] = rng.normal(0, 0.25, (n, 24, 3))
    beta = torch.zeros(n, 10, device=dev)
    t = _dev(theta)
    star = _dev(VO.smooth_field(synth_model["vertices_template"]))
    with torch.no_grad():
        target, _ = smpl.forward_displaced_differentiable(beta, t, star)
    D = torch.zeros(V, 3, device=dev, requires_grad=True)
    losses, errors = [], []
    for _ in range(11):
        verts, _ = smpl.forward_displaced_differentiable(beta, t, D)
        data = ((verts - target) ** 2).sum(-1).mean()
        smooth = (smpl.mesh_laplacian_differentiable(D[None]) ** 2).sum(-1).mean()
        loss = data + lam * smooth
        losses.append((float(loss.detach()), float(data.detach()), float(smooth.detach())))
        errors.append(float((D.detach() - star).norm() / star.norm()))
        (g,) = torch.autograd.grad(loss, D)
        with torch.no_grad():
            D -= 0.25 * V * g
    print("SMPL+D registration: loss %.3e -> %.3e (data %.3e -> %.3e m^2), |D - D*| / |D*| %.3f -> %.3f, rms D* %.4f m" %
          (losses[0][0], losses[-1][0], losses[0][1], losses[-1][1], errors[0], errors[-1], float(star.pow(2).sum(-1).mean().sqrt())))
    assert losses[0][0] > 0 and losses[-1][0] < losses[0][0] and errors[-1] < errors[0]


# ---------------------------------------------------------------------------------------------------- 8. C++ shim
def test_vertex_offsets_cpp_shim(tmp_path):
    from smplpp_amd import model_io

    exe = str(tmp_path / "vertex_offsets_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "vertex_offsets_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    n = 3
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    s = _smpl(model)
    V = s.vertex_num
    fk = s.launch(beta, theta, want=("verts", "xforms", "rest"))
    one = ((np.arange(V * 3, dtype=np.float32).reshape(1, V, 3) % 9) - 4) * np.float32(0.004)
    each = ((np.arange(n * V * 3, dtype=np.float32).reshape(n, V, 3) % 13) - 6) * np.float32(0.003)
    g = ((np.arange(n * V * 3, dtype=np.float32).reshape(n, V, 3) % 5) - 2) * np.float32(0.25)
    av, ar = s.vertexOffsets(fk["verts"], fk["xforms"], one, rest=fk["rest"])
    bv = s.vertexOffsets(fk["verts"], fk["xforms"], each)
    ge, gs = s.vertexOffsetsBackward(fk["xforms"], g), s.vertexOffsetsBackward(fk["xforms"], g, shared=True)
    acc = s.vertexOffsetsBackward(fk["xforms"], g, shared=True, out=np.ones((1, V, 3), np.float32))
    lap = s.meshLaplacian(each)
    lacc = s.meshLaplacian(each, out=np.ones_like(each))
    assert _same_bits(av, VO.forward(model["weights"], fk["verts"], fk["xforms"], one)) and np.abs(gs).max() > 0 and np.abs(lap).max() > 0
    want = b"".join(np.ascontiguousarray(a).tobytes() for a in (av, ar, bv, ge, gs, acc, lap, lacc))
    assert len(raw) == len(want) and raw == want
