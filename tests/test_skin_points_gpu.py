"""The bound points on the MI355X (smplpp_skin_points, smplpp_unskin_points and their vector-Jacobian products): every bit against the
numpy restatement of tests/skin_points_oracle.py on models that keep 4, 8 and 24 skinning weights per vertex, with a dead point of
each kind in the batch; independence of n, slot, space, outputs asked for and work split; the model's own vertices through a one-hot
binding against smplpp_fk; the chains from theta and beta against float64 autograd; a garment fit; the canonicalisation of a scan;
the call rules; the C++ shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import skeleton_oracle as SO  # noqa: E402
import skin_points_oracle as SP  # noqa: E402
import test_skin_points_cpu as CPU  # noqa: E402  (poses, bound_cloud, free_weights: the inputs whose float64 blends are shown alive there)
import vjp_blocks as VB  # noqa: E402
from distance_cases import _rel, _same_bits, _surface_points  # noqa: E402
from test_vertex_offsets_gpu import _dev, _eight_weight_model, _smpl  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NMAX, KMAX = 65, 2049
TINY_V = 61
f32, f64 = np.float32, np.float64
BAR = 1e-5
FWD, BWD = ("out", "blend", "valid"), ("points", "world", "joints", "weights")


def _host(a):
    return None if a is None else a.detach().cpu().numpy()


@pytest.fixture(scope="module")
def cases(synth_model):
    """Per weight width: the handle, the model's tables, NMAX frames of skeleton and KMAX bound points, shared and per frame.  In
    `world_flip` joint 23 is joint 22 turned by pi about its z axis, so that half and half of the two is a collapsed blend; the
    dense weights put nothing else on joint 23, and the face bindings, whose weights are the model's, see `world` as it came."""
    from smplpp_amd import model_io

    out = {}
    for name, model, width in (("synth", synth_model, 4), ("eight", _eight_weight_model(), 8),
                               ("dense", model_io.tiny_model(TINY_V, seed=7), 24)):
        s = _smpl(model)
        assert s.info()["weights_per_vertex"] == width
        beta, theta = CPU.poses(NMAX, seed=41)
        sk = s.skeleton(beta, theta, want=("world", "joints"))
        flip = sk["world"].copy()
        flip[:, 23, :, :3] = (flip[:, 22, :, :3].astype(f64) @ np.diag([-1.0, -1.0, 1.0])).astype(f32)
        weights = {1: CPU.free_weights(KMAX, seed=44), NMAX: CPU.free_weights(KMAX, seed=45, frames=NMAX)}
        for w in weights.values():
            w[..., 0] += w[..., 23]
            w[..., 23] = 0.0
        x1, face1, bary1 = CPU.bound_cloud(model, KMAX, seed=42)
        xn, facen, baryn = CPU.bound_cloud(model, KMAX, seed=43, frames=NMAX)
        rng = np.random.default_rng(width)
        out[name] = dict(s=s, model=model, W=model["weights"].astype(f32), faces=model["face_indices"].astype(np.int64) - 1, beta=beta, theta=theta,
                         world=sk["world"], world_flip=flip, joints=sk["joints"], x={1: x1, NMAX: xn}, face={1: face1, NMAX: facen},
                         bary={1: bary1, NMAX: baryn}, weights=weights,
                         g=rng.standard_normal((NMAX, KMAX, 3)).astype(f32))
    return out


def _inputs(c, n, K, binding, pf_shared, bf_shared, dead=True):
    """The call's arrays at (n, K): dict(world, joints, points, g, and face + bary or weights), with one dead point of each kind
    when K allows it.  Returns (arrays, indices of the dead points that are dead for skinning, for unskinning)."""
    a = dict(world=c["world" if binding == "face" else "world_flip"][:n], joints=c["joints"][:n], g=c["g"][:n, :K])
    cut = lambda d, shared: (d[1][:, :K] if shared else d[NMAX][:n, :K]).copy()  # noqa: E731
    a["points"] = cut(c["x"], pf_shared)
    dead_skin, dead_unskin = [], []
    if binding == "face":
        a["face"], a["bary"] = cut(c["face"], bf_shared), cut(c["bary"], bf_shared)
        if dead and K >= 63:
            a["face"][:, 1] = len(c["faces"])  # past the last face
            a["face"][:, 3] = -1
            a["bary"][:, 5, 0] = np.nan
            a["bary"][:, 9] = 0.0  # s = 0
            a["bary"][:, 11, 2] = np.inf
            dead_skin = [1, 3, 5, 7, 9, 11]
            dead_unskin = dead_skin
    else:
        a["weights"] = cut(c["weights"], bf_shared)
        if dead and K >= 63:
            a["weights"][:, 1] = 0.0  # s = 0
            a["weights"][:, 3, 4] = np.nan
            a["weights"][:, 5] = 0.0
            a["weights"][:, 5, 22:24] = 0.5  # the collapsed blend: dead for unskinning only
            a["weights"][:, 9] *= -1.0  # s < 0
            a["weights"][:, 11, 2] = np.inf
            dead_skin, dead_unskin = [1, 3, 7, 9, 11], [1, 3, 5, 7, 9, 11]
    if dead and K >= 63:
        a["points"][:, 7, 1] = np.inf
    return a, dead_skin, dead_unskin


def _bind_kw(a, device):
    conv = _dev if device else (lambda v: v)
    return {k: conv(a[k]) for k in ("face", "bary", "weights") if k in a}


def _run(s, a, unskin, device=True, want_fwd=("blend", "valid"), want_bwd=BWD):
    """Every output of the forward and the backward call, as numpy."""
    conv = _dev if device else (lambda v: v)
    back = _host if device else (lambda v: v)
    w, j, p, g = conv(a["world"]), conv(a["joints"]), conv(a["points"]), conv(a["g"])
    kw = _bind_kw(a, device)
    fwd = (s.unskinPoints if unskin else s.skinPoints)(w, j, p, want=want_fwd, **kw)
    res = dict(zip(FWD, (back(v) for v in fwd)))
    want = tuple(k for k in want_bwd if k != "weights" or "weights" in a)
    if want:
        grads = (s.unskinPointsBackward if unskin else s.skinPointsBackward)(w, j, p, g, want=want, **kw)
        res.update({k: back(v) for k, v in grads.items()})
    return res


def _oracle(c, a, unskin):
    om, ok = SP.omega_of(c["W"], c["faces"], a.get("face"), a.get("bary"), a.get("weights"))
    bw = SP.backward(a["world"], a["joints"], a["points"], om, ok, a["g"], unskin, want_weights="weights" in a)
    fw = bw.pop("forward")
    return {**{k: fw[k] for k in FWD}, **bw}


# ---------------------------------------------------------------------------------------------------- 1. every bit
# The restatement's cost grows with n and K, so n = 65 and K = 2049 take one combination of shared and per-frame inputs per binding where
# the small sizes take all four; every n, K, binding and frames value is met on every model.
def _combos(n, K):
    if n == 1:
        return [("face", True, True), ("weights", True, True)]
    if n <= 3 and K <= 1025:
        return [(b, p, q) for b in ("face", "weights") for p in (True, False) for q in (True, False)]
    return [("face", True, False), ("weights", False, True)]


@pytest.mark.parametrize("K", [1, 63, 65, 1025, 2049])
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("name", ["synth", "eight", "dense"])
def test_every_output_bit(cases, name, n, K):
    c = cases[name]
    for binding, pf_shared, bf_shared in _combos(n, K):
        a, dead_skin, dead_unskin = _inputs(c, n, K, binding, pf_shared, bf_shared)
        for unskin in (False, True):
            tag = (binding, pf_shared, bf_shared, unskin)
            got, want = _run(c["s"], a, unskin), _oracle(c, a, unskin)
            for key in want:
                assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (tag, key, got[key].shape, want[key].shape)
                assert _same_bits(got[key], want[key]), (tag, key, int((got[key] != want[key]).sum()), got[key].size)
            dead = dead_unskin if unskin else dead_skin
            alive = np.ones(K, bool)
            alive[dead] = False
            assert (got["valid"][:, ~alive] == 0).all() and not got["out"][:, ~alive].any() and not got["blend"][:, ~alive].any(), tag
            # no other point is dead (tests/test_skin_points_cpu.py shows it for these poses on the synthetic and the dense model),
            # but for blends that do collapse: the eight-weight model draws each vertex's joints at random from all over the tree
            others = int((got["valid"][:, alive] == 0).sum())
            assert others == 0 or (name == "eight" and unskin and binding == "face" and others <= 0.01 * n * K), (tag, others)
            assert np.isfinite(got["world"]).all() and np.isfinite(got["joints"]).all() and np.isfinite(got["points"]).all(), tag
            if K > 1:
                assert np.abs(got["world"]).max() > 0 and np.abs(got["points"]).max() > 0


def test_a_dead_point_does_not_touch_its_neighbours(cases):
    c = cases["synth"]
    n, K = 3, 65
    for binding in ("face", "weights"):
        a, dead_skin, dead_unskin = _inputs(c, n, K, binding, False, False)
        clean, _, _ = _inputs(c, n, K, binding, False, False, dead=False)
        for unskin in (False, True):
            same, dead = np.ones(K, bool), np.zeros(K, bool)
            same[dead_unskin] = False  # (every point whose inputs were changed)
            dead[dead_unskin if unskin else dead_skin] = True
            got, ref = _run(c["s"], a, unskin), _run(c["s"], clean, unskin)
            assert ref["valid"].all()
            for key in ("out", "blend", "points") + (("weights",) if binding == "weights" else ()):
                assert _same_bits(got[key][:, same], ref[key][:, same]), (binding, unskin, key)
                assert not got[key][:, dead].any()


# ---------------------------------------------------------------------------------------------------- 2. independence
@pytest.mark.parametrize("binding", ["face", "weights"])
def test_bits_do_not_depend_on_n_slot_space_or_outputs(cases, binding):
    c = cases["synth"]
    s, n, K = c["s"], 34, 1025
    a, _, _ = _inputs(c, n, K, binding, False, False, dead=False)
    for unskin in (False, True):
        full = _run(s, a, unskin)
        # host space
        host = _run(s, a, unskin, device=False)
        assert all(_same_bits(full[k], host[k]) for k in full), (binding, unskin)
        # a frame alone, in another slot of a smaller batch, has the bits it has inside the batch (per-frame outputs)
        for sl in (slice(33, 34), slice(31, 34)):
            sub = {k: (v[sl] if v.shape[0] == n else v) for k, v in a.items()}
            part = _run(s, sub, unskin)
            assert all(_same_bits(part[k], full[k][sl]) for k in part), (binding, unskin, sl)
        # one output at a time
        for key in ("blend", "valid"):
            alone = _run(s, a, unskin, want_fwd=(key,), want_bwd=())
            assert _same_bits(alone["out"], full["out"]) and _same_bits(alone[key], full[key])
        for key in BWD:
            if key in full:
                assert _same_bits(_run(s, a, unskin, want_fwd=(), want_bwd=(key,))[key], full[key]), (binding, unskin, key)


@pytest.mark.parametrize("env", [{"SMPLPP_SKIN_POINTS_FRAMES": "1"}, {"SMPLPP_SKIN_POINTS_FRAMES": "3"}, {"SMPLPP_SKIN_POINTS_FRAMES": "32"},
                                 {"SMPLPP_SKIN_POINTS_SPLIT": "4"}, {"SMPLPP_SKIN_POINTS_SPLIT": "1"}])
def test_bits_do_not_depend_on_the_work_split(cases, synth_model, env):
    """Every frame tile and every holder of the sum's partials the code can choose, forced at model creation, at sizes on both sides of
    the thresholds at which the default changes them."""
    c = cases["synth"]
    forced = _smpl(synth_model, env)
    for n, K in ((3, 63), (34, 65), (3, 1025), (5, 2049)):
        for binding, shared in (("face", True), ("weights", False), ("weights", True)):
            a, _, _ = _inputs(c, n, K, binding, shared, shared)
            for unskin in (False, True):
                got, ref = _run(forced, a, unskin), _run(c["s"], a, unskin)
                assert all(_same_bits(got[k], ref[k]) for k in ref), (env, n, K, binding, shared, unskin)


# ---------------------------------------------------------------------------------------------------- 3. the model's own vertices
def test_one_hot_bindings_reproduce_the_vertices(cases):
    for name in ("synth", "eight", "dense"):
        c = cases[name]
        s, faces = c["s"], c["faces"]
        n = 3
        beta, theta = CPU.poses(n, seed=51)
        fk = s.launch(beta, theta, want=("verts", "rest"))
        sk = s.skeleton(beta, theta, want=("world", "joints"))
        seen = np.unique(faces)  # the vertices some face names
        face = np.zeros(len(seen), np.int64)
        bary = np.zeros((len(seen), 3), f32)
        where = {}
        for t in range(len(faces) - 1, -1, -1):
            for corner in range(3):
                where[int(faces[t, corner])] = (t, corner)
        for i, v in enumerate(seen):
            face[i], corner = where[int(v)]
            bary[i, corner] = 1.0
        rest = np.ascontiguousarray(fk["rest"][:, seen])
        out, blend, valid = s.skinPoints(sk["world"], sk["joints"], rest, face=face, bary=bary)
        assert valid.all()
        err = np.abs(out.astype(f64) - fk["verts"][:, seen]).max()
        print("%s: %d vertices, max |skinPoints - smplpp_fk| = %.3g m" % (name, len(seen), err))
        assert err <= 1e-5
        carried = np.einsum("nkab,nkb->nka", blend[..., :3].astype(f64), rest.astype(f64)) + blend[..., 3]
        assert np.abs(carried - out).max() <= 1e-5
        # and back
        back, _, valid = s.unskinPoints(sk["world"], sk["joints"], out, face=face, bary=bary)
        live = valid.astype(bool)  # (the eight-weight model's random joint sets collapse at a few vertices)
        assert live.all() or (name == "eight" and live.mean() >= 0.99), (name, live.mean())
        assert np.abs(back.astype(f64) - rest)[live].max() <= 1e-5


# ---------------------------------------------------------------------------------------------------- 4. the chains
def _chain_reference(c, beta, theta, x, omega, G, unskin, dtype):
    """(dL/dbeta, dL/dtheta, dL/dpoints, dL/domega) of L = <definition(skeleton(beta, theta), x, omega), G> by autograd in `dtype`."""
    m = SO.cast(FK.model_tensors(c["model"]), dtype)
    t = lambda v: torch.as_tensor(np.asarray(v, f64), dtype=dtype)  # noqa: E731
    leaves = [t(v).clone().requires_grad_(True) for v in (beta, theta, x, omega)]
    sk = SO.skeleton(m, leaves[0], leaves[1])
    (SP.definition_torch(sk["world"], sk["J"], leaves[2], leaves[3], unskin) * t(G)).sum().backward()
    return [v.grad.double().numpy() for v in leaves]


def _held(tag, got, r64, r32, axes):
    e, e32 = VB.block_error(got, r64, axes), VB.block_error(r32, r64, axes)
    print("%s: E %.3g, fp32 autograd %.3g, bar %.3g" % (tag, e, e32, max(4 * e32, BAR)))
    assert np.isfinite(got).all() and np.abs(r64).max() > 0, tag
    assert e <= max(4 * e32, BAR), (tag, e, e32)


@pytest.mark.parametrize("unskin", [False, True])
@pytest.mark.parametrize("name", ["synth", "dense"])
def test_chain_from_theta_and_beta(cases, name, unskin):
    c = cases[name]
    s, n, K = c["s"], 4, 300
    beta, theta = c["beta"][:n], c["theta"][:n]
    G = c["g"][:n, :K]
    # a shared cloud under shared dense weights (grad_points and grad_weights are the frames' sums), then one per frame under faces
    for binding, shared in (("weights", True), ("face", False)):
        a, _, _ = _inputs(c, n, K, binding, shared, shared, dead=False)
        om, _ = SP.omega_of(c["W"], c["faces"], a.get("face"), a.get("bary"), a.get("weights"))
        x = a["points"]
        if unskin:  # posed points: the float64 image of the cloud at these poses
            sk64 = SO.forward(FK.model_tensors(c["model"]), beta, theta)
            x = SP.definition(sk64["world"], sk64["J"], x, om)[0].astype(f32)
            x = x if not shared else x[:1]
        b, th, xp = (_dev(v).requires_grad_(True) for v in (beta, theta, x))
        w = _dev(a["weights"]).requires_grad_(True) if binding == "weights" else None
        world, _, joints = s.skeleton_differentiable(b, th)
        fn = s.unskin_points_differentiable if unskin else s.skin_points_differentiable
        kw = dict(weights=w) if binding == "weights" else dict(face=_dev(a["face"]), bary=_dev(a["bary"]))
        out = fn(world, joints, xp, **kw)
        assert out.shape == (n, K, 3)
        (out * _dev(G)).sum().backward()
        r64 = _chain_reference(c, beta, theta, x, om, G, unskin, torch.float64)
        r32 = _chain_reference(c, beta, theta, x, om, G, unskin, torch.float32)
        tag = "%s %s %s" % (name, "unskin" if unskin else "skin", binding)
        _held(tag + " grad_beta", _host(b.grad), r64[0], r32[0], (1,))
        _held(tag + " grad_theta", _host(th.grad), r64[1], r32[1], VB.THETA)
        _held(tag + " grad_points", _host(xp.grad), r64[2], r32[2], (2,))
        if w is not None:
            _held(tag + " grad_weights", _host(w.grad), r64[3], r32[3], (2,))


# ---------------------------------------------------------------------------------------------------- 5. a fit
def test_garment_fit_through_the_two_calls(cases):
    """A few hundred garment points bound by dense weights, their targets posed by a known theta; Adam on theta from zero through
    skeleton_differentiable and skin_points_differentiable ends within twice the final error of the same loop in float64."""
    c = cases["synth"]
    s, K, steps = c["s"], 300, 80
    rng = np.random.default_rng(61)
    x, w = c["x"][1][:, :K], c["weights"][1][:, :K]
    theta_true = np.zeros((1, 25, 3), f32)
    theta_true[0, 1:] = rng.normal(0, 0.2, (24, 3))
    beta = np.zeros((1, 10), f32)
    m64 = FK.model_tensors(c["model"])
    t64 = lambda v: torch.as_tensor(np.asarray(v, f64))  # noqa: E731
    with torch.no_grad():
        sk = SO.skeleton(m64, t64(beta), t64(theta_true))
        target = SP.definition_torch(sk["world"], sk["J"], t64(x), t64(w))

    def loop(theta, forward):
        opt = torch.optim.Adam([theta], lr=0.03)
        for _ in range(steps):
            opt.zero_grad()
            loss = ((forward(theta) - target.to(theta.device, theta.dtype)) ** 2).sum()
            loss.backward()
            opt.step()
        with torch.no_grad():
            return float(((forward(theta) - target.to(theta.device, theta.dtype)) ** 2).sum(-1).mean().sqrt())

    def cpu64(theta):
        k = SO.skeleton(m64, t64(beta), theta)
        return SP.definition_torch(k["world"], k["J"], t64(x), t64(w))

    db, dx, dw = _dev(beta), _dev(x), _dev(w)

    def gpu32(theta):
        world, _, joints = s.skeleton_differentiable(db, theta)
        return s.skin_points_differentiable(world, joints, dx, weights=dw)

    start = float(((cpu64(torch.zeros(1, 25, 3, dtype=torch.float64)) - target) ** 2).sum(-1).mean().sqrt())
    e64 = loop(torch.zeros(1, 25, 3, dtype=torch.float64, requires_grad=True), cpu64)
    e32 = loop(torch.zeros(1, 25, 3, device="cuda", requires_grad=True), gpu32)
    print("garment fit: rms distance %.3g m at the start, %.3g m in float64, %.3g m through the calls" % (start, e64, e32))
    assert e64 < 0.5 * start and e32 <= 2 * e64, (start, e64, e32)


# ---------------------------------------------------------------------------------------------------- 6. a canonicalisation
def test_canonicalise_a_scan(cases):
    from smplpp_amd import model_io

    c = cases["synth"]
    s, n, K = c["s"], 3, 2000
    beta, theta = model_io.synthetic_inputs(n, seed=71)
    theta[:, 1:] = CPU.poses(n, seed=72)[1][:, 1:]  # N(0, 0.3^2), without the wide tail
    fk = s.launch(beta, theta, want=("verts",))
    sk = s.skeleton(beta, theta, want=("world", "joints"))
    scan = _surface_points(fk["verts"], c["faces"], K, np.random.default_rng(73), off=0.015)
    face, bary, _, _ = s.pointMeshDistance(fk["verts"], scan)
    out, blend, valid = s.unskinPoints(sk["world"], sk["joints"], scan, face=face, bary=bary)
    assert valid.all()
    om, ok = SP.omega_of(c["W"], c["faces"], face, bary)
    assert ok.all()
    ref, _, det = SP.definition(sk["world"], sk["joints"], scan, om, unskin=True)
    t32 = lambda v: torch.as_tensor(np.asarray(v, f32))  # noqa: E731
    plain = SP.definition_torch(t32(sk["world"]), t32(sk["joints"]), t32(scan), t32(om), unskin=True).double().numpy()
    e, e32 = _rel(out, ref), _rel(plain, ref)
    print("canonicalised scan: rel %.3g, fp32 definition %.3g, smallest det %.3g" % (e, e32, det.min()))
    assert det.min() > SP.MIN_DET and e <= max(4 * e32, BAR), (e, e32)
    # the canonical points lie near the rest surface: skinning them again returns the scan
    again, _, _ = s.skinPoints(sk["world"], sk["joints"], out, face=face, bary=bary)
    assert np.abs(again.astype(f64) - scan).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------- 7. the call rules
def test_refusals_leave_the_outputs(cases, synth_model):
    import ctypes as C

    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import _ptr

    L = _lib.load()
    c = cases["synth"]
    s, n, K = c["s"], 2, 5
    a, _, _ = _inputs(c, n, K, "face", True, True, dead=False)
    wts = c["weights"][1][:, :K].copy()
    out = {k: np.full(sh, 7.0, f32) for k, sh in dict(o=(n, K, 3), b=(n, K, 3, 4), gp=(1, K, 3), gw=(n, 24, 3, 4), gj=(n, 24, 3), gwt=(1, K, 24)).items()}
    valid = np.full((n, K), 7, np.uint8)
    p = lambda v: None if v is None else v.ctypes.data  # noqa: E731
    base = dict(m=s.handle, n=n, world=a["world"], joints=a["joints"], K=K, points=a["points"], pf=1, face=a["face"], bary=a["bary"], weights=None,
                bf=1, space=0)

    def fwd(fn, o="o", **kw):
        k = dict(base, **kw)
        return fn(k["m"], k["n"], p(k["world"]), p(k["joints"]), k["K"], p(k["points"]), k["pf"], p(k["face"]), p(k["bary"]), p(k["weights"]),
                  k["bf"], p(out[o]) if o else None, p(out["b"]), p(valid), k["space"], None)

    def vjp(fn, g=a["g"], gp="gp", gw="gw", gj="gj", gwt=None, acc=0, **kw):
        k = dict(base, **kw)
        o = lambda key: p(out[key]) if key else None  # noqa: E731
        return fn(k["m"], k["n"], p(k["world"]), p(k["joints"]), k["K"], p(k["points"]), k["pf"], p(k["face"]), p(k["bary"]), p(k["weights"]),
                  k["bf"], p(g), o(gp), o(gw), o(gj), o(gwt), acc, k["space"], None)

    m = model_io._normalise(synth_model)
    faceless = C.c_void_p()
    _lib.check(L.smplpp_model_create(s.vertex_num, 0, _ptr(m["vertices_template"]), _ptr(m["shape_blend_shapes"]), _ptr(m["pose_blend_shapes"]),
                                     _ptr(m["joint_regressor"]), _ptr(m["weights"]), _ptr(m["kinematic_tree"]), None, 0, C.byref(faceless)))
    bad_face = a["face"].copy()
    bad_face[0, 2] = len(c["faces"])
    common = [dict(n=0), dict(n=-1), dict(K=0), dict(K=-2), dict(world=None), dict(joints=None), dict(points=None), dict(weights=wts),
              dict(face=None, bary=None), dict(bary=None), dict(face=None), dict(m=faceless), dict(pf=3), dict(pf=0), dict(bf=3), dict(bf=0),
              dict(face=bad_face), dict(face=-bad_face - 1), dict(n=2 ** 20, K=2 ** 10, pf=1, bf=1), dict(n=2 ** 23, K=1), dict(space=2)]
    for fn in (L.smplpp_skin_points, L.smplpp_unskin_points):
        for kw in common:
            assert fwd(fn, **kw) == 1 and L.smplpp_last_error(), (fn.__name__, list(kw))
        assert fwd(fn, o=None) == 1
        assert fwd(fn) == 0  # the base call is a good one
        out["o"][:], out["b"][:], valid[:] = 7.0, 7.0, 7
    for fn in (L.smplpp_skin_points_vjp, L.smplpp_unskin_points_vjp):
        for kw in common + [dict(g=None), dict(gp=None, gw=None, gj=None), dict(gwt="gwt"), dict(acc=2), dict(acc=-1)]:
            assert vjp(fn, **kw) == 1 and L.smplpp_last_error(), (fn.__name__, list(kw))
    assert "int32" in (fwd(L.smplpp_skin_points, n=2 ** 20, K=2 ** 10), L.smplpp_last_error().decode())[1]
    assert all((v == 7).all() for v in out.values()) and (valid == 7).all()
    # the binding words its own refusals
    for bad in (dict(points=a["points"][:, :, :2]), dict(bary=a["bary"][:, :3]), dict(weights=wts), dict(face=None), dict(world=a["world"][:, :5])):
        kw = dict(world=a["world"], joints=a["joints"], points=a["points"], face=a["face"], bary=a["bary"])
        kw.update(bad)
        with pytest.raises(_lib.SmplppError):
            s.skinPoints(**kw)
    with pytest.raises(_lib.SmplppError):
        s.skinPointsBackward(a["world"], a["joints"], a["points"], a["g"], face=a["face"], bary=a["bary"], want=("weights",))
    _lib.check(L.smplpp_model_destroy(faceless))


@pytest.mark.parametrize("unskin", [False, True])
def test_accumulate_adds_exactly_once(cases, unskin):
    c = cases["synth"]
    s = c["s"]
    for n, K, shared in ((3, 65, True), (34, 63, False)):
        a, _, _ = _inputs(c, n, K, "weights", shared, shared)
        fn = s.unskinPointsBackward if unskin else s.skinPointsBackward
        args = (a["world"], a["joints"], a["points"], a["g"])
        plain = fn(*args, weights=a["weights"])
        for device in (False, True):
            conv = _dev if device else (lambda v: v)
            acc = {k: conv(np.full(v.shape, 1.5, f32)) for k, v in plain.items()}
            res = fn(*(conv(v) for v in args), weights=conv(a["weights"]), out=acc)
            assert set(res) == set(plain)
            for k, v in plain.items():
                got = _host(acc[k]) if device else acc[k]
                assert _same_bits(got, f32(1.5) + v), (n, K, k, device)


# ---------------------------------------------------------------------------------------------------- 8. C++ shim
def test_skin_points_cpp_shim(tmp_path):
    from smplpp_amd import model_io

    exe = str(tmp_path / "skin_points_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "skin_points_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    n, K = 3, 70
    F = len(model["face_indices"])
    beta = (np.arange(n * 10, dtype=f32).reshape(n, 10) % 7 - 3) * f32(0.1)
    theta = ((np.arange(n * 75, dtype=f32).reshape(n, 25, 3) % 11) - 5) * f32(0.05)
    s = _smpl(model)
    sk = s.skeleton(beta, theta, want=("world", "joints"))
    cloud = ((np.arange(K * 3, dtype=f32).reshape(1, K, 3) % 9) - 4) * f32(0.05)
    g = ((np.arange(n * K * 3, dtype=f32).reshape(n, K, 3) % 5) - 2) * f32(0.25)
    k = np.arange(K)
    abc = np.stack([k % 5 + 1, k % 3 + 1, k % 7 + 1], 1).astype(f32)
    bary = (abc / ((abc[:, 0] + abc[:, 1]) + abc[:, 2])[:, None])[None]
    face = ((k * 5) % F)[None]
    weights = ((np.arange(n * K * 24) * 7) % 5).astype(f32).reshape(n, K, 24) * f32(0.125)
    w, j = sk["world"], sk["joints"]
    posed = s.skinPoints(w, j, cloud, face=face, bary=bary)
    gs = s.skinPointsBackward(w, j, cloud, g, face=face, bary=bary)
    back = s.unskinPoints(w, j, posed[0], weights=weights)
    gu = s.unskinPointsBackward(w, j, posed[0], g, weights=weights)
    assert posed[2].all() and back[2].all() and np.abs(gu["weights"]).max() > 0 and "weights" not in gs
    parts = [posed[0], posed[1], posed[2].astype(np.int64), gs["points"], gs["world"], gs["joints"], back[0], back[1], back[2].astype(np.int64),
             gu["points"], gu["world"], gu["joints"], gu["weights"]]
    want = b"".join(np.ascontiguousarray(v).tobytes() for v in parts)
    assert len(raw) == len(want) and raw == want
