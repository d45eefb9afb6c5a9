"""smplpp_fk_rotmat / smplpp_fk_rotmat_vjp / smplpp_axis_angle_to_rotmat on the MI355X: bit identity with the axis-angle path under
every form, general (not orthonormal) matrices and the backward against the float64 restatement (tests/fk_rotmat_oracle.py), the tie
to smplpp_fk_vjp, call semantics, torch.autograd through the 6-D representation, the SMPL+D composition and the C++ shim.

The fp32 bar, as in test_fk_vjp_gpu.py: relative error (2-norm) against float64 at most max(4 x that of the float32 restatement,
1e-5)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_rotmat_oracle as RO  # noqa: E402
import fk_vjp_oracle as O  # noqa: E402
from vjp_blocks import eight_weights as _eight_weights  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 33, 65]  # 33 and 65 cross the 32- and 64-frame tile edges of every form
FORMS = ["default", "h", "b", "v"]
KEYS = ("verts", "joints", "xforms", "rest")


def _smpl(model, form="default"):
    """A model created under SMPLPP_SKIN = form (read at creation; "default" = unset)."""
    from smplpp_amd.smpl import SMPL

    old = os.environ.pop("SMPLPP_SKIN", None)
    try:
        if form != "default":
            os.environ["SMPLPP_SKIN"] = form
        s = SMPL()
        s.setDevice("cuda:0")
        s.init(model)
    finally:
        os.environ.pop("SMPLPP_SKIN", None)
        if old is not None:
            os.environ["SMPLPP_SKIN"] = old
    return s


@pytest.fixture(scope="module")
def models(synth_model):
    return {form: _smpl(synth_model, form) for form in FORMS}


@pytest.fixture(scope="module")
def smpl(models):
    return models["default"]


@pytest.fixture(scope="module")
def m64(synth_model):
    return RO.model_tensors(synth_model)


def _inputs(n, seed):
    """beta, theta with a theta = 0 joint, a whole zero frame and |theta| = pi joints, at most two of those in a frame."""
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(n, seed=seed)
    rng = np.random.default_rng(seed + 100)
    theta[0, 3] = 0.0
    if n > 2:
        theta[2, 1:] = 0.0
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    theta[n - 1, 7] = (np.pi * ax[n - 1]).astype(np.float32)
    if n > 3:
        theta[1, 2:4] = (np.pi * ax[1]).astype(np.float32)
    return beta, theta


def _at_pi(theta):
    """[n,24] bool: the joints whose axis-angle has norm pi (to fp32 rounding)."""
    return np.abs(np.linalg.norm(theta[:, 1:].astype(np.float64), axis=-1) - np.pi) < 1e-5


def _general(smpl, theta, seed):
    """Rodrigues + 0.05 N(0,1) per entry: not orthonormal, inside form h's range."""
    rng = np.random.default_rng(seed)
    R = smpl.axisAngleToRotmat(theta[:, 1:])
    return (R + 0.05 * rng.standard_normal(R.shape)).astype(np.float32)


def _grads(V, n, seed, kind):
    rng = np.random.default_rng(seed)
    gv = rng.standard_normal((n, V, 3)).astype(np.float32) if kind in ("verts", "both") else None
    gj = rng.standard_normal((n, 24, 3)).astype(np.float32) if kind in ("joints", "both") else None
    return gv, gj


def _rel(a, b):
    return np.linalg.norm((np.asarray(a, np.float64) - b).ravel()) / max(np.linalg.norm(np.asarray(b).ravel()), 1e-30)


def _bar(f32, f64):
    return max(4 * _rel(f32, f64), 1e-5)


_cache = {}


def _cached(key, make):
    """One reference per key for the whole module (the forms and the rest / no-rest runs share it; never modified)."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _frames(n):
    return sorted(set(f for f in (0, 1, 2, n // 2, n - 1) if f < n))


# ---------------------------------------------------------------------------------------------- 1. bit identity
def _assert_same_bits(s, beta, theta):
    a = s.launch(beta, theta)
    a = {k: a[k].copy() for k in KEYS}
    R = s.axisAngleToRotmat(theta[:, 1:])
    assert R.shape == (len(theta), 24, 3, 3) and R.dtype == np.float32
    b = s.launchRotmat(beta, np.ascontiguousarray(theta[:, 0]), R)
    for k in KEYS:
        assert np.isfinite(b[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    return b


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", FORMS)
def test_rotmat_launch_has_the_bits_of_the_axis_angle_launch(models, form, n):
    beta, theta = _inputs(n, seed=n)
    assert _at_pi(theta).any() and (theta[0, 3] == 0).all()
    s = models[form]
    _assert_same_bits(s, beta, theta)
    # the getters serve launchRotmat's outputs
    assert np.array_equal(s.getTransformation(), s._out["xforms"])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["eight", "dense"])
def test_rotmat_launch_bits_with_8_and_24_weights_per_vertex(synth_model, which, form):
    """8 weights per vertex: the default form hands the model to b (MAXW = 8); 24: e and b hand it to the first form."""
    from smplpp_amd import model_io

    model = _cached(("model", which), lambda: _eight_weights(synth_model) if which == "eight" else model_io.tiny_model(61, seed=7))
    s = _smpl(model, form)
    assert s.info()["weights_per_vertex"] == {"eight": 8, "dense": 24}[which]
    beta, theta = _inputs(33, seed=3)
    _assert_same_bits(s, beta, theta)


# ---------------------------------------------------------------------------------------------- 2. general matrices
def _general_case(smpl, m64, n):
    def make():
        beta, theta = _inputs(n, seed=40 + n)
        R = _general(smpl, theta, seed=n)
        trans = np.ascontiguousarray(theta[:, 0])
        return beta, trans, R, RO.forward(m64, beta, trans, R), RO.forward(m64, beta, trans, R, dtype=O.torch.float32)

    return _cached(("general", n), make)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", FORMS)
def test_rotmat_launch_general_matrices_against_float64(models, smpl, m64, form, n):
    beta, trans, R, r64, r32 = _general_case(smpl, m64, n)
    RtR = np.einsum("njab,njac->njbc", R.astype(np.float64), R.astype(np.float64))
    assert np.abs(RtR - np.eye(3)).max() > 0.05  # not orthonormal
    s = models[form]
    out = s.launchRotmat(beta, trans, R)
    if form == "h":
        assert s.launchStatus() == 0  # inside the fp16x2 form's range
    for k in ("verts", "joints", "rest"):
        assert np.isfinite(out[k]).all(), k
        for f in _frames(n):
            err, bar = _rel(out[k][f], r64[k][f]), _bar(r32[k][f], r64[k][f])
            print("general", form, n, k, f, "err %.3g bar %.3g" % (err, bar))
            assert err <= bar, (form, n, k, f, err, bar)
    # trans = NULL and beta = NULL are explicit zeros, to the bit
    zb, zt = np.zeros_like(beta), np.zeros_like(trans)
    a = s.launchRotmat(None, None, R)
    a = {k: a[k].copy() for k in KEYS}
    b = s.launchRotmat(zb, zt, R)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- 3. axis-angle -> matrix
def test_axis_angle_to_rotmat(smpl):
    import torch

    rng = np.random.default_rng(9)
    aa = (rng.standard_normal((517, 3)) * 1.2).astype(np.float32)
    aa[0] = 0.0
    ax = rng.standard_normal((4, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    aa[1], aa[2] = np.pi * ax[0], np.pi * ax[1]
    aa[3], aa[4] = 2 * np.pi * ax[2], 2 * np.pi * ax[3]
    aa[5] = [1e-6, 0, 0]
    R = smpl.axisAngleToRotmat(aa)
    assert R.shape == (517, 3, 3) and np.isfinite(R).all()
    want = RO.rodrigues_np(aa)  # float64, the reference's eps, at the fp32 inputs
    err = np.abs(R - want).max()
    print("axis-angle -> matrix: max |d| = %.3g" % err)
    assert err <= 5e-7  # 4 ulp of 1
    assert np.abs(R[0] - np.eye(3)).max() <= 5e-7
    d = smpl.axisAngleToRotmat(torch.from_numpy(aa).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), R)  # host and device space: the same bits
    assert smpl.axisAngleToRotmat(aa.reshape(11, 47, 3)).shape == (11, 47, 3, 3)


# ---------------------------------------------------------------------------------------------- 4. backward, dense parity
def _backward_case(smpl, m64, n, kind, general):
    def make():
        beta, theta = _inputs(n, seed=60 + n)
        R = _general(smpl, theta, seed=7 + n) if general else smpl.axisAngleToRotmat(theta[:, 1:])
        trans = np.ascontiguousarray(theta[:, 0])
        gv, gj = _grads(smpl.vertex_num, n, seed=7 * n, kind=kind)
        return (beta, theta, trans, R, gv, gj, RO.vjp(m64, beta, trans, R, gv, gj),
                RO.vjp(m64, beta, trans, R, gv, gj, dtype=O.torch.float32))

    return _cached(("backward", n, kind, general), make)


def _check_backward(out, ref64, ref32, n, tag):
    for name, r64, r32 in zip(("beta", "trans", "rot"), ref64, ref32):
        assert np.isfinite(out[name]).all(), name
        for f in _frames(n):
            if not np.any(r64[f]):  # (no cotangent reaches it: joints-only losses and trans / rot)
                assert not np.any(out[name][f]), (tag, name, f)
                continue
            err, bar = _rel(out[name][f], r64[f]), _bar(r32[f], r64[f])
            print("backward", tag, n, name, f, "err %.3g bar %.3g" % (err, bar))
            assert err <= bar, (tag, name, f, err, bar)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", ["verts", "joints", "both"])
def test_rotmat_backward_dense_parity(smpl, m64, n, kind):
    beta, theta, trans, R, gv, gj, r64, r32 = _backward_case(smpl, m64, n, kind, False)
    rest = smpl.launchRotmat(beta, trans, R, want=("rest",))["rest"]
    out = smpl.launchRotmatBackward(beta, trans, R, grad_verts=gv, grad_joints=gj, rest=rest)
    assert out["rot"].shape == (n, 24, 3, 3) and out["trans"].shape == (n, 3)
    _check_backward(out, r64, r32, n, kind)


@pytest.mark.parametrize("n", NS)
def test_rotmat_backward_recomputes_rest(smpl, m64, n):
    beta, theta, trans, R, gv, gj, r64, r32 = _backward_case(smpl, m64, n, "both", False)
    _check_backward(smpl.launchRotmatBackward(beta, trans, R, grad_verts=gv, grad_joints=gj), r64, r32, n, "rest=None")


@pytest.mark.parametrize("n", NS)
def test_rotmat_backward_general_matrices(smpl, m64, n):
    beta, theta, trans, R, gv, gj, r64, r32 = _backward_case(smpl, m64, n, "both", True)
    rest = smpl.launchRotmat(beta, trans, R, want=("rest",))["rest"]
    _check_backward(smpl.launchRotmatBackward(beta, trans, R, grad_verts=gv, grad_joints=gj, rest=rest), r64, r32, n, "general")


# ---------------------------------------------------------------------------------------------- 5. tied to smplpp_fk_vjp
@pytest.mark.parametrize("n", NS)
def test_rotmat_backward_tied_to_the_axis_angle_backward(smpl, m64, n):
    beta, theta, trans, R, gv, gj, r64, r32 = _backward_case(smpl, m64, n, "both", False)
    rest = smpl.launch(beta, theta, want=("rest",))["rest"]
    aa = smpl.launchBackward(beta, theta, grad_verts=gv, grad_joints=gj, rest=rest)
    rm = smpl.launchRotmatBackward(beta, trans, R, grad_verts=gv, grad_joints=gj, rest=rest)
    assert np.array_equal(rm["beta"], aa["beta"])
    assert np.array_equal(rm["trans"], aa["theta"][:, 0])
    assert np.isfinite(rm["rot"]).all()
    # dL/dR contracted with the float64 Rodrigues derivative is dL/dtheta, away from |theta| = pi (where the AXIS-ANGLE side is
    # ill-conditioned; dL/dR itself passed the dense parity on those joints)
    pi = _at_pi(theta)
    assert pi.any() and pi.sum(axis=1).max() <= 2
    back = RO.contract_rodrigues(theta[:, 1:], rm["rot"])
    gb32, gt32 = O.vjp(m64, beta, theta, gv, gj, dtype=O.torch.float32)
    gb64, gt64 = O.vjp(m64, beta, theta, gv, gj)
    keep = ~pi
    for f in _frames(n):
        want = aa["theta"][f, 1:][keep[f]].astype(np.float64)
        err = _rel(back[f][keep[f]], want)
        bar = _bar(gt32[f, 1:][keep[f]], gt64[f, 1:][keep[f]])
        print("tied", n, f, "err %.3g bar %.3g" % (err, bar))
        assert err <= bar, (f, err, bar)


# ---------------------------------------------------------------------------------------------- 6. call semantics
def test_rotmat_call_semantics(smpl, m64):
    import torch
    from smplpp_amd import _lib

    L = _lib.load()
    n, V = 65, smpl.vertex_num
    beta, theta, trans, R, gv, gj, _, _ = _backward_case(smpl, m64, n, "both", True)
    p = lambda a: None if a is None else a.ctypes.data
    full = smpl.launchRotmat(beta, trans, R)
    full = {k: full[k].copy() for k in KEYS}
    # any subset of outputs may be NULL
    for want in (("verts",), ("joints",), ("xforms",), ("rest",), ("joints", "xforms"), ("verts", "rest"), ()):
        o = smpl.launchRotmat(beta, trans, R, want=want)
        for k in KEYS:
            assert (o[k] is None) == (k not in want)
            if k in want:
                assert np.array_equal(o[k], full[k]), (want, k)
    # twice: the same bits; device space: the same bits
    again = smpl.launchRotmat(beta, trans, R)
    dev = lambda a: torch.from_numpy(a).cuda()
    d = smpl.launchRotmat(dev(beta), dev(trans), dev(R))
    torch.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(again[k], full[k]), k
        assert np.array_equal(d[k].cpu().numpy(), full[k]), k
    # a frame alone has the bits it has inside n = 65
    for f in (0, 1, 33, 64):
        one = smpl.launchRotmat(beta[f:f + 1], trans[f:f + 1], R[f:f + 1])
        for k in KEYS:
            assert np.array_equal(one[k][0], full[k][f]), (f, k)
    # backward: deterministic, device == host, NULL outputs (its vertex sums are chunked by the batch: no frame-alone promise)
    b1 = smpl.launchRotmatBackward(beta, trans, R, grad_verts=gv, grad_joints=gj, rest=full["rest"])
    b2 = smpl.launchRotmatBackward(beta, trans, R, grad_verts=gv, grad_joints=gj, rest=full["rest"])
    bd = smpl.launchRotmatBackward(dev(beta), dev(trans), dev(R), grad_verts=dev(gv), grad_joints=dev(gj), rest=dev(full["rest"]))
    torch.cuda.synchronize()
    for k in ("beta", "trans", "rot"):
        assert np.array_equal(b1[k], b2[k]), k
        assert np.array_equal(bd[k].cpu().numpy(), b1[k]), k
    gb, gt, gr = np.empty((n, 10), np.float32), np.empty((n, 3), np.float32), np.empty((n, 24, 3, 3), np.float32)
    for outs in ((gb, None, None), (None, gt, None), (None, None, gr), (gb, None, gr)):
        for a in outs:
            if a is not None:
                a.fill(7.0)
        _lib.check(L.smplpp_fk_rotmat_vjp(smpl.handle, n, p(beta), None, p(R), p(full["rest"]), p(gv), p(gj), p(outs[0]), p(outs[1]),
                                          p(outs[2]), _lib.HOST, None))
        for a, k in zip(outs, ("beta", "trans", "rot")):
            if a is not None:
                assert np.array_equal(a, b1[k]), k
    # zero cotangents: exact zeros
    z = smpl.launchRotmatBackward(beta, trans, R)
    assert not z["beta"].any() and not z["trans"].any() and not z["rot"].any()
    # refusals: the codes of the axis-angle entry points' counterparts, and a message
    def code(rc):
        if rc:
            assert L.smplpp_last_error()
        return rc

    th = np.zeros((n, 25, 3), np.float32)
    v = np.empty((n, V, 3), np.float32)
    assert code(L.smplpp_fk_rotmat(smpl.handle, n, p(beta), p(trans), None, p(v), None, None, None, _lib.HOST, None)) == \
        code(L.smplpp_fk(smpl.handle, n, p(beta), None, p(v), None, None, None, _lib.HOST, None)) != 0
    assert code(L.smplpp_fk_rotmat(smpl.handle, -1, p(beta), p(trans), p(R), p(v), None, None, None, _lib.HOST, None)) == \
        code(L.smplpp_fk(smpl.handle, -1, p(beta), p(th), p(v), None, None, None, _lib.HOST, None)) != 0
    assert code(L.smplpp_fk_rotmat(smpl.handle, n, p(beta), p(trans), p(R), p(v), None, None, None, 5, None)) == \
        code(L.smplpp_fk(smpl.handle, n, p(beta), p(th), p(v), None, None, None, 5, None)) != 0
    assert code(L.smplpp_fk_rotmat_vjp(smpl.handle, n, p(beta), None, None, None, p(gv), None, p(gb), None, None, _lib.HOST, None)) == \
        code(L.smplpp_fk_vjp(smpl.handle, n, p(beta), None, None, p(gv), None, p(gb), None, _lib.HOST, None)) != 0
    assert code(L.smplpp_fk_rotmat_vjp(smpl.handle, -1, p(beta), None, p(R), None, p(gv), None, p(gb), None, None, _lib.HOST, None)) == \
        code(L.smplpp_fk_vjp(smpl.handle, -1, p(beta), p(th), None, p(gv), None, p(gb), None, _lib.HOST, None)) != 0
    # no cotangent and no output: what smplpp_fk_vjp answers
    assert L.smplpp_fk_rotmat_vjp(smpl.handle, n, p(beta), None, p(R), None, None, None, None, None, None, _lib.HOST, None) == \
        L.smplpp_fk_vjp(smpl.handle, n, p(beta), p(th), None, None, None, None, None, _lib.HOST, None)
    with pytest.raises(_lib.SmplppError):
        smpl.launchRotmat(beta, trans, R[:, :23])


def test_rotmat_launch_reports_the_fp16x2_range(models, smpl, m64):
    import torch
    from smplpp_amd._lib import SmplppError

    beta, trans, R, _, _ = _general_case(smpl, m64, 33)
    s = models["h"]
    assert s.launchStatus() == 0
    big = (R * np.float32(1e6)).astype(np.float32)
    with pytest.raises(SmplppError) as ei:
        s.launchRotmat(beta, trans, big, want=("verts",))
    assert ei.value.code == 3
    s.launchRotmat(torch.from_numpy(beta).cuda(), torch.from_numpy(trans).cuda(), torch.from_numpy(big).cuda(), want=("verts",))
    assert s.launchStatus() & 1
    o = s.launchRotmat(beta, trans, R, want=("verts",))  # in range again: clean
    assert np.isfinite(o["verts"]).all() and s.launchStatus() == 0
    # the default form has no such range and raises no bit (a chain of nine such matrices leaves fp32 itself)
    smpl.launchRotmat(beta, trans, big, want=("verts",))
    assert smpl.launchStatus() == 0


def test_rotmat_backward_leaves_the_forward_workspace_alone(smpl, m64):
    """smplpp_fk's results after an interleaved smplpp_fk_rotmat_vjp(rest = NULL), which runs a forward pass of its own."""
    n = 65
    beta, theta, trans, R, gv, gj, _, _ = _backward_case(smpl, m64, n, "both", True)
    ref = smpl.launch(beta, theta)
    ref = {k: ref[k].copy() for k in KEYS}
    refr = smpl.launchRotmat(beta, trans, R)
    refr = {k: refr[k].copy() for k in KEYS}
    smpl.launchRotmatBackward(beta[:40], trans[:40], R[:40], grad_verts=gv[:40], grad_joints=gj[:40])
    again = smpl.launch(beta, theta)
    for k in KEYS:
        assert np.array_equal(again[k], ref[k]), k
    smpl.launchRotmatBackward(beta[:40], trans[:40], R[:40], grad_verts=gv[:40], grad_joints=gj[:40])
    again = smpl.launchRotmat(beta, trans, R)
    for k in KEYS:
        assert np.array_equal(again[k], refr[k]), k
    assert smpl.launchStatus() == 0


# ---------------------------------------------------------------------------------------------- 7. autograd end to end
def test_rotmat_autograd_through_the_6d_representation(smpl, m64):
    import torch
    from smplpp_amd.smpl import rot6d_to_rotmat

    n = 7
    rng = np.random.default_rng(17)
    beta = (rng.standard_normal((n, 10)) * 0.5).astype(np.float32)
    trans = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    x6 = (np.tile([1, 0, 0, 1, 0, 0], (n, 24, 1)) + 0.4 * rng.standard_normal((n, 24, 6))).astype(np.float32)
    gv, gj = _grads(smpl.vertex_num, n, seed=3, kind="both")

    def grads(dtype, run):
        leaf = lambda a: torch.as_tensor(a, dtype=dtype).clone().requires_grad_(True)
        b, t, x = leaf(beta), leaf(trans), leaf(x6)
        verts, joints = run(b, t, x)
        loss = (verts * torch.as_tensor(gv, dtype=dtype, device=verts.device)).sum() + \
            (joints * torch.as_tensor(gj, dtype=dtype, device=verts.device)).sum()
        return [g.detach().cpu().numpy().astype(np.float64) for g in torch.autograd.grad(loss, (b, t, x))]

    def oracle(dtype):
        mm = RO.cast(m64, dtype)

        def run(b, t, x):
            o = RO.fk(mm, b, t, RO.rot6d_to_rotmat(x))
            return o["verts"], o["joints"]

        return grads(dtype, run)

    def device(b, t, x):
        verts, joints, xforms = smpl.forward_rotmat_differentiable(b.cuda(), t.cuda(), rot6d_to_rotmat(x.cuda()))
        assert not xforms.requires_grad and verts.requires_grad and joints.requires_grad
        assert xforms.shape == (n, 24, 4, 4)
        return verts, joints

    r64, r32, got = oracle(torch.float64), oracle(torch.float32), grads(torch.float32, device)
    for name, g, a, b in zip(("beta", "trans", "x6"), got, r64, r32):
        assert np.isfinite(g).all(), name
        for f in range(n):
            err, bar = _rel(g[f], a[f]), _bar(b[f], a[f])
            print("autograd", name, f, "err %.3g bar %.3g" % (err, bar))
            assert err <= bar, (name, f, err, bar)


def _recovery_targets(n=4, seed=31):
    rng = np.random.default_rng(seed)
    beta = (rng.standard_normal((n, 10)) * 0.5).astype(np.float32)
    theta = np.zeros((n, 25, 3), np.float32)
    theta[:, 1:] = rng.standard_normal((n, 24, 3)) * 0.2
    theta[:, 0] = rng.uniform(-0.5, 0.5, (n, 3))
    for f in range(n):
        for j in (1 + (2 + f) % 24, 1 + (13 + 3 * f) % 24):
            ax = rng.standard_normal(3)
            ax /= np.linalg.norm(ax)
            theta[f, j] = (np.pi * ax).astype(np.float32)
    return beta, theta


RECOVERY_STEPS, RECOVERY_LR = 400, 0.1
RECOVERY_RESTATEMENT_RMS = 0.033506  # metres; see the test's docstring
RECOVERY_THRESHOLD = 2 * RECOVERY_RESTATEMENT_RMS


def test_rotmat_adam_recovers_poses_at_pi_from_the_identity(smpl):
    """n = 4 target meshes whose poses have two joints at exactly |theta| = pi; rotations in 6-D from the identity and the
    translation from zero (beta given), Adam(lr 0.1, cosine to 0.001) for 400 steps on the sum over frames of the mean squared vertex
    distance.  The same loop on the float64 restatement on a CPU (fk_rotmat_oracle.fk o rot6d_to_rotmat, targets from
    fk_vjp_oracle.fk) falls from a vertex RMS of 0.69 m to 0.033506 m (the float32 restatement: 0.033506 m too, so the figure is
    the optimiser's, not the arithmetic's); the threshold is twice that, 0.067012 m."""
    import torch
    from smplpp_amd.smpl import rot6d_to_rotmat

    beta, theta = _recovery_targets()
    assert (_at_pi(theta).sum(axis=1) == 2).all()
    target = torch.from_numpy(smpl.launch(beta, theta, want=("verts",))["verts"]).cuda()
    b = torch.from_numpy(beta).cuda()
    x = torch.tensor([1.0, 0, 0, 1, 0, 0]).repeat(4, 24, 1).cuda().requires_grad_(True)
    t = torch.zeros(4, 3).cuda().requires_grad_(True)
    opt = torch.optim.Adam([x, t], lr=RECOVERY_LR)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, RECOVERY_STEPS, eta_min=RECOVERY_LR / 100)
    for _ in range(RECOVERY_STEPS):
        opt.zero_grad()
        verts, _, _ = smpl.forward_rotmat_differentiable(b, t, rot6d_to_rotmat(x))
        ((verts - target) ** 2).sum(-1).mean(-1).sum().backward()
        opt.step()
        sched.step()
    with torch.no_grad():
        verts, _, _ = smpl.forward_rotmat_differentiable(b, t, rot6d_to_rotmat(x))
        rms = float(((verts - target) ** 2).sum(-1).mean().sqrt())
    print("recovery: vertex RMS %.6f m (restatement %.6f, threshold %.6f)" % (rms, RECOVERY_RESTATEMENT_RMS, RECOVERY_THRESHOLD))
    assert np.isfinite(rms) and rms < RECOVERY_THRESHOLD, rms


# ---------------------------------------------------------------------------------------------- 8. SMPL+D composition
def test_rotmat_composes_with_vertex_offsets(smpl, m64):
    n, V = 7, smpl.vertex_num
    beta, theta = _inputs(n, seed=77)
    R = _general(smpl, theta, seed=5)
    trans = np.ascontiguousarray(theta[:, 0])
    rng = np.random.default_rng(4)
    D = (0.01 * rng.standard_normal((n, V, 3))).astype(np.float32)
    gv, gj = _grads(V, n, seed=6, kind="both")
    o = smpl.launchRotmat(beta, trans, R)
    vd, rd = smpl.vertexOffsets(o["verts"], o["xforms"], D, rest=o["rest"])
    g = smpl.launchRotmatBackward(beta, trans, R, grad_verts=gv, grad_joints=gj, rest=rd)
    gD = smpl.vertexOffsetsBackward(o["xforms"], gv)
    mm32 = RO.cast(m64, O.torch.float32)
    t64 = lambda a: O.torch.as_tensor(a, dtype=O.torch.float64)
    with O.torch.no_grad():
        v64 = RO.fk(m64, t64(beta), t64(trans), t64(R), t64(D))["verts"].numpy()
        v32 = RO.fk(mm32, *(t64(a).float() for a in (beta, trans, R, D)))["verts"].numpy().astype(np.float64)
    r64 = RO.vjp(m64, beta, trans, R, gv, gj, offsets=D)
    r32 = RO.vjp(m64, beta, trans, R, gv, gj, dtype=O.torch.float32, offsets=D)
    for f in range(n):
        assert _rel(vd[f], v64[f]) <= _bar(v32[f], v64[f]), f
        for name, got, a, b in (("beta", g["beta"], r64[0], r32[0]), ("trans", g["trans"], r64[1], r32[1]),
                                ("rot", g["rot"], r64[2], r32[2]), ("offsets", gD, r64[3], r32[3])):
            err, bar = _rel(got[f], a[f]), _bar(b[f], a[f])
            print("smpl+d", name, f, "err %.3g bar %.3g" % (err, bar))
            assert err <= bar, (name, f, err, bar)


# ---------------------------------------------------------------------------------------------- 9. C++ shim
def test_rotmat_cpp_shim(tmp_path):
    import __graft_entry__ as g
    from smplpp_amd import model_io

    g.build()
    exe = str(tmp_path / "fk_rotmat_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fk_rotmat_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    n, V = 33, 40
    model = model_io.tiny_model(V, seed=3)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stdout
    vals = {}
    for line in out.stdout.splitlines():
        k, *v = line.split()
        vals[k] = np.array([float(x) for x in v], np.float32)
    # the program's inputs, restated
    ar = lambda count: np.arange(count, dtype=np.float32)
    beta = ((ar(n * 10) % 7 - 3) * np.float32(0.1)).reshape(n, 10)
    trans = ((ar(n * 3) % 9 - 4) * np.float32(0.25)).reshape(n, 3)
    aa = ((ar(n * 72) % 11 - 5) * np.float32(0.05)).reshape(n, 24, 3)
    gv = ((ar(n * V * 3) % 13 - 6) * np.float32(0.1)).reshape(n, V, 3)
    gj = ((ar(n * 72) % 5 - 2) * np.float32(0.1)).reshape(n, 24, 3)
    s = _smpl(model)
    rot = s.axisAngleToRotmat(aa)
    assert np.array_equal(vals["ROT"], rot.ravel())
    bent = rot + ((ar(n * 216) % 17 - 8) * np.float32(0.005)).reshape(n, 24, 3, 3)
    o = s.launchRotmat(beta, trans, bent)
    for key, k in (("VERTS", "verts"), ("JOINTS", "joints"), ("XFORMS", "xforms"), ("REST", "rest")):
        assert np.array_equal(vals[key], o[k].ravel()), key
    gr = s.launchRotmatBackward(beta, trans, bent, grad_verts=gv, grad_joints=gj, rest=o["rest"])
    assert np.array_equal(vals["GRAD_BETA"], gr["beta"].ravel())
    assert np.array_equal(vals["GRAD_TRANS"], gr["trans"].ravel())
    assert np.array_equal(vals["GRAD_ROT"], gr["rot"].ravel())
