"""smplpp_skeleton / smplpp_skeleton_rotmat and their vector-Jacobian products on the MI355X, on three trees (the synthetic SMPL
tree, and tiny_model as a 24-joint chain and as a star: the two shapes off pose_body's fast path):

 1. the bits shared with smplpp_fk / smplpp_fk_rotmat (world[..., :3] = the 3x3 block of xforms, joints), under the default form and
    SMPLPP_SKIN=h, and the derived bound that ties `posed` to the relative transforms' translation;
 2. the forward against the float64 restatement (tests/skeleton_oracle.py), general matrices, theta rows of 0 and of norm pi;
 3. the backward per block (tests/vjp_blocks.py: block_error held to stage_oracle.bar(e32)) against float64 autograd: each
    cotangent alone, all three, the 24 x 12 one-hot grad_world cotangents (the whole transposed Jacobian), and theta = 0 / |theta| =
    pi rows under the per-frame L2 bar of tests/test_fk_vjp_gpu.py, max(4 x fp32 autograd's error, 1e-5);
 4. the ties between the two backward entries;
 5. call semantics: subsets, accumulate, spaces, batch independence, determinism, NaN frames, refusals, and the handle's forward
    state left alone;
 6. the composition with Landmarks, project_points and a 2-D energy against float64 autograd of the oracle graph;
 7. two Adam fits beside the float64 oracle on the CPU;
 8. the C++ shim."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_rotmat_oracle as RO  # noqa: E402
import keypoints_oracle as KP  # noqa: E402
import skeleton_oracle as SO  # noqa: E402
import test_skeleton_cpu as CPU  # noqa: E402  (tree_model and the fits)
import vjp_blocks as VB  # noqa: E402

torch = SO.torch
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK_T = 4  # smplpp_amd/csrc/skeleton.hip: frames (wavefronts) per workgroup
NS = sorted({1, 5, 67, SK_T - 1, SK_T, SK_T + 1})
TREES = CPU.TREES
FORMS = ["default", "h"]
OUT = ("world", "posed", "joints")
COTS = {"world": (1, 0, 0), "posed": (0, 1, 0), "joints": (0, 0, 1), "all": (1, 1, 1)}
EPS = 2.0 ** -24


def _smpl(model, form="default"):
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


_cache = {}


def _cached(key, make):
    """One model, handle or reference per key for the whole module; never modified."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _model(tree):
    return _cached(("model", tree), lambda: CPU.tree_model(tree))


def _handle(tree, form="default"):
    return _cached(("handle", tree, form), lambda: _smpl(_model(tree), form))


def _m64(tree):
    return _cached(("m64", tree), lambda: SO.model_tensors(_model(tree)))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(d):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


def _special(n, seed):
    """tests/test_fk_rotmat_gpu.py::_inputs: a theta = 0 joint, a whole zero frame and |theta| = pi joints (_at_pi's construction)."""
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
    return np.abs(np.linalg.norm(theta[:, 1:].astype(np.float64), axis=-1) - np.pi) < 1e-5


def _generic(n, seed):
    """Generic angles N(0, 0.4^2) on every joint (no zero, none near pi), beta ~ N(0,1), a translation (vjp_blocks.generic_pose)."""
    rng = np.random.default_rng(seed)
    beta = rng.standard_normal((n, 10)).astype(np.float32)
    theta = (0.4 * rng.standard_normal((n, 25, 3))).astype(np.float32)
    theta[:, 0] = rng.uniform(-1, 1, (n, 3))
    return beta, theta


def _general(theta, seed):
    """Rodrigues + 0.05 N(0,1) per entry: not orthonormal."""
    R = RO.rodrigues_np(theta[:, 1:])
    return (R + 0.05 * np.random.default_rng(seed).standard_normal(R.shape)).astype(np.float32)


def _cotangents(n, seed, kind="all"):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal((n, 24, 3, 4)).astype(np.float32), rng.standard_normal((n, 24, 3)).astype(np.float32),
         rng.standard_normal((n, 24, 3)).astype(np.float32))
    return tuple(a if on else None for a, on in zip(g, COTS[kind]))


def _rel(a, b):
    return np.linalg.norm((np.asarray(a, np.float64) - b).ravel()) / max(np.linalg.norm(np.asarray(b).ravel()), 1e-30)


def _l2_bar(f32, f64):
    return max(4 * _rel(f32, f64), 1e-5)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------------------------------------- 1. bits shared with FK
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tree", TREES)
def test_bits_shared_with_fk(tree, form, n):
    s = _handle(tree, form)
    beta, theta = _special(n, seed=n)
    trans = np.ascontiguousarray(theta[:, 0])
    fk = s.launch(beta, theta, want=("joints", "xforms"))
    fk = {k: fk[k].copy() for k in ("joints", "xforms")}
    sk = s.skeleton(beta, theta)
    assert sk["world"].shape == (n, 24, 3, 4) and sk["posed"].shape == (n, 24, 3) and sk["joints"].shape == (n, 24, 3)
    assert all(np.isfinite(sk[k]).all() for k in OUT)
    assert np.array_equal(sk["world"][..., :3], fk["xforms"][:, :, :3, :3])
    assert np.array_equal(sk["joints"], fk["joints"])
    assert np.array_equal(sk["world"][..., 3], sk["posed"])
    rot = s.axisAngleToRotmat(theta[:, 1:])
    fkr = s.launchRotmat(beta, trans, rot, want=("joints", "xforms"))
    skr = s.skeletonRotmat(beta, trans, rot)
    assert np.array_equal(skr["world"][..., :3], fkr["xforms"][:, :, :3, :3])
    assert np.array_equal(skr["joints"], fkr["joints"])
    for k in OUT:
        assert _same(sk[k], skr[k]), k
    # trans = 0: posed - A.J is the relative transform's translation up to relative_t's four roundings (the factor 8: a 2x margin)
    th0 = theta.copy()
    th0[:, 0] = 0.0
    z = s.skeleton(beta, th0)
    A, J, posed = (z["world"][..., :3].astype(np.float64), z["joints"].astype(np.float64), z["posed"].astype(np.float64))
    AJ = np.einsum("njac,njc->nja", A, J)
    mag = np.abs(posed) + np.einsum("njac,njc->nja", np.abs(A), np.abs(J))
    d = np.abs((posed - AJ) - fk["xforms"][:, :, :3, 3].astype(np.float64))
    print("relative translation: max d / (eps mag) = %.3g" % float((d / (EPS * mag)).max()))
    assert (d <= 8 * EPS * mag).all()


# ---------------------------------------------------------------------------------------------- 2. forward against float64
def _forward_ref(tree, n):
    def make():
        beta, theta = _special(n, seed=20 + n)
        R = _general(theta, seed=n)
        trans = np.ascontiguousarray(theta[:, 0])
        m = _m64(tree)
        return (beta, theta, trans, R, SO.forward(m, beta, theta), SO.forward(m, beta, theta, dtype=torch.float32),
                SO.forward_rotmat(m, beta, trans, R), SO.forward_rotmat(m, beta, trans, R, dtype=torch.float32))

    return _cached(("forward", tree, n), make)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("tree", TREES)
def test_forward_against_float64(tree, n):
    s = _handle(tree)
    beta, theta, trans, R, a64, a32, r64, r32 = _forward_ref(tree, n)
    assert (theta[0, 3] == 0).all() and _at_pi(theta).any()
    RtR = np.einsum("njab,njac->njbc", R.astype(np.float64), R.astype(np.float64))
    assert np.abs(RtR - np.eye(3)).max() > 0.05  # not orthonormal
    for tag, out, f64, f32 in (("axis-angle", s.skeleton(beta, theta), a64, a32), ("general rot", s.skeletonRotmat(beta, trans, R), r64, r32)):
        for k in OUT:
            assert np.isfinite(out[k]).all(), (tag, k)
        for k, ko in (("posed", "posed"), ("world", "world"), ("joints", "J")):
            for f in range(n):
                err, bar = _rel(out[k][f], f64[ko][f]), _l2_bar(f32[ko][f], f64[ko][f])
                assert err <= bar, (tag, k, f, err, bar)
    # beta = NULL and trans = NULL are explicit zeros, to the bit
    a, b = s.skeletonRotmat(None, None, R), s.skeletonRotmat(np.zeros_like(beta), np.zeros_like(trans), R)
    c, d = s.skeleton(None, theta), s.skeleton(np.zeros_like(beta), theta)
    for k in OUT:
        assert _same(a[k], b[k]) and _same(c[k], d[k]), k


# ---------------------------------------------------------------------------------------------- 3. backward per block
def _check_blocks(tag, got, r64, r32, axes):
    axes = VB.axes_of(axes, r64)
    assert np.isfinite(got).all(), tag
    e, e32 = VB.block_error(got, r64, axes), VB.block_error(r32, r64, axes)
    print("%s: E %.3g, fp32 autograd %.3g, bar %.3g" % (tag, e, e32, VB.bar(e32)))
    assert e <= VB.bar(e32), (tag, e, e32)


def _backward_ref(tree, n, kind):
    def make():
        beta, theta = _generic(n, seed=50 + n)
        R = _general(theta, seed=3 + n)
        trans = np.ascontiguousarray(theta[:, 0])
        cots = _cotangents(n, 7 * n + 1, kind)
        m = _m64(tree)
        return (beta, theta, trans, R, cots, SO.vjp(m, beta, theta, *cots), SO.vjp(m, beta, theta, *cots, dtype=torch.float32),
                SO.vjp_rotmat(m, beta, trans, R, *cots), SO.vjp_rotmat(m, beta, trans, R, *cots, dtype=torch.float32))

    return _cached(("backward", tree, n, kind), make)


@pytest.mark.parametrize("kind", list(COTS))
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("tree", TREES)
def test_backward_blocks_against_float64(tree, n, kind):
    s = _handle(tree)
    beta, theta, trans, R, (gw, gp, gj), a64, a32, r64, r32 = _backward_ref(tree, n, kind)
    g = s.skeletonBackward(beta, theta, gw, gp, gj)
    assert g["beta"].shape == (n, 10) and g["theta"].shape == (n, 25, 3)
    for (name, axes), x64, x32 in zip(VB.FK_OUTPUTS, a64, a32):
        _check_blocks("%s n=%d %s grad_%s" % (tree, n, kind, name), g[name], x64, x32, axes)
    _check_blocks("%s n=%d %s grad_trans (theta row 0)" % (tree, n, kind), g["theta"][:, 0], a64[1][:, 0], a32[1][:, 0], None)
    h = s.skeletonRotmatBackward(beta, trans, R, gw, gp, gj)
    assert h["trans"].shape == (n, 3) and h["rot"].shape == (n, 24, 3, 3)
    for (name, axes), x64, x32 in zip(VB.ROTMAT_OUTPUTS, r64, r32):
        _check_blocks("%s n=%d %s rotmat grad_%s" % (tree, n, kind, name), h[name], x64, x32, axes)


@pytest.mark.parametrize("tree", TREES)
def test_backward_one_hot_world_cotangents(tree):
    """Frame k's grad_world is one-hot at entry k of the [24,3,4] output, at one generic pose: the 288 rows of the transposed Jacobian."""
    s = _handle(tree)
    K = 24 * 12
    beta, theta = VB.generic_pose()
    beta, theta = np.repeat(beta, K, 0), np.repeat(theta, K, 0)
    gw = np.eye(K, dtype=np.float32).reshape(K, 24, 3, 4)
    m = _m64(tree)
    a64, a32 = SO.vjp(m, beta, theta, gw), SO.vjp(m, beta, theta, gw, dtype=torch.float32)
    g = s.skeletonBackward(beta, theta, grad_world=gw)
    for (name, axes), x64, x32 in zip(VB.FK_OUTPUTS, a64, a32):
        _check_blocks("%s one-hot grad_%s" % (tree, name), g[name], x64, x32, axes)
    R = _general(theta[:1], seed=9).repeat(K, 0)
    trans = np.ascontiguousarray(theta[:, 0])
    r64, r32 = SO.vjp_rotmat(m, beta, trans, R, gw), SO.vjp_rotmat(m, beta, trans, R, gw, dtype=torch.float32)
    h = s.skeletonRotmatBackward(beta, trans, R, grad_world=gw)
    for (name, axes), x64, x32 in zip(VB.ROTMAT_OUTPUTS, r64, r32):
        _check_blocks("%s one-hot rotmat grad_%s" % (tree, name), h[name], x64, x32, axes)


@pytest.mark.parametrize("tree", TREES)
def test_backward_at_zero_and_pi_rows(tree):
    """theta rows of exactly 0 and of norm pi: finite, and per frame within the bar tests/test_fk_vjp_gpu.py holds those points to,
    relative L2 at most max(4 x fp32 autograd's, 1e-5).  (grad_rot has no singularity there: the block bar.)"""
    s, n = _handle(tree), 5
    beta, theta = _special(n, seed=31)
    assert (theta[0, 3] == 0).all() and not theta[2, 1:].any() and _at_pi(theta).sum() >= 3
    gw, gp, gj = _cotangents(n, 32)
    m = _m64(tree)
    a64, a32 = SO.vjp(m, beta, theta, gw, gp, gj), SO.vjp(m, beta, theta, gw, gp, gj, dtype=torch.float32)
    g = s.skeletonBackward(beta, theta, gw, gp, gj)
    for name, x64, x32 in zip(("beta", "theta"), a64, a32):
        assert np.isfinite(g[name]).all(), name
        for f in range(n):
            err, bar = _rel(g[name][f], x64[f]), _l2_bar(x32[f], x64[f])
            print("zero/pi", tree, name, f, "err %.3g bar %.3g" % (err, bar))
            assert err <= bar, (name, f, err, bar)
    rot = s.axisAngleToRotmat(theta[:, 1:])
    trans = np.ascontiguousarray(theta[:, 0])
    r64, r32 = SO.vjp_rotmat(m, beta, trans, rot, gw, gp, gj), SO.vjp_rotmat(m, beta, trans, rot, gw, gp, gj, dtype=torch.float32)
    h = s.skeletonRotmatBackward(beta, trans, rot, gw, gp, gj)
    for (name, axes), x64, x32 in zip(VB.ROTMAT_OUTPUTS, r64, r32):
        _check_blocks("%s zero/pi rotmat grad_%s" % (tree, name), h[name], x64, x32, axes)


# ---------------------------------------------------------------------------------------------- 4. ties
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("tree", TREES)
def test_ties_between_the_two_backward_entries(tree, n):
    s = _handle(tree)
    beta, theta, trans, _, (gw, gp, gj), a64, a32, _, _ = _backward_ref(tree, n, "all")
    rot = s.axisAngleToRotmat(theta[:, 1:])
    g = s.skeletonBackward(beta, theta, gw, gp, gj)
    h = s.skeletonRotmatBackward(beta, trans, rot, gw, gp, gj)
    assert _same(g["beta"], h["beta"])
    assert _same(h["trans"], np.ascontiguousarray(g["theta"][:, 0]))
    back = RO.contract_rodrigues(theta[:, 1:], h["rot"])
    e = VB.block_error(back, g["theta"][:, 1:].astype(np.float64), VB.THETA)
    e32 = VB.block_error(a32[1], a64[1], VB.THETA)
    print("tie %s n=%d: E %.3g, fp32 autograd %.3g" % (tree, n, e, e32))
    assert e <= VB.bar(e32), (e, e32)


# ---------------------------------------------------------------------------------------------- 5. call semantics
def _subsets(keys):
    return [c for r in range(1, len(keys) + 1) for c in itertools.combinations(keys, r)]


@pytest.mark.parametrize("tree", TREES)
def test_subsets_spaces_and_batch_independence(tree):
    s, n = _handle(tree), 67
    beta, theta, trans, R, (gw, gp, gj), _, _, _, _ = _backward_ref(tree, n, "all")
    full = s.skeleton(beta, theta)
    fullr = s.skeletonRotmat(beta, trans, R)
    gfull = s.skeletonBackward(beta, theta, gw, gp, gj)
    gfullr = s.skeletonRotmatBackward(beta, trans, R, gw, gp, gj)
    # every subset of outputs
    for want in _subsets(OUT):
        a, b = s.skeleton(beta, theta, want=want), s.skeletonRotmat(beta, trans, R, want=want)
        assert set(a) == set(want) and set(b) == set(want)
        for k in want:
            assert _same(a[k], full[k]) and _same(b[k], fullr[k]), (want, k)
    for want in _subsets(("beta", "theta")):
        a = s.skeletonBackward(beta, theta, gw, gp, gj, want=want)
        assert set(a) == set(want) and all(_same(a[k], gfull[k]) for k in want), want
    for want in _subsets(("beta", "trans", "rot")):
        a = s.skeletonRotmatBackward(beta, trans, R, gw, gp, gj, want=want)
        assert set(a) == set(want) and all(_same(a[k], gfullr[k]) for k in want), want
    # every subset of cotangents: NULL reads as +0
    zeros = tuple(np.zeros_like(a) for a in (gw, gp, gj))
    for on in itertools.product((0, 1), repeat=3):
        if not any(on):
            continue
        sub = tuple(a if o else None for a, o in zip((gw, gp, gj), on))
        dense = tuple(a if o else z for a, z, o in zip((gw, gp, gj), zeros, on))
        a, b = s.skeletonBackward(beta, theta, *sub), s.skeletonBackward(beta, theta, *dense)
        c, d = s.skeletonRotmatBackward(beta, trans, R, *sub), s.skeletonRotmatBackward(beta, trans, R, *dense)
        assert all(_same(a[k], b[k]) for k in a) and all(_same(c[k], d[k]) for k in c), on
    # twice; device space
    again, gagain = s.skeleton(beta, theta), s.skeletonBackward(beta, theta, gw, gp, gj)
    d = _host(s.skeleton(_dev(beta), _dev(theta)))
    dr = _host(s.skeletonRotmat(_dev(beta), _dev(trans), _dev(R)))
    gd = _host(s.skeletonBackward(_dev(beta), _dev(theta), _dev(gw), _dev(gp), _dev(gj)))
    gdr = _host(s.skeletonRotmatBackward(_dev(beta), _dev(trans), _dev(R), _dev(gw), _dev(gp), _dev(gj)))
    for k in OUT:
        assert _same(again[k], full[k]) and _same(d[k], full[k]) and _same(dr[k], fullr[k]), k
    assert all(_same(gagain[k], gfull[k]) and _same(gd[k], gfull[k]) for k in gfull)
    assert all(_same(gdr[k], gfullr[k]) for k in gfullr)
    # a frame alone has the bits it has inside n = 67
    for f in (0, 1, SK_T - 1, SK_T, 33, 66):
        sl = slice(f, f + 1)
        one, oner = s.skeleton(beta[sl], theta[sl]), s.skeletonRotmat(beta[sl], trans[sl], R[sl])
        g1 = s.skeletonBackward(beta[sl], theta[sl], gw[sl], gp[sl], gj[sl])
        g1r = s.skeletonRotmatBackward(beta[sl], trans[sl], R[sl], gw[sl], gp[sl], gj[sl])
        for k in OUT:
            assert _same(one[k][0], full[k][f]) and _same(oner[k][0], fullr[k][f]), (f, k)
        assert all(_same(g1[k][0], gfull[k][f]) for k in gfull) and all(_same(g1r[k][0], gfullr[k][f]) for k in gfullr), f
    # a frame of NaNs in the middle of a workgroup leaves the others alone
    bad = 2 * SK_T + 1
    keep = np.arange(n) != bad
    bn, tn, Rn = beta.copy(), theta.copy(), R.copy()
    bn[bad], tn[bad], Rn[bad] = np.nan, np.nan, np.nan
    gwn, gpn, gjn = gw.copy(), gp.copy(), gj.copy()
    gwn[bad], gpn[bad], gjn[bad] = np.nan, np.nan, np.nan
    a, b = s.skeleton(bn, tn), s.skeletonRotmat(bn, trans, Rn)
    c, d = s.skeletonBackward(bn, tn, gwn, gpn, gjn), s.skeletonRotmatBackward(bn, trans, Rn, gwn, gpn, gjn)
    for k in OUT:
        assert np.isnan(a[k][bad]).all() and _same(a[k][keep], full[k][keep]) and _same(b[k][keep], fullr[k][keep]), k
    assert all(_same(c[k][keep], gfull[k][keep]) for k in c) and all(_same(d[k][keep], gfullr[k][keep]) for k in d)
    assert np.isnan(c["theta"][bad]).all() and np.isnan(d["rot"][bad]).all()


@pytest.mark.parametrize("tree", TREES)
def test_accumulate_is_one_fp32_add(tree):
    s, n = _handle(tree), SK_T + 1
    beta, theta, trans, R, (gw, gp, gj), _, _, _, _ = _backward_ref(tree, n, "all")
    rng = np.random.default_rng(8)
    val, valr = s.skeletonBackward(beta, theta, gw, gp, gj), s.skeletonRotmatBackward(beta, trans, R, gw, gp, gj)
    for space in ("host", "device"):
        to = _dev if space == "device" else (lambda a: a)
        pre = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in val.items()}
        out = {k: to(v.copy()) for k, v in pre.items()}
        res = s.skeletonBackward(to(beta), to(theta), to(gw), to(gp), to(gj), out=out)
        assert all(res[k] is out[k] or res[k].data_ptr() == out[k].data_ptr() for k in out)
        got = _host(out)
        assert all(_same(got[k], pre[k] + val[k]) for k in pre), space
        prer = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in valr.items()}
        outr = {k: to(v.copy()) for k, v in prer.items()}
        s.skeletonRotmatBackward(to(beta), to(trans), to(R), to(gw), to(gp), to(gj), out=outr)
        got = _host(outr)
        assert all(_same(got[k], prer[k] + valr[k]) for k in prer), space
        # a subset accumulates into what it is given only
        only = {"theta": to(pre["theta"].copy())}
        s.skeletonBackward(to(beta), to(theta), to(gw), None, None, out=only)
        assert _same(_host(only)["theta"], pre["theta"] + s.skeletonBackward(beta, theta, gw, want=("theta",))["theta"])
    # after launchBackward into the same buffers: the gradient of a loss on vertices and skeleton
    gv = rng.standard_normal((n, s.vertex_num, 3)).astype(np.float32)
    base = s.launchBackward(beta, theta, grad_verts=gv)
    both = {k: v.copy() for k, v in base.items()}
    s.skeletonBackward(beta, theta, gw, gp, gj, out=both)
    assert all(_same(both[k], base[k] + val[k]) for k in both)


def test_refusals_leave_the_outputs_untouched():
    from smplpp_amd import _lib

    L, s, n = _lib.load(), _handle("smpl"), 3
    beta, theta = _generic(n, seed=1)
    R = _general(theta, seed=2)
    trans = np.ascontiguousarray(theta[:, 0])
    gw, gp, gj = _cotangents(n, 3)
    p = lambda a: None if a is None else a.ctypes.data
    w, po, jo = (np.full((n, 24, 3, 4), 7, np.float32), np.full((n, 24, 3), 7, np.float32), np.full((n, 24, 3), 7, np.float32))
    gb, gt, gtr, gr = (np.full((n, 10), 7, np.float32), np.full((n, 25, 3), 7, np.float32), np.full((n, 3), 7, np.float32),
                       np.full((n, 24, 3, 3), 7, np.float32))
    H, INV = _lib.HOST, 1

    def refused(rc):
        assert rc == INV and L.smplpp_last_error()
        assert all((a == 7).all() for a in (w, po, jo, gb, gt, gtr, gr))

    h = s.handle
    for bad_n in (0, -1):
        refused(L.smplpp_skeleton(h, bad_n, p(beta), p(theta), p(w), p(po), p(jo), H, None))
        refused(L.smplpp_skeleton_rotmat(h, bad_n, p(beta), p(trans), p(R), p(w), p(po), p(jo), H, None))
        refused(L.smplpp_skeleton_vjp(h, bad_n, p(beta), p(theta), p(gw), p(gp), p(gj), p(gb), p(gt), 0, H, None))
        refused(L.smplpp_skeleton_rotmat_vjp(h, bad_n, p(beta), p(trans), p(R), p(gw), p(gp), p(gj), p(gb), p(gtr), p(gr), 0, H, None))
    refused(L.smplpp_skeleton(h, n, p(beta), None, p(w), p(po), p(jo), H, None))
    refused(L.smplpp_skeleton_rotmat(h, n, p(beta), p(trans), None, p(w), p(po), p(jo), H, None))
    refused(L.smplpp_skeleton_vjp(h, n, p(beta), None, p(gw), p(gp), p(gj), p(gb), p(gt), 0, H, None))
    refused(L.smplpp_skeleton_rotmat_vjp(h, n, p(beta), p(trans), None, p(gw), p(gp), p(gj), p(gb), p(gtr), p(gr), 0, H, None))
    refused(L.smplpp_skeleton(h, n, p(beta), p(theta), None, None, None, H, None))  # no output
    refused(L.smplpp_skeleton_rotmat(h, n, p(beta), p(trans), p(R), None, None, None, H, None))
    refused(L.smplpp_skeleton_vjp(h, n, p(beta), p(theta), None, None, None, p(gb), p(gt), 0, H, None))  # no cotangent
    refused(L.smplpp_skeleton_rotmat_vjp(h, n, p(beta), p(trans), p(R), None, None, None, p(gb), p(gtr), p(gr), 0, H, None))
    refused(L.smplpp_skeleton_vjp(h, n, p(beta), p(theta), p(gw), p(gp), p(gj), None, None, 0, H, None))  # no gradient asked for
    refused(L.smplpp_skeleton_rotmat_vjp(h, n, p(beta), p(trans), p(R), p(gw), p(gp), p(gj), None, None, None, 0, H, None))
    for acc in (2, -1):
        refused(L.smplpp_skeleton_vjp(h, n, p(beta), p(theta), p(gw), p(gp), p(gj), p(gb), p(gt), acc, H, None))
        refused(L.smplpp_skeleton_rotmat_vjp(h, n, p(beta), p(trans), p(R), p(gw), p(gp), p(gj), p(gb), p(gtr), p(gr), acc, H, None))
    refused(L.smplpp_skeleton(h, n, p(beta), p(theta), p(w), p(po), p(jo), 5, None))  # bad memory space
    refused(L.smplpp_skeleton_vjp(h, n, p(beta), p(theta), p(gw), p(gp), p(gj), p(gb), p(gt), 0, 5, None))
    refused(L.smplpp_skeleton(None, n, p(beta), p(theta), p(w), p(po), p(jo), H, None))
    # the binding words its own refusals
    with pytest.raises(_lib.SmplppError):
        s.skeleton(beta, theta, want=())
    with pytest.raises(_lib.SmplppError):
        s.skeletonBackward(beta, theta)
    with pytest.raises(_lib.SmplppError):
        s.skeletonBackward(beta, theta, gw, want=())
    with pytest.raises(_lib.SmplppError):
        s.skeletonRotmat(beta, trans, R[:, :23])
    with pytest.raises(_lib.SmplppError):
        s.skeleton(_dev(beta), theta)


@pytest.mark.parametrize("form", FORMS)
def test_skeleton_calls_leave_the_forward_state_alone(form):
    """smplpp_fk's outputs, status word and profiling record, taken before skeleton calls (both spaces, both directions, another n),
    are what they were after them (tests/test_fk_rotmat_gpu.py::test_rotmat_backward_leaves_the_forward_workspace_alone)."""
    s, n = _smpl(_model("smpl"), form), 67
    beta, theta, trans, R, (gw, gp, gj), _, _, _, _ = _backward_ref("smpl", n, "all")
    keys = ("verts", "joints", "xforms", "rest")
    s.profileEnable(True)
    s.profileRead()
    db, dt = _dev(beta), _dev(theta)
    held = s.launch(db, dt)  # device space: the outputs live in the caller's tensors, the operands in the handle's workspace
    torch.cuda.synchronize()
    ref = {k: held[k].cpu().numpy() for k in keys}
    m = 40
    s.skeleton(db[:m], dt[:m])
    s.skeletonBackward(db[:m], dt[:m], _dev(gw[:m]), _dev(gp[:m]), _dev(gj[:m]))
    s.skeletonRotmat(db[:m], _dev(trans[:m]), _dev(R[:m]))
    s.skeletonRotmatBackward(db[:m], _dev(trans[:m]), _dev(R[:m]), _dev(gw[:m]), _dev(gp[:m]), _dev(gj[:m]))
    s.skeleton(beta[:m], theta[:m])
    s.skeletonBackward(beta[:m], theta[:m], gw[:m], gp[:m], gj[:m])
    torch.cuda.synchronize()
    for k in keys:
        assert np.array_equal(held[k].cpu().numpy(), ref[k]), k
    launches, _ = s.profileRead()
    assert launches == 1  # the record holds the one launch, no more
    assert s.launchStatus() == 0
    # the fused kernel alone, from the operands the pose step left in the workspace, is not reachable from outside; a new launch is,
    # and gives the same bits
    again = s.launch(beta, theta)
    for k in keys:
        assert np.array_equal(again[k], ref[k]), k
    s.profileEnable(False)


# ---------------------------------------------------------------------------------------------- 6. composition
def _bar(got, want64, fp32, what):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    err, ref = _rel(got, want64), _rel(fp32, want64)
    print("%s: rel %.3g, fp32 autograd %.3g" % (what, err, ref))
    assert np.abs(want64).max() > 0 and err <= max(4 * ref, 1e-5), (what, err, ref)


def _camera_rows(n, rng, distance=4.0):
    """tests/test_keypoints_gpu.py::_camera_rows: n cameras `distance` in front of the origin, y down, each turned a little."""
    cam = np.empty((n, 16), np.float32)
    for f in range(n):
        a = rng.normal(0, 0.2)
        c, s = np.cos(a), np.sin(a)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([1.0, -1.0, -1.0])
        cam[f] = np.concatenate([R.reshape(9), [0.02 * f, -0.03, distance], [500.0, 490.0, 320.0, 240.0]])
    return cam


@pytest.mark.parametrize("rho", [0.0, 100.0])
def test_composes_with_landmarks_and_projection(rho):
    """theta, beta -> (smplpp_fk verts, smplpp_skeleton world and posed) -> landmarks over [verts; posed] -> projection -> energy, plus
    the projected bone tips posed_j + 0.1 A_j e_x from `world`: the gradient to theta, beta and the 16 camera entries against float64
    autograd of the oracle graph, within max(4 x fp32 autograd's error, 1e-5) (tests/test_keypoints_gpu.py's bar for its chain)."""
    from smplpp_amd import model_io
    from smplpp_amd import smpl as S
    from smplpp_amd.landmarks import Landmarks

    V, n, near = 97, 3, 0.05
    model = _cached(("model", "tiny97"), lambda: model_io.tiny_model(V))
    s = _cached(("handle", "tiny97"), lambda: _smpl(model))
    row_ptr, col, val = KP.regressor_11(V)
    norm = np.maximum(np.add.reduceat(np.abs(np.append(val, 0)), row_ptr[:-1]) * (np.diff(row_ptr) > 0), 1e-30)
    reg = (row_ptr, col, (val / np.repeat(norm, np.diff(row_ptr))).astype(np.float32))
    lm = Landmarks(s, *reg)
    rng = np.random.default_rng(81)
    beta, theta = model_io.synthetic_inputs(n, seed=82)
    cam = _camera_rows(n, rng)

    def graph(verts, world, posed, landmarks, project, energy, T):
        pts = torch.cat([landmarks(verts, posed), world[..., 3] + 0.1 * world[..., 0]], 1)
        return energy(*project(pts), T)

    m64 = SO.model_tensors(model)

    def ref(dtype, T):
        m = SO.cast(m64, dtype)
        bb, th, cc = (torch.tensor(x, dtype=dtype, requires_grad=True) for x in (beta, theta, cam))
        verts = SO.O.fk(m, bb, th)["verts"]
        sk = SO.skeleton(m, bb, th)
        A = torch.tensor(KP.dense(reg, V + 24), dtype=dtype)
        uv = []

        def project(pts):
            uvr, vr = KP.project_t(pts, cc, near)
            uv.append(uvr.detach().numpy())
            return uvr, vr

        er = graph(verts, sk["world"], sk["posed"], lambda v, j: KP.landmarks_t(A, v, j), project,
                   lambda uvr, vr, T: KP.energy_t(uvr, vr, torch.tensor(T, dtype=dtype), rho), T if T is not None else np.ones((n, 35, 3)))
        if T is None:  # (the projections alone, to place the targets)
            return uv[0]
        er.sum().backward()
        return [x.detach().double().numpy() for x in (er, bb.grad, th.grad, cc.grad)]

    uv0 = ref(torch.float64, None)
    T = np.concatenate([uv0 + rng.normal(0, 20.0, uv0.shape), rng.uniform(0.2, 1.0, uv0.shape[:2] + (1,))], -1).astype(np.float32)
    T[:, 4, 2] = 0.0
    b, t, c = (torch.from_numpy(x).cuda().requires_grad_(True) for x in (beta, theta, cam))
    verts, _ = s.forward_differentiable(b, t)
    world, posed, _ = s.skeleton_differentiable(b, t)
    Td = _dev(T)
    valid = []

    def project(pts):
        uv, e, ok = S.project_points_differentiable(pts, c, Td, rho, near)
        valid.append(ok)
        return (e,)

    e = graph(verts, world, posed, lm.forward_differentiable, project, lambda e, T: e, T)
    assert bool(valid[0].all())
    e.sum().backward()
    r64, r32 = ref(torch.float64, T), ref(torch.float32, T)
    assert _rel(e.detach().cpu().numpy(), r64[0]) < 1e-4
    _bar(b.grad, r64[1], r32[1], "composition beta")
    _bar(t.grad, r64[2], r32[2], "composition theta")
    for name, sl in (("R", slice(0, 9)), ("t", slice(9, 12)), ("f", slice(12, 14)), ("c", slice(14, 16))):
        _bar(c.grad[:, sl], r64[3][:, sl], r32[3][:, sl], "composition camera " + name)


# ---------------------------------------------------------------------------------------------- 7. two fits
@pytest.mark.parametrize("kind", ["posed", "imu"])
def test_fit_beside_float64(kind):
    """n = 4, default_rng(5), theta* ~ N(0, 0.3^2) on all 25 rows, beta = 0, from theta = 0, Adam(lr 0.05), 200 steps, gradients from
    skeleton_differentiable; the float64 oracle runs the same schedule on the CPU.  (a) sum |posed - posed*|^2 (float64: 46.59 ->
    0.012, a factor of 3.8e3) must fall by >= 1e3 and end within 2x of the float64 run; (b) the IMU-style loss on the orientations of
    joints 0, 7, 8, 15, 20, 21 and the root position (float64: 62.36 -> 2e-8) must end below 1e-6 or within 2x of float64."""
    s = _handle("smpl")
    beta = torch.zeros(CPU.FIT_N, 10, device="cuda")

    def forward(theta):
        world, posed, _ = s.skeleton_differentiable(beta, theta)
        return world, posed

    first, last = CPU.run_fit(kind, forward, torch.float32, device="cuda")
    first64, last64 = CPU.run_fit(kind, CPU.oracle_forward(_m64("smpl"), torch.float64), torch.float64)
    print("fit %s: device %.4g -> %.4g, float64 %.4g -> %.4g" % (kind, first, last, first64, last64))
    assert np.isfinite(last) and CPU.fit_passes(kind, first, last, last64), (first, last, last64)


# ---------------------------------------------------------------------------------------------- 8. C++ shim
def test_skeleton_cpp_shim(tmp_path):
    import __graft_entry__ as g
    from smplpp_amd import model_io

    g.build()
    exe = str(tmp_path / "skeleton_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "skeleton_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    n, V = 5, 40
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
    theta = ((ar(n * 75) % 11 - 5) * np.float32(0.05)).reshape(n, 25, 3)
    gw = ((ar(n * 288) % 13 - 6) * np.float32(0.1)).reshape(n, 24, 3, 4)
    gp = ((ar(n * 72) % 9 - 4) * np.float32(0.25)).reshape(n, 24, 3)
    gj = ((ar(n * 72) % 5 - 2) * np.float32(0.1)).reshape(n, 24, 3)
    s = _smpl(model)
    o = s.skeleton(beta, theta)
    for key, k in (("WORLD", "world"), ("POSED", "posed"), ("JOINTS", "joints")):
        assert np.array_equal(vals[key], o[k].ravel()), key
    gr = s.skeletonBackward(beta, theta, gw, gp, gj)
    assert np.array_equal(vals["GRAD_BETA"], gr["beta"].ravel()) and np.array_equal(vals["GRAD_THETA"], gr["theta"].ravel())
    trans = np.ascontiguousarray(theta[:, 0])
    bent = s.axisAngleToRotmat(theta[:, 1:]) + ((ar(n * 216) % 17 - 8) * np.float32(0.005)).reshape(n, 24, 3, 3)
    o = s.skeletonRotmat(beta, trans, bent)
    for key, k in (("R_WORLD", "world"), ("R_POSED", "posed"), ("R_JOINTS", "joints")):
        assert np.array_equal(vals[key], o[k].ravel()), key
    gr = s.skeletonRotmatBackward(beta, trans, bent, gw, None, gj)
    for key, k in (("R_GRAD_BETA", "beta"), ("R_GRAD_TRANS", "trans"), ("R_GRAD_ROT", "rot")):
        assert np.array_equal(vals[key], gr[k].ravel()), key
