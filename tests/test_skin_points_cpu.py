"""The bound points without a GPU: the numpy restatement of smplpp_skin_points / smplpp_unskin_points and their vector-Jacobian products
(tests/skin_points_oracle.py) against itself: float32 beside the float64 definition by matrices, the closed-form gradients in float64
beside autograd, the translation identity, a face binding beside the dense weights it stands for, and the round trip; the conditions on
the inputs that the GPU tests rely on (no dead point at the test poses, a constructed collapse that is dead); and the entry points
(declared, exported, bound, refusing a call without a model)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import skeleton_oracle as SO  # noqa: E402
import skin_points_oracle as SP  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402

NAMES = (("smplpp_skin_points", 16), ("smplpp_unskin_points", 16), ("smplpp_skin_points_vjp", 19), ("smplpp_unskin_points_vjp", 19))
f32, f64 = np.float32, np.float64
BAR = 1e-5  # the project's fp32 bar: max(4 x the error of a float32 evaluation of the definition, 1e-5), relative 2-norm


def poses(n, seed):
    """beta ~ N(0, 1), theta ~ N(0, 0.3^2) rad, the root translation ~ U(-1, 1) m."""
    rng = np.random.default_rng(seed)
    theta = (rng.standard_normal((n, 25, 3)) * 0.3).astype(f32)
    theta[:, 0] = rng.uniform(-1.0, 1.0, (n, 3))
    return rng.standard_normal((n, 10)).astype(f32), theta


def skeleton_of(model, beta, theta):
    """(world [n,24,3,4], joints [n,24,3]) of the float64 skeleton, rounded to float32 as smplpp_skeleton hands them over."""
    out = SO.forward(FK.model_tensors(model), beta, theta)
    return out["world"].astype(f32), out["J"].astype(f32)


def bound_cloud(model, K, seed, frames=1, off=0.02):
    """K points per frame bound to the model's faces: (points [frames,K,3] near the template's surface, face [frames,K],
    bary [frames,K,3])."""
    rng = np.random.default_rng(seed)
    faces = np.asarray(model["face_indices"], np.int64) - 1
    vt = np.asarray(model["vertices_template"], f64)
    face = rng.integers(0, len(faces), (frames, K))
    bary = rng.dirichlet(np.ones(3), (frames, K))
    x = np.einsum("fkc,fkcx->fkx", bary, vt[faces[face]]) + rng.normal(0, off, (frames, K, 3))
    return x.astype(f32), face, bary.astype(f32)


def free_weights(K, seed, frames=1):
    """Dense weights [frames,K,24] that do not sum to 1: about five joints per point (at least one), scaled by 0.5 to 2."""
    rng = np.random.default_rng(seed)
    w = rng.dirichlet(np.ones(24), (frames, K)) * (rng.random((frames, K, 24)) < 0.2)
    first = rng.integers(0, 24, (frames, K))
    np.put_along_axis(w, first[..., None], rng.uniform(0.05, 0.5, (frames, K, 1)), -1)
    w *= rng.uniform(0.5, 2.0, (frames, K, 1)) / w.sum(-1, keepdims=True)
    return w.astype(f32)


@pytest.fixture(scope="module")
def tiny():
    from smplpp_amd import model_io

    return model_io.tiny_model(61, seed=7)


@pytest.fixture(scope="module", params=["synth", "tiny"])
def case(request, synth_model, tiny):
    model = synth_model if request.param == "synth" else tiny
    n, K = 3, 150
    beta, theta = poses(n, seed=5)
    world, joints = skeleton_of(model, beta, theta)
    x, face, bary = bound_cloud(model, K, seed=6)
    faces = np.asarray(model["face_indices"], np.int64) - 1
    W = np.asarray(model["weights"], f32)
    rng = np.random.default_rng(7)
    return dict(model=model, W=W, faces=faces, world=world, joints=joints, x=x, face=face, bary=bary, weights=free_weights(K, seed=8),
                g=rng.standard_normal((n, K, 3)).astype(f32), n=n, K=K)


def _bindings(c, dtype=f32):
    """name -> (omega, ok): the face binding and the free dense weights."""
    return {"face": SP.omega_of(c["W"], c["faces"], c["face"], c["bary"], dtype=dtype), "weights": SP.omega_of(None, None, weights=c["weights"], dtype=dtype)}


def _bar(x32, ref64):
    """max(4 x the error of the float32 evaluation `x32` of the definition, 1e-5)."""
    return max(4 * _rel(x32, ref64), BAR)


@pytest.fixture(autouse=True)
def _the_entry_points_exist():
    """The restatement is the rule of the entry points: no test of it passes on a tree that does not declare them."""
    from smplpp_amd import _lib

    assert {n for n, _ in NAMES} <= set(_lib.declared_symbols())


# ---------------------------------------------------------------------------------------------------- 1. the oracle against itself
def _posed(c, om):
    return SP.definition(c["world"], c["joints"], c["x"], om)[0]


@pytest.mark.parametrize("unskin", [False, True])
def test_float32_restatement_within_the_bar_of_the_definition(case, unskin):
    c = case
    for name, (om, ok) in _bindings(c).items():
        pts = _posed(c, om).astype(f32) if unskin else c["x"]
        ref, _, _ = SP.definition(c["world"], c["joints"], pts, om, unskin)
        t32 = lambda a: torch.as_tensor(np.asarray(a, f32))  # noqa: E731
        plain = SP.definition_torch(t32(c["world"]), t32(c["joints"]), t32(pts), t32(om), unskin).double().numpy()
        got = SP.forward(c["world"], c["joints"], pts, om, ok, unskin)
        assert got["out"].dtype == f32 and got["valid"].all(), name
        assert _rel(got["out"], ref) <= _bar(plain, ref), (name, _rel(got["out"], ref), _rel(plain, ref))
        # blend is the point's own transform: applied to the input it gives the output (skin), or takes the output to the input
        a, b = (got["out"], pts) if unskin else (np.broadcast_to(pts, got["out"].shape), got["out"])
        carried = np.einsum("nkab,nkb->nka", got["blend"][..., :3].astype(f64), a.astype(f64)) + got["blend"][..., 3]
        assert _rel(carried, np.broadcast_to(b, carried.shape).astype(f64)) <= 1e-5, name
        # and the gradients, per output
        ref_g = SP.definition_vjp(c["world"], c["joints"], pts, om, c["g"], unskin)
        plain_g = SP.definition_vjp(c["world"], c["joints"], pts, om, c["g"], unskin, dtype=torch.float32)
        got_g = SP.backward(c["world"], c["joints"], pts, om, ok, c["g"], unskin, want_weights=True)
        for key in ("points", "world", "joints", "weights"):
            assert got_g[key].dtype == f32 and got_g[key].shape == ref_g[key].shape, (name, key)
            assert _rel(got_g[key], ref_g[key]) <= _bar(plain_g[key], ref_g[key]), (name, key, _rel(got_g[key], ref_g[key]))


@pytest.mark.parametrize("unskin", [False, True])
@pytest.mark.parametrize("shared", [True, False])
def test_closed_form_vjps_equal_float64_autograd(case, unskin, shared):
    c = case
    n, K = c["n"], c["K"]
    for name, (om, ok) in _bindings(c, f64).items():
        pts = _posed(c, om) if unskin else c["x"].astype(f64)
        if not shared:  # one cloud and one binding per frame
            rng = np.random.default_rng(11)
            pts = np.broadcast_to(pts, (n, K, 3)) + rng.normal(0, 0.01, (n, K, 3))
            om = np.broadcast_to(om, (n, K, 24)) * rng.uniform(0.8, 1.25, (n, K, 24))
            ok = np.broadcast_to(ok, (n, K))
        got = SP.backward(c["world"], c["joints"], pts, om, ok, c["g"], unskin, dtype=f64, want_weights=True)
        ref = SP.definition_vjp(c["world"], c["joints"], pts, om, c["g"], unskin)
        for key in ("points", "world", "joints", "weights"):
            assert got[key].shape == ref[key].shape, (name, key)
            assert _rel(got[key], ref[key]) <= 1e-9, (name, key, _rel(got[key], ref[key]))
        # sum_j dc_j = sum_k g_k (skin), or the same with the cotangent the blend sees (unskin: -s u): the weights are divided by their sum
        dc = got["world"][..., 3]
        if not unskin:
            assert np.abs(dc.sum(1) - c["g"].astype(f64).sum(1)).max() <= 1e-9 * np.abs(c["g"]).sum(1).max()
        else:  # (grad_points = s u is the sum over the frames when the cloud is shared)
            assert np.abs(dc.sum((0, 1)) + got["points"].sum((0, 1))).max() <= 1e-9 * np.abs(got["points"]).sum()


def test_a_face_binding_is_the_dense_weights_it_stands_for(case):
    c = case
    om, ok = SP.omega_of(c["W"], c["faces"], c["face"], c["bary"])
    dense, dense_ok = SP.omega_of(None, None, weights=om)
    assert _same_bits(om, dense) and (ok == dense_ok).all()
    # the rule itself, joint by joint, beside a plain loop
    tri = c["faces"][c["face"][0]]
    for k in (0, 17, c["K"] - 1):
        for j in range(24):
            b, w = c["bary"][0, k], [c["W"][tri[k, i], j] for i in range(3)]
            assert om[0, k, j] == f32(f32(f32(b[0] * w[0]) + f32(b[1] * w[1])) + f32(b[2] * w[2]))
    for unskin in (False, True):
        pts = _posed(c, om).astype(f32) if unskin else c["x"]
        a = SP.forward(c["world"], c["joints"], pts, om, ok, unskin)
        b = SP.forward(c["world"], c["joints"], pts, dense, dense_ok, unskin)
        assert all(_same_bits(a[key], b[key]) for key in ("out", "blend", "valid"))


def test_unskin_of_skin_returns_the_points(case):
    c = case
    for name, (om, ok) in _bindings(c).items():
        posed = SP.forward(c["world"], c["joints"], c["x"], om, ok)["out"]
        back = SP.forward(c["world"], c["joints"], posed, om, ok, unskin=True)
        assert back["valid"].all()
        t32 = lambda a: torch.as_tensor(np.asarray(a, f32))  # noqa: E731
        w, j, o = t32(c["world"]), t32(c["joints"]), t32(om)
        plain = SP.definition_torch(w, j, SP.definition_torch(w, j, t32(c["x"]), o), o, unskin=True).double().numpy()
        want = np.broadcast_to(c["x"], back["out"].shape).astype(f64)
        assert _rel(back["out"], want) <= _bar(plain, want), (name, _rel(back["out"], want))


# ---------------------------------------------------------------------------------------------------- 2. dead points: conditions on the inputs
def test_no_point_is_dead_at_the_test_poses(synth_model, tiny):
    """theta ~ N(0, 0.3^2): the normalised blend of every bound point keeps det > 1e-4 and a positive weight sum, in float64 and in
    the float32 restatement, so a dead point in a GPU test is one the test put there."""
    for model, K in ((synth_model, 2049), (tiny, 300)):
        beta, theta = poses(8, seed=21)
        world, joints = skeleton_of(model, beta, theta)
        x, face, bary = bound_cloud(model, K, seed=22)
        faces = np.asarray(model["face_indices"], np.int64) - 1
        om, ok = SP.omega_of(np.asarray(model["weights"], f32), faces, face, bary)
        assert ok.all() and (om.astype(f64).sum(-1) > 0).all()
        posed, _, det = SP.definition(world, joints, x, om)
        assert det.min() > SP.MIN_DET and det.max() <= 1 + 1e-6, (det.min(), det.max())
        assert SP.forward(world, joints, x, om, ok)["valid"].all()
        assert SP.forward(world, joints, posed.astype(f32), om, ok, unskin=True)["valid"].all()


def test_a_collapsed_blend_is_dead():
    world, joints, w = SP.collapsed_pair()
    om, ok = SP.omega_of(None, None, weights=w)
    y = np.array([[0.1, 0.2, 0.3]], f32)
    assert SP.definition(world, joints, y, om)[2][0, 0] == 0.0
    un = SP.forward(world, joints, y, om, ok, unskin=True)
    assert un["valid"][0, 0] == 0 and not un["out"].any() and not un["blend"].any()
    # skinning the same point is defined: the blend is singular, not absent
    sk = SP.forward(world, joints, y, om, ok)
    assert sk["valid"][0, 0] == 1 and _same_bits(sk["out"][0, 0], np.array([0.0, 0.0, 0.3], f32))
    # the other kinds: a weight sum that is not positive, a value that is not finite, a face id out of range
    for bad in (np.zeros((1, 24), f32), -w, np.where(w > 0, np.nan, w).astype(f32), np.where(w > 0, np.inf, w).astype(f32)):
        o, k = SP.omega_of(None, None, weights=bad)
        assert SP.forward(world, joints, y, o, k)["valid"][0, 0] == 0
    assert SP.forward(world, joints, np.array([[np.nan, 0, 0]], f32), om, ok)["valid"][0, 0] == 0
    W, faces = np.full((3, 24), 1 / 24, f32), np.array([[0, 1, 2]])
    for fid, b, live in ((0, [0.2, 0.3, 0.5], 1), (1, [0.2, 0.3, 0.5], 0), (-1, [0.2, 0.3, 0.5], 0), (0, [np.nan, 0.3, 0.5], 0)):
        o, k = SP.omega_of(W, faces, np.array([fid]), np.array([b], f32))
        assert SP.forward(world, joints, y, o, k)["valid"][0, 0] == live, (fid, b)


# ---------------------------------------------------------------------------------------------------- 3. the entry points
def test_declared_exported_and_bound_with_the_headers_argument_lists():
    from smplpp_amd import _lib
    from smplpp_amd import smpl as S

    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    L = _lib.load()
    for name, nargs in NAMES:
        mt = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert mt, name
        assert len(mt.group(1).split(",")) == nargs, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is C.c_int, name
    assert "#define SMPLPP_UNSKIN_MIN_DET 1e-4f" in open(_lib.HEADER).read()
    for name in ("skinPoints", "unskinPoints", "skinPointsBackward", "unskinPointsBackward", "skin_points_differentiable",
                 "unskin_points_differentiable"):
        assert callable(getattr(S.SMPL, name)), name
    cpp = open(os.path.join(os.path.dirname(_lib.HEADER), "smplpp", "SMPL.h")).read()
    for name in ("skinPoints", "unskinPoints", "skinPointsBackward", "unskinPointsBackward"):
        assert re.search(r"\b%s\s*\(" % name, cpp), name


def test_a_call_without_a_model_is_refused_and_leaves_the_outputs():
    from smplpp_amd import _lib

    L = _lib.load()
    n, K = 2, 3
    world, joints, pts = np.zeros((n, 24, 3, 4), f32), np.zeros((n, 24, 3), f32), np.zeros((1, K, 3), f32)
    w, g = np.full((1, K, 24), 1 / 24, f32), np.ones((n, K, 3), f32)
    out = {k: np.full(s, 7.0, f32) for k, s in dict(o=(n, K, 3), b=(n, K, 3, 4), gp=(1, K, 3), gw=(n, 24, 3, 4), gj=(n, 24, 3), gwt=(1, K, 24)).items()}
    valid = np.full((n, K), 7, np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    for fn in (L.smplpp_skin_points, L.smplpp_unskin_points):
        assert fn(None, n, p(world), p(joints), K, p(pts), 1, None, None, p(w), 1, p(out["o"]), p(out["b"]), p(valid), 0, None) == 1
        assert b"no model" in L.smplpp_last_error()
    for fn in (L.smplpp_skin_points_vjp, L.smplpp_unskin_points_vjp):
        assert fn(None, n, p(world), p(joints), K, p(pts), 1, None, None, p(w), 1, p(g), p(out["gp"]), p(out["gw"]), p(out["gj"]), p(out["gwt"]), 0,
                  0, None) == 1
        assert b"no model" in L.smplpp_last_error()
    assert all((a == 7).all() for a in out.values()) and (valid == 7).all()
