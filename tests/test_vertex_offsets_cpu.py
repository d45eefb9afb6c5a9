"""The SMPL+D rules without a GPU: the float32 restatements of tests/vertex_offsets_oracle.py (what the kernels are held to, bit for
bit) against the float64 definition LBS(rest + D, G'), its autograd and the dense graph Laplacian, on the synthetic model with G' from
the torch restatement of the forward kinematics.  The bar is the project's: 4 x the error of an fp32 evaluation of the definition
itself, or 1e-5 relative, whichever is larger."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import vertex_offsets_oracle as VO  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402


@pytest.fixture(scope="module")
def case(synth_model):
    """n = 33 frames: W, rest, xforms, root, the undisplaced vertices (all float32) and offsets, shared and per frame."""
    from smplpp_amd import model_io

    n = 33
    beta, theta = model_io.synthetic_inputs(n, seed=11)
    with torch.no_grad():
        out = FK.fk(FK.model_tensors(synth_model), torch.tensor(beta, dtype=torch.float64), torch.tensor(theta, dtype=torch.float64))
    W = synth_model["weights"].astype(np.float32)
    rest, xforms = out["rest"].numpy().astype(np.float32), out["xforms"].numpy().astype(np.float32)
    root = theta[:, 0].astype(np.float32)
    verts = VO.definition(W, rest, xforms, np.zeros_like(rest), root, torch.float32).astype(np.float32)
    rng = np.random.default_rng(3)
    shared = VO.smooth_field(synth_model["vertices_template"])[None]
    each = (shared + rng.normal(0, 0.004, rest.shape)).astype(np.float32)
    g = rng.normal(size=rest.shape).astype(np.float32)
    return dict(n=n, W=W, rest=rest, xforms=xforms, root=root, verts=verts, shared=shared, each=each, g=g)


@pytest.mark.parametrize("kind", ["shared", "each"])
def test_forward_restatement_vs_definition(case, kind):
    c, D = case, case[kind]
    got, rd = VO.forward(c["W"], c["verts"], c["xforms"], D, rest=c["rest"])
    assert got.dtype == np.float32 and _same_bits(rd, c["rest"] + np.broadcast_to(D, c["rest"].shape))
    want = VO.definition(c["W"], c["rest"], c["xforms"], D, c["root"])
    w32 = VO.definition(c["W"], c["rest"], c["xforms"], D, c["root"], torch.float32)
    err, bar = _rel(got, want), max(4 * _rel(w32, want), 1e-5)
    print("forward %s: rel %.3g, fp32 definition %.3g" % (kind, err, _rel(w32, want)))
    assert err <= bar, (err, bar)
    # the correction alone, so that the vertices' own size does not hide it
    base = VO.definition(c["W"], c["rest"], c["xforms"], np.zeros_like(c["rest"]), c["root"])
    derr = _rel(got.astype(np.float64) - c["verts"], want - base)
    print("forward %s: correction alone rel %.3g" % (kind, derr))
    assert derr < 1e-4
    # zero offsets return the input
    assert (VO.forward(c["W"], c["verts"], c["xforms"], np.zeros_like(D)) == c["verts"]).all()


@pytest.mark.parametrize("kind", ["shared", "each"])
def test_backward_restatement_vs_autograd(case, kind):
    c, D = case, case[kind]
    got = VO.backward(c["W"], c["xforms"], c["g"], shared=kind == "shared")
    assert got.dtype == np.float32 and got.shape == D.shape
    want = VO.definition_vjp(c["W"], c["rest"], c["xforms"], D, c["g"])
    w32 = VO.definition_vjp(c["W"], c["rest"], c["xforms"], D, c["g"], torch.float32)
    err, bar = _rel(got, want), max(4 * _rel(w32, want), 1e-5)
    print("backward %s: rel %.3g, fp32 autograd %.3g" % (kind, err, _rel(w32, want)))
    assert np.abs(want).max() > 0 and err <= bar, (err, bar)
    # zero cotangent rows give exactly 0
    g = c["g"].copy()
    g[:, 100:200] = 0.0
    assert (VO.backward(c["W"], c["xforms"], g, shared=kind == "shared")[:, 100:200] == 0).all()


def test_zero_weights_change_no_bit(case):
    """A model that keeps 4 weights per vertex and one that keeps all 24 (zeros included) follow one rule: the sum over all joints,
    zeros included, has the bits of the sum over the non-zero ones."""
    c = case
    W, R = c["W"], c["xforms"][:2, :, :3, :3]
    M = np.zeros((2, W.shape[0], 3, 3), np.float32)
    for j in range(24):
        M = M + W[None, :, j, None, None] * R[:, j][:, None]
    assert _same_bits(M, VO.blend_rotations(W, c["xforms"][:2]))


@pytest.mark.parametrize("n", [31, 32, 33, 65])
def test_shared_sum_follows_the_tree(n):
    t = np.random.default_rng(n).normal(size=(n, 7, 3)).astype(np.float32)
    partials = []
    for k in range((n + 31) // 32):
        p = t[32 * k].copy()
        for f in range(32 * k + 1, min(32 * k + 32, n)):
            for v in range(7):
                for x in range(3):
                    p[v, x] = np.float32(p[v, x] + t[f, v, x])
        partials.append(p)
    want = partials[0]
    for p in partials[1:]:
        want = want + p
    assert VO.TILE == 32 and _same_bits(VO.tree_sum(t), want)
    if n == 65:  # and it is not the plain ascending sum (at 33 the two orders coincide)
        plain = t[0].copy()
        for f in range(1, n):
            plain = plain + t[f]
        assert not _same_bits(plain, want)


def test_laplacian_restatement(synth_model):
    faces = synth_model["face_indices"].astype(np.int64) - 1
    V = synth_model["vertices_template"].shape[0]
    rng = np.random.default_rng(5)
    L = VO.graph_laplacian_dense(faces, V)
    assert (np.diag(L) >= 3).all() and (L.sum(1) == 0).all()
    # integer fields: every fp32 operation is exact, so the comparison is too
    x = rng.integers(-8, 9, (2, V, 3)).astype(np.float32)
    y = rng.integers(-8, 9, (2, V, 3)).astype(np.float32)
    Lx, Ly = VO.laplacian(faces, x), VO.laplacian(faces, y)
    assert Lx.dtype == np.float32 and (Lx.astype(np.float64) == 2.0 * (L @ x.astype(np.float64))).all()
    assert (y.astype(np.float64) * Lx).sum() == (Ly.astype(np.float64) * x).sum()
    # a real field, at the bar, against the dense operator and the torch definition
    z = rng.normal(size=(2, V, 4)).astype(np.float32)
    want = 2.0 * (L @ z.astype(np.float64))
    got = VO.laplacian(faces, z)
    w32 = VO.laplacian_torch(faces, torch.from_numpy(z)).numpy()
    assert _rel(VO.laplacian_torch(faces, torch.from_numpy(z).double()).numpy(), want) < 1e-14
    print("laplacian: rel %.3g, fp32 definition %.3g" % (_rel(got, want), _rel(w32, want)))
    assert _rel(got, want) <= max(4 * _rel(w32, want), 1e-5)
    # constants give exactly 0
    const = np.broadcast_to(np.array([0.37, -1.25e-3, 1e6, 3.0], np.float32), (2, V, 4))
    assert (VO.laplacian(faces, const) == 0).all()
