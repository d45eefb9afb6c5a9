"""smplpp_fk_vjp without a GPU: the entry point is declared, exported and bound; a call fails loudly; and the float64 oracle the GPU
tests compare against is pinned to the reference-generated FK fixtures and to finite differences."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as O  # noqa: E402
from conftest import GOLDEN, model_digest  # noqa: E402


def test_fk_vjp_declared_exported_bound():
    from smplpp_amd import _lib

    assert "smplpp_fk_vjp" in _lib.declared_symbols()
    L = _lib.load()
    fn = L.smplpp_fk_vjp
    assert fn.argtypes is not None and len(fn.argtypes) == 11


def test_fk_vjp_without_gpu_raises():
    from smplpp_amd import _lib

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _lib.load()
    beta = np.zeros((1, 10), np.float32)
    theta = np.zeros((1, 25, 3), np.float32)
    gb = np.full((1, 10), 7.0, np.float32)
    # a null model is refused before any device work; with a model pointer the HIP runtime reports no device
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_fk_vjp(None, 1, beta.ctypes.data, theta.ctypes.data, None, None, None, gb.ctypes.data, None, 0, None))
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    with pytest.raises(_lib.SmplppError):
        s.init(model_io.tiny_model(20, seed=1))
        s.launchBackward(beta, theta, grad_joints=np.ones((1, 24, 3), np.float32))
    assert (gb == 7.0).all()


def _golden_check(model, g, ids=None):
    m = O.model_tensors(model)
    out = O.fk(m, torch.as_tensor(g["beta"], dtype=torch.float64), torch.as_tensor(g["theta"], dtype=torch.float64))
    for k in ("verts", "rest", "joints", "xforms"):
        if k not in g:
            continue
        got = out[k].numpy()
        if ids is not None and k in ("verts", "rest"):
            got = got[:, ids]
        assert np.abs(got - g[k]).max() < 1e-5, k


def test_oracle_forward_matches_fk_synth(synth_model, golden_fk_synth):
    g = golden_fk_synth
    assert str(g["model_sha256"]) == model_digest(synth_model)
    _golden_check(synth_model, g, ids=g["vertex_ids"])


def test_oracle_forward_matches_fk_tiny():
    from smplpp_amd import model_io

    g = np.load(os.path.join(GOLDEN, "fk_tiny.npz"))
    _golden_check(model_io.tiny_model(61, seed=7), g)


def test_oracle_gradients_match_finite_differences():
    from smplpp_amd import model_io

    model = model_io.tiny_model(23, seed=4)
    m = O.model_tensors(model)
    rng = np.random.default_rng(0)
    n = 2
    beta = rng.standard_normal((n, 10))
    theta = rng.standard_normal((n, 25, 3)) * 0.4
    theta[1, 5] = 0.0
    gv = rng.standard_normal((n, 23, 3))
    gj = rng.standard_normal((n, 24, 3))
    gb, gt = O.vjp(m, beta, theta, gv, gj)

    def loss(b, t):
        o = O.fk(m, torch.as_tensor(b), torch.as_tensor(t))
        return float((o["verts"].numpy() * gv).sum() + (o["joints"].numpy() * gj).sum())

    h = 1e-6
    for idx in [(0, 0), (1, 9), (0, 4)]:
        bp, bm = beta.copy(), beta.copy()
        bp[idx] += h
        bm[idx] -= h
        fd = (loss(bp, theta) - loss(bm, theta)) / (2 * h)
        assert abs(fd - gb[idx]) < 1e-6 * max(1.0, abs(fd)), (idx, fd, gb[idx])
    for idx in [(0, 0, 1), (1, 1, 0), (0, 7, 2), (1, 6, 1), (1, 24, 2)]:
        tp, tm = theta.copy(), theta.copy()
        tp[idx] += h
        tm[idx] -= h
        fd = (loss(beta, tp) - loss(beta, tm)) / (2 * h)
        assert abs(fd - gt[idx]) < 1e-6 * max(1.0, abs(fd)), (idx, fd, gt[idx])
