"""smplpp_vposer_vjp without a GPU: the entry point is declared, exported and bound; a call fails loudly; and the float64 oracle the
GPU tests compare against agrees with the fp32 autograd of the reference restatement and with finite differences."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vposer_vjp_oracle as O  # noqa: E402


def _params():
    from smplpp_amd.ik import VPoserDecoder

    return VPoserDecoder.synthetic_params()


def test_vposer_vjp_declared_exported_bound():
    from smplpp_amd import _lib

    assert "smplpp_vposer_vjp" in _lib.declared_symbols()
    fn = _lib.load().smplpp_vposer_vjp
    assert fn.argtypes is not None and len(fn.argtypes) == 9


def test_vposer_vjp_without_gpu_raises():
    from smplpp_amd import _lib
    from smplpp_amd.ik import VPoserDecoder

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _lib.load()
    z = np.zeros((1, 32), np.float32)
    g = np.ones((1, 21, 3), np.float32)
    gz = np.full((1, 32), 7.0, np.float32)
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_vposer_vjp(None, 1, 0, z.ctypes.data, g.ctypes.data, gz.ctypes.data, None, 0, None))
    with pytest.raises(_lib.SmplppError):
        VPoserDecoder(_params()).launchBackward(z, g)
    assert (gz == 7.0).all()


def test_oracle_float64_agrees_with_fp32_autograd():
    params = _params()
    rng = np.random.default_rng(3)
    z = rng.normal(0, 1.0, (6, 32))
    g = rng.standard_normal((6, 21, 3))
    gz64, out64 = O.vjp(O.decoder(params), z, g)
    gz32, out32 = O.vjp(O.decoder(params, torch.float32), z, g, dtype=torch.float32)
    assert np.isfinite(gz64).all()
    assert np.abs(out32 - out64).max() < 1e-5
    for f in range(6):
        assert np.linalg.norm(gz32[f] - gz64[f]) < 1e-4 * np.linalg.norm(gz64[f]), f


def test_oracle_gradients_match_finite_differences():
    params = _params()
    dec = O.decoder(params)
    rng = np.random.default_rng(4)
    n = 3
    z = rng.normal(0, 1.0, (n, 32))
    g = rng.standard_normal((n, 21, 3))
    gz, _ = O.vjp(dec, z, g)

    def loss(zz):
        with torch.no_grad():
            return float((dec(torch.as_tensor(zz)).numpy() * g).sum())

    h = 1e-6
    for idx in [(0, 0), (1, 31), (2, 7), (0, 16), (1, 3)]:
        zp, zm = z.copy(), z.copy()
        zp[idx] += h
        zm[idx] -= h
        fd = (loss(zp) - loss(zm)) / (2 * h)
        assert abs(fd - gz[idx]) < 1e-6 * max(1.0, abs(fd)), (idx, fd, gz[idx])
