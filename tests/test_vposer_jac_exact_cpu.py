"""smplpp_vposer_jacobian without a GPU: the entry point is declared, exported and bound; a call fails loudly; and the float64
Jacobian oracle the GPU tests compare against agrees with finite differences and with the oracle's own vector-Jacobian product."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vposer_jac_oracle as JO  # noqa: E402
import vposer_vjp_oracle as O  # noqa: E402


def _params():
    from smplpp_amd.ik import VPoserDecoder

    return VPoserDecoder.synthetic_params()


def test_vposer_jacobian_declared_exported_bound():
    from smplpp_amd import _lib

    assert "smplpp_vposer_jacobian" in _lib.declared_symbols()
    fn = _lib.load().smplpp_vposer_jacobian
    assert fn.argtypes is not None and len(fn.argtypes) == 8


def test_vposer_jacobian_without_gpu_raises():
    from smplpp_amd import _lib
    from smplpp_amd.ik import VPoserDecoder

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _lib.load()
    z = np.zeros((1, 32), np.float32)
    jac = np.full((1, 63, 32), 7.0, np.float32)
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_vposer_jacobian(None, 1, 0, z.ctypes.data, None, jac.ctypes.data, 0, None))
    with pytest.raises(_lib.SmplppError):
        VPoserDecoder(_params()).jacobian(z)
    assert (jac == 7.0).all()


def test_jacobian_oracle_matches_finite_differences():
    dec = O.decoder(_params())
    rng = np.random.default_rng(9)
    z = rng.normal(0, 1.0, (2, 32))
    z[0] = 0.0
    J = JO.jacobian(dec, z)
    assert J.shape == (2, 63, 32) and np.isfinite(J).all()
    h = 1e-6
    for f in range(2):
        for c in (0, 5, 17, 31):
            zp, zm = z[f:f + 1].copy(), z[f:f + 1].copy()
            zp[0, c] += h
            zm[0, c] -= h
            with torch.no_grad():
                fd = (dec(torch.as_tensor(zp)) - dec(torch.as_tensor(zm))).numpy().reshape(63) / (2 * h)
            assert np.abs(fd - J[f, :, c]).max() < 1e-6 * max(1.0, np.abs(fd).max()), (f, c)


def test_jacobian_oracle_transposed_is_the_vjp_oracle():
    dec = O.decoder(_params())
    rng = np.random.default_rng(10)
    z = rng.normal(0, 1.0, (3, 32))
    g = rng.standard_normal((3, 21, 3))
    J = JO.jacobian(dec, z)
    gz, _ = O.vjp(dec, z, g)
    assert np.abs(np.einsum("nrc,nr->nc", J, g.reshape(3, 63)) - gz).max() < 1e-12 * max(1.0, np.abs(gz).max())


def test_fp32_jacobian_oracle_is_close_to_float64():
    params = _params()
    rng = np.random.default_rng(11)
    z = rng.normal(0, 1.0, (2, 32))
    J64 = JO.jacobian(O.decoder(params), z)
    J32 = JO.jacobian(O.decoder(params, torch.float32), z, dtype=torch.float32)
    for f in range(2):
        assert np.linalg.norm(J32[f] - J64[f]) < 1e-4 * np.linalg.norm(J64[f]), f
