"""The rotation-matrix entry points without a GPU: the float64 restatement with R as the leaf (tests/fk_rotmat_oracle.py) is pinned to
the axis-angle restatement, forward and backward; rot6d_to_rotmat gives rotations; and the binding declares the three symbols with
the header's argument lists."""
import ctypes as C
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_rotmat_oracle as RO  # noqa: E402
import fk_vjp_oracle as O  # noqa: E402


def _case(n=3, V=29, seed=2):
    from smplpp_amd import model_io

    model = model_io.tiny_model(V, seed=seed)
    rng = np.random.default_rng(seed)
    beta = rng.standard_normal((n, 10))
    theta = rng.standard_normal((n, 25, 3)) * 0.4
    theta[0, 4] = 0.0  # a zero rotation
    ax = rng.standard_normal(3)
    theta[1, 6] = np.pi * ax / np.linalg.norm(ax)  # |theta| = pi
    gv = rng.standard_normal((n, V, 3))
    gj = rng.standard_normal((n, 24, 3))
    return O.model_tensors(model), beta, theta, gv, gj


def test_restatement_with_rodrigues_equals_axis_angle_restatement():
    m, beta, theta, _, _ = _case()
    b, t = torch.as_tensor(beta), torch.as_tensor(theta)
    want = O.fk(m, b, t)
    got = RO.fk(m, b, t[:, 0], O.rodrigues(t[:, 1:]))
    for k in ("verts", "joints", "rest", "xforms"):
        assert float((got[k] - want[k]).abs().max()) <= 1e-12, k


def test_restatement_gradient_contracts_to_axis_angle_gradient():
    m, beta, theta, gv, gj = _case()
    gb, gt = O.vjp(m, beta, theta, gv, gj)
    R = RO.rodrigues_np(theta[:, 1:])
    rb, rt, rr = RO.vjp(m, beta, theta[:, 0], R, gv, gj)
    assert np.abs(rb - gb).max() <= 1e-9
    assert np.abs(rt - gt[:, 0]).max() <= 1e-9
    back = RO.contract_rodrigues(theta[:, 1:], rr)
    assert np.abs(back - gt[:, 1:]).max() <= 1e-9


def test_rot6d_to_rotmat_gives_rotations_and_inverts_the_first_two_columns():
    from smplpp_amd.smpl import rot6d_to_rotmat

    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 24, 6, dtype=torch.float64, generator=g)
    R = rot6d_to_rotmat(x)
    assert R.shape == (5, 24, 3, 3)
    eye = torch.eye(3, dtype=torch.float64)
    assert float((R.transpose(-1, -2) @ R - eye).abs().max()) < 1e-12
    assert float((torch.linalg.det(R) - 1).abs().max()) < 1e-12
    assert float((R - RO.rot6d_to_rotmat(x)).abs().max()) < 1e-12
    # the first two columns of a rotation, interleaved as the [..., 3, 2] view reads them, give the rotation back
    # (Q: rotations to the last bit or two; the reference's Rodrigues with its 1e-8 is orthonormal to 1e-8 only)
    Q = torch.linalg.qr(torch.randn(7, 3, 3, dtype=torch.float64, generator=g))[0]
    Q = Q * torch.linalg.det(Q)[:, None, None]
    assert float((rot6d_to_rotmat(Q[..., :, :2].reshape(7, 6)) - Q).abs().max()) < 1e-12
    # differentiable
    x = torch.randn(2, 6, dtype=torch.float64, generator=g, requires_grad=True)
    assert torch.autograd.gradcheck(rot6d_to_rotmat, (x,))
    # float32 in, float32 out
    assert rot6d_to_rotmat(torch.randn(3, 6, generator=g)).dtype == torch.float32


def _header_args(name):
    from smplpp_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_binding_declares_the_symbols_with_the_headers_argument_lists():
    from smplpp_amd import _lib

    L = _lib.load()
    declared = _lib.declared_symbols()
    for name in ("smplpp_axis_angle_to_rotmat", "smplpp_fk_rotmat", "smplpp_fk_rotmat_vjp"):
        assert name in declared
        fn = getattr(L, name)  # exported
        args = _header_args(name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args), (name, args)
        assert fn.restype is C.c_int
        for a, t in zip(args, fn.argtypes):
            if a.startswith("int64_t "):
                assert t is C.c_int64, (name, a)
            elif a.startswith("int "):
                assert t is C.c_int, (name, a)
            else:
                assert "*" in a and t is C.c_void_p, (name, a)
    assert _header_args("smplpp_fk_rotmat")[1:5] == ["int64_t n", "const float * beta", "const float * trans", "const float * rot"]
    assert _header_args("smplpp_fk_rotmat_vjp")[-5:-2] == ["float * grad_beta", "float * grad_trans", "float * grad_rot"]
    assert _header_args("smplpp_axis_angle_to_rotmat") == ["int device", "int64_t n", "const float * aa", "float * rot", "int space",
                                                          "void * stream"]
