"""The forward-mode oracle (tests/fk_jvp_oracle.py) on the CPU: its closed form against float64 forward-mode autograd on the SMPL,
chain and star trees, the adjoint identity against the backward oracles, the ABI declarations, and the Levenberg-Marquardt fit of
tests/test_fk_jvp_gpu.py in float32 beside float64.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_jvp_oracle as JO  # noqa: E402
import skeleton_oracle as SO  # noqa: E402
from test_skeleton_cpu import TREES, tree_model  # noqa: E402

torch = JO.torch
O, RO = JO.O, JO.RO


def _case(n, seed):
    """Inputs with theta rows of exactly 0 and of |theta| = pi, general (non-orthonormal) matrices, and one tangent per frame."""
    rng = np.random.default_rng(seed)
    beta = rng.standard_normal((n, 10))
    theta = 0.5 * rng.standard_normal((n, 25, 3))
    theta[0, 3] = 0.0
    theta[1, 1:] = 0.0
    ax = rng.standard_normal(3)
    theta[2, 7] = np.pi * ax / np.linalg.norm(ax)
    R = RO.rodrigues_np(theta[:, 1:]) + 0.05 * rng.standard_normal((n, 24, 3, 3))
    tan = dict(dbeta=rng.standard_normal((n, 10)), dtheta=rng.standard_normal((n, 25, 3)), dtrans=rng.standard_normal((n, 3)),
               dR=rng.standard_normal((n, 24, 3, 3)))
    return beta, theta, R, tan


@pytest.mark.parametrize("tree", TREES)
def test_closed_form_is_forward_mode_autograd(tree):
    m = JO.model_tensors(tree_model(tree))
    beta, theta, R, t = _case(3, 3)
    col = lambda a: None if a is None else a[:, None]
    for db, dth in ((t["dbeta"], t["dtheta"]), (t["dbeta"], None), (None, t["dtheta"])):
        want = JO.tangent(m, beta, theta, col(db), col(dth))
        got = JO.closed_form_theta(m, beta, theta, db, dth)
        for k in ("verts", "joints", "world"):
            err = float(np.abs(got[k] - want[k][:, 0]).max())
            print(tree, "axis-angle", k, "closed form - forward mode: %.3g" % err)
            assert err <= 1e-12, (tree, k, err)
    for db, dtr, dr in ((t["dbeta"], t["dtrans"], t["dR"]), (None, None, t["dR"]), (t["dbeta"], None, None), (None, t["dtrans"], None)):
        want = JO.tangent_rotmat(m, beta, theta[:, 0], R, col(db), col(dtr), col(dr))
        got = JO.closed_form(m, beta, theta[:, 0], R, db, dtr, dr)
        for k in ("verts", "joints", "world"):
            err = float(np.abs(got[k] - want[k][:, 0]).max())
            print(tree, "rotmat", k, "closed form - forward mode: %.3g" % err)
            assert err <= 1e-12, (tree, k, err)


def test_shared_tangents_and_the_tangent_axis():
    m = JO.model_tensors(tree_model("chain"))
    beta, theta, _, _ = _case(3, 4)
    rng = np.random.default_rng(8)
    db, dth = rng.standard_normal((4, 10)), rng.standard_normal((4, 25, 3))
    sh = JO.tangent(m, beta, theta, db, dth, shared=True)
    pf = JO.tangent(m, beta, theta, np.repeat(db[None], 3, 0), np.repeat(dth[None], 3, 0))
    for k in sh:
        assert sh[k].shape[:2] == (3, 4) and np.array_equal(sh[k], pf[k]), k
    one = JO.closed_form_theta(m, beta, theta, np.repeat(db[2:3], 3, 0), np.repeat(dth[2:3], 3, 0))
    assert float(np.abs(one["verts"] - sh["verts"][:, 2]).max()) <= 1e-12


@pytest.mark.parametrize("tree", TREES)
def test_adjoint_identity_against_the_backward_oracles(tree):
    m = JO.model_tensors(tree_model(tree))
    beta, theta, _, t = _case(3, 5)
    V = m["T"].shape[0]
    rng = np.random.default_rng(6)
    gv, gj = rng.standard_normal((3, V, 3)), rng.standard_normal((3, 24, 3))
    gw = rng.standard_normal((3, 24, 3, 4))
    Jv = JO.closed_form_theta(m, beta, theta, t["dbeta"], t["dtheta"])
    gb, gt = O.vjp(m, beta, theta, gv, gj)
    sb, st = SO.vjp(m, beta, theta, grad_world=gw, grad_joints=gj)
    for f in range(3):  # frame by frame: the frames are independent
        lhs = (gv[f] * Jv["verts"][f]).sum() + (gj[f] * Jv["joints"][f]).sum()
        rhs = (gb[f] * t["dbeta"][f]).sum() + (gt[f] * t["dtheta"][f]).sum()
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (tree, f, lhs, rhs)
        lhs = (gw[f] * Jv["world"][f]).sum() + (gj[f] * Jv["joints"][f]).sum()
        rhs = (sb[f] * t["dbeta"][f]).sum() + (st[f] * t["dtheta"][f]).sum()
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (tree, f, lhs, rhs)


def test_displaced_rest_enters_as_a_value():
    """SMPL+D: with rest + D handed over, the tangent is that of the displaced body (D a constant)."""
    m = JO.model_tensors(tree_model("star"))
    beta, theta, R, t = _case(3, 7)
    D = 0.01 * np.random.default_rng(9).standard_normal((3, m["T"].shape[0], 3))
    rest = RO.forward(m, beta, theta[:, 0], R)["rest"]
    want = JO.tangent_rotmat(m, beta, theta[:, 0], R, t["dbeta"][:, None], t["dtrans"][:, None], t["dR"][:, None], offsets=D)
    got = JO.closed_form(m, beta, theta[:, 0], R, t["dbeta"], t["dtrans"], t["dR"], rest=rest + D)
    assert float(np.abs(got["verts"] - want["verts"][:, 0]).max()) <= 1e-12
    rest = O.fk(m, torch.as_tensor(beta), torch.as_tensor(theta))["rest"].numpy()
    want = JO.tangent(m, beta, theta, t["dbeta"][:, None], t["dtheta"][:, None], rest=rest + D)
    got = JO.closed_form_theta(m, beta, theta, t["dbeta"], t["dtheta"], rest=rest + D)
    assert float(np.abs(got["verts"] - want["verts"][:, 0]).max()) <= 1e-12


# ------------------------------------------------------------------------------------------------ the application: LM on dense Jacobians
def test_lm_fit_in_float32_beside_float64():
    from smplpp_amd import model_io

    m = JO.model_tensors(model_io.synthetic_model())
    f64 = JO.lm_fit(*JO.oracle_lm(m, torch.float64), dtype=np.float64)
    f32 = JO.lm_fit(*JO.oracle_lm(m, torch.float32), dtype=np.float32)
    print("LM float64 %.4g -> %.4g, float32 %.4g -> %.4g" % (f64 + f32))
    assert abs(f64[0] / LM_FIRST64 - 1) < 0.01 and abs(f64[1] / LM_LAST64 - 1) < 0.02, f64
    assert abs(f32[0] / f64[0] - 1) < 1e-3 and abs(f32[1] / f64[1] - 1) < 1e-2, (f32, f64)  # the same path to three digits
    assert JO.lm_passes(*f32, f64[1]), (f32, f64)


LM_FIRST64, LM_LAST64 = 7.24e3, 2.71  # summed energy before the first and after the twelfth iteration, float64


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_declares_the_two_calls():
    import ctypes as C
    import re

    from smplpp_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    L = _lib.load()
    # (m, n, T, beta, theta, rest, dbeta, dtheta, shared, dverts, djoints, dworld, space, stream) and the rotmat entry's two more
    for name, nargs in (("smplpp_fk_jvp", 14), ("smplpp_fk_rotmat_jvp", 16)):
        mt = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert mt, name
        assert len(mt.group(1).split(",")) == nargs, name
        assert name in _lib.declared_symbols()
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is C.c_int, name
    from smplpp_amd.smpl import SMPL, _FKFunction, _FKRotmatFunction

    for meth in ("launchTangent", "launchRotmatTangent", "jacobian"):
        assert callable(getattr(SMPL, meth)), meth
    for fn in (_FKFunction, _FKRotmatFunction):
        assert "jvp" in vars(fn), fn  # forward mode is the class's own, not the base class's refusal
