"""The orientation term and the Rodrigues VJP without a GPU: the entry points (declared, exported, bound, refusing before they touch a
device); the numpy restatement of smplpp_orientation_term / smplpp_orientation_term_vjp (tests/orientation_oracle.py) in float64
against the torch definition and its autograd; q = 4 (1 - cos phi); and the three fits of tests/test_orientation_gpu.py in float32
beside float64 on the oracle."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_rotmat_oracle as RO  # noqa: E402
import orientation_oracle as OR  # noqa: E402
import skeleton_oracle as SO  # noqa: E402
import test_skeleton_cpu as SK  # noqa: E402  (IMU_JOINTS, the IMU fit's target and schedule)

import smplpp_amd.orientation as orientation  # noqa: E402  (every test here belongs to the feature: without the module the file does not load)

NAMES = (("smplpp_orientation_term", 19), ("smplpp_orientation_term_vjp", 23), ("smplpp_axis_angle_to_rotmat_vjp", 8))
f32 = np.float32


@pytest.fixture(autouse=True)
def _the_entry_points_exist():
    """The restatement is the rule of the entry points: no test of it passes on a tree that does not declare them."""
    from smplpp_amd import _lib

    assert {n for n, _ in NAMES} <= set(_lib.declared_symbols())


# ---------------------------------------------------------------------------------------------------- 1. the entry points
def test_abi_declares_the_three_calls():
    from smplpp_amd import _lib
    from smplpp_amd.smpl import SMPL

    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    L = _lib.load()
    for name, nargs in NAMES:
        mt = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert mt, name
        assert len(mt.group(1).split(",")) == nargs, name
        assert name in _lib.declared_symbols()
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is C.c_int, name
    for name in ("term", "termBackward", "term_differentiable", "axis_angle_to_rotmat_differentiable", "axis_angle_to_rotmat_backward",
                 "geodesic_angle"):
        assert callable(getattr(orientation, name))
    assert callable(SMPL.axisAngleToRotmatBackward)


def test_a_call_without_a_device_fails_loudly():
    from smplpp_amd import _lib

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible: the calls run (tests/test_orientation_gpu.py)")
    frames, joint, offset, target, weight = OR.random_case(2, 3, 3, seed=1)
    with pytest.raises(_lib.SmplppError):
        orientation.term(frames, joint, target, offset, weight)
    with pytest.raises(_lib.SmplppError):
        orientation.termBackward(frames, joint, target, offset, weight, grad_energy=np.ones(2, f32))
    with pytest.raises(_lib.SmplppError):
        orientation.axis_angle_to_rotmat_backward(np.zeros((2, 3), f32), np.ones((2, 3, 3), f32))


def test_refusals_come_before_the_device():
    """Every refusal of the list returns SMPLPP_ERR_INVALID with a reason, on a machine without a GPU, and leaves host outputs as they
    were."""
    from smplpp_amd import _lib

    L = _lib.load()
    n, J, S, Cc = 2, 5, 3, 3
    frames, joint, offset, target, weight = OR.random_case(n, S, Cc, J=J, seed=2)
    out = {k: np.full(s, 7.0, f32) for k, s in dict(e=(n,), se=(n, S), r=(n, S, 3, Cc), gf=(n, J, 3, 4), go=(S, 3, Cc), gt=(n, S, 3, Cc),
                                                    ga=(n, 3)).items()}
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def fwd(n_=n, J_=J, rs=4, fr=frames, S_=S, C_=Cc, jt=joint, off=offset, tg=target, Tn=n, w=weight, Wn=n, rho=0.0, e=out["e"], se=out["se"],
            r=out["r"], space=0):
        return L.smplpp_orientation_term(0, n_, J_, rs, p(fr), S_, C_, p(jt), p(off), p(tg), Tn, p(w), Wn, rho, p(e), p(se), p(r), space, None)

    def vjp(n_=n, J_=J, rs=4, fr=frames, S_=S, C_=Cc, jt=joint, off=offset, tg=target, Tn=n, w=weight, Wn=n, rho=0.0, ge=out["e"], gse=None,
            gr=None, gf=out["gf"], go=out["go"], gt=out["gt"], acc=0, space=0):
        return L.smplpp_orientation_term_vjp(0, n_, J_, rs, p(fr), S_, C_, p(jt), p(off), p(tg), Tn, p(w), Wn, rho, p(ge), p(gse), p(gr), p(gf),
                                             p(go), p(gt), acc, space, None)

    common = [dict(n_=0), dict(n_=-1), dict(J_=0), dict(J_=-3), dict(S_=0), dict(S_=-1), dict(C_=0), dict(C_=4), dict(C_=-1), dict(rs=2), dict(rs=5),
              dict(rs=0), dict(Tn=3), dict(Tn=0), dict(Wn=3), dict(Wn=0), dict(rho=-0.5), dict(rho=float("inf")), dict(rho=float("nan")),
              dict(fr=None), dict(jt=None), dict(tg=None), dict(n_=2 ** 24, J_=24, Tn=1, Wn=1), dict(n_=2 ** 20, S_=2 ** 10, Tn=1, Wn=1),
              dict(n_=2 ** 31, Tn=1, Wn=1), dict(space=2), dict(space=-1)]
    calls = [(fwd, kw) for kw in common + [dict(e=None, se=None, r=None)]]
    calls += [(vjp, kw) for kw in common + [dict(ge=None), dict(gf=None, go=None, gt=None), dict(acc=2), dict(acc=-1)]]
    for fn, kw in calls:
        assert fn(**kw) == 1 and L.smplpp_last_error(), (fn.__name__, kw)
    assert "int32" in (fwd(n_=2 ** 24, J_=24, Tn=1, Wn=1), L.smplpp_last_error().decode())[1]
    aa, gr = np.zeros((n, 3), f32), np.ones((n, 3, 3), f32)
    rod = lambda n_=n, a=aa, g=gr, o=out["ga"], acc=0, space=0: L.smplpp_axis_angle_to_rotmat_vjp(0, n_, p(a), p(g), p(o), acc, space, None)  # noqa: E731
    for kw in (dict(n_=0), dict(n_=-2), dict(a=None), dict(g=None), dict(o=None), dict(acc=2), dict(acc=-1), dict(space=3)):
        assert rod(**kw) == 1 and L.smplpp_last_error(), kw
    assert all((a == 7).all() for a in out.values())
    # the binding words its own refusals
    for bad in (dict(frames=frames[:, :, :2]), dict(C=4), dict(target=target[:, :2]), dict(weight=weight[:, :2]), dict(offset=offset[:2])):
        kw = dict(frames=frames, joint=joint, target=target, offset=offset, weight=weight)
        kw.update(bad)
        with pytest.raises(_lib.SmplppError):
            orientation.term(**kw)
    with pytest.raises(_lib.SmplppError):
        orientation.term(frames, joint, target, want=())
    with pytest.raises(_lib.SmplppError):
        orientation.termBackward(frames, joint, target)
    with pytest.raises(_lib.SmplppError):
        orientation.termBackward(frames, joint, target, grad_energy=np.ones(n, f32), want=())


# ---------------------------------------------------------------------------------------------------- 2. the restatement against the definition
def _kill(frames, joint, offset, target, weight, J):
    """Dead sensors of every kind, in place: weight 0 and NaN, NaN in A, O and T, an index of -1 and of J."""
    n, S = weight.shape[0], len(joint)
    weight[0, 0] = 0
    weight[-1, 1 % S] = np.nan
    if S > 4:
        frames[0, joint[2], 1, 1] = np.nan
        target[0, 3, 0, 0] = np.inf
        joint[4] = -1
    if S > 6:
        joint[5] = J
        if offset is not None:
            offset[6, 2, 0] = np.nan


@pytest.mark.parametrize("lead", [(0, 0), (1, 1), (0, 1), (1, 0)], ids=lambda l: "T%dW%d" % l)
@pytest.mark.parametrize("rho", [0.0, 0.5])
@pytest.mark.parametrize("C_", [1, 2, 3])
def test_restatement_against_the_definition(C_, rho, lead):
    """In float64 the restatement's energy, sensor energy and residual equal the torch definition, and its backward equals autograd of
    the definition, to 1e-12: C = 1, 2, 3, rho 0 and 0.5, Tn and Wn in {1, n}, sensors that share joints (S = 9 on J = 5), row strides
    3 and 4, and dead sensors of every kind, which give +0 everywhere."""
    n, J, S = 4, 5, 9
    for rs, dead, offsets in ((4, False, True), (3, True, True), (4, True, False)):
        Tn, Wn = (n if v else 1 for v in lead)
        frames, joint, offset, target, weight = OR.random_case(n, S, C_, J=J, rs=rs, seed=7 + C_ + 2 * lead[0] + lead[1], Tn=Tn, Wn=Wn, offsets=offsets,
                                                               dtype=np.float64)
        assert len(set(joint.tolist())) < S  # shared joints
        if dead:
            _kill(frames, joint, offset, target, weight, J)
        live = OR.live_mask(frames, joint, target, offset, weight, C_)
        assert live.any() and (not dead or (~live).sum() >= 5)
        cot = OR.cotangents(n, S, C_, 3, np.float64)
        want, wgrad = OR.definition_vjp(frames, joint, target, offset, weight, rho, C_, cot)
        got = OR.term(frames, joint, target, offset, weight, rho, C_, dtype=np.float64)
        gf = np.full(frames.shape, 5.0)
        gf, go, gt = OR.term_vjp(frames, joint, target, offset, weight, rho, C_, *cot, gf, np.zeros((S, 3, C_)), np.zeros((Tn, S, 3, C_)), 0,
                                 dtype=np.float64)
        if rs == 4:
            assert (gf[..., 3] == 5.0).all()
        wgt = wgrad[2] if Tn == n else wgrad[2].reshape(1, S, 3, C_)
        errs = [np.abs(a - b).max() for a, b in zip(got, want)] + [np.abs(gf[..., :3] - wgrad[0][..., :3]).max(), np.abs(go - wgrad[1]).max(),
                                                                    np.abs(gt - wgt).max()]
        print("float64 restatement rs=%d dead=%d: energy %.3g, sensor %.3g, residual %.3g, frames %.3g, offset %.3g, target %.3g" % (rs, dead, *errs))
        assert max(errs) <= 1e-12, errs
        assert all(np.abs(a).max() > 0 for a in (gf[..., :3], go, gt))
        # dead sensors: +0 in every output and gradient
        for a in (got[1], got[2], gt if Tn == n else None):
            if a is not None:
                z = a[~live]
                assert (z == 0).all() and not np.signbit(z).any()
        # each cotangent alone; storing against adding
        for i in range(3):
            one = [c if k == i else None for k, c in enumerate(cot)]
            _, h = OR.definition_vjp(frames, joint, target, offset, weight, rho, C_, one)
            a, b, c = OR.term_vjp(frames, joint, target, offset, weight, rho, C_, *one, np.zeros(frames.shape), np.zeros((S, 3, C_)),
                                  np.zeros((Tn, S, 3, C_)), 0, dtype=np.float64)
            assert max(np.abs(a[..., :3] - h[0][..., :3]).max(), np.abs(b - h[1]).max(), np.abs(c - h[2].reshape(c.shape)).max()) <= 1e-12, i
        pre = [np.random.default_rng(4).standard_normal(a.shape) for a in (gf, go, gt)]
        a, b, c = OR.term_vjp(frames, joint, target, offset, weight, rho, C_, *cot, *(x.copy() for x in pre), 1, dtype=np.float64)
        hit = np.zeros((n, J), bool)
        for s in range(S):
            if 0 <= joint[s] < J:
                hit[:, joint[s]] |= live[:, s]
        assert np.array_equal(a[..., :3][hit], (pre[0][..., :3] + gf[..., :3])[hit]) and np.array_equal(a[..., :3][~hit], pre[0][..., :3][~hit])
        assert np.array_equal(a[..., 3:], pre[0][..., 3:]) and np.array_equal(b, pre[1] + go) and np.array_equal(c, pre[2] + gt)


def test_offset_none_is_the_identity_columns():
    for C_ in (1, 2, 3):
        frames, joint, _, target, weight = OR.random_case(3, 7, C_, seed=C_, offsets=False)
        eye = np.eye(3, dtype=f32)[None, :, :C_].repeat(7, 0)
        a, b = OR.term(frames, joint, target, None, weight, 0.5, C_), OR.term(frames, joint, target, eye, weight, 0.5, C_)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def test_q_is_four_one_minus_cos_phi():
    """For rotations and C = 3, q = |A O - T|^2 = 4 (1 - cos phi), phi the angle of (A O)^T T; geodesic_angle gives phi back."""
    rng = np.random.default_rng(3)
    n, S = 5, 6
    frames = np.zeros((n, 24, 3, 4))
    frames[..., :3] = OR.random_rotations(rng, (n, 24))
    O, T = OR.random_rotations(rng, (S,)), OR.random_rotations(rng, (n, S))
    T[0, 0] = frames[0, 0, :, :3] @ O[0]  # phi = 0
    T[0, 1] = frames[0, 1, :, :3] @ O[1] @ np.diag([-1.0, 1.0, -1.0])  # phi = pi
    joint = np.arange(S)
    _, q, _ = OR.term(frames, joint, T, O, None, 0.0, 3, dtype=np.float64)
    rel = np.einsum("nsab,nsac->nsbc", frames[:, :S, :, :3] @ O, T)
    cos = np.clip((np.trace(rel, axis1=2, axis2=3) - 1) / 2, -1, 1)
    assert np.abs(q - 4 * (1 - cos)).max() <= 1e-12
    phi = orientation.geodesic_angle(q)
    assert np.abs(phi - np.arccos(cos))[q > 1e-6].max() <= 1e-7 and phi[0, 0] <= 1e-7 and abs(phi[0, 1] - np.pi) <= 1e-6
    assert torch.allclose(orientation.geodesic_angle(torch.tensor(q)), torch.tensor(phi))


# ---------------------------------------------------------------------------------------------------- 3. the three fits
def _oracle_forward(n, dtype):
    from smplpp_amd import model_io

    mm = SO.cast(SO.model_tensors(model_io.synthetic_model()), dtype)
    beta = torch.zeros(n, 10, dtype=dtype)

    def forward(theta):
        o = SO.skeleton(mm, beta, theta)
        return o["world"], o["posed"]

    return forward


def run_fit(kind, dtype):
    """(first, last, trajectory) of fit `kind` on the oracle in `dtype`."""
    if kind == "imu":
        return OR.imu_fit(_oracle_forward(SK.FIT_N, dtype), OR.oracle_term_energy, dtype)
    if kind == "calibration":
        theta = torch.as_tensor(OR.calibration_case()[0], dtype=dtype)
        with torch.no_grad():
            world = _oracle_forward(OR.CAL_N, dtype)(theta)[0]
        return OR.calibration_fit(world, OR.oracle_term_energy, RO.rot6d_to_rotmat, dtype)
    return OR.smooth_fit(_oracle_forward(OR.SMOOTH_T, dtype), OR.oracle_term_energy, OR.rodrigues, OR.oracle_smooth, dtype)


# The float64 runs of the three fits, first and last loss, as this file's own float64 run gives them:
#   imu          62.36 -> 2.25e-8   (the figures of tests/test_skeleton_cpu.py: the term is that file's loss)
#   calibration  15.16 -> 1.87e-9   (15.16 0.259 0.0136 1.02e-3 7.8e-5 4.6e-6 3.2e-7 4.0e-8 at steps 0, 25, ..., 175)
#   smooth       80.96 -> 1.1426    (what is left is the smoothness energy of the steady motion itself)
FLOAT64 = {"imu": (62.36, None), "calibration": (15.156, None), "smooth": (80.961, 1.1426)}


@pytest.mark.parametrize("kind", ["imu", "calibration", "smooth"])
def test_fits_in_float32_beside_float64(kind):
    f64, f32_ = run_fit(kind, torch.float64), run_fit(kind, torch.float32)
    print("fit %s float64 %.6g -> %.6g, float32 %.6g -> %.6g" % (kind, f64[0], f64[1], f32_[0], f32_[1]))
    print("fit %s float64 trajectory %s" % (kind, " ".join("%.4g" % v for v in f64[2])))
    first, last = FLOAT64[kind]
    assert abs(f64[0] / first - 1) < 1e-3
    if last is None:
        assert f64[1] < 1e-7
    else:
        assert abs(f64[1] / last - 1) < 0.02
    assert OR.fit_passes(f32_[1], f64[1]), (f32_, f64)
