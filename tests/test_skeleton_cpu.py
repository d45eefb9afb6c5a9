"""The skeleton oracle (tests/skeleton_oracle.py) against the FK oracles it is cut from, its closed-form backward against autograd on
the SMPL, chain and star trees, the two fits of tests/test_skeleton_gpu.py in float32 beside float64, and the ABI declarations.
No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_rotmat_oracle as RO  # noqa: E402
import skeleton_oracle as SO  # noqa: E402

torch = SO.torch
TREES = ["smpl", "chain", "star"]


def tree_model(tree):
    """The synthetic SMPL tree, or tiny_model(61, seed=7) as a 24-joint chain or a star (tests/test_model_create_gpu.py)."""
    from smplpp_amd import model_io

    if tree == "smpl":
        return model_io.synthetic_model()
    md = model_io.tiny_model(61, seed=7)
    for i in range(1, 24):
        md["kinematic_tree"][0, i] = i - 1 if tree == "chain" else 0
    return md


def _case(n, seed):
    rng = np.random.default_rng(seed)
    beta = rng.standard_normal((n, 10))
    theta = 0.5 * rng.standard_normal((n, 25, 3))
    R = RO.rodrigues_np(theta[:, 1:]) + 0.05 * rng.standard_normal((n, 24, 3, 3))  # general matrices
    gw, gp, gj = rng.standard_normal((n, 24, 3, 4)), rng.standard_normal((n, 24, 3)), rng.standard_normal((n, 24, 3))
    return beta, theta, R, gw, gp, gj


@pytest.mark.parametrize("tree", TREES)
def test_oracle_is_the_fk_oracles_skeleton(tree):
    m = SO.model_tensors(tree_model(tree))
    beta, theta, R, _, _, _ = _case(3, 1)
    trans = theta[:, 0]
    t = lambda a: torch.as_tensor(a)
    with torch.no_grad():
        sk = SO.chain(m, t(beta), t(trans), t(R))
        fk = RO.fk(m, t(beta), t(trans), t(R))
        aa = SO.skeleton(m, t(beta), t(theta))
        fa = SO.O.fk(m, t(beta), t(theta))
    rel = lambda o: o["g"] - (o["A"] @ o["J"][..., None])[..., 0]
    for o, f in ((sk, fk), (aa, fa)):
        assert float((o["A"] - f["xforms"][:, :, :3, :3]).abs().max()) <= 1e-13
        assert float((rel(o) - f["xforms"][:, :, :3, 3]).abs().max()) <= 1e-13
        assert float((o["J"] - f["joints"]).abs().max()) <= 1e-13
        assert torch.equal(o["posed"], o["g"] + t(trans)[:, None]) and torch.equal(o["world"][..., 3], o["posed"])
        assert torch.equal(o["world"][..., :3], o["A"])


@pytest.mark.parametrize("tree", TREES)
def test_closed_form_recurrence_is_autograd(tree):
    m = SO.model_tensors(tree_model(tree))
    beta, theta, R, gw, gp, gj = _case(3, 2)
    for cots in ((gw, gp, gj), (gw, None, None), (None, gp, None), (None, None, gj)):
        want = SO.vjp_rotmat(m, beta, theta[:, 0], R, *cots)
        got = SO.closed_form(m, beta, theta[:, 0], R, *cots)
        for name, a, b in zip(("beta", "trans", "rot"), got, want):
            err = float(np.abs(a - b).max())
            print(tree, name, "closed form - autograd: %.3g" % err)
            assert err <= 1e-12, (tree, name, err)
        want = SO.vjp(m, beta, theta, *cots)
        got = SO.closed_form_theta(m, beta, theta, *cots)
        for name, a, b in zip(("beta", "theta"), got, want):
            err = float(np.abs(a - b).max())
            assert err <= 1e-12, (tree, name, err)


def test_levels_ascend():
    lv = SO.levels([-1] + [0] * 23)
    assert lv == [[0], list(range(1, 24))]
    assert SO.levels([-1] + list(range(23))) == [[i] for i in range(24)]


# ------------------------------------------------------------------------------------------------ the two fits
IMU_JOINTS = [0, 7, 8, 15, 20, 21]
FIT_N, FIT_STEPS, FIT_LR = 4, 200, 0.05


def fit_target():
    """theta* ~ N(0, 0.3^2) on all 25 rows, default_rng(5); beta = 0."""
    return (0.3 * np.random.default_rng(5).standard_normal((FIT_N, 25, 3))).astype(np.float32)


def fit_loss(kind, world, posed, world_t, posed_t):
    if kind == "posed":
        return ((posed - posed_t) ** 2).sum()
    return ((world[:, IMU_JOINTS, :, :3] - world_t[:, IMU_JOINTS, :, :3]) ** 2).sum() + ((posed[:, 0] - posed_t[:, 0]) ** 2).sum()


def run_fit(kind, forward, dtype, device="cpu"):
    """Adam(lr 0.05), 200 steps from theta = 0 on `fit_loss`; forward(theta) -> (world, posed).  Returns (first loss, last loss)."""
    target = torch.as_tensor(fit_target(), dtype=dtype, device=device)
    with torch.no_grad():
        world_t, posed_t = (a.clone() for a in forward(target))
    theta = torch.zeros(FIT_N, 25, 3, dtype=dtype, device=device, requires_grad=True)
    opt = torch.optim.Adam([theta], lr=FIT_LR)
    first = None
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        loss = fit_loss(kind, *forward(theta), world_t, posed_t)
        loss.backward()
        opt.step()
        first = float(loss.detach()) if first is None else first
    with torch.no_grad():
        last = float(fit_loss(kind, *forward(theta), world_t, posed_t))
    return first, last


def oracle_forward(m, dtype):
    mm = SO.cast(m, dtype)
    beta = torch.zeros(FIT_N, 10, dtype=dtype)

    def forward(theta):
        o = SO.skeleton(mm, beta, theta)
        return o["world"], o["posed"]

    return forward


def fit_passes(kind, first, last, last64):
    if kind == "posed":
        return first / last >= 1e3 and last <= 2 * last64
    return last < 1e-6 or last <= 2 * last64


@pytest.mark.parametrize("kind", ["posed", "imu"])
def test_fits_in_float32_beside_float64(kind):
    from smplpp_amd import model_io

    m = SO.model_tensors(model_io.synthetic_model())
    f64 = run_fit(kind, oracle_forward(m, torch.float64), torch.float64)
    f32 = run_fit(kind, oracle_forward(m, torch.float32), torch.float32)
    print("fit", kind, "float64 %.4g -> %.4g, float32 %.4g -> %.4g" % (f64 + f32))
    if kind == "posed":
        assert abs(f64[0] - 46.59) < 0.01 and abs(f64[1] / 0.0121 - 1) < 0.02  # (0.01203 after the 200th step)
    else:
        assert abs(f64[0] - 62.36) < 0.01 and f64[1] < 1e-7
    assert fit_passes(kind, *f32, f64[1]), (f32, f64)


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_declares_the_four_calls():
    import ctypes as C
    import re

    from smplpp_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    L = _lib.load()
    for name, nargs in (("smplpp_skeleton", 9), ("smplpp_skeleton_rotmat", 10), ("smplpp_skeleton_vjp", 12),
                        ("smplpp_skeleton_rotmat_vjp", 14)):
        mt = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
        assert mt, name
        assert len(mt.group(1).split(",")) == nargs, name
        assert name in _lib.declared_symbols()
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is C.c_int, name
