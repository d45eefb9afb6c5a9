"""The pose priors on the MI355X (smplpp_pose_prior, smplpp_pose_prior_vjp): every bit against the numpy restatement of
tests/pose_prior_oracle.py; independence of batch, slot, space, leading dimension and of the outputs asked for; the edge cases (twin
components, NaN, +-inf limits, a coordinate exactly at a limit); the gradient against float64 autograd, alone and in one graph with the
keypoint term; a single-view fit with and without the prior against the same schedules in float64 on the CPU; the refusals; the C++
shim."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import keypoints_oracle as KP  # noqa: E402
import pose_prior_oracle as PO  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 0.05
OFF = 6  # where the coordinates start in a row of a strided buffer (the body pose in a row of theta)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _same(a, b):
    """_same_bits where neither is NaN, and NaN in the same places (a NaN's sign and payload are not part of the rule)."""
    a, b = np.ascontiguousarray(_host(a)), np.ascontiguousarray(b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and _same_bits(np.where(np.isnan(a), np.float32(0), a), np.where(np.isnan(b), np.float32(0), b))


def _make(p, device="cuda:0"):
    from smplpp_amd.priors import PosePrior

    return PosePrior(device, p["mean"], p["mat"], p["offset"], p["lo"], p["hi"], p["weight"])


def _ld(D):
    return 75 if D <= 69 else D + OFF


def _strided(X, fill=7.0):
    """X [n,D] at offset OFF inside rows of _ld(D) floats filled with `fill`."""
    buf = np.full((X.shape[0], _ld(X.shape[1])), fill, np.float32)
    buf[:, OFF:OFF + X.shape[1]] = X
    return buf


# ---------------------------------------------------------------------------------------------------- 1. bits
# every D in {1, 7, 8, 9, 63, 64, 65, 69, 128}, every M in {1, 3, 8, 32}, every n in {1, 3, 65}; then the two forms of the second round
# of outputs (64 .. D-1) on either side of their threshold at D = 96 / 97, and a lane-per-output second round that is not full
CASES = [(1, 1, 1), (3, 7, 3), (8, 8, 65), (3, 9, 1), (1, 63, 3), (8, 64, 3), (3, 65, 65), (8, 69, 65), (32, 69, 3), (32, 128, 65), (1, 128, 1),
         (3, 96, 3), (3, 97, 3), (3, 100, 3)]


@pytest.fixture(scope="module")
def cases():
    """(M, D, n) -> the prior, the poses, the cotangents and the restatement's results; computed once."""
    out = {}
    for M, D, n in CASES:
        p = PO.prior(M, D, seed=10 * M + D)
        X = PO.poses(n, D, seed=100 * D + n)
        rng = np.random.default_rng(M + D + n)
        ge, gr, gl = rng.normal(size=n).astype(np.float32), rng.normal(size=(n, D)).astype(np.float32), rng.normal(size=n).astype(np.float32)
        fwd = PO.forward(p, X)
        other = (fwd["component"] + 1) % M  # a forced component that is not the best one
        out[M, D, n] = dict(p=p, X=X, ge=ge, gr=gr, gl=gl, fwd=fwd, other=other, base=rng.normal(size=(n, _ld(D))).astype(np.float32),
                            g=PO.backward(p, X, fwd["component"], ge, gr, gl), g_other=PO.backward(p, X, other, ge, gr, gl),
                            g_e=PO.backward(p, X, fwd["component"], ge, None, None), g_r=PO.backward(p, X, fwd["component"], None, gr, None),
                            g_l=PO.backward(p, X, None, None, None, gl), g_el=PO.backward(p, X, fwd["component"], ge, None, gl))
    return out


def _forward_equals(r, want, rows=slice(None)):
    return (_same(r["energy"], want["energy"][rows]) and np.array_equal(_host(r["component"]), want["component"][rows]) and
            _same(r["residual"], want["residual"][rows]) and _same(r["limit_energy"], want["limit_energy"][rows]))


@pytest.mark.parametrize("M,D,n", CASES)
def test_forward_bits(cases, M, D, n):
    c = cases[M, D, n]
    prior, X, want = _make(c["p"]), c["X"], c["fwd"]
    assert prior.info() == dict(component_num=M, dim=D, has_limits=True)
    assert np.isfinite(want["energy"]).all() and (M == 1 or D < 7 or n < 65 or len(np.unique(want["component"])) > 1)
    for put in (lambda a: a, _dev):
        r = prior.evaluate(put(X))
        assert list(r) == ["energy", "component", "residual", "limit_energy"] and _host(r["component"]).dtype == np.int64
        assert _forward_equals(r, want), {k: int((_host(r[k]) != want[k]).sum()) for k in r}
        for k in want:  # each output alone
            alone = prior.evaluate(put(X), want=(k,))
            assert list(alone) == [k] and _same(_host(alone[k]).astype(np.float32), want[k].astype(np.float32)), k
        # the same coordinates inside rows of ld floats
        r = prior.evaluate(put(_strided(X)), ld=_ld(D), offset=OFF)
        assert _forward_equals(r, want)
    for k in {0, n // 2, n - 1}:  # a frame alone has the bits it has at its slot of the batch
        assert _forward_equals(prior.evaluate(X[k:k + 1]), want, slice(k, k + 1))
        assert _forward_equals(prior.evaluate(_dev(X[k:k + 1])), want, slice(k, k + 1))


def _raw_vjp(prior, buf, ld, component, ge, gr, gl, out, acc, dev):
    """smplpp_pose_prior_vjp on rows of ld floats with the coordinates at OFF, into `out` (the same layout)."""
    from smplpp_amd import _lib
    from smplpp_amd.smpl import _ptr, _stream

    args = [buf, component, ge, gr, gl, out]
    if dev:
        args = [_dev(a) for a in args]
    _lib.check(_lib.load().smplpp_pose_prior_vjp(prior.handle, buf.shape[0], _ptr(args[0]) + 4 * OFF, ld, *(_ptr(a) for a in args[1:5]),
                                                 _ptr(args[5]) + 4 * OFF, acc, _lib.DEVICE if dev else _lib.HOST, _stream() if dev else None))
    if dev:
        torch.cuda.synchronize()
    return _host(args[5])


@pytest.mark.parametrize("M,D,n", CASES)
def test_backward_bits(cases, M, D, n):
    c = cases[M, D, n]
    prior, X, ge, gr, gl, comp = _make(c["p"]), c["X"], c["ge"], c["gr"], c["gl"], c["fwd"]["component"]
    assert np.abs(c["g"]).max() > 0 and (D == 1 or np.abs(c["g_l"]).max() > 0) and (M == 1 or not _same_bits(c["g"], c["g_other"]))
    ld = _ld(D)
    for put in (lambda a: a, _dev):
        back = lambda **kw: _host(prior.evaluateBackward(put(X), **{k: put(v) for k, v in kw.items()}))  # noqa: E731
        g = back(grad_energy=ge, grad_residual=gr, grad_limit_energy=gl, component=comp)
        assert g.dtype == np.float32 and _same_bits(g, c["g"]), int((g != c["g"]).sum())
        assert _same_bits(back(grad_energy=ge, grad_residual=gr, grad_limit_energy=gl), c["g"])  # component NULL: chosen as the forward does
        if M > 1:
            assert _same_bits(back(grad_energy=ge, grad_residual=gr, grad_limit_energy=gl, component=c["other"]), c["g_other"])
        # each cotangent alone, and the two energies without the residual
        assert _same_bits(back(grad_energy=ge, component=comp), c["g_e"]) and _same_bits(back(grad_energy=ge), c["g_e"])
        assert _same_bits(back(grad_residual=gr, component=comp), c["g_r"]) and _same_bits(back(grad_limit_energy=gl), c["g_l"])
        assert _same_bits(back(grad_energy=ge, grad_limit_energy=gl), c["g_el"])
        # accumulate: the finished element is added
        base = c["base"][:, :D].copy()
        out = put(base.copy())
        assert prior.evaluateBackward(put(X), put(ge), put(gr), put(gl), component=put(comp), out=out) is out
        assert _same_bits(_host(out), base + c["g"])
    # rows of ld floats: the floats outside the D coordinates stay as they were, with accumulate = 0 and with 1
    for dev in (False, True):
        for acc in (0, 1):
            got = _raw_vjp(prior, _strided(X), ld, comp, ge, gr, gl, c["base"].copy(), acc, dev)
            want = c["base"].copy()
            want[:, OFF:OFF + D] = want[:, OFF:OFF + D] + c["g"] if acc else c["g"]
            assert _same_bits(got, want), (dev, acc)
    z = _host(prior.evaluateBackward(_strided(X), ge, gr, gl, component=comp, ld=ld, offset=OFF))
    assert _same_bits(z[:, OFF:OFF + D], c["g"]) and (np.delete(z, np.s_[OFF:OFF + D], axis=1) == 0).all()
    for k in {0, n // 2, n - 1}:  # a frame alone
        s = slice(k, k + 1)
        assert _same_bits(prior.evaluateBackward(X[s], ge[s], gr[s], gl[s]), c["g"][s])
        assert _same_bits(_host(prior.evaluateBackward(_dev(X[s]), _dev(ge[s]), _dev(gr[s]), _dev(gl[s]), component=_dev(comp[s]))), c["g"][s])


@pytest.mark.parametrize("D,n", [(69, 5), (128, 3)])
def test_limits_only_and_mixture_only(D, n):
    from smplpp_amd.priors import PosePrior

    X = PO.poses(n, D, seed=D)
    rng = np.random.default_rng(D)
    ge, gr, gl = rng.normal(size=n).astype(np.float32), rng.normal(size=(n, D)).astype(np.float32), rng.normal(size=n).astype(np.float32)
    p = PO.prior(0, D, seed=21)
    lim = PosePrior.from_limits("cuda:0", p["lo"], p["hi"], p["weight"])
    assert lim.info() == dict(component_num=0, dim=D, has_limits=True)
    want = PO.forward(p, X)
    assert list(want) == ["limit_energy"] and (want["limit_energy"] > 0).all()
    for put in (lambda a: a, _dev):
        r = lim.evaluate(put(X))
        assert list(r) == ["limit_energy"] and _same_bits(_host(r["limit_energy"]), want["limit_energy"])
        assert _same_bits(_host(lim.evaluateBackward(put(X), grad_limit_energy=put(gl))), PO.backward(p, X, None, None, None, gl))
    q = PO.prior(3, D, seed=22, limits=False)
    mix = _make(q)
    assert mix.info() == dict(component_num=3, dim=D, has_limits=False)
    want = PO.forward(q, X)
    for put in (lambda a: a, _dev):
        r = mix.evaluate(put(X))
        assert list(r) == ["energy", "component", "residual"] and all(_same(_host(r[k]).astype(np.float32), want[k].astype(np.float32)) for k in r)
        assert _same_bits(_host(mix.evaluateBackward(put(X), put(ge), put(gr))), PO.backward(q, X, None, ge, gr, None))
    if D == 69:  # the body pose of theta, in place
        theta = rng.normal(0, 0.3, (n, 25, 3)).astype(np.float32)
        body = theta.reshape(n, 75)[:, 6:]
        want = PO.forward(q, body)
        for put in (lambda a: a, _dev):
            r = mix.evaluate_theta(put(theta))
            assert all(_same(_host(r[k]).astype(np.float32), want[k].astype(np.float32)) for k in want)
            gt = _host(mix.evaluate_theta_backward(put(theta), put(ge), put(gr), component=r["component"])).reshape(n, 75)
            assert (gt[:, :6] == 0).all() and _same_bits(gt[:, 6:], PO.backward(q, body, want["component"], ge, gr, None))
            out = put(np.ones((n, 25, 3), np.float32))
            mix.evaluate_theta_backward(put(theta), put(ge), out=out)
            assert _same_bits(_host(out).reshape(n, 75)[:, 6:], np.float32(1) + PO.backward(q, body, None, ge, None, None))
            assert (_host(out).reshape(n, 75)[:, :6] == 1).all()


def test_from_gmm_and_load(tmp_path):
    """PosePrior.from_gmm and PosePrior.load (an .npz of means, covars, weights) against the plain constructor on the tables of
    tests/pose_prior_oracle.py, bit for bit."""
    from smplpp_amd.priors import PosePrior

    gmm = PO.synthetic_gmm(3, 69, 51)
    lim = PO.prior(0, 69, 52)
    p = dict(zip(("mean", "mat", "offset"), PO.gmm_tables(*gmm)), lo=lim["lo"], hi=lim["hi"], weight=lim["weight"])
    X = PO.poses(5, 69, 53)
    want = PO.forward(p, X)
    path = str(tmp_path / "gmm.npz")
    np.savez(path, means=gmm[0], covars=gmm[1], weights=gmm[2])
    made = [_make(p), PosePrior.from_gmm("cuda:0", *gmm, lo=lim["lo"], hi=lim["hi"], limit_weight=lim["weight"]),
            PosePrior.load(path, lo=lim["lo"], hi=lim["hi"], limit_weight=lim["weight"])]
    for prior in made:
        assert prior.info() == dict(component_num=3, dim=69, has_limits=True) and _forward_equals(prior.evaluate(X), want)
    plain = PosePrior.load(path)  # as written in a fitting script: the default device, no limits
    assert plain.info() == dict(component_num=3, dim=69, has_limits=False)
    r = plain.evaluate(_dev(X))
    assert list(r) == ["energy", "component", "residual"] and _same(r["energy"], want["energy"]) and _same(r["residual"], want["residual"])


# ---------------------------------------------------------------------------------------------------- 2. edge cases
def test_edge_cases():
    D, n = 9, 7
    p = PO.prior(3, D, 4)
    p["mean"][2], p["mat"][2], p["offset"][2] = p["mean"][1], p["mat"][1], p["offset"][1]  # two identical components
    X = PO.poses(n, D, 5)
    X[:3] = p["mean"][1] + np.float32(0.01) * X[:3]  # at the twins' centre: the lower index wins
    X[4, 3] = np.nan
    X[5, 5], X[5, 6] = p["hi"][5], p["lo"][6]  # exactly at a limit: nothing
    X[6, 0], X[6, 1] = 100.0, 100.0  # no limit at all on coordinate 0, none above on coordinate 1
    clean = X.copy()
    clean[4, 3] = 0.1
    prior = _make(p)
    want, want_clean = PO.forward(p, X), PO.forward(p, clean)
    assert (want["component"][:3] == 1).all() and want["component"][4] == 0 and np.isnan(want["energy"][4]) and np.isnan(want["residual"][4]).all()
    v, _ = PO._limit(p, X)
    assert v[5, 5] == 0 and v[5, 6] == 0 and v[4, 3] == 0 and v[6, 0] == 0 and v[6, 1] == 0 and np.isfinite(want["limit_energy"]).all()
    rows = [0, 1, 2, 3, 5, 6]  # the NaN frame's neighbours keep their bits
    assert all(_same_bits(want[k][rows], want_clean[k][rows]) for k in want)
    ge, gl = np.ones(n, np.float32), np.ones(n, np.float32)
    ge[4] = gl[4] = 0  # a cotangent of exactly 0 on the NaN frame: +0 gradients
    wg = PO.backward(p, X, None, ge, None, gl)
    assert (wg[4] == 0).all() and not np.signbit(wg[4]).any() and np.isfinite(wg).all() and wg[5, 5] == PO.backward(p, X, None, ge, None, None)[5, 5]
    for put in (lambda a: a, _dev):
        r = prior.evaluate(put(X))
        assert _forward_equals(r, want)
        assert _same_bits(_host(prior.evaluateBackward(put(X), grad_energy=put(ge), grad_limit_energy=put(gl))), wg)
        assert _same_bits(_host(prior.evaluateBackward(put(X), grad_energy=put(ge), grad_limit_energy=put(gl), component=r["component"])), wg)
    # a device-space component outside [0, M) contributes nothing
    bad = np.array([0, 3, -1, 1, 0, 99, 2], np.int64)
    got = _host(prior.evaluateBackward(_dev(X), grad_energy=_dev(ge), grad_limit_energy=_dev(gl), component=_dev(bad)))
    assert _same_bits(got, PO.backward(p, X, bad, ge, None, gl)) and _same_bits(got[[1, 2, 5]], PO.backward(p, X, None, None, None, gl)[[1, 2, 5]] + np.float32(0))


# ---------------------------------------------------------------------------------------------------- 3. gradients
def _bar(got, want64, fp32, what):
    err, ref = _rel(_host(got), want64), _rel(fp32, want64)
    print("%s: rel %.3g, fp32 autograd %.3g" % (what, err, ref))
    assert np.abs(want64).max() > 0 and err <= max(4 * ref, 1e-5), (what, err, ref)


def test_chain_against_float64_autograd():
    """theta -> lambda energy + mu limit_energy + <c, residual> on the body pose of theta [n,25,3], against float64 autograd."""
    n, lam, mu = 5, 0.7, 1.3
    p = PO.prior(8, 69, seed=31)
    prior = _make(p)
    rng = np.random.default_rng(32)
    theta = rng.normal(0, 0.3, (n, 25, 3)).astype(np.float32)
    c = rng.normal(size=(n, 69)).astype(np.float32)
    r = prior.evaluate_theta(_dev(theta))
    got = prior.evaluate_theta_backward(_dev(theta), _dev(np.full(n, lam, np.float32)), _dev(c), _dev(np.full(n, mu, np.float32)), component=r["component"])
    value = lam * r["energy"].double().sum() + mu * r["limit_energy"].double().sum() + (r["residual"].double() * _dev(c).double()).sum()

    def ref(dtype):
        t = PO.tensors(p, dtype)
        th = torch.tensor(theta, dtype=dtype, requires_grad=True)
        body = th.reshape(n, 75)[:, 6:]
        e, y, comp = PO.energy_t(t, body)
        loss = lam * e.sum() + mu * PO.limit_t(t, body).sum() + (y * torch.tensor(c, dtype=dtype)).sum()
        loss.backward()
        return float(loss.detach()), th.grad.double().numpy(), comp.numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert np.array_equal(_host(r["component"]), r64[2]) and abs(float(value) - r64[0]) <= 1e-5 * abs(r64[0])
    assert (_host(got)[:, :2] == 0).all()
    _bar(got, r64[1], r32[1], "prior chain theta")


def test_keypoints_and_prior_in_one_graph():
    """theta, beta -> smplpp_fk -> landmarks -> projection -> sum of keypoint energies, plus the prior's energy and limit term of the same
    theta, through the autograd wrappers in one graph, against float64 autograd of the restated graph."""
    from smplpp_amd import model_io
    from smplpp_amd import smpl as S
    from smplpp_amd.landmarks import Landmarks
    from smplpp_amd.smpl import SMPL

    V, n, rho = 97, 3, 100.0
    model = model_io.tiny_model(V)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    row_ptr, col, val = KP.regressor_11(V)
    norm = np.maximum(np.add.reduceat(np.abs(np.append(val, 0)), row_ptr[:-1]) * (np.diff(row_ptr) > 0), 1e-30)
    reg = (row_ptr, col, (val / np.repeat(norm, np.diff(row_ptr))).astype(np.float32))
    lm = Landmarks(s, *reg)
    p = PO.prior(8, 69, seed=41)
    prior = _make(p)
    rng = np.random.default_rng(42)
    beta, theta = model_io.synthetic_inputs(n, seed=43)
    cam = np.tile(np.concatenate([np.diag([1.0, -1.0, -1.0]).reshape(9), [0.0, -0.03, 4.0], [500.0, 490.0, 320.0, 240.0]]), (n, 1)).astype(np.float32)
    fk = s.launch(beta, theta, want=("verts", "joints"))
    uv0, _, ok = KP.project(KP.landmarks(reg, fk["verts"], fk["joints"]), cam, NEAR)
    assert ok.all()
    T = np.concatenate([uv0 + rng.normal(0, 20.0, uv0.shape), rng.uniform(0.2, 1.0, uv0.shape[:2] + (1,))], -1).astype(np.float32)
    w_prior, w_limit = 0.01, 0.5
    b, t = (torch.from_numpy(x).cuda().requires_grad_(True) for x in (beta, theta))
    verts, joints = s.forward_differentiable(b, t)
    _, e, _ = S.project_points_differentiable(lm.forward_differentiable(verts, joints), _dev(cam), _dev(T), rho, NEAR)
    pe, le = prior.forward_differentiable(t)
    loss = e.sum() + w_prior * pe.sum() + w_limit * le.sum()
    loss.backward()

    def ref(dtype):
        m = FK.model_tensors(model, dtype)
        bb, th = (torch.tensor(x, dtype=dtype, requires_grad=True) for x in (beta, theta))
        out = FK.fk(m, bb, th)
        pts = KP.landmarks_t(torch.tensor(KP.dense(reg, V + 24), dtype=dtype), out["verts"], out["joints"])
        uvr, vr = KP.project_t(pts, torch.tensor(cam, dtype=dtype), NEAR)
        tt = PO.tensors(p, dtype)
        body = th.reshape(n, 75)[:, 6:]
        parts = (KP.energy_t(uvr, vr, torch.tensor(T, dtype=dtype), rho).sum(), PO.energy_t(tt, body)[0].sum(), PO.limit_t(tt, body).sum())
        (parts[0] + w_prior * parts[1] + w_limit * parts[2]).backward()
        return [float(x.detach()) for x in parts], bb.grad.double().numpy(), th.grad.double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for got, want in zip((e.sum(), pe.sum(), le.sum()), r64[0]):
        assert want > 0 and abs(float(got) - want) <= 1e-4 * want
    _bar(b.grad, r64[1], r32[1], "one graph beta")
    _bar(t.grad, r64[2], r32[2], "one graph theta")
    # the prior's share of the gradient is not lost in the keypoint term's
    only = torch.from_numpy(theta).cuda().requires_grad_(True)
    pe2, le2 = prior.forward_differentiable(only)
    (w_prior * pe2.sum() + w_limit * le2.sum()).backward()
    assert _rel(_host(only.grad), r64[2]) > 1e-3 and float(only.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 4. a fit
FIT_STEPS, FIT_LR, FIT_RHO, FIT_PRIOR = 200, 0.02, 100.0, 0.01
# The seed of the true poses: default_rng(91), each frame's body pose by multivariate_normal(mean, covar) of its component, then the root
# rotations.  In float64 this ends at 210.3 mm without the prior and 137.6 mm with it (ratio 0.654).  The order of the draws matters: the
# root rotations first, or the body poses through a Cholesky factor, give other true poses and ratios between 0.73 and 0.99.
FIT_SEED = 91


def fit_setup(synth_model):
    """The single-view fit of the issue, n = 4: the synthetic model with the 53-row regressor, synthetic_gmm(8, 69, 5); true body poses
    one draw per frame from components 0..3, root rotation from N(0, 0.1^2); the camera fixed at (0, -0.36, 2.5), f = 500;
    confidence 1 on landmarks 24, 26, ..., 46 only.  Returns what the float64 run on the CPU needs, restated on the vertices the
    regressor reads (the same numbers as on the whole body, a tenth of the work)."""
    n = 4
    reg = KP.regressor_53(synth_model)
    V = synth_model["vertices_template"].shape[0]
    gmm = PO.synthetic_gmm(8, 69, 5)
    mean, mat, offset = PO.gmm_tables(*gmm)
    p = dict(mean=mean, mat=mat, offset=offset, lo=None, hi=None, weight=None)
    rng = np.random.default_rng(FIT_SEED)  # the body poses first, frame by frame, then the root rotations
    theta_true = np.zeros((n, 25, 3), np.float32)
    for f in range(n):
        theta_true[f, 2:] = rng.multivariate_normal(gmm[0][f], gmm[1][f]).reshape(23, 3)
    theta_true[:, 1] = rng.normal(0, 0.1, (n, 3))
    cam = np.tile(np.concatenate([np.diag([1.0, -1.0, -1.0]).reshape(9), [0.0, -0.36, 2.5], [500.0, 500.0, 320.0, 240.0]]), (n, 1)).astype(np.float32)
    conf = np.zeros(53, np.float32)
    conf[24:48:2] = 1.0
    used = np.unique(np.concatenate([reg[1][reg[1] < V], np.nonzero(np.abs(synth_model["joint_regressor"]).sum(0))[0]]))
    sub = {k: synth_model[k][used] for k in ("vertices_template", "shape_blend_shapes", "pose_blend_shapes", "weights")}
    sub["joint_regressor"], sub["kinematic_tree"] = synth_model["joint_regressor"][:, used], synth_model["kinematic_tree"]
    m64 = FK.model_tensors(sub, torch.float64)
    A64 = torch.tensor(np.concatenate([KP.dense(reg, V + 24)[:, used], KP.dense(reg, V + 24)[:, V:]], 1))
    beta64, cam64 = torch.zeros(n, 10, dtype=torch.float64), torch.tensor(cam, dtype=torch.float64)

    def points64(theta):
        out = FK.fk(m64, beta64, theta)
        return KP.landmarks_t(A64, out["verts"], out["joints"])

    with torch.no_grad():
        pts_true = points64(torch.tensor(theta_true, dtype=torch.float64))
        uv_true, ok = KP.project_t(pts_true, cam64, NEAR)
    assert bool(ok.all())
    target64 = torch.cat([uv_true, torch.tensor(conf, dtype=torch.float64).expand(n, 53)[..., None]], -1)
    t64 = PO.tensors(p, torch.float64)

    def cpu(theta, with_prior):
        pts = points64(theta)
        uv, valid = KP.project_t(pts, cam64, NEAR)
        loss = KP.energy_t(uv, valid, target64, FIT_RHO).mean()
        if with_prior:
            loss = loss + FIT_PRIOR * PO.energy_t(t64, theta.reshape(n, 75)[:, 6:])[0].mean()
        return loss, pts

    return dict(n=n, reg=reg, prior=p, cam=cam, target64=target64, pts_true=pts_true, cpu=cpu)


def fit_run(loss_and_points, pts_true, with_prior, dev, dtype):
    """FIT_STEPS Adam steps on theta from 0; the mean 3-D error of landmarks 24..52 in mm at the end."""
    theta = torch.zeros(pts_true.shape[0], 25, 3, dtype=dtype, device=dev, requires_grad=True)
    opt = torch.optim.Adam([theta], lr=FIT_LR)
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        loss_and_points(theta, with_prior)[0].backward()
        opt.step()
    with torch.no_grad():
        pts = loss_and_points(theta, with_prior)[1]
        return 1000 * float((pts[:, 24:].double().cpu() - pts_true[:, 24:]).norm(dim=-1).mean())


def test_fit_with_and_without_the_prior(synth_model):
    """Measured, mean 3-D error of landmarks 24..52 after 200 steps, without the prior and with it: float64 on the CPU 210.3 and 137.6 mm
    (ratio 0.654), MI355X 210.3 and 137.6 mm."""
    from smplpp_amd import smpl as S
    from smplpp_amd.landmarks import Landmarks
    from smplpp_amd.smpl import SMPL

    fs = fit_setup(synth_model)
    n = fs["n"]
    ref_without, ref_with = (fit_run(fs["cpu"], fs["pts_true"], w, torch.device("cpu"), torch.float64) for w in (False, True))
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    lm = Landmarks(s, *fs["reg"])
    prior = _make(fs["prior"])
    dev = torch.device("cuda")
    target32, cam32, beta32 = fs["target64"].float().to(dev), torch.from_numpy(fs["cam"]).to(dev), torch.zeros(n, 10, device=dev)

    def gpu(theta, with_prior):
        verts, joints = s.forward_differentiable(beta32, theta)
        pts = lm.forward_differentiable(verts, joints)
        _, e, _ = S.project_points_differentiable(pts, cam32, target32, FIT_RHO, NEAR)
        loss = e.mean()
        if with_prior:
            loss = loss + FIT_PRIOR * prior.forward_differentiable(theta)[0].mean()
        return loss, pts

    got_without, got_with = (fit_run(gpu, fs["pts_true"], w, dev, torch.float32) for w in (False, True))
    print("pose-prior fit, mean 3-D error of landmarks 24..52 in mm (without the prior, with it): float64 CPU %.4g, %.4g; GPU %.4g, %.4g" %
          (ref_without, ref_with, got_without, got_with))
    assert ref_with < 0.8 * ref_without, (ref_without, ref_with)  # a property of the fixture
    assert got_with <= 0.9 * got_without, (got_without, got_with)  # a missing or wrong-signed prior gradient gives a ratio >= 1
    assert got_with <= 2 * ref_with, (got_with, ref_with)


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals():
    from smplpp_amd import _lib

    L = _lib.load()
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)  # noqa: E731
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    D, M, n = 9, 3, 2
    p = PO.prior(M, D, 1)

    def create(M_=M, D_=D, **edit):
        q = dict(p, **edit)
        h = C.c_void_p(7)
        a = [f32(q[k]) for k in ("mean", "mat", "offset", "lo", "hi", "weight")]
        rc = L.smplpp_pose_prior_create(0, M_, D_, *(ptr(x) for x in a), C.byref(h))
        if rc == 0:
            L.smplpp_pose_prior_destroy(h)
        else:
            assert h.value is None  # *out = NULL
        return rc

    def at(key, idx, value):
        a = p[key].copy()
        a.reshape(-1)[idx] = value
        return {key: a}

    assert create() == 0 and create(lo=None, hi=None, weight=None) == 0 and create(M_=0, mean=None, mat=None, offset=None) == 0
    assert create(**at("lo", 2, -np.inf)) == 0 and create(**at("hi", 2, np.inf)) == 0 and create(**at("weight", 2, 0.0)) == 0
    assert create(M_=-1) == 1 and create(M_=33) == 1 and create(D_=0) == 1 and create(D_=129) == 1
    assert create(M_=0, lo=None, hi=None, weight=None) == 1 and create(mean=None) == 1 and create(mat=None) == 1 and create(offset=None) == 1
    assert create(lo=None) == 1 and create(hi=None) == 1 and create(weight=None) == 1
    assert create(**at("mean", 1, np.nan)) == 1 and create(**at("mat", 5, np.inf)) == 1 and create(**at("offset", 0, -np.inf)) == 1
    assert create(**at("lo", 3, np.nan)) == 1 and create(**at("hi", 3, np.nan)) == 1 and create(**at("lo", 3, 1.0)) == 1
    assert create(**at("weight", 4, -0.5)) == 1 and create(**at("weight", 4, np.inf)) == 1 and create(**at("weight", 4, np.nan)) == 1
    assert L.smplpp_pose_prior_create(0, M, D, None, None, None, None, None, None, None) == 1  # no out

    full, mix_only, lim_only = _make(p), _make(PO.prior(M, D, 1, limits=False)), _make(PO.prior(0, D, 1))
    for dev in (False, True):  # host space, then device space, where no staging copy could hide a write
        put = _dev if dev else (lambda a: a)
        adr = (lambda a: None if a is None else a.data_ptr()) if dev else ptr
        space = 1 if dev else 0
        X = put(PO.poses(n, D, 2))
        ge, gr, gl = put(np.ones(n, np.float32)), put(np.ones((n, D), np.float32)), put(np.ones(n, np.float32))
        comp = put(np.zeros(n, np.int64))
        e, c, r, le = (put(np.full(n, 7.0, np.float32)), put(np.full(n, 7, np.int64)), put(np.full((n, D), 7.0, np.float32)),
                       put(np.full(n, 7.0, np.float32)))
        gp = put(np.full((n, D), 7.0, np.float32))

        def fwd(h=full, nn=n, x=X, ld=D, o=(e, c, r, le), space=space):
            return L.smplpp_pose_prior(h.handle if h else None, nn, adr(x), ld, *(adr(a) for a in o), space, None)

        def bwd(h=full, nn=n, x=X, ld=D, cp=comp, g=(ge, gr, gl), o=gp, acc=0, space=space):
            return L.smplpp_pose_prior_vjp(h.handle if h else None, nn, adr(x), ld, adr(cp), *(adr(a) for a in g), adr(o), acc, space, None)

        def untouched():
            torch.cuda.synchronize()
            return all((_host(a) == 7).all() for a in (e, c, r, le, gp))

        for call in (fwd, bwd):
            assert call(h=None) == 1 and call(nn=0) == 1 and call(nn=-3) == 1 and call(ld=D - 1) == 1 and call(x=None) == 1
            assert call(space=2) == 1 and call(space=-1) == 1
            assert call(nn=2 ** 31 // D + 1) == 1 and call(nn=2 ** 20, ld=2 ** 11) == 1  # n ld beyond int32 indexing
        assert fwd(o=(None,) * 4) == 1 and bwd(g=(None,) * 3) == 1 and bwd(o=None) == 1
        assert bwd(acc=2) == 1 and bwd(acc=-1) == 1
        # a mixture output or cotangent without a mixture; a limit output or cotangent without limits
        for o in ((e, None, None, None), (None, c, None, None), (None, None, r, None)):
            assert fwd(h=lim_only, o=o) == 1
        assert fwd(h=mix_only, o=(None, None, None, le)) == 1 and fwd(h=mix_only) == 1 and fwd(h=lim_only) == 1
        assert bwd(h=lim_only, g=(ge, None, None)) == 1 and bwd(h=lim_only, g=(None, gr, None)) == 1
        assert bwd(h=mix_only, g=(None, None, gl)) == 1 and bwd(h=mix_only) == 1
        if not dev:  # a host-space component outside [0, M)
            assert bwd(cp=np.array([0, M], np.int64)) == 1 and bwd(cp=np.array([-1, 0], np.int64)) == 1
        assert untouched()
        # the calls that succeed, each into a buffer of its own where the shared ones are checked afterwards
        other = put(np.full((n, D), 7.0, np.float32))
        stray = put(np.array([M, -1], np.int64))  # ignored where no mixture cotangent is given, in either space
        assert bwd(h=lim_only, g=(None, None, gl), cp=None, o=other) == 0 and bwd(h=lim_only, g=(None, None, gl), cp=stray, o=other) == 0
        assert bwd(g=(None, None, gl), cp=stray, o=other) == 0
        assert untouched() and (_host(other) != 7).any()
        assert fwd() == 0 and bwd() == 0 and bwd(cp=None) == 0 and fwd(h=mix_only, o=(e, c, r, None)) == 0 and fwd(h=lim_only, o=(None, None, None, le)) == 0
        torch.cuda.synchronize()
        assert (_host(e) != 7).all() and (_host(c) != 7).all() and (_host(r) != 7).any() and (_host(gp) != 7).any()


# ---------------------------------------------------------------------------------------------------- 6. C++ shim
def test_pose_prior_cpp_shim(tmp_path):
    from smplpp_amd.priors import PosePrior

    exe = str(tmp_path / "pose_prior_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_prior_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    n, M, f = 5, 3, np.float32
    want = []
    for D in (7, 69):
        i = np.arange(M * D * D)
        mean = ((np.arange(M * D) % 13 - 6) * f(0.03125)).astype(f).reshape(M, D)
        mat = ((i % 17 - 8) * f(0.0625) + np.where(i % (D + 1) == 0, f(2), f(0))).astype(f).reshape(M, D, D)
        offset = (np.arange(M) * f(0.5)).astype(f)
        k = np.arange(D)
        lo, hi, w = np.full(D, -0.125, f), (f(0.0625) * (k % 3)).astype(f), (f(0.25) * (k % 4)).astype(f)
        prior = PosePrior("cuda:0", mean, mat, offset, lo, hi, w)
        j = np.arange(n)
        ge, gl = ((j % 3) * f(0.5)).astype(f), ((j % 2 + 1) * f(0.25)).astype(f)
        gr = ((np.arange(n * D) % 5 - 2) * f(0.125)).astype(f).reshape(n, D)
        if D == 7:
            pose = ((np.arange(n * D) % 11 - 5) * f(0.0625)).astype(f).reshape(n, D)
            t = prior.evaluate(pose)
            g = prior.evaluateBackward(pose, ge, gr, gl, component=t["component"])
            assert len(np.unique(t["component"])) > 1 and (t["limit_energy"] > 0).any() and np.abs(g).max() > 0
            want += [t["energy"], t["component"].astype(f), t["residual"], t["limit_energy"], g]
        else:
            theta = ((np.arange(n * 75) % 11 - 5) * f(0.0625)).astype(f).reshape(n, 25, 3)
            t = prior.evaluate_theta(theta)
            g = prior.evaluate_theta_backward(theta, ge, None, gl)
            acc = prior.evaluate_theta_backward(theta, ge, None, gl, out=np.ones((n, 25, 3), f))
            assert np.abs(g).max() > 0 and (g[:, :2] == 0).all()
            want += [t["energy"], t["limit_energy"], g, acc]
    assert len(raw) == 4 * sum(x.size for x in want)
    off = 0
    for k, x in enumerate(want):
        got = np.frombuffer(raw, np.float32, x.size, off).reshape(x.shape)
        off += 4 * x.size
        assert _same_bits(got, x), k
