"""The keypoint term on the MI355X (smplpp_landmarks, smplpp_landmarks_vjp, smplpp_project_points, smplpp_project_points_vjp): every
bit against the numpy restatements of tests/keypoints_oracle.py; independence of batch, slot, space and of the outputs asked for;
the chain theta, beta -> smplpp_fk -> landmarks -> projection -> sum of energies, and the gradient to all 16 camera entries,
against float64 autograd of the restated graph; a two-stage fit (camera translation, then pose) against the same schedule in
float64 on the CPU; the refusals; the C++ shim."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import keypoints_oracle as KP  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NMAX = 65
TINY_V = 97
NEAR = 0.05


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _same_energy(a, b):
    """_same_bits where neither is NaN, and NaN in the same places (a NaN's sign and payload are not part of the rule)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and _same_bits(np.where(np.isnan(a), np.float32(0), a), np.where(np.isnan(b), np.float32(0), b))


def _smpl(model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    return s


@pytest.fixture(scope="module")
def tiny():
    """tiny_model(97) with the 11-row regressor: one launch of NMAX frames, a cotangent, and the restatement's results for them."""
    from smplpp_amd import model_io
    from smplpp_amd.landmarks import Landmarks

    model = model_io.tiny_model(TINY_V)
    s = _smpl(model)
    reg = KP.regressor_11(TINY_V)
    lm = Landmarks(s, *reg)
    assert lm.info() == dict(landmark_num=11, nnz=len(reg[1]))
    beta, theta = model_io.synthetic_inputs(NMAX, seed=71)
    fk = s.launch(beta, theta, want=("verts", "joints"))
    g = np.random.default_rng(72).normal(size=(NMAX, 11, 3)).astype(np.float32)
    want_gv, want_gj = KP.landmarks_vjp(reg, g, TINY_V)
    return dict(model=model, s=s, lm=lm, reg=reg, verts=fk["verts"], joints=fk["joints"], g=g, pts=KP.landmarks(reg, fk["verts"], fk["joints"]),
                gv=want_gv, gj=want_gj)


@pytest.fixture(scope="module")
def synth(synth_model):
    """The synthetic 6890-vertex model with the 53-row regressor."""
    from smplpp_amd.landmarks import Landmarks

    s = _smpl(synth_model)
    reg = KP.regressor_53(synth_model)
    assert len(reg[0]) - 1 == 53 and np.diff(reg[0])[24:48].tolist() == [30] * 24
    return dict(s=s, reg=reg, lm=Landmarks(s, *reg))


# ---------------------------------------------------------------------------------------------------- 1. landmark bits
@pytest.mark.parametrize("n", [1, 3, NMAX])
def test_landmark_forward_bits(tiny, n):
    lm, v, j, want = tiny["lm"], tiny["verts"][:n], tiny["joints"][:n], tiny["pts"][:n]
    got = lm.regress(v, j)
    assert got.dtype == np.float32 and _same_bits(got, want), int((got != want).sum())
    assert (got[:, 0] == 0).all() and not np.signbit(got[:, 0]).any()  # the empty row: +0
    assert _same_bits(got[:, 1], v[:, TINY_V // 2]) and _same_bits(got[:, 2], j[:, 5])
    assert _same_bits(lm.regress(_dev(v), _dev(j)).cpu().numpy(), want)
    for k in {0, n // 2, n - 1}:  # a frame alone has the bits it has at its slot of the batch
        assert _same_bits(lm.regress(v[k:k + 1], j[k:k + 1])[0], want[k])
        assert _same_bits(lm.regress(_dev(v[k:k + 1]), _dev(j[k:k + 1])).cpu().numpy()[0], want[k])


@pytest.mark.parametrize("n", [1, 3, NMAX])
def test_landmark_backward_bits(tiny, n):
    lm, g, wv, wj = tiny["lm"], tiny["g"][:n], tiny["gv"][:n], tiny["gj"][:n]
    for put in (lambda a: a, _dev):
        r = lm.regressBackward(put(g))
        assert _same_bits(_host(r["verts"]), wv) and _same_bits(_host(r["joints"]), wj)
        # each output alone
        assert _same_bits(_host(lm.regressBackward(put(g), want=("verts",))["verts"]), wv)
        assert _same_bits(_host(lm.regressBackward(put(g), want=("joints",))["joints"]), wj)
        # accumulate: the finished sum is added
        rng = np.random.default_rng(n)
        bv, bj = rng.normal(size=wv.shape).astype(np.float32), rng.normal(size=wj.shape).astype(np.float32)
        out = {"verts": put(bv.copy()), "joints": put(bj.copy())}
        assert lm.regressBackward(put(g), out=out) is not None
        assert _same_bits(_host(out["verts"]), bv + wv) and _same_bits(_host(out["joints"]), bj + wj)
        only = {"joints": put(bj.copy())}
        lm.regressBackward(put(g), out=only)
        assert _same_bits(_host(only["joints"]), bj + wj)
    assert np.abs(wv).max() > 0 and np.abs(wj).max() > 0
    for k in {0, n // 2, n - 1}:
        r = lm.regressBackward(g[k:k + 1])
        assert _same_bits(r["verts"][0], wv[k]) and _same_bits(r["joints"][0], wj[k])


def test_landmark_bits_on_the_synthetic_model(synth):
    from smplpp_amd import model_io

    s, lm, reg, n = synth["s"], synth["lm"], synth["reg"], 16
    beta, theta = model_io.synthetic_inputs(n, seed=73)
    fk = s.launch(beta, theta, want=("verts", "joints"))
    want = KP.landmarks(reg, fk["verts"], fk["joints"])
    got = lm.regress(fk["verts"], fk["joints"])
    assert _same_bits(got, want) and _same_bits(got[:, :24], fk["joints"])
    assert _rel(got[:, 24:48], fk["joints"]) > 0  # (the regressed joints of the POSED vertices are other points)
    assert _same_bits(lm.regress(_dev(fk["verts"]), _dev(fk["joints"])).cpu().numpy(), want)
    g = np.random.default_rng(74).normal(size=(n, 53, 3)).astype(np.float32)
    wv, wj = KP.landmarks_vjp(reg, g, s.vertex_num)
    for put in (lambda a: a, _dev):
        r = lm.regressBackward(put(g))
        assert _same_bits(_host(r["verts"]), wv) and _same_bits(_host(r["joints"]), wj)
    untouched = np.setdiff1d(np.arange(s.vertex_num), reg[1])  # sources no row names get 0
    assert len(untouched) > 6000 and (wv[:, untouched] == 0).all() and np.abs(wv).max() > 0


def test_from_dense(tiny):
    from smplpp_amd.landmarks import Landmarks

    rng = np.random.default_rng(75)
    Av = np.where(rng.random((4, TINY_V)) < 0.1, rng.normal(size=(4, TINY_V)), 0).astype(np.float32)
    Aj = np.where(rng.random((4, 24)) < 0.2, rng.normal(size=(4, 24)), 0).astype(np.float32)
    lm = Landmarks.from_dense(tiny["s"], Av, Aj)
    rows = [[(c, A[c]) for c in np.nonzero(A)[0]] for A in np.concatenate([Av, Aj], 1)]
    assert lm.info()["nnz"] == sum(len(r) for r in rows)
    v, j = tiny["verts"][:3], tiny["joints"][:3]
    assert _same_bits(lm.regress(v, j), KP.landmarks(KP.csr(rows), v, j))
    assert Landmarks.from_dense(tiny["s"], Av).info()["nnz"] == int((Av != 0).sum())


# ---------------------------------------------------------------------------------------------------- 2. projection bits
@pytest.fixture(scope="module")
def scenes():
    """(K, n) -> the scene and, per rho, the restatement's results; computed once."""
    out = {}
    for K in (1, 63, 64, 65, 200):
        for n in (1, 5):
            sc = KP.scene(n, K, seed=100 * K + n, bad=2)
            P, cam, T, guv, ge = (sc[k] for k in ("points", "camera", "target", "grad_uv", "grad_energy"))
            for rho in (0.0, 100.0):
                sc[rho] = dict(fwd=KP.project(P, cam, NEAR, T, rho), bwd=KP.project_vjp(P, cam, NEAR, T, rho, guv, ge))
            sc["uv_only"] = KP.project_vjp(P, cam, NEAR, None, 0.0, guv, None)
            out[K, n] = sc
    return out


@pytest.mark.parametrize("rho", [0.0, 100.0])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 200])
def test_projection_bits(scenes, K, n, rho):
    from smplpp_amd import smpl as S

    sc = scenes[K, n]
    P, cam, T, guv, ge = (sc[k] for k in ("points", "camera", "target", "grad_uv", "grad_energy"))
    (wuv, we, wvalid), (wgp, wgc) = sc[rho]["fwd"], sc[rho]["bwd"]
    if K > 8:  # behind the camera, exactly at near (frame 0), NaN; a NaN target under confidence 0
        assert not wvalid[:, 0].any() and not wvalid[0, 1] and not wvalid[:, 2].any() and wvalid[:, 3:].all()
        # (point 4: a NaN target under a live confidence, so a NaN energy, and a cotangent of exactly 0, so no NaN in any gradient)
        assert np.isnan(we[:, 4]).all() and np.isfinite(np.delete(we, 4, axis=1)).all() and (we[:, 3] == 0).all()
        assert np.isfinite(wgp).all() and np.isfinite(wgc).all()
    for put in (lambda a: a, _dev):
        r = S.project_points(put(P), put(cam), put(T), rho, NEAR)
        assert _same_bits(_host(r["uv"]), wuv) and _same_energy(_host(r["energy"]), we) and _same_bits(_host(r["valid"]), wvalid)
        r = S.project_points(put(P), put(cam), near=NEAR, want=("uv",))  # without a target
        assert list(r) == ["uv"] and _same_bits(_host(r["uv"]), wuv)
        g = S.project_points_backward(put(P), put(cam), put(T), rho, put(guv), put(ge), NEAR)
        assert _same_bits(_host(g["points"]), wgp), int((_host(g["points"]) != wgp).sum())
        assert _same_bits(_host(g["camera"]), wgc), (_host(g["camera"]) - wgc)
        # each output alone (grad_points alone runs the per-point kernel)
        assert _same_bits(_host(S.project_points_backward(put(P), put(cam), put(T), rho, put(guv), put(ge), NEAR, want=("points",))["points"]), wgp)
        assert _same_bits(_host(S.project_points_backward(put(P), put(cam), put(T), rho, put(guv), put(ge), NEAR, want=("camera",))["camera"]), wgc)
        # target = NULL with grad_uv only
        g = S.project_points_backward(put(P), put(cam), None, rho, put(guv), None, NEAR)
        assert _same_bits(_host(g["points"]), sc["uv_only"][0]) and _same_bits(_host(g["camera"]), sc["uv_only"][1])
        # accumulate
        rng = np.random.default_rng(K + n)
        bp, bc = rng.normal(size=wgp.shape).astype(np.float32), rng.normal(size=wgc.shape).astype(np.float32)
        out = {"points": put(bp.copy()), "camera": put(bc.copy())}
        S.project_points_backward(put(P), put(cam), put(T), rho, put(guv), put(ge), NEAR, out=out)
        assert _same_bits(_host(out["points"]), bp + wgp) and _same_bits(_host(out["camera"]), bc + wgc)
    for k in {0, n // 2, n - 1}:  # a frame alone
        r = S.project_points(P[k:k + 1], cam[k:k + 1], T[k:k + 1], rho, NEAR)
        assert _same_bits(r["uv"][0], wuv[k]) and _same_energy(r["energy"][0], we[k]) and _same_bits(r["valid"][0], wvalid[k])
        g = S.project_points_backward(_dev(P[k:k + 1]), _dev(cam[k:k + 1]), _dev(T[k:k + 1]), rho, _dev(guv[k:k + 1]), _dev(ge[k:k + 1]), NEAR)
        assert _same_bits(_host(g["points"])[0], wgp[k]) and _same_bits(_host(g["camera"])[0], wgc[k])


# ---------------------------------------------------------------------------------------------------- 3. gradients
def _bar(got, want64, fp32, what):
    err, ref = _rel(_host(got), want64), _rel(fp32, want64)
    print("%s: rel %.3g, fp32 autograd %.3g" % (what, err, ref))
    assert np.abs(want64).max() > 0 and err <= max(4 * ref, 1e-5), (what, err, ref)


def _camera_rows(n, rng, distance=4.0):
    """n cameras `distance` in front of the origin, y down, each turned a little."""
    cam = np.empty((n, 16), np.float32)
    for f in range(n):
        a = rng.normal(0, 0.2)
        c, s = np.cos(a), np.sin(a)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([1.0, -1.0, -1.0])
        cam[f] = np.concatenate([R.reshape(9), [0.02 * f, -0.03, distance], [500.0, 490.0, 320.0, 240.0]])
    return cam


@pytest.mark.parametrize("rho", [0.0, 100.0])
def test_chain_to_pose_shape_and_camera(tiny, rho):
    """theta, beta -> smplpp_fk -> landmarks -> projection -> sum of energies through the autograd wrappers, and the gradient to all 16
    camera entries, against float64 autograd of the restated graph, within max(4 x fp32 autograd's error, 1e-5)."""
    from smplpp_amd import model_io
    from smplpp_amd import smpl as S

    from smplpp_amd.landmarks import Landmarks

    s, n = tiny["s"], 3
    # the 11 rows with their weights scaled to sum |w| = 1, so that every landmark stays within the body's extent, in front of the camera
    row_ptr, col, val = tiny["reg"]
    norm = np.maximum(np.add.reduceat(np.abs(np.append(val, 0)), row_ptr[:-1]) * (np.diff(row_ptr) > 0), 1e-30)
    reg = (row_ptr, col, (val / np.repeat(norm, np.diff(row_ptr))).astype(np.float32))
    lm = Landmarks(s, *reg)
    rng = np.random.default_rng(81)
    beta, theta = model_io.synthetic_inputs(n, seed=82)
    cam = _camera_rows(n, rng)
    fk = s.launch(beta, theta, want=("verts", "joints"))
    uv0, _, ok = KP.project(KP.landmarks(reg, fk["verts"], fk["joints"]), cam, NEAR)
    assert ok.all()
    T = np.concatenate([uv0 + rng.normal(0, 20.0, uv0.shape), rng.uniform(0.2, 1.0, uv0.shape[:2] + (1,))], -1).astype(np.float32)
    T[:, 4, 2] = 0.0
    b, t, c = (torch.from_numpy(x).cuda().requires_grad_(True) for x in (beta, theta, cam))
    verts, joints = s.forward_differentiable(b, t)
    uv, e, valid = S.project_points_differentiable(lm.forward_differentiable(verts, joints), c, _dev(T), rho, NEAR)
    assert valid.dtype == torch.bool and bool(valid.all())
    e.sum().backward()

    def ref(dtype):
        m = FK.model_tensors(tiny["model"], dtype)
        bb, th, cc = (torch.tensor(x, dtype=dtype, requires_grad=True) for x in (beta, theta, cam))
        out = FK.fk(m, bb, th)
        pts = KP.landmarks_t(torch.tensor(KP.dense(reg, TINY_V + 24), dtype=dtype), out["verts"], out["joints"])
        uvr, vr = KP.project_t(pts, cc, NEAR)
        er = KP.energy_t(uvr, vr, torch.tensor(T, dtype=dtype), rho)
        er.sum().backward()
        return [x.detach().double().numpy() for x in (er, bb.grad, th.grad, cc.grad)]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert _rel(_host(e.detach()), r64[0]) < 1e-4
    _bar(b.grad, r64[1], r32[1], "chain beta")
    _bar(t.grad, r64[2], r32[2], "chain theta")
    for name, sl in (("R", slice(0, 9)), ("t", slice(9, 12)), ("f", slice(12, 14)), ("c", slice(14, 16))):
        _bar(c.grad[:, sl], r64[3][:, sl], r32[3][:, sl], "chain camera " + name)


# ---------------------------------------------------------------------------------------------------- 4. a fit
FIT_STEPS, FIT_LR, FIT_RHO = 100, 0.02, 100.0


def _fit(energy_and_uv, theta0, t0, target_uv, dev):
    """Stage 1: FIT_STEPS Adam steps on the camera translation alone; stage 2: FIT_STEPS Adam steps on theta; the loss is the mean
    energy.  Returns the mean reprojection error in pixels before, between and after."""
    theta = theta0.clone().to(dev).requires_grad_(True)
    t = t0.clone().to(dev).requires_grad_(True)
    errors = []

    def error():
        with torch.no_grad():
            _, uv = energy_and_uv(theta, t)
            return float((uv - target_uv).norm(dim=-1).mean())

    errors.append(error())
    for params in ([t], [theta]):
        opt = torch.optim.Adam(params, lr=FIT_LR)
        for _ in range(FIT_STEPS):
            opt.zero_grad()
            e, _ = energy_and_uv(theta, t)
            e.mean().backward()
            opt.step()
        errors.append(error())
    return errors


def test_fit_camera_then_pose(synth, synth_model):
    """n = 2 on the synthetic model with the 53-row regressor: targets from a known theta and camera; from theta = 0 and the camera
    0.5 m off, Adam on the camera translation through grad_camera, then on theta.  The identical schedule runs on the float64
    restatement on the CPU; the GPU run's final mean reprojection error must fall and be within 2 x of that run's."""
    from smplpp_amd import smpl as S

    s, lm, reg, n = synth["s"], synth["lm"], synth["reg"], 2
    V = s.vertex_num
    rng = np.random.default_rng(91)
    theta_true = np.zeros((n, 25, 3), np.float32)
    theta_true[:, 1:] = rng.normal(0, 0.2, (n, 24, 3))
    t_true = np.array([[0.0, -0.36, 2.5], [0.05, -0.3, 2.6]], np.float32)
    fixed = np.concatenate([np.diag([1.0, -1.0, -1.0]).reshape(9), [500.0, 500.0, 320.0, 240.0]]).astype(np.float32)
    t0 = torch.from_numpy(t_true + np.array([0.3, 0.0, 0.4], np.float32))
    theta0 = torch.zeros(n, 25, 3)
    beta = np.zeros((n, 10), np.float32)

    # the float64 restatement on the vertices the regressor reads (its own picks and the joint regressor's columns): the same numbers
    # as on the whole body, a tenth of the work
    used = np.unique(np.concatenate([reg[1][reg[1] < V], np.nonzero(np.abs(synth_model["joint_regressor"]).sum(0))[0]]))
    sub = {k: synth_model[k][used] for k in ("vertices_template", "shape_blend_shapes", "pose_blend_shapes", "weights")}
    sub["joint_regressor"], sub["kinematic_tree"] = synth_model["joint_regressor"][:, used], synth_model["kinematic_tree"]
    m64 = FK.model_tensors(sub, torch.float64)
    A64 = torch.tensor(np.concatenate([KP.dense(reg, V + 24)[:, used], KP.dense(reg, V + 24)[:, V:]], 1))
    fixed64, beta64 = torch.tensor(fixed, dtype=torch.float64), torch.tensor(beta, dtype=torch.float64)

    def camera(t, fx):
        return torch.cat([fx[:9].expand(n, 9), t, fx[9:].expand(n, 4)], 1)

    def uv64(theta, t):
        out = FK.fk(m64, beta64, theta)
        return KP.project_t(KP.landmarks_t(A64, out["verts"], out["joints"]), camera(t, fixed64), NEAR)

    with torch.no_grad():
        uv_true, ok = uv64(torch.tensor(theta_true, dtype=torch.float64), torch.tensor(t_true, dtype=torch.float64))
    assert bool(ok.all())
    target64 = torch.cat([uv_true, torch.ones(n, 53, 1, dtype=torch.float64)], -1)

    def cpu(theta, t):
        uv, valid = uv64(theta, t)
        return KP.energy_t(uv, valid, target64, FIT_RHO), uv

    dev = torch.device("cuda")
    target32, fixed32, beta32 = target64.float().to(dev), torch.from_numpy(fixed).to(dev), torch.from_numpy(beta).to(dev)

    def gpu(theta, t):
        verts, joints = s.forward_differentiable(beta32, theta)
        uv, e, _ = S.project_points_differentiable(lm.forward_differentiable(verts, joints), camera(t, fixed32), target32, FIT_RHO, NEAR)
        return e, uv

    ref = _fit(cpu, theta0.double(), t0.double(), uv_true, torch.device("cpu"))
    got = _fit(gpu, theta0, t0, target32[..., :2], dev)
    print("keypoint fit, mean reprojection error in px (start, after the camera stage, after the pose stage): GPU %s, float64 CPU %s" %
          (["%.4g" % x for x in got], ["%.4g" % x for x in ref]))
    assert ref[2] < ref[1] < ref[0] and got[2] < got[1] < got[0]
    assert got[2] <= 2 * ref[2], (got, ref)


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals(tiny):
    from smplpp_amd import _lib

    L = _lib.load()
    s, lm = tiny["s"], tiny["lm"]
    S_ = TINY_V + 24
    i64 = lambda a: np.ascontiguousarray(a, np.int64)  # noqa: E731
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def create(Lr, row_ptr, col, val):
        h = C.c_void_p(7)
        rp, cl, vl = i64(row_ptr), i64(col), np.ascontiguousarray(val, np.float32)
        rc = L.smplpp_landmarks_create(s.handle, Lr, p(rp), p(cl), p(vl), C.byref(h))
        if rc == 0:
            L.smplpp_landmarks_destroy(h)
        else:
            assert h.value is None  # *out = NULL
        return rc

    assert create(2, [0, 1, 2], [0, S_ - 1], [1, 1]) == 0
    assert create(0, [0], [], []) == 1 and create(65536, np.zeros(65537), [], []) == 1
    assert create(2, [1, 1, 2], [0, 1], [1, 1]) == 1 and create(2, [0, 2, 1], [0, 1], [1, 1]) == 1
    assert create(2, [0, 1, 2], [0, S_], [1, 1]) == 1 and create(2, [0, 1, 2], [-1, 0], [1, 1]) == 1
    assert create(2, [0, 1, 2], [0, 1], [1, np.inf]) == 1 and create(2, [0, 1, 2], [0, 1], [np.nan, 1]) == 1
    assert create(1, [0, 2 ** 31], [0], [1]) == 1  # nnz beyond int32: refused before col is read

    n = 2
    v, j, g = tiny["verts"][:n].copy(), tiny["joints"][:n].copy(), tiny["g"][:n].copy()
    pts = np.full((n, 11, 3), 7.0, np.float32)
    gv, gj = np.full((n, TINY_V, 3), 7.0, np.float32), np.full((n, 24, 3), 7.0, np.float32)
    fwd = lambda nn=n, vv=v, jj=j, oo=pts, space=0: L.smplpp_landmarks(lm.handle, nn, p(vv), p(jj), p(oo), space, None)  # noqa: E731
    bwd = lambda nn=n, gg=g, a=gv, b=gj, acc=0, space=0: L.smplpp_landmarks_vjp(lm.handle, nn, p(gg), p(a), p(b), acc, space, None)  # noqa: E731
    big = 2 ** 31 // S_ + 1  # n (V + 24) beyond int32
    assert fwd(nn=0) == 1 and fwd(nn=big) == 1 and fwd(vv=None) == 1 and fwd(jj=None) == 1 and fwd(oo=None) == 1 and fwd(space=2) == 1
    assert bwd(nn=0) == 1 and bwd(nn=big) == 1 and bwd(gg=None) == 1 and bwd(a=None, b=None) == 1 and bwd(acc=2) == 1 and bwd(acc=-1) == 1
    assert bwd(space=3) == 1
    assert (pts == 7).all() and (gv == 7).all() and (gj == 7).all()
    assert fwd() == 0 and bwd() == 0 and bwd(a=None) == 0 and bwd(b=None) == 0 and (pts != 7).any()

    K = 11
    sc = KP.scene(n, K, seed=5)
    P, cam, T, guv, ge = (sc[k] for k in ("points", "camera", "target", "grad_uv", "grad_energy"))
    uv, e, valid = np.full((n, K, 2), 7.0, np.float32), np.full((n, K), 7.0, np.float32), np.full((n, K), 7, np.uint8)
    gp, gc = np.full((n, K, 3), 7.0, np.float32), np.full((n, 16), 7.0, np.float32)

    def proj(nn=n, KK=K, pp=P, cc=cam, near=NEAR, tt=T, rho=100.0, o=(uv, e, valid), space=0):
        return L.smplpp_project_points(0, nn, KK, p(pp), p(cc), near, p(tt), rho, p(o[0]), p(o[1]), p(o[2]), space, None)

    def back(nn=n, KK=K, pp=P, cc=cam, near=NEAR, tt=T, rho=100.0, gu=guv, gE=ge, o=(gp, gc), acc=0, space=0):
        return L.smplpp_project_points_vjp(0, nn, KK, p(pp), p(cc), near, p(tt), rho, p(gu), p(gE), p(o[0]), p(o[1]), acc, space, None)

    for call in (proj, back):
        assert call(rho=-1.0) == 1 and call(rho=np.inf) == 1 and call(rho=np.nan) == 1
        assert call(near=0.0) == 1 and call(near=np.nan) == 1
        assert call(nn=0) == 1 and call(KK=0) == 1 and call(nn=2 ** 20, KK=2 ** 10) == 1  # n K 3 beyond int32
        assert call(pp=None) == 1 and call(cc=None) == 1 and call(tt=None) == 1  # energy / grad_energy needs target
        assert call(o=(None,) * (3 if call is proj else 2)) == 1 and call(space=2) == 1
    assert back(acc=2) == 1 and back(gu=None, gE=None) == 1
    assert (uv == 7).all() and (e == 7).all() and (valid == 7).all() and (gp == 7).all() and (gc == 7).all()
    assert proj() == 0 and back() == 0 and proj(tt=None, o=(uv, None, valid)) == 0 and back(tt=None, gE=None) == 0
    assert proj(rho=0.0) == 0 and back(o=(None, gc)) == 0 and back(o=(gp, None)) == 0
    assert (uv != 7).any() and (gc != 7).all()


# ---------------------------------------------------------------------------------------------------- 6. C++ shim
def test_landmarks_cpp_shim(tmp_path):
    from smplpp_amd import model_io
    from smplpp_amd import smpl as S
    from smplpp_amd.landmarks import Landmarks

    exe = str(tmp_path / "landmarks_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "landmarks_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    n, Lr, V = 3, 6, 40
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    s = _smpl(model)
    fk = s.launch(beta, theta, want=("verts", "joints"))
    rows = [[(V + 3, 1.0)], [(7, 1.0)]]
    rows += [[((l * 7 + i * 5) % (V + 24), np.float32(i % 4 + 1) * np.float32(0.125) - np.float32(0.2)) for i in range(9)] for l in range(2, Lr)]
    reg = KP.csr(rows)
    lm = Landmarks(s, *reg)
    points = lm.regress(fk["verts"], fk["joints"])
    assert _same_bits(points, KP.landmarks(reg, fk["verts"], fk["joints"]))
    cam = np.array([1, 0, 0, 0, -1, 0, 0, 0, -1, 0, 0, 3, 300, 300, 160, 120], np.float32)
    i = np.arange(n * Lr)
    T = np.stack([160 + (i % 7) * 3, 120 - (i % 5) * 4, (i % 3) * 0.5], -1).astype(np.float32).reshape(n, Lr, 3)
    ge = ((i % 4) * np.float32(0.25)).astype(np.float32).reshape(n, Lr)
    guv = ((np.arange(n * Lr * 2) % 5 - 2) * np.float32(0.5)).astype(np.float32).reshape(n, Lr, 2)
    p = S.project_points(points, cam, T, 100.0)
    g = S.project_points_backward(points, cam, T, 100.0, guv, ge)
    acc = S.project_points_backward(points, cam, T, 100.0, guv, ge, out={"camera": np.ones((n, 16), np.float32)})
    back = lm.regressBackward(g["points"])
    assert p["valid"].all() and np.abs(p["energy"]).max() > 0 and np.abs(back["verts"]).max() > 0
    want = [points, p["uv"], p["energy"], p["valid"].astype(np.float32), g["points"], g["camera"], acc["camera"], back["verts"], back["joints"]]
    assert len(raw) == 4 * sum(w.size for w in want)
    off = 0
    for k, w in enumerate(want):
        got = np.frombuffer(raw, np.float32, w.size, off).reshape(w.shape)
        off += 4 * w.size
        assert _same_bits(got, w), k
