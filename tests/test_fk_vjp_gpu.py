"""smplpp_fk_vjp on the MI355X: dense parity with float64 autograd of the torch restatement (tests/fk_vjp_oracle.py), the
reference's own autograd Jacobian (when the reference build exists), model variety, call semantics, torch.autograd end to end and
the C++ shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as O  # noqa: E402
from vjp_blocks import eight_weights as _eight_weights  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _smpl(model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    return s


@pytest.fixture(scope="module")
def smpl(synth_model):
    return _smpl(synth_model)


@pytest.fixture(scope="module")
def m64(synth_model):
    return O.model_tensors(synth_model)


def _inputs(n, seed):
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(n, seed=seed)
    rng = np.random.default_rng(seed + 100)
    theta[0, 3] = 0.0  # theta = 0 rows
    if n > 2:
        theta[2, 1:] = 0.0
    # |theta| = pi rows
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    theta[n - 1, 7] = (np.pi * ax[n - 1]).astype(np.float32)
    if n > 3:
        theta[1, 2:5] = (np.pi * ax[1]).astype(np.float32)
    return beta, theta


def _grads(V, n, seed, kind):
    rng = np.random.default_rng(seed)
    gv = rng.standard_normal((n, V, 3)).astype(np.float32) if kind in ("verts", "both") else None
    gj = rng.standard_normal((n, 24, 3)).astype(np.float32) if kind in ("joints", "both") else None
    return gv, gj


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30)


def _check_frames(m64, beta, theta, gv, gj, out, frames):
    for f in frames:
        sl = slice(f, f + 1)
        a = gv[sl] if gv is not None else None
        b = gj[sl] if gj is not None else None
        gb64, gt64 = O.vjp(m64, beta[sl], theta[sl], a, b)
        gb32, gt32 = O.vjp(m64, beta[sl], theta[sl], a, b, dtype=O.torch.float32)
        for name, got, ref, f32 in (("beta", out["beta"][sl], gb64, gb32), ("theta", out["theta"][sl], gt64, gt32)):
            assert np.isfinite(got).all(), (f, name)
            bar = max(4 * _rel(f32, ref), 1e-5)
            err = _rel(got.astype(np.float64), ref)
            assert err <= bar, (f, name, err, bar)


@pytest.mark.parametrize("n", [1, 7, 64, 65, 1024])
@pytest.mark.parametrize("kind", ["verts", "joints", "both"])
def test_vjp_dense_parity(smpl, m64, n, kind):
    beta, theta = _inputs(n, seed=n)
    gv, gj = _grads(smpl.vertex_num, n, seed=7 * n, kind=kind)
    rest = smpl.launch(beta, theta, want=("rest",))["rest"]
    out = smpl.launchBackward(beta, theta, grad_verts=gv, grad_joints=gj, rest=rest)
    assert np.isfinite(out["beta"]).all() and np.isfinite(out["theta"]).all()
    frames = sorted(set([0, 1, 2, n // 2, n - 1] + list(range(0, n, max(1, n // 8)))))
    _check_frames(m64, beta, theta, gv, gj, out, [f for f in frames if f < n])


def test_vjp_pinned_to_reference_autograd(synth_model, smpl):
    from oracle import ref

    if not ref.available():
        pytest.skip("reference build (oracle/_ref) not present")
    from smplpp_amd.ik import reference_task_faces

    K = 6
    _, faces = reference_task_faces(K)
    faces = np.asarray(faces, np.int64)
    rm = ref.RefModel(synth_model)
    F = np.asarray(synth_model["face_indices"], np.int64) - 1
    rng = np.random.default_rng(3)
    beta, theta = _inputs(3, seed=11)
    for f in range(3):
        bary = rng.dirichlet(np.ones(3), size=K).astype(np.float32)
        r = rm.ik_eval(beta[f], theta[f], faces, np.zeros((K, 3), np.float32), np.tile([0, 0, 1.0], (K, 1)).astype(np.float32),
                       np.ones(K), np.zeros(K), np.zeros(K), np.zeros(K), bary, optimize_beta=True)
        vw = r["vertex_weights"]
        u = rng.standard_normal((K, 3))
        gv = np.zeros((1, smpl.vertex_num, 3), np.float64)
        for k in range(K):
            for c in range(3):
                gv[0, F[faces[k], c]] += u[k] * vw[k, c]
        J = r["J"]
        D = J.shape[1]
        want = np.zeros(D)
        for k in range(K):
            want += u[k] @ J[4 * k:4 * k + 3]
        out = smpl.launchBackward(beta[f:f + 1], theta[f:f + 1], grad_verts=gv.astype(np.float32))
        gt, gb = want[:75], want[D - 10:]
        assert _rel(out["theta"].reshape(-1).astype(np.float64), gt) < 1e-4, f
        assert _rel(out["beta"].reshape(-1).astype(np.float64), gb) < 1e-4, f


@pytest.mark.parametrize("form", ["e", "h", "b"])
@pytest.mark.parametrize("which", ["tiny", "eight", "synth"])
def test_vjp_model_variety(synth_model, form, which, monkeypatch):
    from smplpp_amd import model_io

    monkeypatch.setenv("SMPLPP_SKIN", form)
    model = {"tiny": lambda: model_io.tiny_model(61, seed=7), "eight": lambda: _eight_weights(synth_model),
             "synth": lambda: synth_model}[which]()
    s = _smpl(model)
    assert s.info()["weights_per_vertex"] == {"tiny": 24, "eight": 8, "synth": 4}[which]
    n = 37
    beta, theta = _inputs(n, seed=5)
    gv, gj = _grads(s.vertex_num, n, seed=9, kind="both")
    rest = s.launch(beta, theta, want=("rest",))["rest"]
    a = s.launchBackward(beta, theta, grad_verts=gv, grad_joints=gj, rest=rest)
    b = s.launchBackward(beta, theta, grad_verts=gv, grad_joints=gj)
    for k in ("beta", "theta"):
        assert np.isfinite(a[k]).all()
        assert _rel(b[k].astype(np.float64), a[k].astype(np.float64)) < 1e-5, k
    _check_frames(O.model_tensors(model), beta, theta, gv, gj, a, [0, 1, 2, 18, n - 1])


def test_vjp_call_semantics(smpl):
    import torch

    n = 65
    beta, theta = _inputs(n, seed=21)
    gv, gj = _grads(smpl.vertex_num, n, seed=4, kind="both")
    ref_fk = smpl.launch(beta, theta)
    ref_fk = {k: v.copy() for k, v in ref_fk.items()}
    h1 = smpl.launchBackward(beta, theta, grad_verts=gv, grad_joints=gj, rest=ref_fk["rest"])
    h2 = smpl.launchBackward(beta, theta, grad_verts=gv, grad_joints=gj, rest=ref_fk["rest"])
    for k in ("beta", "theta"):
        assert np.array_equal(h1[k], h2[k]), k  # deterministic
    hn = smpl.launchBackward(beta, theta, grad_verts=gv, grad_joints=gj)
    for k in ("beta", "theta"):
        assert _rel(hn[k].astype(np.float64), h1[k].astype(np.float64)) < 1e-5, k
    # device space == host space
    dev = lambda a: torch.from_numpy(a).cuda()
    d = smpl.launchBackward(dev(beta), dev(theta), grad_verts=dev(gv), grad_joints=dev(gj), rest=dev(ref_fk["rest"]))
    torch.cuda.synchronize()
    for k in ("beta", "theta"):
        assert np.array_equal(d[k].cpu().numpy(), h1[k]), k
    # zero gradients -> exact zeros
    z = smpl.launchBackward(beta, theta, grad_verts=np.zeros_like(gv), grad_joints=np.zeros_like(gj), rest=ref_fk["rest"])
    assert not z["beta"].any() and not z["theta"].any()
    z = smpl.launchBackward(beta, theta)
    assert not z["beta"].any() and not z["theta"].any()
    # NULL outputs
    from smplpp_amd import _lib

    L = _lib.load()
    gb = np.empty((n, 10), np.float32)
    _lib.check(L.smplpp_fk_vjp(smpl.handle, n, beta.ctypes.data, theta.ctypes.data, None, gv.ctypes.data, None, gb.ctypes.data, None,
                               _lib.HOST, None))
    ref_b = smpl.launchBackward(beta, theta, grad_verts=gv)["beta"]
    assert np.array_equal(gb, ref_b)
    gt = np.empty((n, 25, 3), np.float32)
    _lib.check(L.smplpp_fk_vjp(smpl.handle, n, beta.ctypes.data, theta.ctypes.data, None, None, gj.ctypes.data, None, gt.ctypes.data,
                               _lib.HOST, None))
    assert np.array_equal(gt, smpl.launchBackward(beta, theta, grad_joints=gj)["theta"])
    _lib.check(L.smplpp_fk_vjp(smpl.handle, n, beta.ctypes.data, theta.ctypes.data, None, gv.ctypes.data, None, None, None, _lib.HOST,
                               None))
    # the forward after a backward (rest = NULL recomputation included) returns the same bits
    again = smpl.launch(beta, theta)
    for k in ("verts", "rest", "joints", "xforms"):
        assert np.array_equal(again[k], ref_fk[k]), k


def test_vjp_autograd_matches_launch_backward(smpl):
    import torch

    n = 33
    beta, theta = _inputs(n, seed=8)
    gv, gj = _grads(smpl.vertex_num, n, seed=2, kind="both")
    b = torch.from_numpy(beta).cuda().requires_grad_(True)
    t = torch.from_numpy(theta).cuda().requires_grad_(True)
    verts, joints = smpl.forward_differentiable(b, t)
    gvt, gjt = torch.from_numpy(gv).cuda(), torch.from_numpy(gj).cuda()
    db, dt = torch.autograd.grad((verts * gvt).sum() + (joints * gjt).sum(), (b, t))
    ref = smpl.launchBackward(b.detach(), t.detach(), grad_verts=gvt, grad_joints=gjt)
    assert torch.equal(db, ref["beta"]) and torch.equal(dt, ref["theta"])
    # a loss on the vertices only: the joints' gradient arrives as None / zeros
    verts, joints = smpl.forward_differentiable(b, t)
    db2, dt2 = torch.autograd.grad((verts * gvt).sum(), (b, t))
    ref2 = smpl.launchBackward(b.detach(), t.detach(), grad_verts=gvt)
    assert torch.equal(db2, ref2["beta"]) and torch.equal(dt2, ref2["theta"])
    verts, joints = smpl.forward_differentiable(b, t)
    db3, = torch.autograd.grad((joints * gjt).sum(), (b,))
    assert torch.equal(db3, smpl.launchBackward(b.detach(), t.detach(), grad_joints=gjt)["beta"])


def test_vjp_adam_fit_recovers_target(smpl):
    import torch

    n = 256
    rng = np.random.default_rng(12)
    beta_t = (rng.standard_normal((n, 10)) * 0.5).astype(np.float32)
    theta_t = np.zeros((n, 25, 3), np.float32)
    theta_t[:, 1:] = rng.standard_normal((n, 24, 3)) * 0.2
    theta_t[:, 0] = rng.uniform(-0.5, 0.5, (n, 3))
    target = torch.from_numpy(smpl.launch(beta_t, theta_t, want=("verts",))["verts"]).cuda()
    b = torch.from_numpy(beta_t + 0.1 * rng.standard_normal((n, 10)).astype(np.float32)).cuda().requires_grad_(True)
    t = torch.from_numpy(theta_t + 0.02 * rng.standard_normal((n, 25, 3)).astype(np.float32)).cuda().requires_grad_(True)
    opt = torch.optim.Adam([b, t], lr=0.01)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 200, eta_min=1e-4)
    for _ in range(200):
        opt.zero_grad()
        verts, _ = smpl.forward_differentiable(b, t)
        loss = ((verts - target) ** 2).sum(-1).mean(-1).sum()
        loss.backward()
        opt.step()
        sched.step()
    with torch.no_grad():
        verts, _ = smpl.forward_differentiable(b, t)
        err = float((verts - target).norm(dim=-1).mean())
    assert err < 1e-3, err


def test_vjp_cpp_shim(tmp_path):
    import __graft_entry__ as g
    from smplpp_amd import model_io

    g.build()
    exe = str(tmp_path / "fk_vjp_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fk_vjp_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=3)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stdout
    vals = {}
    for line in out.stdout.splitlines():
        k, *v = line.split()
        vals[k] = np.array([float(x) for x in v], np.float32)
    # the program's inputs, restated
    n, V = 2, 40
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    gv = ((np.arange(n * V * 3, dtype=np.float32).reshape(n, V, 3) % 13) - 6) * np.float32(0.1)
    gj = ((np.arange(n * 72, dtype=np.float32).reshape(n, 24, 3) % 5) - 2) * np.float32(0.1)
    s = _smpl(model)
    rest = s.launch(beta, theta, want=("rest",))["rest"]
    ref = s.launchBackward(beta, theta, grad_verts=gv, grad_joints=gj, rest=rest)
    assert np.array_equal(vals["GRAD_BETA"], ref["beta"].ravel())
    assert np.array_equal(vals["GRAD_THETA"], ref["theta"].ravel())
