"""smplpp_vposer_vjp on the MI355X: parity with float64 autograd of the torch restatement of the decoder (tests/vposer_vjp_oracle.py)
and with J^T g from the Jacobian call, the axis-angle branch points, bits (the forward it differentiates, determinism, batch and
shard invariance), call semantics, torch.autograd through the decoder and through SMPL, a latent-space fit, and the C++ shim."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FO  # noqa: E402
import vposer_vjp_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def params():
    from smplpp_amd.ik import VPoserDecoder

    return VPoserDecoder.synthetic_params()


@pytest.fixture(scope="module")
def gpu(params):
    from smplpp_amd.ik import VPoserDecoder

    return VPoserDecoder(params)


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30)


def _check_frames(params, z, g, gz, frames, floor=1e-5):
    """Per frame: the error against float64 autograd within max(4 x the error of an fp32 autograd of the same graph, floor)."""
    d64, d32 = O.decoder(params), O.decoder(params, torch.float32)
    for f in frames:
        sl = slice(f, f + 1)
        ref, _ = O.vjp(d64, z[sl], g[sl])
        r32, _ = O.vjp(d32, z[sl], g[sl], dtype=torch.float32)
        assert np.isfinite(gz[sl]).all(), f
        bar = max(4 * _rel(r32, ref), floor)
        err = _rel(gz[sl].astype(np.float64), ref)
        assert err <= bar, (f, err, bar)


@pytest.mark.parametrize("n", [1, 7, 64, 257, 513])
def test_vjp_parity(gpu, params, n):
    rng = np.random.default_rng(n)
    z = rng.normal(0, 1.0, (n, 32)).astype(np.float32)
    z[0] = 0.0
    g = rng.standard_normal((n, 21, 3)).astype(np.float32)
    gz = gpu.launchBackward(z, g)
    assert gz.shape == (n, 32) and gz.dtype == np.float32
    frames = sorted(set([0, n // 2, n - 1] + list(rng.integers(0, n, 3))))
    _check_frames(params, z, g, gz, frames)
    # J^T g from the existing Jacobian call (fp16x2 operands, 22 bits)
    _, jac = gpu.forward(z, want_jac=True)
    jtg = np.einsum("nrc,nr->nc", jac.astype(np.float64), g.reshape(n, 63).astype(np.float64))
    for f in range(n):
        assert _rel(gz[f].astype(np.float64), jtg[f]) < 2e-4, f


def _branch_point_decoder():
    """test_vposer_gpu.py::test_decoder_jacobian_is_finite_at_the_axis_angle_branch_points's construction: at z = 0 the 21 joints
    decode exactly to the identity (joint 0), pi about seven axes (1-7), 1e-4 / 1e-3 rad below pi about x, y, z (8-13), 1e-4 /
    1e-3 rad from the identity (14-19) and a generic rotation (20)."""
    from scipy.spatial.transform import Rotation
    from oracle import vposer_torch as VT
    from smplpp_amd.ik import VPoserDecoder

    axes = [np.array(a, np.float64) / np.linalg.norm(a) for a in
            ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, -2, 3], [0.3, 0.5, -0.8], [-1, 0.2, 0.1])]
    rots = [np.eye(3)]
    rots += [Rotation.from_rotvec(np.pi * a).as_matrix() for a in axes]
    rots += [Rotation.from_rotvec((np.pi - d) * a).as_matrix() for a in axes[:3] for d in (1e-4, 1e-3)]
    rots += [Rotation.from_rotvec(d * a).as_matrix() for a in axes[3:6] for d in (1e-4, 1e-3)]
    rots += [Rotation.from_rotvec(0.7 * axes[4]).as_matrix()]
    R = np.stack(rots)
    params = VPoserDecoder.synthetic_params(seed=8)
    params["decoder_net.5.weight"] = (params["decoder_net.5.weight"] * np.float32(0.05)).astype(np.float32)
    target = R[:, :, :2].reshape(-1).astype(np.float32)
    params["decoder_net.5.bias"] = np.zeros(126, np.float32)
    hidden0 = VT.VPoserDecoder(params).net(torch.zeros(1, 32)).detach().numpy()[0]
    params["decoder_net.5.bias"] = (target - hidden0).astype(np.float32)
    return params


def test_vjp_at_the_axis_angle_branch_points():
    """grad_z is finite with a gradient on every joint.  Against float64 autograd: with the gradient on the joints whose branch is
    decided robustly (the identity, near zero, the generic one) by the 4 x fp32 rule; on the joints 1e-4 / 1e-3 rad below pi, where
    sqrt(s + eps) multiplies the rounding of the decoder's output by ~1e3, within 1e-3.  Exactly pi (joints 1-7) is where one fp32
    ulp of the decode picks the sign of the axis (src/VPoser.cpp:62-103; see the forward's test): finiteness only."""
    from smplpp_amd.ik import VPoserDecoder

    params = _branch_point_decoder()
    gpu = VPoserDecoder(params)
    rng = np.random.default_rng(12)
    z = np.zeros((3, 32), np.float32)
    z[1] = rng.normal(0, 1e-3, 32)
    z[2] = rng.normal(0, 0.3, 32)
    g = rng.standard_normal((3, 21, 3)).astype(np.float32)
    gz = gpu.launchBackward(z, g)
    assert np.isfinite(gz).all()
    near0 = [0] + list(range(14, 21))
    g0 = np.zeros_like(g)
    g0[:, near0] = g[:, near0]
    _check_frames(params, z, g0, gpu.launchBackward(z, g0), range(3))
    gpi = np.zeros_like(g)
    gpi[:, 8:14] = g[:, 8:14]
    _check_frames(params, z[:2], gpi[:2], gpu.launchBackward(z[:2], gpi[:2]), range(2), floor=1e-3)


def test_vjp_bits(gpu):
    """`out` is smplpp_vposer_forward's (jac NULL) output bit for bit; two calls give the same bits; a frame's grad_z does not depend
    on the batch or shard it travels in; and a VJP call leaves the forward's bits (value and Jacobian paths) as they were."""
    rng = np.random.default_rng(21)
    n = 513
    z = rng.normal(0, 1.0, (n, 32)).astype(np.float32)
    g = rng.standard_normal((n, 21, 3)).astype(np.float32)
    val0 = gpu.forward(z)
    out0, jac0 = gpu.forward(z, want_jac=True)
    gz, out = gpu.launchBackward(z, g, want_out=True)
    assert np.array_equal(out, val0)
    gz2, out2 = gpu.launchBackward(z, g, want_out=True)
    assert np.array_equal(gz2, gz) and np.array_equal(out2, out)
    for lo, hi in [(0, 1), (5, 6), (0, 7), (1, 8), (128, 256), (129, 400), (255, 513), (512, 513)]:
        for base in (0, lo, lo + 3):
            part = gpu.launchBackward(z[lo:hi], g[lo:hi], frame_base=base)
            assert np.array_equal(part, gz[lo:hi]), (lo, hi, base)
    assert np.array_equal(gpu.forward(z), val0)
    out1, jac1 = gpu.forward(z, want_jac=True)
    assert np.array_equal(out1, out0) and np.array_equal(jac1, jac0)


def test_vjp_call_semantics(gpu):
    from smplpp_amd import _lib

    L = _lib.load()
    rng = np.random.default_rng(5)
    n = 9
    z = rng.normal(0, 1.0, (n, 32)).astype(np.float32)
    g = rng.standard_normal((n, 21, 3)).astype(np.float32)
    ref = gpu.launchBackward(z, g)
    gz = np.full((n, 32), 7.0, np.float32)
    p = lambda a: a.ctypes.data
    for args in [(None, n, 0, p(z), p(g), p(gz), None, 0, None), (gpu._h, 0, 0, p(z), p(g), p(gz), None, 0, None),
                 (gpu._h, -1, 0, p(z), p(g), p(gz), None, 0, None), (gpu._h, n, -1, p(z), p(g), p(gz), None, 0, None),
                 (gpu._h, n, 0, None, p(g), p(gz), None, 0, None), (gpu._h, n, 0, p(z), None, p(gz), None, 0, None),
                 (gpu._h, n, 0, p(z), p(g), None, None, 0, None), (gpu._h, n, 0, p(z), p(g), p(gz), None, 5, None)]:
        assert L.smplpp_vposer_vjp(*args) == 1, args
    assert (gz == 7.0).all()
    # host space overwrites grad_z
    assert L.smplpp_vposer_vjp(gpu._h, n, 0, p(z), p(g), p(gz), None, 0, None) == 0
    assert np.array_equal(gz, ref)
    # device space, on a stream that is not the default one
    zt, gt = torch.from_numpy(z).cuda(), torch.from_numpy(g).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gzt, outt = gpu.launchBackward(zt, gt, want_out=True)
    s.synchronize()
    assert np.array_equal(gzt.cpu().numpy(), ref)
    assert np.array_equal(outt.cpu().numpy(), gpu.forward(z))
    # raw device pointers on an explicit stream, into a pre-filled buffer
    gzd = torch.full((n, 32), float("nan"), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert L.smplpp_vposer_vjp(gpu._h, n, 0, zt.data_ptr(), gt.data_ptr(), gzd.data_ptr(), None, 1, C.c_void_p(s.cuda_stream)) == 0
    s.synchronize()
    assert np.array_equal(gzd.cpu().numpy(), ref)


def test_vjp_autograd_through_the_decoder(gpu):
    rng = np.random.default_rng(6)
    n = 40
    z = rng.normal(0, 1.0, (n, 32)).astype(np.float32)
    g = rng.standard_normal((n, 21, 3)).astype(np.float32)
    zt = torch.from_numpy(z).cuda().requires_grad_(True)
    gt = torch.from_numpy(g).cuda()
    out = gpu.forward_differentiable(zt)
    assert np.array_equal(out.detach().cpu().numpy(), gpu.forward(z))
    dz, = torch.autograd.grad((out * gt).sum(), zt)
    assert torch.equal(dz, gpu.launchBackward(zt.detach(), gt))


def test_vjp_autograd_through_smpl(gpu, params, synth_model):
    """q [n,44] -> theta_from_latent_layout -> SMPL.forward_differentiable: the gradient on q against float64 autograd of the
    decoder restatement spliced into tests/fk_vjp_oracle.py's SMPL, per frame by the 4 x fp32 rule."""
    from smplpp_amd.ik import theta_from_latent_layout
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    rng = np.random.default_rng(7)
    n = 3
    q = np.zeros((n, 44), np.float32)
    q[:, :3] = rng.normal(0, 0.1, (n, 3))
    q[:, 3:6] = rng.normal(0, 0.3, (n, 3))
    q[:, 6:38] = rng.normal(0, 0.7, (n, 32))
    q[:, 38:] = rng.normal(0, 0.2, (n, 6))
    beta = (rng.standard_normal((n, 10)) * 0.5).astype(np.float32)
    gv = rng.standard_normal((n, synth_model["vertices_template"].shape[0], 3)).astype(np.float32)
    gj = rng.standard_normal((n, 24, 3)).astype(np.float32)
    qt = torch.from_numpy(q).cuda().requires_grad_(True)
    theta = theta_from_latent_layout(gpu, qt)
    assert theta.shape == (n, 25, 3)
    verts, joints = s.forward_differentiable(torch.from_numpy(beta).cuda(), theta)
    dq, = torch.autograd.grad((verts * torch.from_numpy(gv).cuda()).sum() + (joints * torch.from_numpy(gj).cuda()).sum(), qt)
    dq = dq.cpu().numpy()

    def oracle(dtype, f):
        m = FO.model_tensors(synth_model, dtype)
        dec = O.decoder(params, dtype)
        qq = torch.as_tensor(q[f:f + 1], dtype=dtype).clone().requires_grad_(True)
        th = torch.cat([qq[:, :6].reshape(1, 2, 3), dec(qq[:, 6:38]), qq[:, 38:].reshape(1, 2, 3)], 1)
        o = FO.fk(m, torch.as_tensor(beta[f:f + 1], dtype=dtype), th)
        loss = (o["verts"] * torch.as_tensor(gv[f:f + 1], dtype=dtype)).sum() + (o["joints"] * torch.as_tensor(gj[f:f + 1], dtype=dtype)).sum()
        return torch.autograd.grad(loss, qq)[0].detach().numpy().astype(np.float64)

    for f in range(n):
        ref, r32 = oracle(torch.float64, f), oracle(torch.float32, f)
        bar = max(4 * _rel(r32, ref), 1e-5)
        err = _rel(dq[f:f + 1].astype(np.float64), ref)
        assert err <= bar, (f, err, bar)


def test_latent_fit_recovers_hidden_poses(gpu, synth_model):
    """Adam in the 44-d layout (the reference's capture configuration) on the synthetic decoder: hidden poses drawn in latent space
    as configs[4]'s latent tests draw them, a start near them, a loss on the posed mesh: the fit lands within 1e-3 m mean vertex
    error."""
    from smplpp_amd.ik import theta_from_latent_layout
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    rng = np.random.default_rng(13)
    n = 64
    qh = np.zeros((n, 44), np.float32)
    qh[:, 3:6] = rng.normal(0, 0.05, (n, 3))
    qh[:, 6:38] = rng.normal(0, 0.7, (n, 32))
    qh[:, 38:] = rng.normal(0, 0.05, (n, 6))
    beta = torch.zeros((n, 10), device="cuda")
    with torch.no_grad():
        target, _ = s.forward_differentiable(beta, theta_from_latent_layout(gpu, torch.from_numpy(qh).cuda()))
    q = torch.from_numpy(qh + rng.normal(0, 0.05, qh.shape).astype(np.float32)).cuda().requires_grad_(True)
    steps = 800
    opt = torch.optim.Adam([q], lr=0.01)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, steps, eta_min=1e-4)
    for _ in range(steps):
        opt.zero_grad()
        verts, _ = s.forward_differentiable(beta, theta_from_latent_layout(gpu, q))
        loss = ((verts - target) ** 2).sum(-1).mean(-1).sum()
        loss.backward()
        opt.step()
        sched.step()
    with torch.no_grad():
        verts, _ = s.forward_differentiable(beta, theta_from_latent_layout(gpu, q))
        err = float((verts - target).norm(dim=-1).mean())
    assert err < 1e-3, err


def test_vjp_cpp_shim(tmp_path, params):
    import __graft_entry__ as g

    g.build()
    exe = str(tmp_path / "vposer_vjp_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "vposer_vjp_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    path = str(tmp_path / "vposer.json")
    import json

    with open(path, "w") as f:
        json.dump({k: np.asarray(v).tolist() for k, v in params.items()}, f)
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stdout
    vals = {}
    for line in out.stdout.splitlines():
        k, *v = line.split()
        vals[k] = np.array([float(x) for x in v], np.float32)
    # the program's inputs, restated
    n = 3
    z = ((np.arange(n * 32, dtype=np.float32).reshape(n, 32) % 9) - 4) * np.float32(0.2)
    go = ((np.arange(n * 63, dtype=np.float32).reshape(n, 21, 3) % 7) - 3) * np.float32(0.1)
    from smplpp_amd.ik import VPoserDecoder

    ref = VPoserDecoder(params).launchBackward(z, go)
    assert np.array_equal(vals["GRAD_Z"], ref.ravel())
