"""smplpp_vposer_jacobian on the MI355X: parity with the float64 autograd Jacobian of the torch restatement of the decoder
(tests/vposer_jac_oracle.py), the decode it is taken at, agreement with the vector-Jacobian product, bits (determinism, batch and
shard invariance), the axis-angle branch points, call semantics and the C++ shim."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vposer_jac_oracle as JO  # noqa: E402
import vposer_vjp_oracle as O  # noqa: E402
from test_vposer_vjp_gpu import _branch_point_decoder  # noqa: E402

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


def _check_frames(params, z, jac, frames, floor=1e-5, other=None):
    """Per frame: the relative Frobenius error against the float64 Jacobian within max(4 x the error of an fp32 autograd Jacobian
    of the same graph, floor).  `other`: a second Jacobian whose error on the same frames is printed (not asserted)."""
    d64, d32 = O.decoder(params), O.decoder(params, torch.float32)
    worst = []
    for f in frames:
        sl = slice(f, f + 1)
        ref = JO.jacobian(d64, z[sl])
        r32 = JO.jacobian(d32, z[sl], dtype=torch.float32)
        assert np.isfinite(jac[sl]).all(), f
        bar = max(4 * _rel(r32, ref), floor)
        err = _rel(jac[sl].astype(np.float64), ref)
        assert err <= bar, (f, err, bar)
        worst.append((f, err, bar, None if other is None else _rel(other[sl].astype(np.float64), ref)))
    for f, err, bar, e16 in worst:
        print("frame %d: exact %.3g (bar %.3g)%s" % (f, err, bar, "" if e16 is None else ", fp16x2 %.3g" % e16))


@pytest.mark.parametrize("n", [1, 7, 64, 257, 513, 601])
def test_jacobian_parity(gpu, params, n):
    rng = np.random.default_rng(100 + n)
    z = rng.normal(0, 1.0, (n, 32)).astype(np.float32)
    z[0] = 0.0
    jac = gpu.jacobian(z)
    assert jac.shape == (n, 63, 32) and jac.dtype == np.float32
    _, j16 = gpu.forward(z, want_jac=True)
    frames = sorted(set([0, n // 2, n - 1] + [int(i) for i in rng.integers(0, n, 3)]))
    _check_frames(params, z, jac, frames, other=j16)


def test_jacobian_out_and_vjp(gpu):
    """`out` is forward(z) (jac NULL) and launchBackward's `out` bit for bit; g^T J in float64 agrees with launchBackward(z, g)."""
    rng = np.random.default_rng(31)
    n = 300
    z = rng.normal(0, 1.0, (n, 32)).astype(np.float32)
    g = rng.standard_normal((n, 21, 3)).astype(np.float32)
    jac, out = gpu.jacobian(z, want_out=True)
    assert np.array_equal(out, gpu.forward(z))
    gz, outb = gpu.launchBackward(z, g, want_out=True)
    assert np.array_equal(out, outb)
    jtg = np.einsum("nrc,nr->nc", jac.astype(np.float64), g.reshape(n, 63).astype(np.float64))
    for f in range(n):
        assert _rel(gz[f].astype(np.float64), jtg[f]) <= 1e-5, f


def test_jacobian_bits(gpu):
    """Two calls give the same bits; a frame's rows do not depend on the batch (1, n) or the shard (2, 4, 8 shards, frame_base)."""
    rng = np.random.default_rng(41)
    n = 520
    z = rng.normal(0, 1.0, (n, 32)).astype(np.float32)
    jac, out = gpu.jacobian(z, want_out=True)
    jac2, out2 = gpu.jacobian(z, want_out=True)
    assert np.array_equal(jac, jac2) and np.array_equal(out, out2)
    for f in (0, 1, 259, 519):
        assert np.array_equal(gpu.jacobian(z[f:f + 1], frame_base=f), jac[f:f + 1]), f
    for shards in (2, 4, 8):
        cuts = np.linspace(0, n, shards + 1).astype(int)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            assert np.array_equal(gpu.jacobian(z[lo:hi], frame_base=lo), jac[lo:hi]), (shards, lo)
    # small batches: layer 1's rows spread over more workgroups per frame
    for lo, hi in [(0, 3), (5, 12), (100, 164), (200, 457)]:
        for base in (0, lo):
            assert np.array_equal(gpu.jacobian(z[lo:hi], frame_base=base), jac[lo:hi]), (lo, hi, base)


def test_jacobian_at_the_axis_angle_branch_points():
    """Finite everywhere; against float64 where float64 is finite, on the joints near the identity and the generic one by the 4 x
    fp32 rule, on the joints 1e-4 / 1e-3 rad below pi by the same rule with a floor of
    1e-3 (the rounding of the decode is amplified there); exactly pi: where
    one fp32 ulp picks the axis's sign, finiteness only (see test_vposer_vjp_gpu.py)."""
    from smplpp_amd.ik import VPoserDecoder

    params = _branch_point_decoder()
    gpu = VPoserDecoder(params)
    rng = np.random.default_rng(12)
    z = np.zeros((3, 32), np.float32)
    z[1] = rng.normal(0, 1e-3, 32)
    z[2] = rng.normal(0, 0.3, 32)
    jac = gpu.jacobian(z)
    assert np.isfinite(jac).all()
    d64, d32 = O.decoder(params), O.decoder(params, torch.float32)
    near0 = [0] + list(range(14, 21))
    rows0 = [3 * j + i for j in near0 for i in range(3)]
    rowspi = [3 * j + i for j in range(8, 14) for i in range(3)]
    for f in range(3):
        ref = JO.jacobian(d64, z[f:f + 1])[0]
        r32 = JO.jacobian(d32, z[f:f + 1], dtype=torch.float32)[0]
        if np.isfinite(ref[rows0]).all():
            assert _rel(jac[f][rows0].astype(np.float64), ref[rows0]) <= max(4 * _rel(r32[rows0], ref[rows0]), 1e-5), f
        if f < 2 and np.isfinite(ref[rowspi]).all():
            assert _rel(jac[f][rowspi].astype(np.float64), ref[rowspi]) <= max(4 * _rel(r32[rowspi], ref[rowspi]), 1e-3), f


def test_jacobian_call_semantics(gpu):
    from smplpp_amd import _lib

    L = _lib.load()
    rng = np.random.default_rng(5)
    n = 9
    z = rng.normal(0, 1.0, (n, 32)).astype(np.float32)
    ref, refo = gpu.jacobian(z, want_out=True)
    jac = np.full((n, 63, 32), 7.0, np.float32)
    p = lambda a: a.ctypes.data
    for args in [(None, n, 0, p(z), None, p(jac), 0, None), (gpu._h, 0, 0, p(z), None, p(jac), 0, None),
                 (gpu._h, -1, 0, p(z), None, p(jac), 0, None), (gpu._h, n, -1, p(z), None, p(jac), 0, None),
                 (gpu._h, n, 0, None, None, p(jac), 0, None), (gpu._h, n, 0, p(z), None, None, 0, None),
                 (gpu._h, n, 0, p(z), None, p(jac), 5, None)]:
        assert L.smplpp_vposer_jacobian(*args) == 1, args
    assert (jac == 7.0).all()
    # host space, out NULL
    assert L.smplpp_vposer_jacobian(gpu._h, n, 0, p(z), None, p(jac), 0, None) == 0
    assert np.array_equal(jac, ref)
    # device tensors on a stream that is not the default one: enqueued on torch's current stream
    zt = torch.from_numpy(z).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        jt, ot = gpu.jacobian(zt, want_out=True)
        jt2 = gpu.jacobian(zt)
    s.synchronize()
    assert np.array_equal(jt.cpu().numpy(), ref) and np.array_equal(ot.cpu().numpy(), refo)
    assert np.array_equal(jt2.cpu().numpy(), ref)
    # raw device pointers on an explicit stream, into a pre-filled buffer
    jd = torch.full((n, 63, 32), float("nan"), device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        assert L.smplpp_vposer_jacobian(gpu._h, n, 0, zt.data_ptr(), None, jd.data_ptr(), 1, C.c_void_p(s.cuda_stream)) == 0
    s.synchronize()
    assert np.array_equal(jd.cpu().numpy(), ref)


def test_jacobian_cpp_shim(tmp_path, params):
    import __graft_entry__ as g

    g.build()
    exe = str(tmp_path / "vposer_jac_exact_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "vposer_jac_exact_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    path = str(tmp_path / "vposer.json")
    with open(path, "w") as f:
        json.dump({k: np.asarray(v).tolist() for k, v in params.items()}, f)
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stdout
    vals = {}
    for line in out.stdout.splitlines():
        k, *v = line.split()
        vals[k] = np.array([float(x) for x in v], np.float32)
    n = 3
    z = ((np.arange(n * 32, dtype=np.float32).reshape(n, 32) % 9) - 4) * np.float32(0.2)
    from smplpp_amd.ik import VPoserDecoder

    jac, o = VPoserDecoder(params).jacobian(z, want_out=True)
    assert np.array_equal(vals["JAC"], jac.ravel())
    assert np.array_equal(vals["OUT"], o.ravel())
