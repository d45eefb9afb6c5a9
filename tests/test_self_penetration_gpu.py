"""Self-intersections and the self-penetration energy on the MI355X (smplpp_self_intersections, smplpp_self_penetration,
smplpp_self_penetration_vjp): the pair lists' bits against the float32 restatement on the synthetic model, two overlapping spheres
and a mesh past the LDS sort; float64 agreement beyond a margin; batch, slot and space independence; truncation, NaN and zero-area
rules; energies and the backward pass against float64; call semantics; the chain to theta, a separation fit and the C++ shim."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import self_penetration_oracle as SP  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model_for(verts, faces):
    """An SMPL handle whose faces are `faces` (the template is `verts`; the calls here take vertices directly)."""
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    m = model_io.tiny_model(len(verts), seed=3, faces=np.asarray(faces) + 1)
    m["vertices_template"] = np.asarray(verts, m["vertices_template"].dtype)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(m)
    return s


@pytest.fixture(scope="module")
def smpl(synth_model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    return s


@pytest.fixture(scope="module")
def faces(synth_model):
    return synth_model["face_indices"].astype(np.int64) - 1


@pytest.fixture(scope="module")
def synth_verts(smpl):
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(8)
    return smpl.launch(beta, theta, want=("verts",))["verts"]


@pytest.fixture(scope="module")
def two_spheres():
    v, f = SP.spheres(4, [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0)])
    return _model_for(v, f), v, f


def _sphere_frames(v, shifts, seed=0):
    rng = np.random.default_rng(seed)
    half = len(v) // 2
    out = []
    for d in shifts:
        w = v.copy()
        w[half:] += d
        out.append(w + rng.normal(0, 2e-4, w.shape))
    return np.stack(out).astype(np.float32)


def _check_bits(pairs, count, verts, faces):
    for i in range(len(verts)):
        want = SP.intersections(verts[i], faces)
        assert count[i] == len(want), (i, count[i], len(want))
        assert np.array_equal(pairs[i, :len(want)], want), i
        assert (pairs[i, len(want):] == -1).all()


# ---------------------------------------------------------------------------------------------------- detection
def test_bits_synthetic(smpl, faces, synth_verts):
    pairs, count = smpl.selfIntersections(synth_verts, max_pairs=65536)
    _check_bits(pairs, count, synth_verts, faces)
    assert (count > 0).sum() >= 6
    rest = smpl.launch(np.zeros((1, 10), np.float32), np.zeros((1, 25, 3), np.float32), want=("verts",))["verts"]
    _, c0 = smpl.selfIntersections(rest)
    assert c0[0] == 0


def test_bits_two_spheres_and_float64(two_spheres):
    s, v, f = two_spheres
    V = _sphere_frames(v, [(0.8, 0.02, 0.01), (0.95, 0.0, 0.0), (0.6, 0.3, 0.0), (2.0, 0.0, 0.0)], seed=1)
    pairs, count = s.selfIntersections(V)
    _check_bits(pairs, count, V, f)
    assert count[0] >= 100 and count[3] == 0
    for i in range(3):
        a = {tuple(p) for p in pairs[i, :count[i]].tolist()}
        b = {tuple(p) for p in SP.intersections(V[i], f, np.float64).tolist()}
        assert a ^ b <= SP.near_degenerate(V[i], f, 1e-4), i


def test_bits_large_mesh():
    v, f = SP.spheres(4, [(0, 0, 0), (0.8, 0.0, 0.0), (0.4, 0.6, 0.0), (0.4, 0.3, 0.7)])
    assert len(f) > 16384
    s = _model_for(v, f)
    rng = np.random.default_rng(4)
    V = np.stack([v + rng.normal(0, 2e-3, v.shape), v + rng.normal(0, 2e-3, v.shape)]).astype(np.float32)
    pairs, count = s.selfIntersections(V, max_pairs=65536)
    _check_bits(pairs, count, V, f)
    assert (count > 100).all()


def test_batch_slot_and_space_independence(smpl, synth_verts):
    alone = [smpl.selfIntersections(synth_verts[i:i + 1], max_pairs=65536) for i in range(3)]
    batch = smpl.selfIntersections(synth_verts, max_pairs=65536)
    perm = np.array([5, 0, 7, 2, 1, 4, 6, 3])
    moved = smpl.selfIntersections(synth_verts[perm], max_pairs=65536)
    dv = torch.from_numpy(synth_verts).cuda()
    dp, dc = smpl.selfIntersections(dv, max_pairs=65536)
    for i in range(3):
        assert _same_bits(alone[i][0][0], batch[0][i]) and alone[i][1][0] == batch[1][i]
    for j, i in enumerate(perm):
        assert _same_bits(moved[0][j], batch[0][i]) and moved[1][j] == batch[1][i]
    assert _same_bits(dp.cpu().numpy(), batch[0]) and _same_bits(dc.cpu().numpy(), batch[1])


def test_truncation(two_spheres):
    from smplpp_amd._lib import SmplppError

    s, v, f = two_spheres
    V = _sphere_frames(v, [(0.8, 0.02, 0.01), (0.9, 0.0, 0.0)], seed=2)
    full, count = s.selfIntersections(V)
    M = int(count.min()) // 2
    with pytest.raises(SmplppError):
        s.selfIntersections(V, max_pairs=M)
    p, c = s.selfIntersections(V, max_pairs=M, check=False)
    assert np.array_equal(c, count) and np.array_equal(p, full[:, :M])
    p0, c0 = s.selfIntersections(V, max_pairs=0, check=False)
    assert p0.shape == (2, 0, 2) and np.array_equal(c0, count)
    pe, ce, e = s.selfPenetration(V, max_pairs=M, check=False)
    assert np.array_equal(pe, p) and (e >= 0).all()
    short = int(count.max()) + 7
    p2, _ = s.selfIntersections(V, max_pairs=short)
    for i in range(2):
        assert (p2[i, count[i]:] == -1).all()


def test_nan_frame_and_zero_area_face(two_spheres):
    s, v, f = two_spheres
    V = _sphere_frames(v, [(0.8, 0.02, 0.01), (0.8, 0.02, 0.01), (0.8, 0.02, 0.01)], seed=3)
    ref, rc = s.selfIntersections(V[:1])
    V[1, f[ref[0, :5]].ravel()] = np.nan  # the vertices of the first five pairs
    V[2] = np.nan
    # a zero-area face among the intersecting ones: one of its vertices moved onto another
    g = int(ref[0, 0, 1])
    V[0, f[g, 1]] = V[0, f[g, 0]]
    pairs, count = s.selfIntersections(V)
    _check_bits(pairs, count, V, f)
    assert count[2] == 0 and 0 < count[1] < rc[0]
    pe, ce, e = s.selfPenetration(V)
    assert np.isfinite(e).all() and (e[2] == 0).all()


def test_refusals(smpl, synth_model, synth_verts):
    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import _ptr

    L = _lib.load()
    v = synth_verts[:1]
    cnt = np.zeros(1, np.int64)
    pairs = np.zeros((1, 4, 2), np.int64)
    e = np.zeros((1, 4), np.float32)
    for args in ((-1, 2.0), (4, 0.0), (4, float("nan")), (4, float("inf"))):
        with pytest.raises(_lib.SmplppError):
            _lib.check(L.smplpp_self_penetration(smpl.handle, 1, _ptr(v), args[0], args[1], _ptr(pairs), _ptr(cnt), _ptr(e), _lib.HOST, None))
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_self_intersections(smpl.handle, 1 << 20, _ptr(v), 1 << 12, _ptr(pairs), _ptr(cnt), _lib.HOST, None))
    # host-space ids out of range
    bad = np.array([[[0, smpl.face_num], [-1, -1], [-1, -1], [-1, -1]]], np.int64)
    gv = np.zeros((1, smpl.vertex_num, 3), np.float32)
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_self_penetration_vjp(smpl.handle, 1, _ptr(v), 4, 2.0, _ptr(bad), _ptr(np.ones(1, np.int64)), _ptr(e), _ptr(gv), 0,
                                                 _lib.HOST, None))
    m = model_io._normalise(synth_model)
    V = m["vertices_template"].shape[0]
    h = C.c_void_p()
    _lib.check(L.smplpp_model_create(V, 0, _ptr(m["vertices_template"]), _ptr(m["shape_blend_shapes"]), _ptr(m["pose_blend_shapes"]),
                                     _ptr(m["joint_regressor"]), _ptr(m["weights"]), _ptr(m["kinematic_tree"]), None, 0, C.byref(h)))
    try:
        with pytest.raises(_lib.SmplppError):
            _lib.check(L.smplpp_self_intersections(h, 1, _ptr(v), 4, _ptr(pairs), _ptr(cnt), _lib.HOST, None))
    finally:
        L.smplpp_model_destroy(h)


# ---------------------------------------------------------------------------------------------------- energy and backward
@pytest.mark.parametrize("sigma", [0.5, 2.0, 3.0])
def test_energy_vs_float64(smpl, faces, synth_verts, sigma):
    pairs, count, e = smpl.selfPenetration(synth_verts, sigma=sigma, max_pairs=65536)
    for i in range(len(synth_verts)):
        P = pairs[i, :count[i]]
        assert (e[i, count[i]:] == 0).all()
        if len(P) == 0:
            continue
        r64 = SP.pair_energy(torch.tensor(synth_verts[i], dtype=torch.float64), faces, P, sigma).numpy()
        r32 = SP.pair_energy(torch.tensor(synth_verts[i]), faces, P, sigma).numpy()
        bar = max(4 * _rel(r32, r64), 1e-5)
        assert _rel(e[i, :count[i]], r64) <= bar, (i, _rel(e[i, :count[i]], r64), bar)
        assert (e[i, :count[i]] > 0).mean() > (0.9 if sigma == 2.0 else 0.3)


def test_vjp_vs_float64_and_semantics(two_spheres):
    s, v, f = two_spheres
    V = _sphere_frames(v, [(0.8, 0.02, 0.01), (0.9, 0.0, 0.05)], seed=5)
    pairs, count, e = s.selfPenetration(V, sigma=2.0)
    rng = np.random.default_rng(6)
    g = rng.normal(size=e.shape).astype(np.float32)
    gv = s.selfPenetrationBackward(V, pairs, count, g)
    for i in range(2):
        P, gi = pairs[i, :count[i]], g[i, :count[i]]
        r64 = SP.vjp(torch.tensor(V[i], dtype=torch.float64), f, P, gi, 2.0).numpy()
        r32 = SP.vjp(torch.tensor(V[i]), f, P, gi, 2.0).numpy()
        bar = max(4 * _rel(r32, r64), 1e-5)
        assert _rel(gv[i], r64) <= bar, (i, _rel(gv[i], r64), bar)
    # repeat: the same bits; device space: the same bits
    assert _same_bits(s.selfPenetrationBackward(V, pairs, count, g), gv)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    assert _same_bits(s.selfPenetrationBackward(dev(V), dev(pairs), dev(count), dev(g)).cpu().numpy(), gv)
    # accumulate
    base = rng.normal(size=gv.shape).astype(np.float32)
    out = base.copy()
    r = s.selfPenetrationBackward(V, pairs, count, g, out=out)
    assert r is out and _same_bits(out, base + gv)
    # zero cotangent on a NaN row contributes nothing; device ids out of range contribute nothing
    V2, g2, p2 = V.copy(), g.copy(), pairs.copy()
    vtx = f[p2[0, 3, 0], 0]
    V2[0, vtx] = np.nan
    touched = (f[pairs[0, :count[0]]] == vtx).any(axis=(1, 2))
    g2[0, :count[0]][touched] = 0.0
    gn = s.selfPenetrationBackward(V2, p2, count, g2)
    assert np.isfinite(gn).all()
    p3 = pairs.copy()
    p3[1, 0] = (10 ** 7, 0)
    g3 = g.copy()
    gd = s.selfPenetrationBackward(dev(V), dev(p3), dev(count), dev(g3)).cpu().numpy()
    g3[1, 0] = 0.0
    assert _same_bits(gd, s.selfPenetrationBackward(V, pairs, count, g3))


def test_end_to_end_theta_gradient(smpl, synth_model, faces):
    import fk_vjp_oracle as FK
    from smplpp_amd import model_io

    dev = torch.device("cuda")
    beta, theta = model_io.synthetic_inputs(2, seed=21)
    b = torch.from_numpy(beta).to(dev).requires_grad_(True)
    t = torch.from_numpy(theta).to(dev).requires_grad_(True)
    verts, _ = smpl.forward_differentiable(b, t)
    pairs, count, e = smpl.self_penetration_differentiable(verts, max_pairs=65536)
    assert not pairs.requires_grad and e.requires_grad
    e.sum().backward()
    pairs, count = pairs.cpu().numpy(), count.cpu().numpy()
    assert (count > 0).all()

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        bb = torch.tensor(beta, dtype=dtype, requires_grad=True)
        tt = torch.tensor(theta, dtype=dtype, requires_grad=True)
        vv = FK.fk(m, bb, tt)["verts"]
        sum(SP.pair_energy(vv[i], faces, pairs[i, :count[i]], 2.0).sum() for i in range(2)).backward()
        return bb.grad.double().numpy(), tt.grad.double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for got, want, f32, name in ((b.grad, r64[0], r32[0], "beta"), (t.grad, r64[1], r32[1], "theta")):
        got = got.cpu().numpy()
        bar = max(4 * _rel(f32, want), 1e-5)
        assert _rel(got, want) <= bar, (name, _rel(got, want), bar)


def test_separation_fit(two_spheres):
    """Two spheres of one mesh, 0.8 apart at radius 0.5 (220 pairs): Adam on one sphere's translation against pair_energy.sum() leaves no
    intersecting pair within 300 steps."""
    s, v, f = two_spheres
    dev = torch.device("cuda")
    base = torch.tensor(v, dtype=torch.float32, device=dev)
    half = len(v) // 2
    shift = torch.tensor([0.8, 0.02, 0.01], device=dev, requires_grad=True)
    opt = torch.optim.Adam([shift], lr=0.005)
    counts = []
    for it in range(300):
        opt.zero_grad()
        verts = torch.cat([base[:half], base[half:] + shift])[None].contiguous()
        pairs, count, e = s.self_penetration_differentiable(verts)
        counts.append(int(count[0]))
        if counts[-1] == 0:
            break
        e.sum().backward()
        opt.step()
    assert counts[0] >= 100 and counts[-1] == 0, (counts[0], counts[-1], len(counts))


def test_self_penetration_cpp_shim(tmp_path):
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    exe = str(tmp_path / "self_penetration_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "self_penetration_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    n, M = 2, 4096
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    v = s.launch(beta, theta, want=("verts",))["verts"]
    p1, c1 = s.selfIntersections(v, max_pairs=M)
    p2, c2, e = s.selfPenetration(v, sigma=1.5, max_pairs=M)
    assert (c1 > 0).all()
    g = ((np.arange(n * M, dtype=np.float32).reshape(n, M) % 5) - 2) * np.float32(0.25)
    gv = s.selfPenetrationBackward(v, p2, c2, g, sigma=1.5)
    want = b"".join(np.ascontiguousarray(x).tobytes() for x in (p1, c1, p2, c2, e, gv))
    assert len(raw) == len(want) and raw == want
