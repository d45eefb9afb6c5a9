"""The batched winding numbers and the signed point-to-mesh distance on the MI355X (smplpp_point_mesh_winding,
smplpp_point_mesh_signed_distance, smplpp_point_mesh_signed_distance_vjp): the winding numbers' bits against the sweep grid's at the
same fp32 positions, alone and inside a batch; the values against the float64 oracle on classes of points; independence of batch,
slot and split; the signed forward's bits against pointMeshDistance and pointMeshWinding; the backward's bits against
pointMeshDistanceBackward at the cotangent sigma g, against float64 autograd, and its call semantics; end-to-end gradients, a
penetration fit through forward_differentiable, and the C++ shim."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_ref as cr  # noqa: E402
import signed_distance_oracle as SO  # noqa: E402
from distance_cases import _rel, _same_bits, _surface_points, _verts  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _vertex_normals(v, faces):
    fn = cr.face_normals(v, faces)
    vn = np.zeros(v.shape)
    for j in range(3):
        np.add.at(vn, faces[:, j], fn)
    return vn / np.linalg.norm(vn, axis=1, keepdims=True)


def _classes(v, faces, rng, count=300):
    """Points of several classes for one frame: random in the AABB, +-1 mm and +-1 cm along vertex normals, 10 m away."""
    lo, hi = v.min(0), v.max(0)
    vn = _vertex_normals(v, faces)
    idx = rng.choice(len(v), count, replace=False)
    parts = {"aabb": rng.uniform(lo, hi, (count, 3))}
    for name, off in (("in_1mm", -0.001), ("out_1mm", 0.001), ("in_1cm", -0.01), ("out_1cm", 0.01)):
        parts[name] = v[idx] + off * vn[idx]
    parts["far"] = v[idx[:32]] + 10.0 * rng.normal(size=(32, 3)) / np.sqrt(3)
    names = np.concatenate([[k] * len(p) for k, p in parts.items()])
    return np.concatenate(list(parts.values())).astype(np.float32), names


# ---------------------------------------------------------------------------------------------------- winding numbers
def test_sweep_grid_bits(smpl):
    """At np.float32(0.025) * grid_idx (the sweep kernel's own fp32 cell positions) the winding numbers and inside flags are the
    sweep grid's, bit for bit: the frame alone, and at slot 3 of a batch of 8 whose other frames differ."""
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(8, seed=17)
    theta[3] *= 0.3  # a milder pose in slot 3
    v = smpl.launch(beta, theta, want=("verts",))["verts"]
    g = smpl.calcSweepGrid(frame=3)
    P = g["grid_idx"].astype(np.float32) * np.float32(0.025)
    w1, in1 = smpl.pointMeshWinding(v[3:4], P[None])
    assert _same_bits(w1[0], g["winding"]) and (in1[0] == g["inside"]).all()
    assert 0 < g["inside"].sum() < len(P)
    rng = np.random.default_rng(17)
    Pb = np.repeat(P[None], 8, axis=0) + rng.normal(0, 0.01, (8, len(P), 3)).astype(np.float32)
    Pb[3] = P
    wb, inb = smpl.pointMeshWinding(v, Pb)
    assert _same_bits(wb[3], g["winding"]) and (inb[3] == g["inside"]).all()


@pytest.mark.parametrize("pose", ["rest", "posed", "crumpled"])
def test_winding_vs_oracle(smpl, oracle_synth, synth_model, faces, pose):
    from smplpp_amd import model_io

    rng = np.random.default_rng({"rest": 1, "posed": 2, "crumpled": 3}[pose])
    beta, theta = model_io.synthetic_inputs(2, seed=23)
    if pose == "rest":
        beta[:], theta[:] = 0, 0
    elif pose == "crumpled":
        theta[:, 1:] = rng.normal(0, 0.9, theta[:, 1:].shape)  # self-intersecting
    v = smpl.launch(beta, theta, want=("verts",))["verts"]
    pts = [_classes(v[f], faces, rng) for f in range(2)]
    P = np.stack([p for p, _ in pts])
    names = pts[0][1]
    P[1, 5:9] = np.nan  # NaN rows
    P[0, 40] = (np.nan, 0.0, 0.0)
    w, ins = smpl.pointMeshWinding(v, P)
    assert w.shape == P.shape[:2] and w.dtype == np.float32 and ins.dtype == bool
    assert np.isnan(w[1, 5:9]).all() and not ins[1, 5:9].any() and np.isnan(w[0, 40]) and not ins[0, 40]
    ok = np.isfinite(P).all(-1)
    for f in range(2):
        ref = oracle_synth.winding_numbers(v[f], np.where(ok[f, :, None], P[f], 0))
        assert np.abs(w[f][ok[f]] - ref[ok[f]]).max() < 2e-4, (pose, f)
        sure = ok[f] & (np.abs(ref - 0.5) > 1e-3)
        assert (ins[f][sure] == (ref[sure] > 0.5)).all()
        if pose == "crumpled":
            continue
        for name, want in (("in_1cm", True), ("out_1cm", False), ("far", False)):
            m = (names == name) & ok[f]
            if pose == "rest" or name == "far":
                assert (ins[f][m] == want).all(), (pose, f, name)
    if pose == "rest":
        # a closed, outward-facing genus-0 mesh: 1 inside, 0 outside
        m = ok[0] & np.isin(names, ["in_1mm", "in_1cm"])
        assert np.abs(w[0][m] - 1).max() < 2e-4
        m = ok[0] & np.isin(names, ["out_1mm", "out_1cm", "far"])
        assert np.abs(w[0][m]).max() < 2e-4


def test_numpy_restatement_agrees_on_device_points(smpl, faces, oracle_synth):
    v = _verts(smpl, 1, seed=29)
    P = _surface_points(v, faces, 64, np.random.default_rng(29), off=0.05)
    w, _ = smpl.pointMeshWinding(v, P)
    ref = SO.winding64(v[0], faces, P[0])
    assert np.abs(ref - oracle_synth.winding_numbers(v[0], P[0])).max() < 1e-9
    assert np.abs(w[0] - ref).max() < 2e-4


def test_split_and_batch_independence_and_repeat(smpl, faces):
    """A frame alone and inside a batch gives the same bits, winding and signed distance.  Under the split rule (the 54 chunks of
    256 faces dealt over workgroups, from n and K) K = 4096 alone is cut into 54 slices, in a batch of 64 into 2; K = 64 alone into
    54, in a batch of 300 into 27; K = 1024 alone into 54, in a batch of 512 not at all."""
    for K, nb, slot in ((4096, 64, 37), (64, 300, 201), (1024, 512, 300)):
        v = _verts(smpl, nb, seed=K + 3)
        rng = np.random.default_rng(K)
        P = _surface_points(v, faces, K, rng, off=0.03)
        dv, dP = torch.from_numpy(v).cuda(), torch.from_numpy(P).cuda()
        bw, bi = smpl.pointMeshWinding(dv, dP)
        bs = smpl.pointMeshSignedDistance(dv, dP)
        runs = []
        for _ in range(2):
            aw, ai = smpl.pointMeshWinding(dv[slot:slot + 1].contiguous(), dP[slot:slot + 1].contiguous())
            a_s = smpl.pointMeshSignedDistance(dv[slot:slot + 1].contiguous(), dP[slot:slot + 1].contiguous())
            runs.append([x.cpu().numpy() for x in (aw, ai) + a_s])
        torch.cuda.synchronize()
        batch = [x.cpu().numpy()[slot:slot + 1] for x in (bw, bi) + bs]
        # (weights are pointMeshDistance's, whose per-query and tiled forms may differ in their last bits: compared per call in
        # test_signed_forward_bits, not across n here)
        names = ("winding", "inside", "face", "weights", "closest", "winding", "inside", "signed_sqdist")
        for r in runs:
            assert [nm for nm, a, b in zip(names, r, batch) if nm != "weights" and not _same_bits(a, b)] == [], K
        assert 0 < runs[0][1].sum() < K  # both sides of the surface


def test_model_without_faces_refused(synth_model):
    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import _ptr

    m = model_io._normalise(synth_model)
    L = _lib.load()
    V = m["vertices_template"].shape[0]
    h = C.c_void_p()
    _lib.check(L.smplpp_model_create(V, 0, _ptr(m["vertices_template"]), _ptr(m["shape_blend_shapes"]), _ptr(m["pose_blend_shapes"]),
                                     _ptr(m["joint_regressor"]), _ptr(m["weights"]), _ptr(m["kinematic_tree"]), None, 0, C.byref(h)))
    try:
        v = np.zeros((1, V, 3), np.float32)
        P = np.zeros((1, 4, 3), np.float32)
        w = np.full((1, 4), 7.0, np.float32)
        with pytest.raises(_lib.SmplppError):
            _lib.check(L.smplpp_point_mesh_winding(h, 1, _ptr(v), 4, _ptr(P), _ptr(w), None, _lib.HOST, None))
        assert (w == 7.0).all()
    finally:
        L.smplpp_model_destroy(h)


# ---------------------------------------------------------------------------------------------------- signed distance
def test_signed_forward_bits(smpl, faces):
    for n, K in ((3, 500), (2, 4096)):  # the per-query and the tiled point-to-mesh forms
        v = _verts(smpl, n, seed=K + 11)
        rng = np.random.default_rng(K)
        P = _surface_points(v, faces, K, rng, off=0.03)
        P[0, 3] = np.nan
        face, w, closest, wn, ins, sq = smpl.pointMeshSignedDistance(v, P)
        rf, rw, rc, rs = smpl.pointMeshDistance(v, P)
        ww, wi = smpl.pointMeshWinding(v, P)
        assert _same_bits(face, rf) and _same_bits(w, rw) and _same_bits(closest, rc)
        assert _same_bits(wn, ww) and (ins == wi).all() and ins.dtype == bool
        assert _same_bits(np.abs(sq), np.abs(rs)) and _same_bits(np.where(ins, -rs, rs), sq)
        assert ins.any() and (~ins).any() and not ins[0, 3]


def _raw_vjp(s, v, P, face, inside, g, gv, gp, acc, space=0):
    from smplpp_amd import _lib
    from smplpp_amd.smpl import _ptr

    n, K = P.shape[:2]
    return _lib.load().smplpp_point_mesh_signed_distance_vjp(s.handle, n, _ptr(v), K, _ptr(P), _ptr(face), _ptr(inside), _ptr(g), _ptr(gv),
                                                             _ptr(gp), acc, space, None)


@pytest.mark.parametrize("n,K", [(1, 7), (3, 500), (2, 4096)])
def test_signed_backward_bits_and_float64(smpl, faces, n, K):
    v = _verts(smpl, n, seed=K + 5)
    rng = np.random.default_rng(K + 5)
    P = _surface_points(v, faces, K, rng, off=0.03)
    face, _, _, _, ins, _ = smpl.pointMeshSignedDistance(v, P)
    g = rng.normal(size=(n, K)).astype(np.float32)
    gv, gp = smpl.pointMeshSignedDistanceBackward(v, P, face, ins, g)
    sg = np.where(ins, -g, g).astype(np.float32)
    rv, rp = smpl.pointMeshDistanceBackward(v, P, face, sg)
    assert _same_bits(gv, rv) and _same_bits(gp, rp)
    for f in range(n):
        sl = slice(f, f + 1)
        r64 = SO.vjp(torch.tensor(v[sl], dtype=torch.float64), faces, torch.tensor(P[sl], dtype=torch.float64), face[sl], ins[sl], g[sl])
        r32 = SO.vjp(torch.tensor(v[sl]), faces, torch.tensor(P[sl]), face[sl], ins[sl], g[sl])
        for got, ref, f32 in ((gv[sl], r64[0], r32[0]), (gp[sl], r64[1], r32[1])):
            bar = max(4 * _rel(f32.numpy(), ref.numpy()), 1e-5)
            assert np.isfinite(got).all() and _rel(got, ref.numpy()) <= bar


def test_signed_backward_call_semantics(smpl, faces):
    from smplpp_amd import _lib
    from smplpp_amd._lib import SmplppError, check
    from smplpp_amd.smpl import _ptr

    v = _verts(smpl, 2, seed=51)
    rng = np.random.default_rng(51)
    K, V = 300, smpl.vertex_num
    P = _surface_points(v, faces, K, rng, off=0.03)
    face, _, _, _, ins, _ = smpl.pointMeshSignedDistance(v, P)
    ins8 = ins.astype(np.uint8)
    g = rng.normal(size=(2, K)).astype(np.float32)
    gv, gp = smpl.pointMeshSignedDistanceBackward(v, P, face, ins, g)
    # accumulate = 0 overwrites; 1 adds
    ov, op = np.full((2, V, 3), 7.0, np.float32), np.full((2, K, 3), 7.0, np.float32)
    assert _raw_vjp(smpl, v, P, face, ins8, g, ov, op, 0) == 0 and _same_bits(ov, gv) and _same_bits(op, gp)
    base_v, base_p = rng.normal(size=(2, V, 3)).astype(np.float32), rng.normal(size=(2, K, 3)).astype(np.float32)
    av, ap = smpl.pointMeshSignedDistanceBackward(v, P, face, ins, g, out=base_v.copy(), grad_points=base_p.copy())
    assert _same_bits(av, base_v + gv) and _same_bits(ap, base_p + gp)
    # either output NULL
    ov = np.full((2, V, 3), 7.0, np.float32)
    assert _raw_vjp(smpl, v, P, face, ins8, g, ov, None, 0) == 0 and _same_bits(ov, gv)
    op = np.full((2, K, 3), 7.0, np.float32)
    assert _raw_vjp(smpl, v, P, face, ins8, g, None, op, 0) == 0 and _same_bits(op, gp)
    # zero-cotangent NaN rows contribute nothing
    Pn, gz = P.copy(), g.copy()
    Pn[1, 10:20] = np.nan
    gz[1, 10:20] = 0
    zv, zp = smpl.pointMeshSignedDistanceBackward(v, Pn, face, ins, gz)
    g0 = g.copy()
    g0[1, 10:20] = 0
    rv, rp = smpl.pointMeshSignedDistanceBackward(v, P, face, ins, g0)
    assert _same_bits(zv, rv) and (zp[1, 10:20] == 0).all() and _same_bits(np.delete(zp, range(10, 20), 1), np.delete(rp, range(10, 20), 1))
    # host and device space
    dv, dP, df, di, dg = (torch.from_numpy(x).cuda() for x in (v, P, face, ins, g))
    dfw = smpl.pointMeshSignedDistance(dv, dP)
    dbw = smpl.pointMeshSignedDistanceBackward(dv, dP, df, di, dg)
    dww = smpl.pointMeshWinding(dv, dP)
    torch.cuda.synchronize()
    hfw = smpl.pointMeshSignedDistance(v, P)
    hww = smpl.pointMeshWinding(v, P)
    assert all(_same_bits(a, b.cpu().numpy()) for a, b in zip(hfw + (gv, gp) + hww, dfw + dbw + dww))
    # host-space face ids out of range: refused, outputs untouched; device space: contributes nothing
    for bad in (-1, len(faces)):
        bf = face.copy()
        bf[1, 100] = bad
        ov, op = np.full((2, V, 3), 7.0, np.float32), np.full((2, K, 3), 7.0, np.float32)
        with pytest.raises(SmplppError):
            check(_raw_vjp(smpl, v, P, bf, ins8, g, ov, op, 1))
        assert (ov == 7.0).all() and (op == 7.0).all()
    bad = df.clone()
    bad[1, 100] = len(faces)
    gd0 = dg.clone()
    gd0[1, 100] = 0
    b1 = smpl.pointMeshSignedDistanceBackward(dv, dP, bad, di, dg)
    b0 = smpl.pointMeshSignedDistanceBackward(dv, dP, df, di, gd0)
    torch.cuda.synchronize()
    assert _same_bits(b1[0].cpu().numpy(), b0[0].cpu().numpy())
    # invalid arguments
    L = _lib.load()
    h = smpl.handle
    w8 = np.zeros((2, K), np.float32)
    sq = np.zeros((2, K), np.float32)
    wo = np.zeros((2, K, 3), np.float32)
    bad_calls = [
        (L.smplpp_point_mesh_winding, (None, 2, _ptr(v), K, _ptr(P), _ptr(w8), None, 0, None)),
        (L.smplpp_point_mesh_winding, (h, 0, _ptr(v), K, _ptr(P), _ptr(w8), None, 0, None)),
        (L.smplpp_point_mesh_winding, (h, 2, _ptr(v), 0, _ptr(P), _ptr(w8), None, 0, None)),
        (L.smplpp_point_mesh_winding, (h, 2, _ptr(v), K, _ptr(P), None, None, 0, None)),
        (L.smplpp_point_mesh_winding, (h, 2, _ptr(v), K, _ptr(P), _ptr(w8), None, 5, None)),
        (L.smplpp_point_mesh_winding, (h, 1 << 16, _ptr(v), 1 << 16, _ptr(P), _ptr(w8), None, 0, None)),
        (L.smplpp_point_mesh_signed_distance, (h, 2, _ptr(v), K, _ptr(P), _ptr(face), _ptr(wo), None, None, None, _ptr(sq), 0, None)),
        (L.smplpp_point_mesh_signed_distance, (h, 2, _ptr(v), K, _ptr(P), None, _ptr(wo), None, None, _ptr(ins8), _ptr(sq), 0, None)),
        (L.smplpp_point_mesh_signed_distance, (h, 2, _ptr(v), K, _ptr(P), _ptr(face), None, None, None, _ptr(ins8), None, 0, None)),
        (L.smplpp_point_mesh_signed_distance_vjp, (h, 2, _ptr(v), K, _ptr(P), _ptr(face), _ptr(ins8), _ptr(g), None, None, 0, 0, None)),
        (L.smplpp_point_mesh_signed_distance_vjp, (h, 2, _ptr(v), K, _ptr(P), _ptr(face), None, _ptr(g), _ptr(gv), None, 0, 0, None)),
        (L.smplpp_point_mesh_signed_distance_vjp, (h, 2, _ptr(v), K, _ptr(P), _ptr(face), _ptr(ins8), _ptr(g), _ptr(gv), None, 2, 0, None)),
        (L.smplpp_point_mesh_signed_distance_vjp, (h, 1 << 16, _ptr(v), 1 << 16, _ptr(P), _ptr(face), _ptr(ins8), _ptr(g), _ptr(gv), None, 0, 0,
                                                   None)),
    ]
    for fn, args in bad_calls:
        with pytest.raises(SmplppError):
            check(fn(*args))


# ---------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_beta_theta_gradient(smpl, synth_model, faces):
    import fk_vjp_oracle as FK
    from smplpp_amd import model_io

    dev = torch.device("cuda")
    beta, theta = model_io.synthetic_inputs(2, seed=81)
    rng = np.random.default_rng(81)
    vt = _verts(smpl, 2, seed=82)
    P = _surface_points(vt, faces, 1000, rng, off=0.03)
    b = torch.from_numpy(beta).to(dev).requires_grad_(True)
    t = torch.from_numpy(theta).to(dev).requires_grad_(True)
    Pd = torch.from_numpy(P).to(dev)
    verts, _ = smpl.forward_differentiable(b, t)
    face, w, inside, sq = smpl.point_mesh_signed_distance_differentiable(verts, Pd)
    assert not face.requires_grad and not inside.requires_grad and sq.requires_grad and inside.dtype == torch.bool
    sq.mean().backward()
    face, inside = face.cpu().numpy(), inside.cpu().numpy()
    assert inside.any() and (~inside).any()

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        bb = torch.tensor(beta, dtype=dtype, requires_grad=True)
        tt = torch.tensor(theta, dtype=dtype, requires_grad=True)
        vv = FK.fk(m, bb, tt)["verts"]
        SO.signed_sqdist(vv, faces, torch.tensor(P, dtype=dtype), face, inside).mean().backward()
        return bb.grad.double().numpy(), tt.grad.double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for got, want, f32, name in ((b.grad, r64[0], r32[0], "beta"), (t.grad, r64[1], r32[1], "theta")):
        got = got.cpu().numpy()
        bar = max(4 * _rel(f32, want), 1e-5)
        assert _rel(got, want) <= bar, (name, _rel(got, want), bar)
    # points differentiable too
    Pg = Pd.clone().requires_grad_(True)
    _, _, ins2, sq2 = smpl.point_mesh_signed_distance_differentiable(verts.detach(), Pg)
    sq2.sum().backward()
    rv, rp = SO.vjp(verts.detach().double().cpu(), faces, Pd.double().cpu(), face, ins2.cpu().numpy(), np.ones(face.shape))
    assert _rel(Pg.grad.cpu().numpy(), rp.numpy()) <= 1e-5


def test_penetration_fit(smpl, faces):
    """Two bodies in the rest pose placed overlapping, 20 cm apart front to back (about 2000 vertices of each inside the other);
    each mesh's vertices are the other's query points and the loss is relu(-signed_sqdist).sum() in both directions.  Adam on one
    body's root translation separates them: no vertex of either inside the other within 300 steps."""
    dev = torch.device("cuda")
    with torch.no_grad():
        base, _ = smpl.forward_differentiable(torch.zeros(1, 10, device=dev), torch.zeros(1, 25, 3, device=dev))
    A = base.contiguous()
    shift = torch.tensor([[0.02, 0.0, 0.2]], device=dev, requires_grad=True)  # root translation of body B
    opt = torch.optim.Adam([shift], lr=0.005)
    counts = []
    for it in range(300):
        opt.zero_grad()
        B = (base + shift[:, None, :]).contiguous()
        _, _, inAB, sAB = smpl.point_mesh_signed_distance_differentiable(A, B)  # B's vertices inside A
        _, _, inBA, sBA = smpl.point_mesh_signed_distance_differentiable(B, A)  # A's vertices inside B
        counts.append(int(inAB.sum()) + int(inBA.sum()))
        if counts[-1] == 0:
            break
        loss = torch.relu(-sAB).sum() + torch.relu(-sBA).sum()
        loss.backward()
        opt.step()
    assert counts[0] > 1000 and counts[-1] == 0, (counts[0], counts[-1], len(counts))


def test_signed_distance_cpp_shim(tmp_path):
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    exe = str(tmp_path / "signed_distance_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "signed_distance_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    n, K = 2, 24
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    P = ((np.arange(n * K * 3, dtype=np.float32).reshape(n, K, 3) % 17) - 8) * np.float32(0.03)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    g = ((np.arange(n * K, dtype=np.float32).reshape(n, K) % 5) - 2) * np.float32(0.25)
    v = s.launch(beta, theta, want=("verts",))["verts"]
    w, wi = s.pointMeshWinding(v, P)
    face, wt, closest, wn, ins, sq = s.pointMeshSignedDistance(v, P)
    gv, gp = s.pointMeshSignedDistanceBackward(v, P, face, ins, g)
    i64 = lambda b: b.astype(np.int64)  # noqa: E731
    want = b"".join(np.ascontiguousarray(x).tobytes() for x in (w, i64(wi), face, wt, closest, wn, i64(ins), sq, gv, gp))
    assert len(raw) == len(want) and raw == want
