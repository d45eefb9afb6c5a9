"""The normals' VJPs on the MI355X (smplpp_face_normals_vjp, smplpp_vertex_normals_vjp, smplpp_mesh_vertex_normals_vjp): parity with
float64 autograd of the torch restatement (tests/normals_vjp_oracle.py), model variety, call semantics, the differentiable
forwards, the reference's IK Jacobian rebuilt by torch autograd, a fit through the normals and the C++ shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_vjp_oracle as O  # noqa: E402

torch = O.torch
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("face", "vertex", "mesh")


def _smpl(model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    return s


def _mesh(model):
    return O.Mesh(np.asarray(model["face_indices"], np.int64) - 1, model["vertices_template"].shape[0])


@pytest.fixture(scope="module")
def smpl(synth_model):
    return _smpl(synth_model)


@pytest.fixture(scope="module")
def mesh(synth_model):
    return _mesh(synth_model)


def _verts(s, n, seed):
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(n, seed=seed)
    return s.launch(beta, theta, want=("verts",))["verts"]


def _ids(s, kind, seed, count=123):
    rng = np.random.default_rng(seed)
    hi = s.face_num if kind == "face" else s.vertex_num
    ids = rng.integers(0, hi, count).astype(np.int64)
    ids[5] = ids[2]  # a repeated id
    return ids


def _call(s, kind, v, ids, g, out=None):
    if kind == "face":
        return s.calcNormalBackward(v, ids, g, out=out)
    if kind == "vertex":
        return s.calcVertexNormalBackward(v, ids, g, out=out)
    return s.calcMeshVertexNormalsBackward(v, g, out=out)


def _fn(mesh, kind, ids):
    if kind == "face":
        return lambda x: O.face_normals(mesh, x, ids)
    if kind == "vertex":
        return lambda x: O.vertex_normals(mesh, x, ids)
    return lambda x: O.vertex_normals(mesh, x)


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30)


def _check_frames(mesh, kind, ids, v, g, got, frames):
    fn = _fn(mesh, kind, ids)
    for f in frames:
        sl = slice(f, f + 1)
        ref = O.vjp(fn, v[sl], g[sl])
        f32 = O.vjp(fn, v[sl], g[sl], dtype=torch.float32)
        assert np.isfinite(got[sl]).all(), f
        bar = max(4 * _rel(f32, ref), 1e-5)
        err = _rel(got[sl].astype(np.float64), ref)
        assert err <= bar, (kind, f, err, bar)


@pytest.mark.parametrize("n", [1, 7, 64, 257, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_normals_vjp_parity(smpl, mesh, n, kind):
    v = _verts(smpl, n, seed=n)
    ids = None if kind == "mesh" else _ids(smpl, kind, n)
    rows = smpl.vertex_num if kind == "mesh" else len(ids)
    g = np.random.default_rng(n + 1).standard_normal((n, rows, 3)).astype(np.float32)
    got = _call(smpl, kind, v, ids, g)
    _check_frames(mesh, kind, ids, v, g, got, sorted({0, n // 2, n - 1}))


def _grid_model(side):
    """A side x side grid: V = side^2 vertices, two faces per cell."""
    from smplpp_amd import model_io

    f = []
    for r in range(side - 1):
        for c in range(side - 1):
            a, b, d, e = r * side + c, r * side + c + 1, (r + 1) * side + c, (r + 1) * side + c + 1
            f += [(a, b, e), (a, e, d)]
    return model_io.tiny_model(side * side, seed=5, faces=np.array(f, np.int64) + 1)


def _fan_verts(md, n, seed):
    rng = np.random.default_rng(seed)
    vt = md["vertices_template"].astype(np.float64)
    return (vt[None] + rng.normal(0, 0.01, (n,) + vt.shape)).astype(np.float32)


def test_normals_vjp_large_mesh_fallback():
    """V = 14400: G (V x 12 bytes) exceeds a workgroup's LDS, so the whole-mesh product runs its staged form."""
    md = _grid_model(120)
    s = _smpl(md)
    m = _mesh(md)
    v = _fan_verts(md, 3, 1)
    v[..., 2] += np.sin(3 * v[..., 0]) * 0.1
    g = np.random.default_rng(2).standard_normal((3, 14400, 3)).astype(np.float32)
    got = s.calcMeshVertexNormalsBackward(v, g)
    _check_frames(m, "mesh", None, v, g, got, [0, 2])


def test_normals_vjp_staged_matches_onchip(smpl, monkeypatch):
    """The staged whole-mesh form and the on-chip one compute the same sums in the same order: the same bits."""
    v = _verts(smpl, 9, seed=4)
    g = np.random.default_rng(5).standard_normal(v.shape).astype(np.float32)
    a = smpl.calcMeshVertexNormalsBackward(v, g)
    monkeypatch.setenv("SMPLPP_NORMALS_VJP_STAGED", "1")
    b = smpl.calcMeshVertexNormalsBackward(v, g)
    ids = _ids(smpl, "vertex", 3)
    gl = g[:, :len(ids)].copy()
    c = smpl.calcVertexNormalBackward(v, ids, gl)
    monkeypatch.delenv("SMPLPP_NORMALS_VJP_STAGED")
    d = smpl.calcVertexNormalBackward(v, ids, gl)
    assert np.array_equal(a, b) and np.array_equal(c, d)


def _double_fan_model(N):
    """Closed double cone: apex 0 and bottom centre N + 1 each meet N faces (valence N), the N ring vertices 4."""
    from smplpp_amd import model_io

    top = [(0, 1 + i, 1 + (i + 1) % N) for i in range(N)]
    bottom = [(N + 1, 1 + (i + 1) % N, 1 + i) for i in range(N)]
    faces = np.array(top + bottom, np.int64) + 1
    md = model_io.tiny_model(N + 2, seed=3, faces=faces)
    ang = 2 * np.pi * np.arange(N) / N
    vt = md["vertices_template"].copy()
    vt[0] = (0, 0, 0.25)
    vt[1:N + 1] = np.stack([0.3 * np.cos(ang), 0.3 * np.sin(ang), 0.02 * np.cos(3 * ang)], axis=1)
    vt[N + 1] = (0, 0, -0.2)
    md["vertices_template"] = vt.astype(np.float32)
    return md


@pytest.mark.parametrize("N", [12, 16, 20])
def test_normals_vjp_high_valence(N):
    """No valence limit: the apex of a 20-face fan is differentiated through all its faces."""
    md = _double_fan_model(N)
    s = _smpl(md)
    m = _mesh(md)
    v = _fan_verts(md, 4, N)
    rng = np.random.default_rng(N)
    for kind in KINDS:
        ids = None if kind == "mesh" else np.array([0, N + 1, 1, 0], np.int64)
        rows = N + 2 if kind == "mesh" else 4
        g = rng.standard_normal((4, rows, 3)).astype(np.float32)
        got = _call(s, kind, v, ids, g)
        _check_frames(m, kind, ids, v, g, got, [0, 3])


def test_normals_vjp_degenerate_and_isolated():
    """A zero-area face (two coincident corners) and a vertex without faces: finite, equal to torch's gradient (g / 1e-12 on the
    clamped branch; zero for the isolated vertex)."""
    from smplpp_amd import model_io

    faces = np.array([[0, 1, 2], [0, 2, 3], [1, 2, 3], [0, 3, 1]], np.int64)
    md = model_io.tiny_model(5, seed=2, faces=faces + 1)
    s = _smpl(md)
    m = _mesh(md)
    v = np.zeros((2, 5, 3), np.float32)
    v[:, 0] = (0.1, 0.2, 0.3)
    v[:, 1] = (0.1, 0.2, 0.3)  # coincides with vertex 0: faces 0 and 3 have zero area
    v[:, 2] = (0.4, 0.2, 0.3)
    v[:, 3] = (0.1, 0.6, 0.1)
    v[:, 4] = (1.0, 1.0, 1.0)  # in no face
    rng = np.random.default_rng(0)
    for kind in KINDS:
        ids = None if kind == "mesh" else np.array([0, 3, 1], np.int64) if kind == "face" else np.array([0, 4, 2], np.int64)
        rows = 5 if kind == "mesh" else 3
        g = (rng.standard_normal((2, rows, 3)) * 1e-12).astype(np.float32)
        got = _call(s, kind, v, ids, g)
        assert np.isfinite(got).all(), kind
        assert (got[:, 4] == 0).all(), kind
        _check_frames(m, kind, ids, v, g, got, [0, 1])


@pytest.mark.parametrize("kind", KINDS)
def test_normals_vjp_call_semantics(smpl, kind):
    n = 5
    v = _verts(smpl, n, seed=8)
    V = smpl.vertex_num
    ids = None if kind == "mesh" else _ids(smpl, kind, 8, count=20)
    rows = V if kind == "mesh" else len(ids)
    rng = np.random.default_rng(9)
    g = rng.standard_normal((n, rows, 3)).astype(np.float32)
    a = _call(smpl, kind, v, ids, g)
    # bits over two calls
    assert np.array_equal(a, _call(smpl, kind, v, ids, g))
    # accumulate = 1 adds into `out`
    base = rng.standard_normal((n, V, 3)).astype(np.float32)
    acc = base.copy()
    r = _call(smpl, kind, v, ids, g, out=acc)
    assert r is acc
    assert np.array_equal(acc, base + a)
    if kind != "mesh":
        # untouched vertices are exactly 0 with accumulate = 0 (and untouched by accumulate = 1)
        faces0 = smpl.getFaceIndex().astype(np.int64) - 1
        fl = ids if kind == "face" else np.concatenate([list(smpl.getAdjacentFaces(int(u))) for u in ids]).astype(np.int64)
        touched = np.zeros(V, bool)
        touched[faces0[fl].ravel()] = True
        assert (a[:, ~touched] == 0).all() and (acc[:, ~touched] == base[:, ~touched]).all()
        # a repeated id: the cotangents sum (the same as one id with the summed cotangent, to rounding)
        dup = np.concatenate([ids, ids[:3]])
        gd = np.concatenate([g, g[:, :3]], axis=1)
        b = _call(smpl, kind, v, dup, gd)
        g2 = g.copy()
        g2[:, :3] *= 2
        assert _rel(b, _call(smpl, kind, v, ids, g2)) < 1e-6
    # device space: the same bits; accumulate on the device too
    tv, tg = torch.from_numpy(v).cuda(), torch.from_numpy(g).cuda()
    tids = None if ids is None else torch.from_numpy(ids).cuda()
    d = _call(smpl, kind, tv, tids, tg)
    tacc = torch.from_numpy(base).cuda()
    _call(smpl, kind, tv, tids, tg, out=tacc)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), a) and np.array_equal(tacc.cpu().numpy(), acc)
    # a frame's bits do not depend on n or on its position in the batch
    for sel in ([3], [4, 3], [3, 0, 1, 2, 4, 3, 3]):
        sub = _call(smpl, kind, np.ascontiguousarray(v[sel]), ids, np.ascontiguousarray(g[sel]))
        assert np.array_equal(sub, a[sel]), sel


def test_normals_vjp_bad_arguments(smpl):
    from smplpp_amd._lib import SmplppError

    v = _verts(smpl, 1, seed=1)
    with pytest.raises(SmplppError):
        smpl.calcNormalBackward(v, np.array([smpl.face_num]), np.ones((1, 1, 3), np.float32))
    with pytest.raises(SmplppError):
        smpl.calcVertexNormalBackward(v, np.array([-1]), np.ones((1, 1, 3), np.float32))
    with pytest.raises(SmplppError):
        smpl.calcMeshVertexNormalsBackward(v, np.ones((1, 3, 3), np.float32))


def test_normals_differentiable_forward_bits_and_grad(smpl):
    n = 6
    v = _verts(smpl, n, seed=12)
    smpl.launch(*__import__("smplpp_amd.model_io", fromlist=["x"]).synthetic_inputs(n, seed=12), want=("verts",))
    fids, vids = _ids(smpl, "face", 1), _ids(smpl, "vertex", 2)
    tv = torch.from_numpy(v).cuda().requires_grad_(True)
    fn = smpl.face_normals_differentiable(tv, fids)
    vn = smpl.vertex_normals_differentiable(tv, vids)
    mn = smpl.vertex_normals_differentiable(tv)
    assert np.array_equal(fn.detach().cpu().numpy(), smpl.calcNormalBatch(fids))
    assert np.array_equal(vn.detach().cpu().numpy(), smpl.calcVertexNormalBatch(vids))
    assert np.array_equal(mn.detach().cpu().numpy(), smpl.calcMeshVertexNormals())
    rng = np.random.default_rng(3)
    gs = [rng.standard_normal(t.shape).astype(np.float32) for t in (fn, vn, mn)]
    loss = sum((t * torch.from_numpy(g).cuda()).sum() for t, g in zip((fn, vn, mn), gs))
    (grad,) = torch.autograd.grad(loss, tv)
    want = smpl.calcNormalBackward(v, fids, gs[0])
    smpl.calcVertexNormalBackward(v, vids, gs[1], out=want)
    smpl.calcMeshVertexNormalsBackward(v, gs[2], out=want)
    assert _rel(grad.cpu().numpy().astype(np.float64), want.astype(np.float64)) < 1e-6


# ---- the IK Jacobian of node/node.cpp:803-869 rebuilt with torch autograd
def _rebuild_J(smpl, beta, theta, faces, bary, tangents, tp, tn, pw, nw, phil, off):
    """Rows [4K, 75 + 2K + 10] of the reference's J for one frame: posError / normalError (node.cpp:806-818) through
    forward_differentiable -> task_surface_differentiable, with the vertex weights a torch calcTriangleVertexWeights of
    pos0 + tangents phi (IkTask::calcVertexWeights, src/IkTask.cpp:47-56) so that phi has its columns."""
    from smplpp_amd.ik import task_surface_differentiable

    K = len(faces)
    dev = torch.device("cuda")
    b = torch.from_numpy(np.asarray(beta, np.float32).reshape(1, 10)).to(dev).requires_grad_(True)
    t = torch.from_numpy(np.asarray(theta, np.float32).reshape(1, 25, 3)).to(dev).requires_grad_(True)
    phi = torch.zeros(1, K, 2, device=dev, requires_grad=True)
    verts, _ = smpl.forward_differentiable(b, t)
    fi = torch.from_numpy(np.asarray(faces, np.int64).reshape(1, K)).to(dev)
    offs = torch.from_numpy(np.asarray(off, np.float32).reshape(1, K)).to(dev)
    with torch.no_grad():
        pos0, _ = task_surface_differentiable(smpl, verts, fi, torch.from_numpy(np.asarray(bary, np.float32)).to(dev)[None], offs)
        faces0 = torch.from_numpy(smpl.getFaceIndex().astype(np.int64) - 1).to(dev)
        tri = verts[0][faces0[fi[0]]][None]  # [1,K,3,3], detached like the reference's clone().detach()
    T = torch.from_numpy(np.asarray(tangents, np.float32)).to(dev)[None]  # [1,K,3,2]
    w = O.triangle_vertex_weights(pos0 + (T @ phi[..., None])[..., 0], tri)
    pos, nrm = task_surface_differentiable(smpl, verts, fi, w, offs)
    tpt, tnt = torch.from_numpy(np.asarray(tp, np.float32)).to(dev), torch.from_numpy(np.asarray(tn, np.float32)).to(dev)
    pe = torch.from_numpy(np.asarray(pw, np.float32)).to(dev)[:, None] * (pos[0] - tpt)
    ne = torch.from_numpy(np.asarray(nw, np.float32)).to(dev) * ((nrm[0] * tnt).sum(-1) + 1.0)
    D = 75 + 2 * K + 10
    J = np.zeros((4 * K, D))
    for k in range(K):
        for r, y in enumerate([pe[k, 0], pe[k, 1], pe[k, 2], ne[k]]):
            if r == 3 and nw[k] <= 0:
                continue
            gt, gp, gb = torch.autograd.grad(y, (t, phi, b), retain_graph=True, allow_unused=True)
            row = J[4 * k + r]
            row[:75] = gt.reshape(-1).double().cpu().numpy()
            if phil[k] > 0 and gp is not None:
                row[75:75 + 2 * K] = gp.reshape(-1).double().cpu().numpy()
            row[D - 10:] = gb.reshape(-1).double().cpu().numpy()
    return J, w.detach().cpu().numpy()[0]


def _ik_config(K, seed):
    from smplpp_amd import model_io

    rng = np.random.default_rng(seed)
    beta, theta = model_io.synthetic_inputs(2, seed=seed)
    theta[0, 1:] *= 0.5
    bary = rng.dirichlet(np.ones(3) * 4, size=K).astype(np.float32)
    tp = rng.normal(0, 0.3, (K, 3)).astype(np.float32)
    tn = rng.normal(0, 1, (K, 3)).astype(np.float32)
    tn /= np.linalg.norm(tn, axis=1, keepdims=True)
    pw = np.full(K, 1.0)
    nw = np.linspace(0.5, 1.5, K)
    phil = np.full(K, 0.04)
    off = np.linspace(0.01, 0.03, K)
    return beta[0], theta[0], bary, tp, tn, pw, nw, phil, off


def _check_rows(J, want, K):
    for k in range(K):
        for name, rows in (("pos", slice(4 * k, 4 * k + 3)), ("normal", slice(4 * k + 3, 4 * k + 4))):
            err = _rel(J[rows], want[rows])
            assert err <= 1e-4, (k, name, err)


def test_normals_vjp_rebuilds_reference_ik_jacobian(synth_model, smpl):
    """Capstone: every row block of the reference's libtorch-autograd J (θ, φ and β columns; position rows with normal offsets
    and normal rows) from torch autograd through the engine's FK and normals VJPs, to 1e-4 relative."""
    from oracle import ref

    if not ref.available():
        pytest.skip("reference build (oracle/_ref) not present")
    from smplpp_amd.ik import reference_task_faces

    K = 6
    _, faces = reference_task_faces(K)
    rm = ref.RefModel(synth_model)
    for seed in (1, 2):
        beta, theta, bary, tp, tn, pw, nw, phil, off = _ik_config(K, seed)
        r = rm.ik_eval(beta, theta, faces, tp, tn, pw, nw, phil, off, bary, optimize_beta=True)
        J, w = _rebuild_J(smpl, beta, theta, faces, bary, r["tangents"], tp, tn, pw, nw, phil, off)
        assert np.abs(w - r["vertex_weights"]).max() < 1e-4
        _check_rows(J, r["J"], K)


def test_normals_vjp_rebuilds_engine_ik_jacobian(synth_model, smpl):
    """The same rebuild against smplpp_ik_eval's analytic J in exact mode (no reference needed)."""
    from smplpp_amd.ik import IkSolver, reference_task_faces

    K = 6
    _, faces = reference_task_faces(K)
    beta, theta, bary, tp, tn, pw, nw, phil, off = _ik_config(K, 3)
    sol = IkSolver(smpl, 1, K, exact=True)
    sol.setTasks(face_idx=faces, vertex_weights=bary, target_pos=tp, target_normal=tn, pos_task_weight=pw, normal_task_weight=nw,
                 phi_limit=phil, normal_offset=off)
    sol.setConfig(beta[None], theta[None])
    _, Je = sol.eval(optimize_beta=True)
    tasks = sol.getTasks()
    J, w = _rebuild_J(smpl, beta, theta, faces, bary, tasks["tangents"][0], tp, tn, pw, nw, phil, off)
    assert np.abs(w - tasks["vertex_weights"][0]).max() < 1e-4
    _check_rows(J, Je[0], K)


def test_normals_adam_fit_through_normals(synth_model, smpl):
    """An Adam fit of θ whose loss has offset positions and normal terms, written only with forward_differentiable and
    task_surface_differentiable, reaches the target pose's residual; with the normal terms detached the normals are not matched."""
    from smplpp_amd.ik import reference_task_faces, task_surface_differentiable

    K = 6
    _, faces = reference_task_faces(K)
    dev = torch.device("cuda")
    rng = np.random.default_rng(7)
    theta_t = np.zeros((1, 25, 3), np.float32)
    theta_t[0, 1:] = rng.normal(0, 0.25, (24, 3))
    beta = torch.zeros(1, 10, device=dev)
    fi = torch.from_numpy(faces[None]).to(dev)
    w = torch.from_numpy(rng.dirichlet(np.ones(3) * 4, size=(1, K)).astype(np.float32)).to(dev)
    off = torch.full((1, K), 0.02, device=dev)
    with torch.no_grad():
        vt, _ = smpl.forward_differentiable(beta, torch.from_numpy(theta_t).to(dev))
        tpos, tnrm = task_surface_differentiable(smpl, vt, fi, w, off)

    def fit(detach_normals):
        th = torch.zeros(1, 25, 3, device=dev)
        th[0, 0] = torch.from_numpy(theta_t[0, 0]).to(dev)
        th.requires_grad_(True)
        opt = torch.optim.Adam([th], lr=0.02)
        for _ in range(300):
            opt.zero_grad()
            v, _ = smpl.forward_differentiable(beta, th)
            pos, nrm = task_surface_differentiable(smpl, v, fi, w, off)
            if detach_normals:
                nrm = nrm.detach()
            loss = ((pos - tpos) ** 2).sum() + 0.05 * (1.0 - (nrm * tnrm).sum(-1)).sum()
            loss.backward()
            opt.step()
        with torch.no_grad():
            v, _ = smpl.forward_differentiable(beta, th)
            pos, nrm = task_surface_differentiable(smpl, v, fi, w, off)
            return float((pos - tpos).norm(dim=-1).max()), float((1.0 - (nrm * tnrm).sum(-1)).max())

    pe, ne = fit(False)
    assert pe < 1e-2 and ne < 1e-3, (pe, ne)
    _, ne_det = fit(True)
    assert ne_det > 5 * ne, (ne_det, ne)


def test_normals_vjp_cpp_shim(tmp_path):
    from smplpp_amd import model_io

    exe = str(tmp_path / "normals_vjp_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "normals_vjp_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "g.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    got = np.fromfile(outp, np.float32)
    # the program's inputs, restated
    n, V = 2, 40
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    gm = ((np.arange(n * V * 3, dtype=np.float32).reshape(n, V, 3) % 13) - 6) * np.float32(0.1)
    g1 = ((np.arange(n * 12, dtype=np.float32).reshape(n, 4, 3) % 5) - 2) * np.float32(0.1)
    g2 = ((np.arange(n * 12, dtype=np.float32).reshape(n, 4, 3) % 3) - 1) * np.float32(0.2)
    s = _smpl(model)
    v = s.launch(beta, theta, want=("verts",))["verts"]
    ids = np.array([3, 7, 3, 11], np.int64)
    want = s.calcMeshVertexNormalsBackward(v, gm)
    s.calcVertexNormalBackward(v, ids, g1, out=want)
    s.calcNormalBackward(v, ids, g2, out=want)
    assert got.shape == want.reshape(-1).shape
    assert np.array_equal(got, want.reshape(-1))
