"""The normals' VJP entry points without a GPU: declared, exported and bound; a call fails loudly; and the float64 restatement the
GPU tests compare against (tests/normals_vjp_oracle.py) is pinned to the C oracle's normals and to finite differences."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_vjp_oracle as O  # noqa: E402

SYMBOLS = {"smplpp_face_normals_vjp": 10, "smplpp_vertex_normals_vjp": 10, "smplpp_mesh_vertex_normals_vjp": 8}


def test_normals_vjp_declared_exported_bound():
    from smplpp_amd import _lib

    L = _lib.load()
    for name, nargs in SYMBOLS.items():
        assert name in _lib.declared_symbols()
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name


def test_normals_vjp_without_gpu_raises():
    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import SMPL

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = _lib.load()
    v = np.zeros((1, 4, 3), np.float32)
    g = np.ones((1, 4, 3), np.float32)
    out = np.full((1, 4, 3), 7.0, np.float32)
    ids = np.array([0], np.int64)
    # a null model is refused before any device work
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_face_normals_vjp(None, 1, v.ctypes.data, 1, ids.ctypes.data, g.ctypes.data, out.ctypes.data, 0, 0, None))
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_vertex_normals_vjp(None, 1, v.ctypes.data, 1, ids.ctypes.data, g.ctypes.data, out.ctypes.data, 0, 0, None))
    with pytest.raises(_lib.SmplppError):
        _lib.check(L.smplpp_mesh_vertex_normals_vjp(None, 1, v.ctypes.data, g.ctypes.data, out.ctypes.data, 0, 0, None))
    s = SMPL()
    s.setDevice("cuda:0")
    with pytest.raises(_lib.SmplppError):
        s.init(model_io.tiny_model(20, seed=1))
        s.calcMeshVertexNormalsBackward(np.zeros((1, 20, 3), np.float32), np.ones((1, 20, 3), np.float32))
    assert (out == 7.0).all()


@pytest.fixture(scope="module")
def synth_verts(synth_model):
    from oracle import cpu
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(2, seed=5)
    return cpu.OracleModel(synth_model).fk(beta, theta)["verts"]


def test_oracle_forward_matches_c_oracle(synth_model, synth_verts):
    from oracle import cpu

    o = cpu.OracleModel(synth_model)
    V = synth_model["vertices_template"].shape[0]
    mesh = O.Mesh(synth_model["face_indices"].astype(np.int64) - 1, V)
    rng = np.random.default_rng(1)
    fids = rng.integers(0, len(synth_model["face_indices"]), 64)
    vids = rng.integers(0, V, 64)
    v = torch.as_tensor(synth_verts[:1], dtype=torch.float64)
    fn = O.face_normals(mesh, v, fids)[0].numpy()
    vn = O.vertex_normals(mesh, v, vids)[0].numpy()
    for i, f in enumerate(fids):
        assert np.abs(fn[i] - o.face_normal(synth_verts[0], int(f))).max() < 2e-6
    for i, u in enumerate(vids):
        assert np.abs(vn[i] - o.vertex_normal(synth_verts[0], int(u))).max() < 2e-6


def _fd_check(fn, v, g, idx, h=1e-6):
    ana = O.vjp(fn, v, g)
    for (a, b, c) in idx:
        vp, vm = v.copy(), v.copy()
        vp[a, b, c] += h
        vm[a, b, c] -= h
        num = ((fn(torch.as_tensor(vp)) - fn(torch.as_tensor(vm))) * torch.as_tensor(g)).sum().item() / (2 * h)
        assert abs(num - ana[a, b, c]) <= 1e-6 * max(1.0, abs(num)), (a, b, c, num, ana[a, b, c])


def test_oracle_gradients_match_finite_differences():
    from smplpp_amd import model_io

    md = model_io.tiny_model(30, seed=3)
    mesh = O.Mesh(md["face_indices"].astype(np.int64) - 1, 30)
    rng = np.random.default_rng(2)
    v = rng.uniform(-0.5, 0.5, (2, 30, 3))
    idx = [(int(rng.integers(2)), int(rng.integers(30)), int(rng.integers(3))) for _ in range(24)]
    fids = rng.integers(0, len(md["face_indices"]), 9)
    _fd_check(lambda x: O.face_normals(mesh, x, fids), v, rng.standard_normal((2, 9, 3)), idx)
    _fd_check(lambda x: O.vertex_normals(mesh, x), v, rng.standard_normal((2, 30, 3)), idx)
    fi = rng.integers(0, len(md["face_indices"]), (2, 4))
    w = torch.as_tensor(rng.dirichlet(np.ones(3), (2, 4)))
    off = np.array([[0.02, 0.0, 0.05, -0.01], [0.03, 0.01, 0.0, 0.02]])
    gp, gn = rng.standard_normal((2, 4, 3)), rng.standard_normal((2, 4, 3))
    _fd_check(lambda x: (O.task_surface(mesh, x, fi, w, off)[0] * torch.as_tensor(gp)).sum(-1, keepdim=True)
              + (O.task_surface(mesh, x, fi, w, off)[1] * torch.as_tensor(gn)).sum(-1, keepdim=True), v, np.ones((2, 4, 1)), idx)


def test_oracle_zero_length_branch():
    """A zero-area face: torch's normalize clamps |c| to 1e-12, so the gradient of the cross product is g / 1e-12 (finite)."""
    faces = np.array([[0, 1, 2], [0, 2, 3], [0, 0, 1]], np.int64)
    mesh = O.Mesh(faces, 5)  # vertex 4 has no faces
    v = np.zeros((1, 5, 3))
    v[0, 0] = (0.1, 0.2, 0.3)
    v[0, 1] = (0.1, 0.2, 0.3)  # face 0: v1 == v0, zero area
    v[0, 2] = (0.4, 0.2, 0.3)
    v[0, 3] = (0.1, 0.6, 0.3)
    g = np.array([[[0.3, -0.2, 0.5]]])
    got = O.vjp(lambda x: O.face_normals(mesh, x, [0]), v, g)
    assert np.isfinite(got).all()
    gc = g[0, 0] / 1e-12
    a, b = v[0, 1] - v[0, 0], v[0, 2] - v[0, 0]
    ga, gb = np.cross(b, gc), np.cross(gc, a)
    np.testing.assert_allclose(got[0, 1], ga, rtol=1e-12)
    np.testing.assert_allclose(got[0, 2], gb, rtol=1e-12)
    np.testing.assert_allclose(got[0, 0], -(ga + gb), rtol=1e-12)
    gv = O.vjp(lambda x: O.vertex_normals(mesh, x), v, np.ones((1, 5, 3)))
    assert np.isfinite(gv).all() and (gv[0, 4] == 0).all()
