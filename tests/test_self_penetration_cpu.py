"""The oracles of the self-intersection rule and the self-penetration energy, without a GPU: hand cases of the rule, the sweep against
the brute force, the synthetic rest pose, the energy against float64 finite differences, and the float32 rule against float64
beyond a margin; and the library's three entry points, exported and refusing calls without a model."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import self_penetration_oracle as SP  # noqa: E402

TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def _pairs(v, faces):
    return SP.intersections(np.asarray(v, np.float32), np.asarray(faces)).tolist()


def test_crossing_pair():
    # a vertical triangle through the interior of the horizontal one
    v = np.concatenate([TRI, [[0.2, 0.2, -0.5], [0.3, 0.25, 0.5], [0.25, 0.35, 0.5]]])
    assert _pairs(v, [[0, 1, 2], [3, 4, 5]]) == [[0, 1]]
    assert SP.brute_force(v, np.array([[0, 1, 2], [3, 4, 5]])).tolist() == [[0, 1]]


def test_shared_vertex_or_edge_excluded():
    # the second face shares a vertex (then an edge) with the first and passes through its plane
    v = np.concatenate([TRI, [[0.3, 0.3, -0.5], [0.3, 0.3, 0.5]]])
    assert _pairs(v, [[0, 1, 2], [0, 3, 4]]) == []
    assert _pairs(v, [[0, 1, 2], [0, 1, 3]]) == []


def test_disjoint_coplanar_touching_not_reported():
    disjoint = np.concatenate([TRI, TRI + [0, 0, 1.0]])
    coplanar = np.concatenate([TRI, TRI + [0.2, 0.2, 0.0]])
    # the second triangle's vertex lies on the first one's interior; its edges end there
    touching = np.concatenate([TRI, [[0.25, 0.25, 0.0], [0.3, 0.3, 1.0], [0.2, 0.4, 1.0]]])
    for v in (disjoint, coplanar, touching):
        assert _pairs(v, [[0, 1, 2], [3, 4, 5]]) == []
    # a NaN coordinate: the face intersects nothing
    v = np.concatenate([TRI, [[0.2, 0.2, -0.5], [0.3, 0.25, np.nan], [0.25, 0.35, 0.5]]])
    assert _pairs(v, [[0, 1, 2], [3, 4, 5]]) == []


def test_sweep_matches_brute_force_two_spheres():
    v, f = SP.spheres(3, [(0.0, 0.0, 0.0), (0.8, 0.05, 0.02)])
    assert len(f) == 2560
    a = SP.intersections(v, f)
    b = SP.brute_force(v, f)
    assert len(a) > 50 and np.array_equal(a, b)
    # every pair joins the two spheres (each sphere alone is embedded)
    assert ((a[:, 0] < 1280) & (a[:, 1] >= 1280)).all()


def test_synthetic_rest_pose_has_no_pairs(synth_model):
    from oracle import cpu

    faces = synth_model["face_indices"].astype(np.int64) - 1
    v = cpu.OracleModel(synth_model).fk(np.zeros((1, 10), np.float32), np.zeros((1, 25, 3), np.float32))["verts"][0]
    assert len(SP.intersections(v, faces)) == 0


def test_energy_matches_finite_differences():
    v, f = SP.spheres(2, [(0.0, 0.0, 0.0), (0.85, 0.0, 0.03)])
    P = SP.intersections(v, f)
    assert len(P) > 0
    vt = torch.tensor(v, dtype=torch.float64)
    for sigma in (0.5, 2.0, 3.0):
        e = SP.pair_energy(vt, f, P, sigma)
        assert (e >= 0).all() and (e > 0).any()
        g = np.random.default_rng(3).normal(size=len(P))
        an = SP.vjp(vt, f, P, g, sigma).numpy()
        rng = np.random.default_rng(5)
        touched = np.unique(f[P].reshape(-1))
        for k in rng.choice(touched, 8, replace=False):
            for x in range(3):
                h = 1e-7
                vp, vm = vt.clone(), vt.clone()
                vp[k, x] += h
                vm[k, x] -= h
                fd = float(((SP.pair_energy(vp, f, P, sigma) - SP.pair_energy(vm, f, P, sigma)) * torch.tensor(g)).sum()) / (2 * h)
                assert abs(fd - an[k, x]) <= 1e-6 * max(1.0, abs(an[k, x])), (sigma, k, x, fd, an[k, x])


def test_energy_pushes_intruders_out():
    # an intruder corner just below a receiver's plane: gradient descent moves it out along the receiver's normal (+z)
    v = np.concatenate([TRI, [[0.3, 0.3, -0.01], [0.3, 0.3, 0.5], [0.4, 0.2, 0.5]]]).astype(np.float64)
    f = np.array([[0, 1, 2], [3, 4, 5]])
    g = SP.vjp(torch.tensor(v), f, np.array([[0, 1]]), np.ones(1), 2.0).numpy()
    assert g[3, 2] < 0


def test_float32_agrees_with_float64_beyond_margin():
    rng = np.random.default_rng(11)
    for level, d in ((3, 0.8), (3, 0.95), (2, 0.6)):
        v, f = SP.spheres(level, [(0.0, 0.0, 0.0), (d, 0.01, 0.02)])
        v = v + rng.normal(0, 1e-3, v.shape)
        a = {tuple(p) for p in SP.intersections(v, f, np.float32).tolist()}
        b = {tuple(p) for p in SP.intersections(v.astype(np.float32), f, np.float64).tolist()}
        assert len(a) > 0
        assert a ^ b <= SP.near_degenerate(v.astype(np.float32), f, 1e-4)


def test_library_entry_points_refuse_bad_calls_without_a_gpu():
    """The three entry points are exported with their ctypes signatures and refuse a call without a model before touching a device."""
    import pytest

    import __graft_entry__ as g

    g.build()
    from smplpp_amd import _lib
    from smplpp_amd.smpl import SMPL, _ptr

    L = _lib.load()
    for name in ("smplpp_self_intersections", "smplpp_self_penetration", "smplpp_self_penetration_vjp"):
        assert getattr(L, name).argtypes is not None, name
    for name in ("selfIntersections", "selfPenetration", "selfPenetrationBackward", "self_penetration_differentiable"):
        assert callable(getattr(SMPL, name)), name
    v = np.zeros((1, 3, 3), np.float32)
    pairs, cnt, e = np.zeros((1, 4, 2), np.int64), np.zeros(1, np.int64), np.zeros((1, 4), np.float32)
    calls = ((L.smplpp_self_intersections, (None, 1, _ptr(v), 4, _ptr(pairs), _ptr(cnt), _lib.HOST, None)),
             (L.smplpp_self_penetration, (None, 1, _ptr(v), 4, 2.0, _ptr(pairs), _ptr(cnt), _ptr(e), _lib.HOST, None)),
             (L.smplpp_self_penetration_vjp, (None, 1, _ptr(v), 4, 2.0, _ptr(pairs), _ptr(cnt), _ptr(e), _ptr(v), 0, _lib.HOST, None)))
    for fn, args in calls:
        with pytest.raises(_lib.SmplppError):
            _lib.check(fn(*args))
