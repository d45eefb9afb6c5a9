"""The float64 closest-point reference (tests/closest_ref.py) against hand-made triangles and against the C oracle's exhaustive
two-pass scan: the reference's distances hold the oracle's fp32 ones within the error budget eta, and the oracle's faces pass
the band check.  No GPU."""
import numpy as np
import pytest

import closest_ref as cr


def _one(p, tri):
    D, C = cr.tri_sqdist(np.asarray(p, np.float64), *np.asarray(tri, np.float64))
    return float(D), C


def test_hand_made_triangle_regions():
    tri = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    cases = [  # (query, squared distance, closest point)
        ([0.25, 0.25, 0.5], 0.25, [0.25, 0.25, 0]),  # interior (above the face)
        ([0.25, 0.25, 0.0], 0.0, [0.25, 0.25, 0]),  # on the face
        ([0.5, -1.0, 0.0], 1.0, [0.5, 0, 0]),  # edge ab
        ([1.0, 1.0, 0.0], 0.5, [0.5, 0.5, 0]),  # edge bc
        ([-2.0, 0.5, 1.0], 5.0, [0, 0.5, 0]),  # edge ca
        ([-1.0, -1.0, 1.0], 3.0, [0, 0, 0]),  # vertex a
        ([2.0, -1.0, 0.0], 2.0, [1, 0, 0]),  # vertex b
        ([0.0, 3.0, 4.0], 20.0, [0, 1, 0]),  # vertex c
    ]
    for p, d, c in cases:
        D, C = _one(p, tri)
        assert abs(D - d) < 1e-15 and np.abs(C - c).max() < 1e-15, (p, D, C)


def test_hand_made_degenerate_triangles():
    D, C = _one([0.5, 1.0, 0.0], [[0, 0, 0], [1, 0, 0], [2, 0, 0]])  # collinear: the segments
    assert abs(D - 1.0) < 1e-15 and np.abs(C - [0.5, 0, 0]).max() < 1e-15
    D, C = _one([3.0, 1.0, 0.0], [[0, 0, 0], [2, 0, 0], [1, 0, 0]])  # collinear, beyond the far end
    assert abs(D - 2.0) < 1e-15 and np.abs(C - [2, 0, 0]).max() < 1e-15
    D, C = _one([1.0, 2.0, 2.0], [[0, 0, 0]] * 3)  # a point
    assert abs(D - 9.0) < 1e-15 and not C.any()
    faces = np.array([[0, 0, 0]])
    assert np.isinf(cr.eps_c(np.zeros((1, 3), np.float32), faces, np.ones((1, 3), np.float32))).all()


def _two_faces(dist):
    """Faces 0 (B) and 1 (A) share the edge v0-v1 (the y axis) at a convex fold; the query lies on A, `dist` from the edge."""
    v = np.array([[0.2, 0.1, 0.3], [0.2, 0.14, 0.3], [0.17, 0.12, 0.31], [0.23, 0.12, 0.29]], np.float32)
    faces = np.array([[0, 1, 2], [0, 3, 1]])
    a, b, c = v[faces[1]].astype(np.float64)
    e = (c - a) / np.linalg.norm(c - a)
    u = (b - a) - np.dot(b - a, e) * e
    u /= np.linalg.norm(u)
    p = (a + 0.5 * (c - a) + dist * u).astype(np.float32)
    return v, faces, p


@pytest.mark.parametrize("dist", [0.3e-6, 0.5e-6, 0.7e-6])
def test_band_rejects_the_higher_id_next_to_a_shared_edge(dist):
    """0.5 um from the shared edge on face 1: the exact distance to face 1 is ~0, to face 0 ~dist^2 (inside 1e-12), so the rule's
    answer is face 0, and the helper must tell the two apart — face 1 is rejected, face 0 accepted."""
    v, faces, p = _two_faces(dist)
    D = cr.mesh_sqdist(v, faces, p[None])[0]
    ec = cr.eps_c(v, faces, p[None])[0]
    assert D[1] < 1e-15 and abs(D[0] - dist * dist) < 0.05 * dist * dist
    allowed, must = cr.band(D, ec)
    assert allowed.all() and must[0]
    assert cr.check_choice(D, ec, 0) is None
    msg = cr.check_choice(D, ec, 1)
    assert msg is not None and "lower face 0" in msg
    # 2 um away the lower face is out of the band: face 1 is the only answer
    v, faces, p = _two_faces(2e-6)
    D = cr.mesh_sqdist(v, faces, p[None])[0]
    ec = cr.eps_c(v, faces, p[None])[0]
    assert cr.check_choice(D, ec, 1) is None and cr.check_choice(D, ec, 0) is not None


def test_pruned_faces_keep_a_lower_bound():
    rng = np.random.default_rng(4)
    v = rng.normal(0, 0.3, (60, 3)).astype(np.float32)
    faces = rng.integers(0, 60, (100, 3))
    P = rng.normal(0, 0.5, (20, 3)).astype(np.float32)
    D = cr.mesh_sqdist(v, faces, P)
    full = cr.tri_sqdist(P[:, None].astype(np.float64), *[v[faces[:, i]].astype(np.float64)[None] for i in range(3)])[0]
    assert (D <= full * (1 + 1e-12) + 1e-18).all()
    near = full <= full.min(axis=1, keepdims=True) * 1.01
    assert np.allclose(D[near], full[near], rtol=1e-12, atol=0)


@pytest.fixture(scope="module")
def frames(oracle_synth):
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(2, seed=5)
    theta[:, 0] *= 0.3
    return oracle_synth.fk(beta, theta, want=("verts",))["verts"]


@pytest.mark.parametrize("cls", cr.CLASSES)
def test_reference_vs_oracle(oracle_synth, synth_model, frames, cls):
    """1000 queries of the class on each of two posed frames: the oracle's fp32 squared distance is within eta of the float64
    one, its face passes the band check, and its closest point is the float64 closest point of that face."""
    faces = synth_model["face_indices"].astype(np.int64) - 1
    edges = cr.shared_edges(faces)
    rng = np.random.default_rng(cr.CLASSES.index(cls) + 100)
    for fr in range(len(frames)):
        v = frames[fr]
        P = cr.make_queries(v, faces, cls, 1000, rng, edges)
        of, oc, osq = oracle_synth.closest_points(v, P)
        D = cr.mesh_sqdist(v, faces, P, also=of)
        ec = cr.eps_c(v, faces, P)
        k = np.arange(len(P))
        Df, ef = D[k, of], ec[k, of]
        err = np.abs(osq.astype(np.float64) - Df) / cr.eta(Df, ef)
        assert (err <= 1).all(), (cls, fr, int(np.argmax(err)), float(err.max()))
        for q in range(len(P)):
            msg = cr.check_choice(D[q], ec[q], of[q])
            assert msg is None, (cls, fr, q, msg)
        tri = v[faces[of]].astype(np.float64)
        C = cr.tri_sqdist(P.astype(np.float64), tri[:, 0], tri[:, 1], tri[:, 2])[1]
        assert (np.abs(C - oc).max(axis=1) <= np.maximum(1e-6, 4 * ef)).all()
