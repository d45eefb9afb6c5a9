"""Closest-point queries on the GPU against the exhaustive rule (tests/closest_ref.py): the standalone query smplpp_closest_points
and the IK re-projection (proj_scan_kernel / proj_finish_kernel, node.cpp:970-1001) in every form the dispatch of ik.hip can take.

Rule (mesh_device.h, smpl_oracle.c:521-547): among the faces whose fp32 squared distance is at most mn * (1 + 1e-6) + 1e-12, the
lowest face id wins.  The constructed queries that decide it lie 0.3 / 0.7 um from an edge on its higher-id face: there the
lower-id neighbour is inside the band although the query's own face is ~0 away."""
import re

import numpy as np
import pytest

import closest_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def smpl(synth_model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    return s


@pytest.fixture(scope="module")
def mesh(synth_model):
    faces = synth_model["face_indices"].astype(np.int64) - 1
    return faces, cr.shared_edges(faces)


def _closest_points(smpl, verts, points):
    """smplpp_closest_points on explicit vertices (SMPL.closestPoints would use the last launch's)."""
    from smplpp_amd import _lib
    from smplpp_amd._lib import HOST, check
    from smplpp_amd.smpl import _ptr

    verts = np.ascontiguousarray(verts, np.float32)
    points = np.ascontiguousarray(points, np.float32)
    n, K = points.shape[:2]
    face = np.empty((n, K), np.int64)
    closest = np.empty((n, K, 3), np.float32)
    sq = np.empty((n, K), np.float32)
    check(_lib.load().smplpp_closest_points(smpl.handle, n, _ptr(verts), K, _ptr(points), _ptr(face), _ptr(closest), _ptr(sq),
                                            HOST, None))
    return face, closest, sq


def _check_queries(v, faces, P, face, closest=None, sq=None, weights=None):
    """Band check of every chosen face, plus the closest point / squared distance / weights when given.  One frame."""
    F = len(faces)
    assert ((face >= 0) & (face < F)).all()
    D = cr.mesh_sqdist(v, faces, P, also=face)
    ec = cr.eps_c(v, faces, P)
    for q in range(len(P)):
        msg = cr.check_choice(D[q], ec[q], face[q])
        assert msg is None, (q, P[q], msg)
    k = np.arange(len(P))
    tri = np.asarray(v, np.float64)[faces[face]]
    Dc, C = cr.tri_sqdist(np.asarray(P, np.float64), tri[:, 0], tri[:, 1], tri[:, 2])
    ef = ec[k, face]
    if closest is not None:
        err = np.abs(C - closest).max(axis=1)
        assert (err <= np.maximum(1e-6, 4 * ef)).all(), (int(np.argmax(err)), float(err.max()))
    if sq is not None:
        err = np.abs(sq.astype(np.float64) - Dc) / cr.eta(Dc, ef)
        assert (err <= 1).all(), (int(np.argmax(err)), float(err.max()))
    if weights is not None:
        # area-ratio weights of the closest point: 1e-5, or a closest point's error budget over the face's smallest altitude
        L = np.max([np.linalg.norm(tri[:, (i + 1) % 3] - tri[:, i], axis=1) for i in range(3)], axis=0)
        h = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) / L
        for q in range(len(P)):
            w = cr.barycentric(C[q], tri[q])
            assert np.abs(weights[q] - w).max() <= max(1e-5, 8 * ef[q] / h[q]), (q, weights[q], w)


# ------------------------------------------------------------------------------------------------ standalone query
@pytest.mark.parametrize("n,K", [(n, K) for n in (1, 3, 37) for K in (1, 7, 48)] + [(3, 300)])
def test_closest_points_vs_exhaustive_rule(smpl, oracle_synth, mesh, n, K):
    from smplpp_amd import model_io

    faces, edges = mesh
    beta, theta = model_io.synthetic_inputs(n, seed=40 + n)
    theta[:, 0] *= 0.3
    verts = oracle_synth.fk(beta, theta, want=("verts",))["verts"]
    rng = np.random.default_rng(1000 * n + K)
    P = np.empty((n, K, 3), np.float32)
    for f in range(n):
        cls = rng.choice(len(cr.CLASSES), K)
        for c in np.unique(cls):
            P[f, cls == c] = cr.make_queries(verts[f], faces, cr.CLASSES[c], int((cls == c).sum()), rng, edges)
    face, closest, sq = _closest_points(smpl, verts, P)
    for f in range(n):
        _check_queries(verts[f], faces, P[f], face[f], closest[f], sq[f])


# ------------------------------------------------------------------------------------------------ IK re-projection
def _scan_form(n, K, F, scan_blocks=None, scan_form=-1):
    """The dispatch of ik.hip (smplpp_ik_create's scan_blocks, the SCAN_ branches of ik_iterate_enqueue): (chunks, KPR, NBT)."""
    if scan_blocks is None:
        scan_blocks = 2 * n if 256 <= n < 512 else 1536
        if n >= 512 and K <= 8 and (F + 767) // 768 <= 32:
            scan_blocks = n * ((F + 767) // 768)
    chunks = min(max(scan_blocks // n, 1), 32)
    small = (F + chunks - 1) // chunks <= 3 * 256
    many = (n >= 512 and small) if scan_form < 0 else scan_form == 0
    if K <= 8 and many:
        return chunks, 0, 3 if small else 6
    if K <= 4:
        return chunks, 2, 6
    if K <= 8:
        return chunks, 4, 6
    return chunks, 0, 3 if small else 6


def _near_edge_tasks(verts, faces, edges, K, rng):
    """Per frame: face ids and vertex weights of K tasks — 0.3 um and 0.7 um from an edge on its higher-id face, on a shared edge
    (weights 0, 1/2, 1/2) and interior, in turn.  Edges are taken between two well-shaped faces (kappa <= 4) whose coordinates
    stay below 1 m, where the band check can tell the neighbour is certainly inside the band."""
    A, B, i, j = edges
    n = len(verts)
    face = np.empty((n, K), np.int64)
    w = np.empty((n, K, 3), np.float32)
    near = np.zeros((n, K), bool)
    for f in range(n):
        t = verts[f].astype(np.float64)[faces]
        L = np.max([np.linalg.norm(t[:, (a + 1) % 3] - t[:, a], axis=1) for a in range(3)], axis=0)
        kap = L ** 2 / np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
        small = np.abs(t).max(axis=(1, 2)) < 0.95
        good = np.nonzero((kap[A] <= 4) & (kap[B] <= 4) & small[A] & small[B])[0]
        for k in range(K):
            e = good[rng.integers(len(good))]
            kind = k % 4
            face[f, k] = A[e]
            if kind < 2:
                w[f, k] = cr.near_edge_weights(t[A[e]], i[e], j[e], (0.3e-6, 0.7e-6)[kind])
                near[f, k] = True
            elif kind == 2:
                w[f, k] = 0.0
                w[f, k, i[e]] = w[f, k, j[e]] = 0.5
            else:
                w[f, k] = rng.dirichlet(np.ones(3))
    return face, w, near


def _reproject(smpl, n, K, face, w, beta, theta, env, monkeypatch, offset=None):
    """eval() at the configuration, targets := the actual positions, iterate(1): (tasks before, tasks after, mesh)."""
    from smplpp_amd.ik import IkSolver

    for k in ("SMPLPP_IK_OVERLAP", "SMPLPP_DEBUG_SYNC", "SMPLPP_SCAN_BLOCKS", "SMPLPP_SCAN_FORM", "SMPLPP_IK_DBG_STOP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = IkSolver(smpl, n, K)
    s.setTasks(face_idx=face, vertex_weights=w, target_pos=np.zeros((n, K, 3), np.float32), phi_limit=np.zeros(K),
               normal_task_weight=np.zeros(K), pos_task_weight=np.ones(K),
               normal_offset=np.zeros(K) if offset is None else offset)
    s.setConfig(beta, theta)
    s.eval()
    t0 = s.getTasks()
    s.setTasks(target_pos=t0["actual_pos"])
    s.iterate(1)
    t1 = s.getTasks()
    verts = s.getVertices()
    for k in env:
        monkeypatch.delenv(k)
    # the query the re-projection used is the iteration's own actual position (phi is locked: no tangent step); it is the
    # constructed one up to rounding (the iteration's evaluation refreshes the weights first)
    if offset is None:
        assert np.abs(t1["actual_pos"] - t0["actual_pos"]).max() < 1e-6
    return t0, t1, verts


_LIST_RE = re.compile(r"project lists: tasks (\d+), empty (\d+), overflow (\d+), nan (\d+), max cnt (\d+)")


CASES = [  # (n, K, env, expected (KPR, NBT), what the case reaches)
    (4, 3, {}, (2, 6), "paired queries, one pair"),
    (4, 5, {}, (4, 6), "paired queries, odd K"),
    (4, 6, {}, (4, 6), "paired queries"),
    (4, 6, {"SMPLPP_SCAN_FORM": "0"}, (0, 3), "queries from LDS, small chunks"),
    (4, 6, {"SMPLPP_SCAN_FORM": "0", "SMPLPP_SCAN_BLOCKS": "4"}, (0, 6), "queries from LDS, one chunk per frame"),
    (4, 17, {}, (0, 3), "K > 8, small chunks"),
    (4, 17, {"SMPLPP_SCAN_BLOCKS": "8"}, (0, 6), "K > 8, two chunks per frame"),
    (300, 3, {}, (2, 6), "two chunks per frame"),
    (512, 6, {}, (0, 3), "the default 18-chunk form"),
    (64, 48, {}, (0, 3), "finish kernel: two passes of 8 tasks in each of 4 task splits"),
]


@pytest.mark.parametrize("case", range(len(CASES)), ids=["n%d-K%d-%s" % (c[0], c[1], "-".join("%s=%s" % (k[7:], v) for k, v in c[2].items()) or "default")
                                                          for c in CASES])
def test_reprojection_vs_exhaustive_rule(smpl, oracle_synth, mesh, monkeypatch, capfd, case):
    n, K, env, form, _ = CASES[case]
    faces, edges = mesh
    F = len(faces)
    chunks, kpr, nbt = _scan_form(n, K, F, int(env["SMPLPP_SCAN_BLOCKS"]) if "SMPLPP_SCAN_BLOCKS" in env else None,
                                  int(env.get("SMPLPP_SCAN_FORM", -1)))
    assert (kpr, nbt) == form
    if n == 300:
        assert chunks == 2
    if n == 512:
        assert chunks == 18
    rng = np.random.default_rng(7 + case)
    beta = np.zeros((n, 10), np.float32)
    theta = np.zeros((n, 25, 3), np.float32)
    theta[:, 1:] = rng.normal(0, 0.15, (n, 24, 3))
    pre = smpl.launch(beta, theta, want=("verts",))["verts"]
    face, w, near = _near_edge_tasks(pre, faces, edges, K, rng)
    runs = {}
    for mode, extra in (("side stream", {}), ("one stream", {"SMPLPP_IK_OVERLAP": "0"}), ("debug sync", {"SMPLPP_DEBUG_SYNC": "1"})):
        capfd.readouterr()
        t0, t1, verts = _reproject(smpl, n, K, face, w, beta, theta, dict(env, **extra), monkeypatch)
        err = capfd.readouterr().err
        if mode == "debug sync":
            stats = _LIST_RE.findall(err)
            assert len(stats) == 1, err[-2000:]
            tasks, empty, overflow, nan, _ = map(int, stats[0])
            assert (tasks, empty, overflow, nan) == (n * K, 0, 0, 0), stats[0]
        P = t1["actual_pos"]
        got = t1["face_idx"]
        # 1: the standalone exhaustive query on the same fp32 mesh and query picks the same face, every frame
        ref, _, _ = _closest_points(smpl, verts, P)
        bad = np.argwhere(got != ref)
        if len(bad):
            f, k = bad[0]
            D = cr.mesh_sqdist(verts[f], faces, P[f, k][None], also=[got[f, k]])[0]
            pytest.fail("%s: %d of %d tasks differ from the exhaustive query; frame %d task %d: re-projection face %d (D %.4g), "
                        "exhaustive face %d (D %.4g)" % (mode, len(bad), n * K, f, k, got[f, k], D[got[f, k]], ref[f, k], D[ref[f, k]]))
        # 2 + 3: the float64 band check and the weights, on sampled frames (every near-edge query of them)
        for f in sorted({0, n // 2, n - 1}):
            D = cr.mesh_sqdist(verts[f], faces, P[f], also=face[f])
            ec = cr.eps_c(verts[f], faces, P[f])
            for k in np.nonzero(near[f])[0]:  # the precondition: the constructed query still has its lower neighbour in the band
                _, must = cr.band(D[k], ec[k])
                assert must[:face[f, k]].any(), (mode, f, k)
            _check_queries(verts[f], faces, P[f], got[f], weights=t1["vertex_weights"][f])
        runs[mode] = (got, t1["vertex_weights"])
    # the three schedules run the same kernels on the same bits
    for mode in ("one stream", "debug sync"):
        assert np.array_equal(runs[mode][0], runs["side stream"][0]) and np.array_equal(runs[mode][1], runs["side stream"][1])


def test_reprojection_list_overflow_falls_back_to_the_exhaustive_rule(smpl, oracle_synth, mesh, monkeypatch, capfd):
    """A query 0.25 m off the surface of a folded pose has thousands of faces nearer than its own: the list overflows and the
    finish kernel's exhaustive scan decides — its face still passes the checks."""
    faces, edges = mesh
    n, K = 2, 3
    rng = np.random.default_rng(0)
    theta = np.zeros((n, 25, 3), np.float32)
    theta[:, 1:] = rng.normal(0, 1.0, (24, 3))
    beta = np.zeros((n, 10), np.float32)
    pre = smpl.launch(beta, theta, want=("verts",))["verts"]
    face, w, near = _near_edge_tasks(pre, faces, edges, K, rng)
    face[:, 2] = 10806
    w[:, 2] = 1.0 / 3.0
    off = np.array([0.0, 0.0, 0.25])
    for extra in ({}, {"SMPLPP_DEBUG_SYNC": "1"}):
        capfd.readouterr()
        t0, t1, verts = _reproject(smpl, n, K, face, w, beta, theta, extra, monkeypatch, offset=off)
        err = capfd.readouterr().err
        P, got = t1["actual_pos"], t1["face_idx"]
        if extra:
            stats = _LIST_RE.findall(err)
            assert len(stats) == 1, err[-2000:]
            tasks, empty, overflow, nan, mx = map(int, stats[0])
            assert tasks == n * K and overflow == n and empty == 0 and mx > 512, stats[0]
        ref, _, _ = _closest_points(smpl, verts, P)
        assert np.array_equal(got, ref)
        for f in range(n):
            _check_queries(verts[f], faces, P[f], got[f], weights=t1["vertex_weights"][f])
