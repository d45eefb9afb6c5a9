"""The scan-preparation restatement (tests/cloud_oracle.py) against definitions, on the CPU: kNN against a float64 brute force on a
cloud without near ties and on an integer lattice full of them; farthest-point sampling against a plain Python loop; the normals against
float64 eigh of the mean-centred covariance on noisy surface samples; the sphere; and the package surface without a GPU.

The constants below were measured with this file's own clouds (each test prints its figure before it asserts); the bars are four times
the measured value, the project's margin.  DESIGN §3.32 records them."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_oracle as CL  # noqa: E402

f32 = np.float32
GAP_JUDGED = 0.05         # the points judged: (l1 - l0) / l2 of the float64 definition above this
LEFT_OUT_MAX = 0.05       # at most this share of a cloud may be left out
# angle x gap of the restated normal against float64 eigh, radians: the largest of the 18 clouds below was 2.141e-7 = 3.59 * 2^-24
ANGLE_GAP_MEASURED = 2.141e-7
ANGLE_GAP_BAR = 4 * ANGLE_GAP_MEASURED
# the float64 definition's largest angle to the radial direction on the sphere cloud below (8192 points, k = 16): 0.04441 rad
SPHERE_ANGLE_MEASURED = 0.04441
SPHERE_ANGLE_BAR = 4 * SPHERE_ANGLE_MEASURED


def _angle(a, b):
    """The angle between the lines of a and b [m,3] in float64 (sign-free), by the cross product: exact near 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(1)))


# ---------------------------------------------------------------------------------------------------- kNN
@pytest.mark.parametrize("self_query", (True, False))
def test_knn_random_cloud_against_float64(self_query):
    """No two candidate distances of a query within 1e-6 relative in float64 (checked here), so float32 cannot reorder them."""
    n, K, Q, k = 2, 60, 21, 9
    p = CL.random_cloud(n, K, 11)
    q = None if self_query else CL.random_cloud(n, Q, 12)
    want_i, sorted_d = CL.knn_definition(p, k, q)
    rel = (sorted_d[..., 1:] - sorted_d[..., :-1]) / sorted_d[..., 1:]
    print("smallest relative separation of candidate distances: %.3g" % rel.min())
    assert rel.min() > 1e-6
    index, dist, count = CL.knn(p, k, q)
    assert np.array_equal(index, want_i) and (count == k).all()
    assert np.allclose(dist, sorted_d[..., :k], rtol=1e-6, atol=0)


@pytest.mark.parametrize("self_query", (True, False))
def test_knn_lattice_against_float64(self_query):
    """Integer coordinates: every distance is exact in both precisions and equal distances abound, so the order (d, j) decides."""
    n, K, Q, k = 2, 257, 40, 17
    p = CL.lattice_cloud(n, K, 21)
    q = None if self_query else CL.lattice_cloud(n, Q, 22)
    want_i, sorted_d = CL.knn_definition(p, k, q)
    ties = (sorted_d[..., 1:k] == sorted_d[..., :k - 1]).mean()
    print("share of adjacent listed ranks with equal distances: %.3f" % ties)
    assert ties > 0.3
    index, dist, count = CL.knn(p, k, q)
    assert np.array_equal(index, want_i) and (count == k).all()
    assert np.array_equal(dist.astype(np.float64), sorted_d[..., :k])
    if self_query:  # a duplicated point is listed at d = 0; the query's own index never is
        assert (dist[..., 0] == 0).any() and not (index == np.arange(K)[None, :, None]).any()


def test_knn_cap_padding_and_non_finite():
    p = CL.lattice_cloud(1, 50, 31)
    p[0, 7] = np.nan
    p[0, 9, 1] = np.inf
    q = CL.lattice_cloud(1, 6, 32)
    q[0, 2, 0] = np.nan
    index, dist, count = CL.knn(p, 8, q, max_sqdist=3.0)
    assert count[0, 2] == 0 and (index[0, 2] == -1).all()
    assert not np.isin(index, (7, 9)).any()
    for a in range(6):
        c = count[0, a]
        assert (index[0, a, c:] == -1).all() and (dist[0, a, c:] == 0).all() and (dist[0, a, :c] <= 3).all()
    assert 0 < count.sum() < 6 * 8
    index, _, count = CL.knn(p[:, :3], 5)  # k > candidates
    assert (count == 2).all() and (index[..., 2:] == -1).all()


# ---------------------------------------------------------------------------------------------------- farthest points
@pytest.mark.parametrize("cloud,K,M,start", [("lattice", 60, 60, 0), ("lattice", 97, 31, 5), ("random", 120, 40, 0), ("random", 64, 64, 63)])
def test_farthest_points_against_a_plain_loop(cloud, K, M, start):
    p = (CL.lattice_cloud if cloud == "lattice" else CL.random_cloud)(1, K, 41)
    index, radius, cover = CL.farthest_points(p, M, np.array([start]))
    li, lr, lc = CL.farthest_points_loop(p[0], M, start)
    assert np.array_equal(index[0], li) and radius[0].tobytes() == lr.tobytes() and cover[0].tobytes() == lc.tobytes()
    assert index[0, 0] == start and radius[0, 0] == np.inf and (np.diff(radius[0, 1:]) <= 0).all()
    assert len(set(index[0].tolist())) == M and (cover[0, index[0]] == 0).all()
    if M < K:  # the coverage: no point is farther from the sample than the last radius
        assert cover[0].max() <= radius[0, -1]


def test_farthest_points_special_cases():
    p = CL.lattice_cloud(2, 12, 51)
    p[0, 0] = np.nan                     # the default start is not a finite point: the lowest finite index
    p[1, 3:] = np.nan                    # fewer finite points than M
    index, radius, cover = CL.farthest_points(p, 6)
    assert index[0, 0] == 1 and (index[0] >= 0).all() and cover[0, 0] == 0
    assert (index[1, :3] >= 0).all() and (index[1, 3:] == -1).all() and (radius[1, 3:] == 0).all() and (cover[1] == 0).all()
    index, _, _ = CL.farthest_points(np.full((1, 4, 3), np.nan, f32), 2)
    assert (index == -1).all()


# ---------------------------------------------------------------------------------------------------- normals
@pytest.fixture(scope="module")
def normal_trials(synth_model):
    """The 18 clouds of the trial: (K, k, noise, restated normals, status, definition normals, definition eigenvalues)."""
    out = []
    for K in (2048, 4096):
        for noise in (0.0, 0.002, 0.005):
            p, _, _ = CL.surface_samples(synth_model, K, 1000 + K + int(noise * 1e4), noise)
            for k in (8, 16, 32):
                index, _, _ = CL.knn(p[None], k)
                nr, _, st = CL.normals(p[None], index)
                dn, lam = CL.normals_definition(p, index[0])
                out.append((K, k, noise, p, index, nr[0], st[0], dn, lam))
    return out


def test_normals_against_float64_eigh(normal_trials):
    worst, left = 0.0, 0.0
    for K, k, noise, _, _, nr, st, dn, lam in normal_trials:
        gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
        judged = gap > GAP_JUDGED
        fig = (_angle(nr[judged], dn[judged]) * gap[judged]).max()
        print("K %d k %2d noise %.3f: left out %.2f %%, angle x gap %.3g rad = %.2f * 2^-24" % (K, k, noise, 100 * (1 - judged.mean()), fig, fig * 2 ** 24))
        worst, left = max(worst, fig), max(left, 1 - judged.mean())
        assert (st == 0).all()
    print("largest angle x gap %.4g rad (bar %.4g), most left out %.2f %%" % (worst, ANGLE_GAP_BAR, 100 * left))
    assert left <= LEFT_OUT_MAX
    assert worst <= ANGLE_GAP_BAR


def test_four_sweeps_are_enough(normal_trials):
    """The constant of the rule: three sweeps leave a visible error on these clouds, four give what eight give."""
    three, four_vs_eight = 0.0, 0.0
    for K, k, noise, p, index, nr, _, dn, lam in normal_trials[::4]:
        gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
        judged = gap > GAP_JUDGED
        n3 = CL.normals(p[None], index, sweeps=3)[0][0]
        n8 = CL.normals(p[None], index, sweeps=8)[0][0]
        three = max(three, _angle(n3[judged], dn[judged]).max())
        four_vs_eight = max(four_vs_eight, _angle(nr[judged], n8[judged]).max())
    print("three sweeps: %.3g rad against float64; four against eight sweeps: %.3g rad" % (three, four_vs_eight))
    assert four_vs_eight <= ANGLE_GAP_BAR / GAP_JUDGED


def test_normals_on_a_sphere():
    """Oriented by a viewpoint at the centre every normal points inward; without one, it is radial to the angle the float64 definition
    itself shows on this cloud (the curvature of the sphere inside a neighbourhood), with the margin."""
    p = CL.sphere_cloud(8192, 61)
    index, _, _ = CL.knn(p[None], 16)
    inward, _, st = CL.normals(p[None], index, viewpoint=np.zeros(3, f32))
    assert (st == 0).all() and ((inward[0].astype(np.float64) * p).sum(1) < 0).all()
    free, curv, _ = CL.normals(p[None], index)
    dn, _ = CL.normals_definition(p, index[0])
    print("sphere: float64 definition %.4g rad from radial, restatement %.4g rad (bar %.4g); largest curvature %.3g"
          % (_angle(dn, p).max(), _angle(free[0], p).max(), SPHERE_ANGLE_BAR, curv.max()))
    assert _angle(dn, p).max() <= SPHERE_ANGLE_MEASURED * 1.001
    assert _angle(free[0], p).max() <= SPHERE_ANGLE_BAR
    big = np.abs(free[0]).argmax(1)
    assert (free[0][np.arange(len(p)), big] > 0).all()
    assert (curv >= 0).all() and curv.max() < 0.05


def test_normals_status_and_degenerate_neighbourhoods():
    p, index, status = CL.degenerate_neighbourhoods()
    nr, cv, st = CL.normals(p, index)
    assert st[0].tolist() == status[0.0]
    dead = [i for i, v in enumerate(status[0.0]) if v == 1]
    live = [i for i, v in enumerate(status[0.0]) if v != 1]
    assert (nr[0, dead] == 0).all() and (cv[0, dead] == 0).all()
    assert (np.abs(np.linalg.norm(nr[0, live].astype(np.float64), axis=1) - 1) < 1e-6).all()
    for min_gap in (0.01, 10.0):
        assert CL.normals(p, index, min_gap=min_gap)[2][0].tolist() == status[min_gap], min_gap


# ---------------------------------------------------------------------------------------------------- the package without a GPU
def test_python_surface_refuses_before_the_library():
    import __graft_entry__ as g

    g.build()
    from smplpp_amd import _lib, cloud

    names = {"smplpp_cloud_knn": 13, "smplpp_cloud_normals": 14, "smplpp_cloud_farthest_points": 11}
    assert set(names) <= set(_lib.declared_symbols())
    for name, args in names.items():  # declared, exported, and bound with the header's argument list
        fn = getattr(_lib.load(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == args and fn.restype is ctypes.c_int, name
    for name in ("knn", "estimate_normals", "normals_from_index", "farthest_points", "gather", "statistical_outlier_mask"):
        assert callable(getattr(cloud, name))
    p = CL.random_cloud(1, 5, 1)
    for bad in (lambda: cloud.knn(p, 0), lambda: cloud.knn(p, 33), lambda: cloud.knn(p[0], 3), lambda: cloud.farthest_points(p, 6),
                lambda: cloud.farthest_points(p, 0), lambda: cloud.knn(p, 3, want=("nearest",)), lambda: cloud.knn(p, 3, max_dist=-1.0)):
        with pytest.raises(_lib.SmplppError):
            bad()
    # the helpers that run in plain array arithmetic
    index = np.array([[4, -1, 0]])
    got = cloud.gather(p, index)
    assert np.array_equal(got[0, 0], p[0, 4]) and np.isnan(got[0, 1]).all() and np.array_equal(got[0, 2], p[0, 0])
    ix, d, c = CL.knn(CL.random_cloud(1, 200, 2), 8)
    far = CL.random_cloud(1, 200, 2)
    far[0, 17] += 50
    ix, d, c = CL.knn(far, 8)
    keep = cloud.statistical_outlier_mask(d, c, 2.0)
    assert keep.shape == (1, 200) and not keep[0, 17] and keep.mean() > 0.9
