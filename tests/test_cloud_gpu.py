"""Scan preparation on the MI355X (smplpp_cloud_knn, smplpp_cloud_normals, smplpp_cloud_farthest_points): every output bit against the
float32 restatement of tests/cloud_oracle.py at the smallest shapes that can go wrong (both sides of the LDS tile, of every list capacity,
of every form of the sampling kernel), ties, caps, points that are not finite, independence of the batch, the slot, the memory space and
the outputs asked for, canaries, the refusals, repeated calls, the C++ shim, and one chain from a single-view scan without normals to
normal-compatible correspondences."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_oracle as CL  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FILL = 7.0
TILE = 1024                                                          # CLD_TILE of cloud.hip
KNN_K = (1, 2, 8, 9, 33, 255, 256, 257, 1023, 1024, 1025, 2049)      # the cloud sizes: the tile and one either side among them
KNN_k = (1, 3, 8, 9, 16, 17, 32)                                     # both sides of the list capacities 8, 16, 32
FPS_REG = 16384                                                      # CLD_FPS_T * CLD_FPS_PPT: above it dmin lives in min_sqdist
FPS_K = (1, 2, 1023, 1024, 1025, 4096, 4097, FPS_REG, FPS_REG + 1)   # both sides of every form of the kernel (1, 4, 16 points a thread)
# The chain: the share of scan points matched with estimated normals may fall short of the share matched with the sampled faces' own
# normals by at most this.  Measured with the numpy restatements on the CPU (four seeds of the scan below): both shares were 1.0, the
# difference 0; doubled it is still 0.
CHAIN_MARGIN = 0.0


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _same(a, b):
    """The same bits (the outputs hold no NaN)."""
    a, b = np.ascontiguousarray(_host(a)), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _knn_slice(want, k):
    """The restatement at k from the one at 32: the first k ranks, the count capped."""
    index, dist, count = want
    return {"index": np.ascontiguousarray(index[..., :k]), "sqdist": np.ascontiguousarray(dist[..., :k]), "count": np.minimum(count, k).astype(np.int32)}


def _check_knn(got, want, case):
    for key in ("index", "sqdist", "count"):
        assert _same(got[key], want[key]), (case, key)


# ---------------------------------------------------------------------------------------------------- 1. kNN
@pytest.mark.parametrize("K", KNN_K)
def test_knn_bits(K):
    """Self-query and separate queries (Q != K), n = 3 and its middle frame alone, every k: the restatement once per cloud at k = 32."""
    from smplpp_amd import cloud

    Q = 70 if K != 70 else 71
    p, q = CL.random_cloud(3, K, 100 + K), CL.random_cloud(3, Q, 200 + K)
    if K >= 8:  # duplicated points: equal distances, and a neighbour at d = 0
        p[:, 5] = p[:, 2]
        q[:, 3] = p[:, 2]
    dp, dq = _dev(p), _dev(q)
    for queries, dqq in ((None, None), (q, dq)):
        want = CL.knn(p, 32, queries)
        for k in KNN_k:
            _check_knn(cloud.knn(dp, k, dqq), _knn_slice(want, k), (K, k, queries is None, 3))
            alone = cloud.knn(dp[1:2].contiguous(), k, None if dqq is None else dqq[1:2].contiguous())
            _check_knn(alone, _knn_slice(tuple(w[1:2] for w in want), k), (K, k, queries is None, 1))


def test_knn_lattice_cap_and_non_finite():
    from smplpp_amd import cloud

    K, Q = 300, 41
    p, q = CL.lattice_cloud(2, K, 301), CL.lattice_cloud(2, Q, 302)
    for k in (3, 8, 17, 32):
        _check_knn(cloud.knn(_dev(p), k), _knn_slice(CL.knn(p, 32), k), ("lattice self", k))
        _check_knn(cloud.knn(_dev(p), k, _dev(q)), _knn_slice(CL.knn(p, 32, q), k), ("lattice", k))
    # a cap that cuts lists short: lattice distances are integers, and float32 sqrt(3) squared is 3 exactly: d <= 3 is listed
    cap = float(f32(np.sqrt(3.0)) * f32(np.sqrt(3.0)))
    want = CL.knn(p, 16, q, max_sqdist=cap)
    assert 0 < want[2].min() < 16 and (want[2] < 16).any() and (want[0] == -1).any()
    _check_knn(cloud.knn(_dev(p), 16, _dev(q), max_dist=np.sqrt(3.0)), _knn_slice(want, 16), "cap")
    _check_knn(cloud.knn(_dev(p), 16, max_dist=1.0), _knn_slice(CL.knn(p, 16, max_sqdist=1.0), 16), "cap self")
    # NaN and inf among the points and the queries
    p[0, 7], p[1, 11, 2], p[0, 290, 0] = np.nan, np.inf, -np.inf
    q[0, 2, 1], q[1, 40] = np.nan, np.inf
    for k in (8, 32):
        got = cloud.knn(_dev(p), k, _dev(q))
        _check_knn(got, _knn_slice(CL.knn(p, 32, q), k), ("non-finite", k))
        assert int(got["count"][0, 2]) == 0 and int(got["count"][1, 40]) == 0
        _check_knn(cloud.knn(_dev(p), k), _knn_slice(CL.knn(p, 32), k), ("non-finite self", k))


def test_knn_space_outputs_canaries_and_repeat():
    """Host space against device space, each output alone, guard elements beside every output, and the same bits from a second call."""
    from smplpp_amd import _lib, cloud

    n, K, Q, k = 2, 257, 65, 9
    p, q = CL.random_cloud(n, K, 401), CL.random_cloud(n, Q, 402)
    want = _knn_slice(CL.knn(p, k, q), k)
    _check_knn(cloud.knn(p, k, q), want, "host")
    _check_knn(cloud.knn(p, k), _knn_slice(CL.knn(p, k), k), "host self")
    for key in want:
        assert _same(cloud.knn(_dev(p), k, _dev(q), want=(key,))[key], want[key]), key
    G = 64
    oi = torch.full((n * Q * k + 2 * G,), 9, dtype=torch.int32, device="cuda")
    od = torch.full((n * Q * k + 2 * G,), FILL, device="cuda")
    oc = torch.full((n * Q + 2 * G,), 9, dtype=torch.int32, device="cuda")
    dp, dq = _dev(p), _dev(q)
    for turn in range(2):
        rc = _lib.load().smplpp_cloud_knn(0, n, K, dp.data_ptr(), Q, dq.data_ptr(), k, float("inf"), oi.data_ptr() + 4 * G, od.data_ptr() + 4 * G,
                                          oc.data_ptr() + 4 * G, _lib.DEVICE, None)
        assert rc == 0
        torch.cuda.synchronize()
        assert _same(oi[G:-G].reshape(n, Q, k), want["index"]) and _same(od[G:-G].reshape(n, Q, k), want["sqdist"]), turn
        assert _same(oc[G:-G].reshape(n, Q), want["count"]), turn
        for t, v in ((oi, 9), (od, FILL), (oc, 9)):
            assert (t[:G] == v).all() and (t[-G:] == v).all(), turn


def test_refusals():
    """Every refusal on device tensors: SMPLPP_ERR_INVALID, and the outputs keep their values."""
    from smplpp_amd import _lib

    Lb, D = _lib.load(), _lib.DEVICE
    n, K, Q, k, M = 2, 6, 4, 3, 3
    p, q = _dev(CL.random_cloud(n, K, 1)), _dev(CL.random_cloud(n, Q, 2))
    ints = lambda *shape: torch.full(shape, 9, dtype=torch.int32, device="cuda")  # noqa: E731
    flts = lambda *shape: torch.full(shape, FILL, device="cuda")  # noqa: E731
    o = dict(ki=ints(n, K, k), kd=flts(n, K, k), kc=ints(n, K), nn=flts(n, K, 3), nc=flts(n, K), ns=ints(n, K), fi=ints(n, M), fr=flts(n, M), fd=flts(n, K))
    ix = torch.zeros((n, K, k), dtype=torch.int32, device="cuda")
    view = torch.zeros((n, 3), device="cuda")
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def knn(n_=n, K_=K, p_=p, Q_=Q, q_=None, k_=k, cap=float("inf"), i=o["ki"], d=o["kd"], c=o["kc"], space=D):
        return Lb.smplpp_cloud_knn(0, n_, K_, P(p_), Q_, P(q_), k_, cap, P(i), P(d), P(c), space, None)

    def nrm(n_=n, K_=K, p_=p, k_=k, ix_=ix, v=None, Vn=0, mg=0.0, nn=o["nn"], c=o["nc"], s=o["ns"], space=D):
        return Lb.smplpp_cloud_normals(0, n_, K_, P(p_), k_, P(ix_), P(v), Vn, mg, P(nn), P(c), P(s), space, None)

    def fps(n_=n, K_=K, p_=p, M_=M, st=None, i=o["fi"], r=o["fr"], d=o["fd"], space=D):
        return Lb.smplpp_cloud_farthest_points(0, n_, K_, P(p_), M_, P(st), P(i), P(r), P(d), space, None)

    refused = [knn(**kw) for kw in (dict(k_=0), dict(k_=33), dict(k_=-1), dict(n_=-1), dict(K_=-2), dict(q_=q, Q_=-1), dict(cap=float("nan")),
                                    dict(i=None, d=None, c=None), dict(p_=None), dict(n_=2 ** 16, K_=2 ** 14), dict(n_=2 ** 12, K_=2 ** 14, k_=32),
                                    dict(space=2))]
    refused += [nrm(**kw) for kw in (dict(k_=0), dict(n_=-1), dict(K_=-1), dict(Vn=3), dict(Vn=1), dict(v=view, Vn=5), dict(mg=-0.5),
                                     dict(mg=float("inf")), dict(mg=float("nan")), dict(nn=None, c=None, s=None), dict(p_=None), dict(ix_=None),
                                     dict(n_=2 ** 16, K_=2 ** 14), dict(space=2))]
    refused += [fps(**kw) for kw in (dict(M_=0), dict(M_=K + 1), dict(M_=-1), dict(n_=-1), dict(K_=-1), dict(d=None), dict(p_=None),
                                     dict(n_=2 ** 16, K_=2 ** 14), dict(space=2))]
    torch.cuda.synchronize()
    assert all(rc == 1 for rc in refused), refused
    for key, t in o.items():
        assert (t == (9 if t.dtype == torch.int32 else FILL)).all(), key
    # host space alone looks at the values: a neighbour index >= K and a start outside [0, K)
    hp = CL.random_cloud(1, 4, 3)
    hix = np.array([[[1, 2], [0, 4], [0, 1], [1, -1]]], np.int32)
    hn = np.full((1, 4, 3), FILL, f32)
    assert Lb.smplpp_cloud_normals(0, 1, 4, hp.ctypes.data, 2, hix.ctypes.data, None, 0, 0.0, hn.ctypes.data, None, None, _lib.HOST, None) == 1
    hs, hd = np.array([4], np.int32), np.full((1, 4), FILL, f32)
    assert Lb.smplpp_cloud_farthest_points(0, 1, 4, hp.ctypes.data, 2, hs.ctypes.data, None, None, hd.ctypes.data, _lib.HOST, None) == 1
    assert (hn == FILL).all() and (hd == FILL).all()
    # and the same calls go through once the argument is put right (n, K or Q = 0 is no work)
    assert knn() == 0 and knn(q_=q) == 0 and nrm() == 0 and nrm(v=view, Vn=n) == 0 and fps() == 0 and fps(i=None, r=None) == 0
    assert knn(n_=0) == 0 and knn(q_=q, Q_=0) == 0 and nrm(n_=0) == 0 and fps(n_=0) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 2. normals
def _check_normals(got, want, case):
    for key, w in zip(("normal", "curvature", "status"), want):
        assert _same(got[key], w), (case, key)


@pytest.mark.parametrize("k", (3, 8, 16, 32))
def test_normals_bits(k):
    """On the kernel's own kNN output (bit-equal to the restatement's, checked above): surface samples with noise, every viewpoint form,
    the middle frame alone, host space, each output alone."""
    from smplpp_amd import cloud
    from smplpp_amd import model_io

    model = model_io.synthetic_model()
    n, K = 3, 700
    p = np.stack([CL.surface_samples(model, K, 500 + f, 0.002 * f)[0] for f in range(n)])
    index = CL.knn(p, k)[0]
    dp, dix = _dev(p), _dev(index)
    views = {"none": None, "one": np.array([0.1, -0.3, 2.0], f32), "per frame": np.array([[0, 0, 2], [0, -0.36, 0.01], [3, 1, -2]], f32)}
    for name, vp in views.items():
        want = CL.normals(p, index, vp, min_gap=0.05)
        got = cloud.normals_from_index(dp, dix, viewpoint=vp, min_gap=0.05)
        _check_normals(got, want, (k, name))
        assert (want[2] == 0).any()
        one = None if vp is None else vp.reshape(-1, 3)[1 if vp.ndim == 2 else 0]
        alone = cloud.normals_from_index(dp[1:2].contiguous(), dix[1:2].contiguous(), viewpoint=one, min_gap=0.05)
        _check_normals(alone, tuple(w[1:2] for w in want), (k, name, "alone"))
    vp = views["per frame"]
    want = CL.normals(p, index, vp)
    _check_normals(cloud.normals_from_index(p, index, viewpoint=vp), want, (k, "host"))
    for key, w in zip(("normal", "curvature", "status"), want):
        assert _same(cloud.normals_from_index(dp, dix, viewpoint=vp, want=(key,))[key], w), (k, key)
    est = cloud.estimate_normals(dp, k, viewpoint=vp)
    _check_normals(est, want, (k, "estimate_normals"))
    assert _same(est["index"], index)


def test_normals_degenerate_neighbourhoods():
    """Too few neighbours, -1-padded lists, collinear and coincident neighbourhoods, a NaN point, min_gap; a capped search that leaves
    points without neighbours; coplanar lattice points (l0 = 0 exactly)."""
    from smplpp_amd import cloud

    p, index, status = CL.degenerate_neighbourhoods()
    for min_gap, st in status.items():
        got = cloud.normals_from_index(_dev(p), _dev(index), min_gap=min_gap)
        _check_normals(got, CL.normals(p, index, min_gap=min_gap), ("degenerate", min_gap))
        assert _host(got["status"])[0].tolist() == st
    # an index >= K is skipped on the device
    wild = index.copy()
    wild[0, 4, 1] = 10
    skipped = index.copy()
    skipped[0, 4, 1] = -1
    _check_normals(cloud.normals_from_index(_dev(p), _dev(wild)), CL.normals(p, skipped), "index >= K")
    # sparse cloud under a cap: lists of every length, some points alone
    q = CL.random_cloud(2, 400, 601)
    nb = CL.knn(q, 8, max_sqdist=0.09)
    assert (nb[2] == 0).any() and (nb[2] == 1).any() and (nb[2] == 8).any()
    want = CL.normals(q, nb[0], min_gap=0.1)
    assert set(np.unique(want[2]).tolist()) == {0, 1, 2}
    got = cloud.estimate_normals(_dev(q), 8, max_dist=0.3, min_gap=0.1)
    assert _same(got["index"], nb[0]) and _same(got["count"], nb[2])
    _check_normals(got, want, "capped")
    # a plane of lattice points, and a line of them
    flat = CL.lattice_cloud(1, 200, 602)
    flat[0, :, 2] = 3
    flat[0, 150:, 1] = 5
    flat[0, 150:, 0] += 20
    ix = CL.knn(flat, 8)[0]
    want = CL.normals(flat, ix, min_gap=0.01)
    assert (want[2][0, :150] == 0).any() and (want[2][0, 150:] == 2).all()
    _check_normals(cloud.normals_from_index(_dev(flat), _dev(ix), min_gap=0.01), want, "plane and line")


# ---------------------------------------------------------------------------------------------------- 3. farthest points
def _check_fps(got, want, case):
    for key, w in zip(("index", "radius_sq", "min_sqdist"), want):
        assert _same(got[key], w), (case, key)


@pytest.mark.parametrize("K", FPS_K)
def test_farthest_points_bits(K):
    """M = 1, K / 3 and K from one run of the restatement; duplicated points; three frames with their own starts up to 4097 points."""
    from smplpp_amd import cloud

    n = 3 if K <= 4097 else 1
    p = CL.random_cloud(n, K, 700 + K)
    if K >= 8:
        p[:, K // 2] = p[:, 1]
        p[:, K - 1] = p[:, 1]
    start = np.array([0, K - 1, K // 2], np.int32)[:n]
    Ms = sorted({1, max(1, K // 3), K})
    want = CL.farthest_points(p, K, start, also=Ms[:-1]) if len(Ms) > 1 else {K: CL.farthest_points(p, K, start)}
    for M in Ms:
        _check_fps(cloud.farthest_points(_dev(p), M, _dev(start)), want[M], (K, M))
    if n == 3:  # the slot and the default start
        w0 = CL.farthest_points(p[1:2], Ms[-2] if len(Ms) > 1 else K)
        _check_fps(cloud.farthest_points(_dev(p[1:2]), Ms[-2] if len(Ms) > 1 else K), w0, (K, "alone"))


def test_farthest_points_special_cases():
    from smplpp_amd import cloud

    p = CL.lattice_cloud(3, 1500, 801)         # ties in dmin: the lowest index wins
    p[0, 0] = np.nan                           # the default start is not a finite point
    p[1, 40:] = np.inf                         # fewer finite points than M
    p[2, ::3, 1] = np.nan
    for start in (None, np.array([0, 41, 3], np.int32)):   # 41 and 3: starts on points that are not finite
        want = CL.farthest_points(p, 90, start)
        assert want[0][0, 0] == 1 and (want[0][1, 40:] == -1).all() and (want[0][1, :40] >= 0).all() and (want[1][0, -1] == want[1][0, -2])
        _check_fps(cloud.farthest_points(_dev(p), 90, None if start is None else _dev(start)), want, "special")
        _check_fps(cloud.farthest_points(p, 90, start), want, "special, host")
    nan = np.full((1, 5, 3), np.nan, f32)
    _check_fps(cloud.farthest_points(_dev(nan), 3), CL.farthest_points(nan, 3), "no finite point")
    # a start out of range reads as "not a finite point" on the device; the global form with its own special points
    big = CL.lattice_cloud(1, FPS_REG + 5, 802)
    big[0, 0], big[0, 77] = np.nan, np.inf
    want = CL.farthest_points(big, 40, np.array([FPS_REG + 5], np.int32))
    got = cloud.farthest_points(_dev(big), 40, _dev(np.array([FPS_REG + 5], np.int32)))
    _check_fps(got, want, "global form")
    again = cloud.farthest_points(_dev(big), 40, _dev(np.array([FPS_REG + 5], np.int32)))
    _check_fps(again, want, "repeat")


# ---------------------------------------------------------------------------------------------------- 4. C++ shim
def test_cloud_cpp_shim(tmp_path):
    from smplpp_amd import cloud

    exe = str(tmp_path / "cloud_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cloud_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    n, K, Q, k, M = 2, 40, 7, 5, 12
    j = np.arange(n * K * 3)
    p = (((j * 7) % 23 - 11).astype(f32) * f32(0.0625) + ((j * 3) % 5).astype(f32) * f32(0.03125)).reshape(n, K, 3)
    jq = np.arange(n * Q * 3)
    q = (((jq * 5) % 19 - 9).astype(f32) * f32(0.125)).reshape(n, Q, 3)
    view = np.array([0.5, -0.25, 4.0], f32)
    a = cloud.knn(p, k, q, max_dist=0.5)
    b = cloud.knn(p, k)
    c = cloud.normals_from_index(p, b["index"], viewpoint=view, min_gap=0.01)
    d = cloud.farthest_points(p, M, np.array([3, 0], np.int32))
    want = [a["index"], a["sqdist"], a["count"], b["index"], b["sqdist"], b["count"], c["normal"], c["curvature"], c["status"], d["index"],
            d["radius_sq"], d["min_sqdist"]]
    assert (a["count"] < k).any() and (a["count"] > 0).any() and (c["status"] == 0).any()
    want = [w.astype(f32) for w in want]  # (the shim writes every tensor as float32)
    raw = open(outp, "rb").read()
    assert len(raw) == 4 * sum(v.size for v in want)
    off = 0
    for i, v in enumerate(want):
        got = np.frombuffer(raw, f32, v.size, off).reshape(v.shape)
        off += 4 * v.size
        assert _same(got, np.ascontiguousarray(v)), i


# ---------------------------------------------------------------------------------------------------- 5. one chain
def test_single_view_scan_chain(synth_model):
    """Depth sensor -> points -> thin -> normals -> compatible correspondences, without leaving the library: a front view of a posed
    body with 3 mm of noise and no normals, thinned to 2048 points, normals towards the camera, then pointMeshDistanceCompatible."""
    from smplpp_amd import cloud
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    theta = np.zeros((1, 25, 3), f32)
    theta[0, 2:] = np.random.default_rng(5).normal(0, 0.015, (23, 3))
    theta[0, 1] = [0.0, 0.3, 0.0]
    verts = s.launch(np.zeros((1, 10), f32), theta, want=("verts",))["verts"]
    camera = np.array([0.0, -0.36, 2.5], f32)
    scan, face_normal = CL.single_view_scan(synth_model, verts[0], camera, 6144, 71)
    dscan = _dev(scan[None])
    thin = cloud.farthest_points(dscan, 2048)
    assert int(thin["index"].min()) >= 0 and float(thin["min_sqdist"].max()) <= float(thin["radius_sq"][0, -1])
    pts = cloud.gather(dscan, thin["index"]).contiguous()
    true_n = face_normal[_host(thin["index"])[0]]
    est = cloud.estimate_normals(pts, 16, viewpoint=camera, min_gap=0.05)
    nr, clear = _host(est["normal"])[0].astype(np.float64), _host(est["status"])[0] == 0
    dots = (nr * true_n).sum(1)
    print("clear gap: %.4f of the points; smallest cosine to the sampled face's normal among them: %.3f" % (clear.mean(), dots[clear].min()))
    assert clear.mean() > 0.95 and (dots[clear] > 0).all()
    dverts = _dev(verts)
    m_true = s.pointMeshDistanceCompatible(dverts, pts, _dev(true_n[None].astype(f32)), cos_min=0.5)[4]
    m_est = s.pointMeshDistanceCompatible(dverts, pts, est["normal"], cos_min=0.5)[4]
    share_true, share_est = float(m_true.float().mean()), float(m_est.float().mean())
    print("matched with the faces' normals %.4f, with estimated normals %.4f" % (share_true, share_est))
    assert share_est >= share_true - CHAIN_MARGIN
