"""The normal-compatible, distance-capped correspondences on the MI355X (smplpp_point_mesh_distance_compatible,
smplpp_mesh_point_distance_compatible): without a filter the bits of the existing calls at every size class and in both dispatch
forms; with one normal per frame the bits of the existing search run on a second model that holds only the compatible faces; with a
normal per query the exhaustive float64 rule of tests/closest_ref.py on the candidate set and, mesh to point, the bits of the numpy
restatement of tests/scan_compat_oracle.py; the cap on and just below an attained distance; two facing sheets (the case the filter
exists for); independence of batch, slot, space, split and nullable outputs; non-finite rows; refusals; gradients through the
autograd wrappers against float64; and the C++ shim."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import closest_ref as cr  # noqa: E402
import mesh_point_distance_oracle as MO  # noqa: E402
import point_distance_oracle as PO  # noqa: E402
import scan_compat_oracle as O  # noqa: E402
from distance_cases import _rel, _same_bits, _surface_points, _verts  # noqa: E402

torch = PO.torch
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("query", "tiled")
INF = float("inf")


def _smpl(model, form="auto"):
    from smplpp_amd.smpl import SMPL

    old = os.environ.pop("SMPLPP_POINT_DISTANCE_FORM", None)
    try:
        if form != "auto":
            os.environ["SMPLPP_POINT_DISTANCE_FORM"] = form  # read once, at model creation
        s = SMPL()
        s.setDevice("cuda:0")
        s.init(model)
    finally:
        os.environ.pop("SMPLPP_POINT_DISTANCE_FORM", None)
        if old is not None:
            os.environ["SMPLPP_POINT_DISTANCE_FORM"] = old
    return s


@pytest.fixture(scope="module")
def forms(synth_model):
    return {f: _smpl(synth_model, f) for f in FORMS}


@pytest.fixture(scope="module")
def faces(synth_model):
    return synth_model["face_indices"].astype(np.int64) - 1


@pytest.fixture(scope="module")
def tiny():
    """A model of 288 vertices: two 12 x 12 sheets, A (faces 0..241, normal +z) and B (faces 242..483, normal -z)."""
    from smplpp_amd import model_io

    G = 12
    quad = np.array([(i * G + j, i * G + j + 1, (i + 1) * G + j, (i + 1) * G + j + 1) for i in range(G - 1) for j in range(G - 1)])
    fa = np.concatenate([quad[:, [0, 2, 1]], quad[:, [1, 2, 3]]])  # x = i, y = j: (0, G, 1) turns counter-clockwise about +z
    fb = fa[:, [0, 2, 1]] + G * G
    tf = np.concatenate([fa, fb])
    model = model_io.tiny_model(2 * G * G, seed=3, faces=tf + 1)
    ij = np.stack(np.meshgrid(np.arange(G), np.arange(G), indexing="ij"), -1).reshape(-1, 2) * 0.01
    sheet = np.concatenate([np.c_[ij, np.zeros(G * G)], np.c_[ij, np.full(G * G, 0.02)]]).astype(np.float32)
    return dict(model=model, faces=tf, sheet=sheet, FA=len(fa), forms={f: _smpl(model, f) for f in FORMS})


def _far(P, rng, frac=0.1, dist=0.25):
    far = rng.random(P.shape[:2]) < frac
    P[far] += np.float32(dist) * rng.normal(size=(int(far.sum()), 3)).astype(np.float32)
    return P


def _scan(v, faces, K, rng, off=0.015):
    """K scan-like points per frame with the normal of the face each was sampled from: (points, normals), float32."""
    n = len(v)
    P, N = np.empty((n, K, 3), np.float32), np.empty((n, K, 3), np.float32)
    for f in range(n):
        fid = rng.integers(0, len(faces), K)
        w = rng.dirichlet(np.ones(3), K)
        nrm = cr.face_normals(v[f], faces)[fid]
        tri = v[f].astype(np.float64)[faces[fid]]
        P[f] = np.einsum("ki,kix->kx", w, tri) + rng.uniform(-off, off, (K, 1)) * nrm
        N[f] = nrm
    return P, N


def _mixed_normals(N, rng):
    """The sampled faces' normals, of any length, a third of them turned at random, some reversed, some zero or non-finite."""
    N = (N * 10.0 ** rng.uniform(-2, 2, N.shape[:2] + (1,))).astype(np.float32)
    r = rng.random(N.shape[:2])
    t = r < 0.33
    N[t] = rng.normal(size=(int(t.sum()), 3)).astype(np.float32)
    N[(r >= 0.33) & (r < 0.45)] *= -1
    N[(r >= 0.45) & (r < 0.48)] = 0
    N[(r >= 0.48) & (r < 0.50), 1] = np.nan
    N[(r >= 0.50) & (r < 0.52), 2] = np.inf
    return N


def _assert_same_across_forms(a, b, v, faces):
    """Two dispatch forms of the point-to-mesh call: face, closest, sqdist and matched bit for bit.  The weights come from an
    evaluation inlined into each form's kernel, as in smplpp_point_mesh_distance, whose two forms fuse its products differently
    (the difference grows with a sliver's condition number); they are held to the bits of the existing call form by form, and here
    each form's to the bar test_point_distance_gpu.py::test_weights sets: they sum to 1 and rebuild the one closest point to 1e-6."""
    face, w, closest, sq, matched = a
    for x, y in zip((face, closest, sq, matched), (b[0], b[2], b[3], b[4])):
        assert _same_bits(x, y)
    tri = np.stack([v[f][faces[np.maximum(face[f], 0)]] for f in range(len(v))]).astype(np.float64)
    for wf in (w, b[1]):
        rec = np.einsum("nkj,nkjx->nkx", wf.astype(np.float64), tri)
        assert np.abs(rec - closest)[matched].max() <= 1e-6 * (1 + np.abs(tri).max())
        assert np.abs(wf.sum(-1) - 1)[matched].max() <= 1e-6 and (wf[matched] >= -2e-6).all()


def _unmatched_rows_are_zero(ids, *rest):
    un = ids < 0
    assert (ids[un] == -1).all()
    for a in rest:
        assert (a[un] == 0).all() and not np.signbit(a[un]).any()


# ---------------------------------------------------------------------------------------------------- no filter: the existing bits
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,K", [(3, 1), (2, 63), (5, 64), (2, 257), (1, 4096)])
def test_point_mesh_unfiltered_is_the_existing_call(forms, faces, form, n, K):
    s = forms[form]
    v = _verts(s, n, seed=K)
    rng = np.random.default_rng(n * 1000 + K)
    P = _far(_surface_points(v, faces, K, rng), rng)
    want = s.pointMeshDistance(v, P)
    got = s.pointMeshDistanceCompatible(v, P, None)
    assert got[4].all() and got[4].dtype == bool
    for a, b, name in zip(got, want, ("face", "weights", "closest", "sqdist")):
        assert _same_bits(a, b), (name, np.nonzero(np.asarray(a != b).reshape(n, K, -1).any(-1)))


@pytest.mark.parametrize("K", [1, 255, 1024, 1025, 2600])
def test_mesh_point_unfiltered_is_the_existing_call(forms, faces, K):
    s = forms["query"]
    v = _verts(s, 1, seed=K)
    rng = np.random.default_rng(K)
    P = _far(_surface_points(v, faces, K, rng), rng)
    wi, ws = s.meshPointDistance(v, P)
    gi, gs, gm = s.meshPointDistanceCompatible(v, P, None)
    assert _same_bits(gi, wi) and _same_bits(gs, ws) and gm.all()


def test_many_frames_tiny_model(tiny):
    """2100 frames of 288 vertices: the mesh-to-point call does not split K (2100 workgroups), a frame alone does (K = 700 in two
    chunks).  Without a filter the existing bits in both directions; with one the bits of a frame alone."""
    n, K, slot = 2100, 700, 1234
    rng = np.random.default_rng(8)
    v = (tiny["sheet"][None] + rng.normal(0, 0.002, (n, 288, 3))).astype(np.float32)
    P = (rng.uniform(-0.01, 0.12, (n, K, 3)) * (1, 1, 0.25)).astype(np.float32)
    N = rng.normal(size=(n, K, 3)).astype(np.float32)
    vn = rng.normal(size=(n, 288, 3)).astype(np.float32)
    one = slice(slot, slot + 1)
    for form in FORMS:
        s = tiny["forms"][form]
        wi, ws = s.meshPointDistance(v, P)
        gi, gs, _ = s.meshPointDistanceCompatible(v, P, None)
        assert _same_bits(gi, wi) and _same_bits(gs, ws)
        Kq = 5  # 10500 queries
        want = s.pointMeshDistance(v, P[:, :Kq])
        got = s.pointMeshDistanceCompatible(v, P[:, :Kq], None)
        assert all(_same_bits(a, b) for a, b in zip(got, want))
        # filtered: the frame inside the batch and alone
        bi, bs, bm = s.meshPointDistanceCompatible(v, P, N, vert_normals=vn, cos_min=0.3, max_dist=0.006)
        ai, asq, _ = s.meshPointDistanceCompatible(v[one], P[one], N[one], vert_normals=vn[one], cos_min=0.3, max_dist=0.006)
        assert _same_bits(ai, bi[one]) and _same_bits(asq, bs[one])
        ri, rs = O.mesh_point_forward(v[one], vn[one], P[one], N[one], 0.3, np.float32(0.006) * np.float32(0.006))
        assert _same_bits(ai, ri) and _same_bits(asq, rs)
        assert 0.02 < bm.mean() < 0.98
        bf = s.pointMeshDistanceCompatible(v, P[:, :Kq], N[:, :Kq], cos_min=0.3, max_dist=0.006)
        af = s.pointMeshDistanceCompatible(v[one], P[one, :Kq], N[one, :Kq], cos_min=0.3, max_dist=0.006)
        assert all(_same_bits(a, b[one]) for a, b in zip(af, bf))


# ---------------------------------------------------------------------------------------------------- one normal per frame
@pytest.mark.parametrize("cos_min", [0.0, 0.5])
def test_shared_normal_is_the_existing_search_on_the_compatible_faces(forms, synth_model, faces, cos_min):
    """Every query of a frame carries the frame's normal q, so the candidate set is one face subset per frame.  A second model
    whose face list is that subset, in ascending id, goes through the existing smplpp_point_mesh_distance in the same form; with its
    ids mapped back, face, weights, closest and sqdist must agree bit for bit, in both forms (F = 13776 is no multiple of either
    tile)."""
    n, K = 2, 200
    v = _verts(forms["query"], n, seed=77)
    rng = np.random.default_rng(77)
    P = _far(_surface_points(v, faces, K, rng), rng)
    q = np.array([[0.3, -2.0, 0.4], [-0.001, 0.0005, 0.002]], np.float32)
    N = np.repeat(q[:, None, :], K, 1)
    subsets = [np.nonzero(O.compatible(O.face_normals(v[f], faces), q[f], cos_min))[0] for f in range(n)]
    for form in FORMS:
        want = []
        for f, ids in enumerate(subsets):
            assert 1000 < len(ids) < len(faces) - 1000
            sub = dict(synth_model)
            sub["face_indices"] = faces[ids] + 1
            r = _smpl(sub, form).pointMeshDistance(v[f:f + 1], P[f:f + 1])
            want.append((ids[r[0]],) + tuple(r[1:]))
        want = [np.concatenate([w[i] for w in want]) for i in range(4)]
        assert (want[0] != forms[form].pointMeshDistance(v, P)[0]).mean() > 0.2  # the filter changes the answer
        got = forms[form].pointMeshDistanceCompatible(v, P, N, cos_min=cos_min)
        assert got[4].all()
        for a, b, name in zip(got, want, ("face", "weights", "closest", "sqdist")):
            assert _same_bits(a, b), (form, name, np.nonzero(np.asarray(a != b).reshape(n, K, -1).any(-1)))


# ---------------------------------------------------------------------------------------------------- a normal per query
def test_point_mesh_per_query_normals(forms, faces):
    n, K = 2, 64
    v = _verts(forms["query"], n, seed=78)
    rng = np.random.default_rng(78)
    P, N = _scan(v, faces, K, rng)
    N = _mixed_normals(N, rng)
    P[1, 5] = np.nan
    P[0, 9, 2] = np.inf
    results = {form: forms[form].pointMeshDistanceCompatible(v, P, N, cos_min=0.5) for form in FORMS}
    _assert_same_across_forms(results["query"], results["tiled"], v, faces)
    face, w, closest, sq, matched = results["tiled"]
    _unmatched_rows_are_zero(face, w, closest, sq)
    assert (matched == (face >= 0)).all()
    for f in range(n):
        cand = O.candidates(v[f], faces, P[f], N[f], 0.5)
        assert ((face[f] < 0) == ~cand.any(1)).all()  # the unmatched set, exactly
        msg = O.masked_choice_check(v[f], faces, P[f], cand, face[f])
        assert msg is None, (f, msg)
    assert 0.5 < matched.mean() < 1 and not matched[1, 5] and not matched[0, 9]


@pytest.mark.parametrize("n,K", [(1, 1500), (2, 300)])  # K split in five chunks; no split
def test_mesh_point_per_vertex_normals_bits(forms, faces, n, K):
    s = forms["query"]
    v = _verts(s, n, seed=K + 3)
    vn = np.ascontiguousarray(s.calcMeshVertexNormals())  # of the launch _verts made
    rng = np.random.default_rng(K)
    P, N = _scan(v, faces, K, rng)
    N = _mixed_normals(N, rng)
    P[0, 4] = np.nan
    cap = np.float32(0.02) * np.float32(0.02)
    gi, gs, gm = s.meshPointDistanceCompatible(v, P, N, cos_min=0.5, max_dist=0.02)  # the library's own vertex normals
    ri, rs = O.mesh_point_forward(v, vn, P, N, 0.5, cap)
    assert _same_bits(gi, ri) and _same_bits(gs, rs), np.nonzero(gi != ri)
    _unmatched_rows_are_zero(gi, gs)
    assert 0.02 < gm.mean() < 0.95 and not (gi[0] == 4).any()
    # the caller's normals: unnormalised, some zero or non-finite, and pairs whose dot product is zero only when nothing is fused
    vn2 = _mixed_normals(vn.copy(), rng)
    a = np.float32(1 + 2.0 ** -12)
    vn2[:, 100:140] = (a, a, 0)
    N2 = N.copy()
    N2[:, 0:K:2] = (a, -a, 0)
    N2[:, 1:K:2] = (-a, a, 0)
    gi, gs, gm = s.meshPointDistanceCompatible(v, P, N2, vert_normals=vn2, cos_min=0.0)
    ri, rs = O.mesh_point_forward(v, vn2, P, N2, 0.0, np.inf)
    assert _same_bits(gi, ri) and _same_bits(gs, rs), np.nonzero(gi != ri)
    assert gm[:, 100:140].all()
    wi, _ = s.meshPointDistance(v, P)
    assert (gi[:, 100:140] == wi[:, 100:140]).all()  # s = 0 exactly for every point: compatible at cos_min = 0


# ---------------------------------------------------------------------------------------------------- the cap
def test_cap_on_and_below_an_attained_distance(forms, faces):
    n, K = 1, 300
    v = _verts(forms["query"], n, seed=79)
    rng = np.random.default_rng(79)
    P, _ = _scan(v, faces, K, rng)
    for form in FORMS:
        s = forms[form]
        base = s.pointMeshDistance(v, P)
        k = int(np.argsort(base[3][0])[K // 2])
        cap = base[3][0, k]
        on = s.pointMeshDistanceCompatible(v, P, None, max_sqdist=cap)
        below = s.pointMeshDistanceCompatible(v, P, None, max_sqdist=np.nextafter(cap, np.float32(0)))
        assert on[4][0, k] and all(_same_bits(a[0, k], b[0, k]) for a, b in zip(on, base))  # <= keeps it
        assert not below[4][0, k]
        for r in (on, below):
            keep = r[4]
            assert (keep == (base[3] <= (cap if r is on else np.nextafter(cap, np.float32(0))))).all()
            assert all(_same_bits(a[keep], b[keep]) for a, b in zip(r, base))
            _unmatched_rows_are_zero(*r[:4])
        assert on[4].sum() == below[4].sum() + 1 == K // 2 + 1
    s = forms["query"]
    wi, ws = s.meshPointDistance(v, P)
    u = int(np.argsort(ws[0])[3000])
    cap = ws[0, u]
    for c in (cap, np.nextafter(cap, np.float32(0))):
        gi, gs, gm = s.meshPointDistanceCompatible(v, P, None, max_sqdist=c)
        assert (gm == (ws <= c)).all() and _same_bits(gi[gm], wi[gm]) and _same_bits(gs[gm], ws[gm])
        _unmatched_rows_are_zero(gi, gs)
        assert bool(gm[0, u]) == (c == cap)


# ---------------------------------------------------------------------------------------------------- what the filter is for
def test_two_facing_sheets(tiny):
    """Sheet A (z = 0, normal +z) and sheet B (z = 2 cm, normal -z); scan points 1.2 cm above A carry A's normal.  The plain
    nearest face is on B for every one of them; the compatible search finds A; capped below 1.2 cm nothing matches."""
    rng = np.random.default_rng(6)
    K = 100
    v = tiny["sheet"][None]
    P = np.c_[rng.uniform(0.01, 0.10, (K, 2)), np.full(K, 0.012)].astype(np.float32)[None]
    N = np.repeat(np.array([[[0, 0, 1]]], np.float32), K, 1)
    for form in FORMS:
        s = tiny["forms"][form]
        plain = s.pointMeshDistance(v, P)
        assert (plain[0] >= tiny["FA"]).all() and np.allclose(plain[3], 0.008 ** 2, rtol=1e-3)
        face, w, closest, sq, matched = s.pointMeshDistanceCompatible(v, P, N, cos_min=0.5)
        assert matched.all() and (face < tiny["FA"]).all() and np.allclose(sq, 0.012 ** 2, rtol=1e-3)
        assert np.abs(closest[..., 2]).max() == 0 and np.abs(closest[..., :2] - P[..., :2]).max() <= 1e-6
        r = s.pointMeshDistanceCompatible(v, P, N, cos_min=0.5, max_dist=0.0119)
        assert not r[4].any()
        _unmatched_rows_are_zero(*r[:4])
        # the mesh side: A's vertices see only the points with A's orientation
        N2 = N.copy()
        N2[0, ::2] = (0, 0, -1)
        index, _, m = s.meshPointDistanceCompatible(v, P, N2, cos_min=0.5)
        assert m.all() and (index[0, :144] % 2 == 1).all() and (index[0, 144:] % 2 == 0).all()


# ---------------------------------------------------------------------------------------------------- invariance
def test_invariance_batch_slot_space_repeat_nullable(forms, faces):
    from smplpp_amd import _lib
    from smplpp_amd.smpl import _ptr

    n, K = 4, 300
    v = _verts(forms["query"], n, seed=80)
    vn = np.ascontiguousarray(forms["query"].calcMeshVertexNormals())
    rng = np.random.default_rng(80)
    P, N = _scan(v, faces, K, rng)
    N = _mixed_normals(N, rng)
    P[2, 7] = np.nan
    kw = dict(cos_min=0.4, max_dist=0.05)
    first = None
    for form in FORMS:
        s = forms[form]
        ref = s.pointMeshDistanceCompatible(v, P, N, **kw) + s.meshPointDistanceCompatible(v, P, N, vert_normals=vn, **kw)
        if first is None:
            first = ref
        _assert_same_across_forms(ref[:5], first[:5], v, faces)
        assert all(_same_bits(a, b) for a, b in zip(ref[5:], first[5:]))
        fw = s.pointMeshDistanceCompatible(v, P, N, **kw)
        mw = s.meshPointDistanceCompatible(v, P, N, vert_normals=vn, **kw)
        assert all(_same_bits(a, b) for a, b in zip(fw + mw, ref)), form  # a repeated run
        for sel in ([2], [2, 0], [3, 1, 2]):
            i = sel.index(2)
            f1 = s.pointMeshDistanceCompatible(v[sel], P[sel], N[sel], **kw)
            m1 = s.meshPointDistanceCompatible(v[sel], P[sel], N[sel], vert_normals=vn[sel], **kw)
            assert all(_same_bits(a[i], b[2]) for a, b in zip(f1 + m1, ref)), (form, sel)
        dv, dP, dN, dvn = (torch.from_numpy(x).cuda() for x in (v, P, N, vn))
        fd = s.pointMeshDistanceCompatible(dv, dP, dN, **kw)
        md = s.meshPointDistanceCompatible(dv, dP, dN, vert_normals=dvn, **kw)
        torch.cuda.synchronize()
        assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(fd + md, ref)), form
        # weights and closest NULL
        f2, s2 = np.empty((n, K), np.int64), np.empty((n, K), np.float32)
        cap = float(np.float32(0.05) * np.float32(0.05))
        assert _lib.load().smplpp_point_mesh_distance_compatible(s.handle, n, _ptr(v), K, _ptr(P), _ptr(N), 0.4, cap, _ptr(f2), None, None,
                                                                 _ptr(s2), 0, None) == 0
        assert _same_bits(f2, ref[0]) and _same_bits(s2, ref[3])


def test_non_finite_rows(forms, faces):
    n, K = 2, 70
    v = _verts(forms["query"], n, seed=81)
    rng = np.random.default_rng(81)
    P, N = _scan(v, faces, K, rng)
    bad_p, bad_n = [3, 17, 64], [5, 40, 69]
    P[0, 3] = np.nan
    P[0, 17, 1] = -np.inf
    P[0, 64, 0] = np.inf
    N[0, 5] = np.nan
    N[0, 40, 2] = np.inf
    N[0, 69, 0] = -np.inf
    P[1] = np.nan  # a frame of padding
    for form in FORMS:
        s = forms[form]
        for normals in (N, None):
            face, w, closest, sq, matched = s.pointMeshDistanceCompatible(v, P, normals, cos_min=0.0)
            bad = bad_p + (bad_n if normals is not None else [])
            assert (face[0, bad] == -1).all() and (face[1] == -1).all() and not matched[1].any()
            assert (np.delete(face[0], bad) >= 0).all()
            _unmatched_rows_are_zero(face, w, closest, sq)
    s = forms["query"]
    vn = np.ascontiguousarray(s.calcMeshVertexNormals())
    vn[0, 11] = np.nan
    vn[0, 6000, 1] = np.inf
    v2 = v.copy()
    v2[0, 13, 2] = np.nan
    index, sq, matched = s.meshPointDistanceCompatible(v2, P, N, vert_normals=vn, cos_min=0.0)
    assert (index[0, [11, 6000, 13]] == -1).all() and not np.isin(index[0], bad_p + bad_n).any()
    assert (index[1] == -1).all() and matched[0].mean() > 0.3
    _unmatched_rows_are_zero(index, sq)


def test_invalid_arguments(forms):
    from smplpp_amd import _lib
    from smplpp_amd._lib import SmplppError, check
    from smplpp_amd.smpl import _ptr

    s = forms["query"]
    L = _lib.load()
    V, K = s.vertex_num, 4
    v, vn = np.zeros((1, V, 3), np.float32), np.ones((1, V, 3), np.float32)
    P, N = np.zeros((1, K, 3), np.float32), np.ones((1, K, 3), np.float32)
    face, sq = np.full((1, K), 5, np.int64), np.full((1, K), 7.0, np.float32)
    w, c = np.full((1, K, 3), 7.0, np.float32), np.full((1, K, 3), 7.0, np.float32)
    index, vsq = np.full((1, V), 5, np.int64), np.full((1, V), 7.0, np.float32)
    h = s.handle
    nan = float("nan")

    def pm(*a):
        check(L.smplpp_point_mesh_distance_compatible(*a))

    def mp(*a):
        check(L.smplpp_mesh_point_distance_compatible(*a))

    out = (_ptr(face), _ptr(w), _ptr(c), _ptr(sq))
    bad_calls = [(pm, (h, 1, _ptr(v), K, _ptr(P), _ptr(N), cm, cap) + out + (0, None))
                 for cm, cap in ((-0.1, INF), (1.5, INF), (nan, INF), (0.5, -1.0), (0.5, nan), (0.5, -INF))]
    bad_calls += [(mp, (h, 1, _ptr(v), _ptr(vn), K, _ptr(P), _ptr(N), cm, cap, _ptr(index), _ptr(vsq), 0, None))
                  for cm, cap in ((-0.1, INF), (1.0000001, INF), (nan, 1.0), (0.5, -1e-30), (0.5, nan))]
    bad_calls += [
        (pm, (None, 1, _ptr(v), K, _ptr(P), _ptr(N), 0.5, INF) + out + (0, None)),
        (pm, (h, 0, _ptr(v), K, _ptr(P), _ptr(N), 0.5, INF) + out + (0, None)),
        (pm, (h, 1, _ptr(v), 0, _ptr(P), _ptr(N), 0.5, INF) + out + (0, None)),
        (pm, (h, 1, None, K, _ptr(P), _ptr(N), 0.5, INF) + out + (0, None)),
        (pm, (h, 1, _ptr(v), K, None, _ptr(N), 0.5, INF) + out + (0, None)),
        (pm, (h, 1, _ptr(v), K, _ptr(P), _ptr(N), 0.5, INF, None, _ptr(w), _ptr(c), _ptr(sq), 0, None)),
        (pm, (h, 1, _ptr(v), K, _ptr(P), _ptr(N), 0.5, INF, _ptr(face), _ptr(w), _ptr(c), None, 0, None)),
        (pm, (h, 1, _ptr(v), K, _ptr(P), _ptr(N), 0.5, INF) + out + (5, None)),
        (pm, (h, 1 << 16, _ptr(v), 1 << 16, _ptr(P), _ptr(N), 0.5, INF) + out + (0, None)),
        (mp, (None, 1, _ptr(v), _ptr(vn), K, _ptr(P), _ptr(N), 0.5, INF, _ptr(index), _ptr(vsq), 0, None)),
        (mp, (h, 0, _ptr(v), _ptr(vn), K, _ptr(P), _ptr(N), 0.5, INF, _ptr(index), _ptr(vsq), 0, None)),
        (mp, (h, 1, _ptr(v), _ptr(vn), 0, _ptr(P), _ptr(N), 0.5, INF, _ptr(index), _ptr(vsq), 0, None)),
        (mp, (h, 1, _ptr(v), _ptr(vn), K, _ptr(P), _ptr(N), 0.5, INF, None, _ptr(vsq), 0, None)),
        (mp, (h, 1, _ptr(v), _ptr(vn), K, _ptr(P), _ptr(N), 0.5, INF, _ptr(index), None, 0, None)),
        (mp, (h, 1, _ptr(v), _ptr(vn), K, _ptr(P), _ptr(N), 0.5, INF, _ptr(index), _ptr(vsq), 5, None)),
        (mp, (h, 1 << 19, _ptr(v), _ptr(vn), 1, _ptr(P), _ptr(N), 0.5, INF, _ptr(index), _ptr(vsq), 0, None)),
    ]
    for fn, args in bad_calls:
        with pytest.raises(SmplppError):
            fn(*args)
    for a in (w, c, sq, vsq):
        assert (a == 7.0).all()
    assert (face == 5).all() and (index == 5).all()
    # the bounds themselves are accepted
    for cm, cap in ((0.0, 0.0), (1.0, INF), (0.5, 0.0)):
        pm(h, 1, _ptr(v), K, _ptr(P), _ptr(N), cm, cap, *out, 0, None)
        mp(h, 1, _ptr(v), _ptr(vn), K, _ptr(P), _ptr(N), cm, cap, _ptr(index), _ptr(vsq), 0, None)


# ---------------------------------------------------------------------------------------------------- backward
def test_host_space_backward_of_unmatched_queries(forms, faces):
    """The wrappers' backward at the compatible search's faces: an unmatched query contributes nothing, in either space."""
    s = forms["query"]
    n, K = 2, 120
    v = _verts(s, n, seed=82)
    rng = np.random.default_rng(82)
    P, N = _scan(v, faces, K, rng)
    N = _mixed_normals(N, rng)
    face, _, _, _, matched = s.pointMeshDistanceCompatible(v, P, N)
    assert 0.5 < matched.mean() < 1
    g = rng.normal(size=(n, K)).astype(np.float32)
    gv, gp = s.pointMeshDistanceCompatibleBackward(v, P, face, g)
    assert (gp[~matched] == 0).all() and np.abs(gp[matched]).max() > 0
    rv, rp = s.pointMeshDistanceBackward(v, P, np.where(matched, face, 0), np.where(matched, g, np.float32(0)))
    assert _same_bits(gv, rv) and _same_bits(gp, rp)
    dv, dP, dg, df = (torch.from_numpy(x).cuda() for x in (v, P, g, face))
    dgv, dgp = s.pointMeshDistanceCompatibleBackward(dv, dP, df, dg)  # device space: -1 goes straight through
    torch.cuda.synchronize()
    assert _same_bits(dgv.cpu().numpy(), gv) and _same_bits(dgp.cpu().numpy(), gp)


def test_autograd_beta_theta_and_points(forms, synth_model, faces):
    """Gradients to beta and theta through FK, and to the points, at the forward's correspondences, against float64 autograd (the
    project's fp32 bar: 4x the error of an fp32 autograd of the same graph, or 1e-5), on a cloud with unmatched queries."""
    import fk_vjp_oracle as FK
    from smplpp_amd import model_io

    s = forms["tiled"]
    dev = torch.device("cuda")
    n, K = 2, 600
    beta, theta = model_io.synthetic_inputs(n, seed=83)
    rng = np.random.default_rng(83)
    vt = s.launch(beta, theta, want=("verts",))["verts"]
    P, N = _scan(vt, faces, K, rng)
    N = _mixed_normals(N, rng)
    b = torch.from_numpy(beta).to(dev).requires_grad_(True)
    t = torch.from_numpy(theta).to(dev).requires_grad_(True)
    Pd = torch.from_numpy(P).to(dev).requires_grad_(True)
    Nd = torch.from_numpy(N).to(dev).requires_grad_(True)
    verts, _ = s.forward_differentiable(b, t)
    face, w, matched, sq = s.point_mesh_distance_compatible_differentiable(verts, Pd, Nd, cos_min=0.5, max_dist=0.03)
    index, vmatched, vsq = s.mesh_point_distance_compatible_differentiable(verts, Pd, Nd, cos_min=0.5, max_dist=0.03)
    assert not face.requires_grad and not w.requires_grad and not matched.requires_grad and sq.requires_grad
    assert not index.requires_grad and not vmatched.requires_grad and vsq.requires_grad
    (sq.mean() + vsq.mean()).backward()
    assert Nd.grad is None  # the normals steer the selection only
    face, index = face.cpu().numpy(), index.cpu().numpy()
    m, vm = matched.cpu().numpy(), vmatched.cpu().numpy()
    assert 0.2 < m.mean() < 0.95 and 0.05 < vm.mean() < 0.98
    assert (sq.detach().cpu().numpy()[~m] == 0).all() and ((face >= 0) == m).all() and ((index >= 0) == vm).all()

    def ref(dtype):
        mt = FK.model_tensors(synth_model, dtype)
        bb = torch.tensor(beta, dtype=dtype, requires_grad=True)
        tt = torch.tensor(theta, dtype=dtype, requires_grad=True)
        pp = torch.tensor(P, dtype=dtype, requires_grad=True)
        vv = FK.fk(mt, bb, tt)["verts"]
        a = (PO.sqdist(vv, faces, pp, np.maximum(face, 0)) * torch.tensor(m, dtype=dtype)).sum() / (n * K)
        c = MO.sqdist(vv, pp, index).mean()
        (a + c).backward()
        return bb.grad.double().numpy(), tt.grad.double().numpy(), pp.grad.double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for got, want, f32, name in zip((b.grad, t.grad, Pd.grad), r64, r32, ("beta", "theta", "points")):
        got = got.cpu().numpy()
        bar = max(4 * _rel(f32, want), 1e-5)
        assert _rel(got, want) <= bar, (name, _rel(got, want), bar)
    pg = Pd.grad.cpu().numpy()
    used = np.zeros((n, K), bool)
    for f in range(n):
        used[f, index[f][index[f] >= 0]] = True
    assert (pg[~m & ~used] == 0).all()  # an unmatched point no vertex chose gets nothing


def test_scan_compat_cpp_shim(tmp_path):
    from smplpp_amd import model_io

    exe = str(tmp_path / "scan_compat_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "scan_compat_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    # the program's inputs, restated
    n, K = 2, 24
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    P = ((np.arange(n * K * 3, dtype=np.float32).reshape(n, K, 3) % 17) - 8) * np.float32(0.03)
    N = ((np.arange(n * K * 3, dtype=np.float32).reshape(n, K, 3) % 13) - 6) * np.float32(0.25)
    s = _smpl(model)
    V = s.vertex_num
    v = s.launch(beta, theta, want=("verts",))["verts"]
    cap = C.c_float(0.04).value
    face, w, closest, sq, matched = s.pointMeshDistanceCompatible(v, P, N, cos_min=0.25, max_sqdist=cap)
    g = ((np.arange(n * K, dtype=np.float32).reshape(n, K) % 5) - 2) * np.float32(0.25)
    gv, gp = s.pointMeshDistanceCompatibleBackward(v, P, face, g)
    index, vsq, vmatched = s.meshPointDistanceCompatible(v, P, N, cos_min=0.25, max_sqdist=cap)
    h = ((np.arange(n * V, dtype=np.float32).reshape(n, V) % 5) - 2) * np.float32(0.25)
    hv, hp = s.meshPointDistanceBackward(v, P, index, h)
    assert 0 < matched.sum() < matched.size or 0 < vmatched.sum() < vmatched.size  # some row of either call is unmatched
    want = b"".join(np.ascontiguousarray(x).tobytes() for x in (face, w, closest, sq, gv, gp, index, vsq, hv, hp))
    assert len(raw) == len(want) and raw == want
