"""Surface geodesics and the self-contact search on the MI355X (smplpp_mesh_geodesic, smplpp_self_contact_*): every output bit against
the float32 restatements of tests/geodesic_oracle.py.  Geodesics on tori of 1023, 1024 and 1025 vertices (both sides of the
workgroup's thread count), an icosphere, two disjoint spheres and one torus of 16510 vertices (the LDS opt-in): single sources, sets, a
repeat, an empty set, lattice coordinates, a cap, NaN and inf vertices, coincident vertices, n = 3 against a frame alone, host against
device space, guard elements, repeated calls, the refusals.  The far mask in full on the small meshes and on a sample of sources of the
synthetic body.  The search on folded, jittered and lattice frames with ties, caps, normals and values that are not finite, on both
sides of every tile constant of its kernel and on both of its paths, and on the folded synthetic body.  The backward pass against the
two existing calls it is defined by, and a chain from theta and beta against float64 autograd.  The C++ shim.

The folded synthetic body (test_search_on_the_folded_synthetic_body): the share of vertices with a partner within 10 cm, measured with
the fp32 restatement on the CPU, is 0.458 (0.259 on the unfolded template); the test asserts it lies in [0.2, 0.8]."""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import geodesic_oracle as GO  # noqa: E402
import vjp_blocks as VB  # noqa: E402
from test_vertex_offsets_gpu import _dev, _smpl  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
INF = float("inf")
FILL = 7.0
GEO_THREADS = 1024                                   # geodesic.hip: threads of the relaxation's workgroup
GEO_LDS_STATIC = 16380                               # the most vertices whose field (and 16 bytes of flags) fit without the LDS opt-in
SC_VBLOCK, SC_TILE, SC_GROUP = 1024, 1024, 32        # geodesic.hip: query vertices per workgroup, candidates per tile and per mask word
SC_TARGET_WG, SC_MIN_CHUNK = 2048, 256               # ... and the split of the candidates into chunks


def sc_chunks(n, V):
    """geodesic.hip::sc_chunk_len restated: the chunks a call splits the candidates into."""
    wg = n * ((V + SC_VBLOCK - 1) // SC_VBLOCK)
    if wg >= SC_TARGET_WG or V < 2 * SC_MIN_CHUNK:
        return 1
    s = min((SC_TARGET_WG + wg - 1) // wg, V // SC_MIN_CHUNK)
    chunk = ((V + s - 1) // s + SC_GROUP - 1) // SC_GROUP * SC_GROUP
    return (V + chunk - 1) // chunk


MESHES = {
    "torus1023": lambda: GO.torus(31, 33),
    "torus1024": lambda: GO.torus(32, 32),
    "torus1025": lambda: GO.torus(25, 41),
    "torus511": lambda: GO.torus(7, 73),
    "torus512": lambda: GO.torus(16, 32),
    "ico642": lambda: GO.icosphere(3),
    "two_spheres": lambda: GO.two_spheres(2),
    "torus32": lambda: GO.torus(4, 8),
    "torus33": lambda: GO.torus(3, 11),
    "ico42": lambda: GO.icosphere(1),
    "torus16380": lambda: GO.torus(126, 130),
    "torus16510": lambda: GO.torus(127, 130),
}
_cache = {}


def _mesh(name):
    """(verts, faces0, SMPL on tiny_model(V, faces)) built once."""
    from smplpp_amd import model_io

    if name not in _cache:
        verts, faces0 = MESHES[name]()
        _cache[name] = (verts, faces0, _smpl(model_io.tiny_model(len(verts), faces=GO.model_faces(faces0))))
    return _cache[name]


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


class _BareModel:
    """A model handle without faces (the Python binding does not make one): smplpp_model_create with F = 0."""

    def __init__(self, V=8):
        import ctypes as C

        from smplpp_amd import _lib, model_io

        m = model_io.tiny_model(V)
        self.handle = C.c_void_p()
        _lib.check(_lib.load().smplpp_model_create(V, 0, m["vertices_template"].ctypes.data, m["shape_blend_shapes"].ctypes.data,
                                                   m["pose_blend_shapes"].ctypes.data, m["joint_regressor"].ctypes.data, m["weights"].ctypes.data,
                                                   m["kinematic_tree"].ctypes.data, None, 0, C.byref(self.handle)))

    def close(self):
        from smplpp_amd import _lib

        _lib.load().smplpp_model_destroy(self.handle)


def _same(a, b):
    a, b = np.ascontiguousarray(_host(a)), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _frames(verts, seed):
    """Three distinct frames: the mesh, a jittered and scaled copy, and integer-lattice coordinates (exact ties, coincident
    vertices: zero-length edges)."""
    rng = np.random.default_rng(seed)
    return np.stack([verts, (1.3 * verts + rng.normal(0, 0.01, verts.shape)).astype(f32), np.round(verts * 5).astype(f32)])


def _source_sets(V):
    return [[0], [V // 2], [V - 1], [0, V // 3, V - 1], [1, 1], []]


def _fields(frames, faces0, sets, max_dist=None):
    V = frames.shape[1]
    off, adj = GO.edge_table(V, faces0)
    return np.stack([GO.relax(V, off, adj, GO.edge_weights(x, off, adj), sets, max_dist)[0] for x in frames])


# ---------------------------------------------------------------------------------------------------- 1. geodesics
@pytest.fixture(scope="module")
def geo_case():
    """name -> (frames [3,V,3] with a NaN and an inf vertex in the middle frame, the sets, the restatement [3,S,V]), once per mesh."""
    made = {}

    def get(name):
        if name not in made:
            verts, faces0, _ = _mesh(name)
            fr = _frames(verts, 11)
            fr[1, 5], fr[1, 9, 1] = np.nan, np.inf
            sets = _source_sets(len(verts))
            made[name] = (fr, sets, _fields(fr, faces0, sets))
        return made[name]

    return get


@pytest.mark.parametrize("name", ["torus1023", "torus1024", "torus1025", "ico642", "two_spheres"])
def test_geodesic_bits(name, geo_case):
    """n = 3 distinct frames and the middle frame alone, device and host space; a NaN and an inf vertex are routed around."""
    s = _mesh(name)[2]
    fr, sets, want = geo_case(name)
    V = fr.shape[1]
    assert np.isinf(want[:, 5]).all() and np.isfinite(want[0, :4]).any()
    assert np.isinf(want[1, 0, 5]) and np.isinf(want[1, 0, 9]) and np.isfinite(want[1, 0, 6])  # the dead vertices, and a live one
    if name != "two_spheres":  # the lattice frame: ties, and coincident vertices at 0
        lat = want[2, 0][np.isfinite(want[2, 0])]
        assert len(np.unique(lat)) < len(lat) // 2 and (lat[1:] == 0).any()
    if name == "two_spheres":
        assert np.isinf(want[0, 0, V - 1]) and np.isfinite(want[0, 2, V - 1])
    assert _same(s.meshGeodesic(_dev(fr), sets), want)
    assert _same(s.meshGeodesic(_dev(fr[1:2]), sets), want[1:2])
    assert _same(s.meshGeodesic(fr, sets), want)
    singles = np.array([0, V // 2, V - 1])
    assert _same(s.meshGeodesic(_dev(fr[1:2]), singles), want[1:2, :3])  # fewer fields, the same bits


def test_geodesic_cap(geo_case):
    s = _mesh("torus1025")[2]
    fr, sets, want = geo_case("torus1025")
    cap = f32(np.median(want[0, 0]))
    capped = np.where(want > cap, f32(np.inf), want).astype(f32)
    share = np.isfinite(capped[:, :5]).mean()
    assert 0.1 <= share <= 0.9, share
    assert _same(s.meshGeodesic(_dev(fr), sets, max_dist=cap), capped)
    zero = s.meshGeodesic(_dev(fr[:1]), sets, max_dist=0.0)  # only the sources (and what coincides with them) stay
    assert _same(zero, np.where(want[:1] > 0, f32(np.inf), want[:1]).astype(f32))


@pytest.mark.parametrize("name", ["torus16380", "torus16510"])
def test_geodesic_lds_opt_in(name):
    """16380 vertices: exactly the 64 KiB a kernel gets without asking.  16510: 66056 bytes, by opt-in.  Two sources."""
    verts, faces0, s = _mesh(name)
    V = len(verts)
    assert (V > GEO_LDS_STATIC) == (name == "torus16510")
    sets = [[0], [V // 2]]
    want = _fields(verts[None], faces0, sets)
    assert np.isfinite(want).all()
    assert _same(s.meshGeodesic(_dev(verts[None]), sets), want)


def test_geodesic_guards_repeat_and_space(geo_case):
    from smplpp_amd import _lib

    s = _mesh("torus1023")[2]
    fr, sets, want = geo_case("torus1023")
    n, S, V = want.shape
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in sets])]).astype(np.int64)
    ids = np.array([v for x in sets for v in x], np.int64)
    G = 64
    out = torch.full((n * S * V + 2 * G,), FILL, device="cuda")
    dv, dp, di = _dev(fr), _dev(ptr), _dev(ids)
    for turn in range(2):
        rc = _lib.load().smplpp_mesh_geodesic(s.handle, n, dv.data_ptr(), S, dp.data_ptr(), di.data_ptr(), INF, out.data_ptr() + 4 * G, _lib.DEVICE,
                                              None)
        assert rc == 0
        torch.cuda.synchronize()
        assert _same(out[G:-G].reshape(n, S, V), want), turn
        assert (out[:G] == FILL).all() and (out[-G:] == FILL).all(), turn
    # a device-space source outside [0, V) is ignored
    di2 = _dev(np.concatenate([ids, [V + 5, -3]]).astype(np.int64))
    dp2 = _dev(np.concatenate([ptr[:-1], [ptr[-1] + 2]]).astype(np.int64))
    o2 = torch.empty((n, S, V), device="cuda")
    assert _lib.load().smplpp_mesh_geodesic(s.handle, n, dv.data_ptr(), S, dp2.data_ptr(), di2.data_ptr(), INF, o2.data_ptr(), _lib.DEVICE, None) == 0
    assert _same(o2, want)


def test_geodesic_refusals():
    from smplpp_amd import _lib

    Lb, D, H = _lib.load(), _lib.DEVICE, _lib.HOST
    verts, faces0, s = _mesh("ico42")
    V = len(verts)
    v = _dev(verts[None])
    ptr, ids = _dev(np.array([0, 1, 2], np.int64)), _dev(np.array([0, 3], np.int64))
    out = torch.full((2, 2, V), FILL, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def geo(h=s.handle, n=1, v_=v, S=2, p=ptr, i=ids, cap=INF, o=out, space=D):
        return Lb.smplpp_mesh_geodesic(h, n, P(v_), S, P(p), P(i), cap, P(o), space, None)

    assert geo() == 0
    out.fill_(FILL)
    bad_start, decreasing = _dev(np.array([1, 1, 2], np.int64)), _dev(np.array([0, 2, 1], np.int64))
    refused = [geo(**kw) for kw in (dict(h=None), dict(n=0), dict(n=-1), dict(S=0), dict(v_=None), dict(p=None), dict(i=None), dict(o=None),
                                    dict(p=bad_start), dict(p=decreasing), dict(cap=-1.0), dict(cap=float("nan")), dict(space=2),
                                    dict(n=2 ** 20, S=2 ** 10))]
    # host space: a source outside [0, V)
    hv, hp, ho = verts[None].copy(), np.array([0, 1, 2], np.int64), np.full((1, 2, V), FILL, f32)
    for bad in (V, -1):
        hi = np.array([0, bad], np.int64)
        refused.append(Lb.smplpp_mesh_geodesic(s.handle, 1, hv.ctypes.data, 2, hp.ctypes.data, hi.ctypes.data, INF, ho.ctypes.data, H, None))
    # a model without faces
    bare = _BareModel(8)
    refused.append(geo(h=bare.handle, v_=_dev(np.zeros((1, 8, 3), f32))))
    torch.cuda.synchronize()
    bare.close()
    assert all(rc == 1 for rc in refused), refused
    assert (out == FILL).all() and (ho == FILL).all()


def test_geodesic_refuses_more_than_32768_vertices():
    from smplpp_amd import _lib, contact, model_io

    V = 32769
    faces = np.stack([np.arange(V - 2), np.arange(1, V - 1), np.arange(2, V)], 1) + 1
    s = _smpl(model_io.tiny_model(V, faces=faces))
    with pytest.raises(_lib.SmplppError):
        s.meshGeodesic(torch.zeros((1, V, 3), device="cuda"), [[0]])
    with pytest.raises(_lib.SmplppError):
        contact.SelfContact(s, geo_min=0.1)


# ---------------------------------------------------------------------------------------------------- 2. the far mask
GEO_MIN = (0.0, 1.0, 100.0)  # none, a middle value, above every mesh's diameter


@pytest.fixture(scope="module")
def all_fields():
    made = {}

    def get(name):
        if name not in made:
            verts, faces0, _ = _mesh(name)
            made[name] = GO.single_source_fields(verts, faces0)
        return made[name]

    return get


@pytest.mark.parametrize("name", ["torus1023", "torus1024", "torus1025", "ico642", "torus32", "torus33", "ico42"])
def test_mask_bits(name, all_fields):
    """The full matrix and far_pairs at geo_min 0, a middle value, and above the diameter (no far pair: every search row is -1)."""
    from smplpp_amd import contact

    verts, faces0, s = _mesh(name)
    V = len(verts)
    D = all_fields(name)
    for geo_min in GEO_MIN:
        far, _ = GO.far_matrix(verts, faces0, geo_min, fields=D)
        sc = contact.SelfContact(s, rest=verts, geo_min=geo_min)
        assert sc.words_per_row == (V + 31) // 32 and sc.geo_min == f32(geo_min)
        assert _same(sc.mask(), GO.pack_bits(far)), (name, geo_min)
        assert _same(sc.mask("cuda").cpu().numpy().view(np.uint32), GO.pack_bits(far))
        assert sc.far_pairs == far.sum() // 2, (name, geo_min)
        if geo_min == 0.0:
            assert sc.far_pairs == V * (V - 1) // 2
        elif geo_min == 1.0:
            assert 0.1 < sc.far_pairs / (V * (V - 1) // 2) < 0.9
        else:
            assert sc.far_pairs == 0
            index, sq, matched = sc.search(_dev(verts[None]))
            assert (_host(index) == -1).all() and not _host(matched).any() and _same(sq, np.zeros((1, V), f32))


def test_mask_on_the_synthetic_body(synth_model):
    """Every bit (v, u) whose min(v, u) lies in a fixed sample of 48 sources, at geo_min = 0.3 on the template."""
    from smplpp_amd import contact

    s = _smpl(synth_model)
    rest = np.ascontiguousarray(synth_model["vertices_template"], f32)
    faces0 = synth_model["face_indices"].astype(np.int64) - 1
    V = len(rest)
    src = np.unique(np.linspace(0, V - 1, 48).astype(np.int64))
    assert len(src) == 48
    far, known = GO.far_matrix(rest, faces0, 0.3, sources=src)
    sc = contact.SelfContact(s)  # rest = the template, geo_min = 0.3
    got = GO.unpack_bits(sc.mask(), V)
    assert known.sum() == 2 * (V - 1 - src).sum() and (got[known] == far[known]).all()
    assert 0.2 < far[known].mean() < 0.98
    assert not got.diagonal().any() and (got == got.T).all()
    assert sc.far_pairs == got.sum() // 2
    W = sc.words_per_row
    assert (sc.mask()[:, W - 1] >> np.uint32(V - 32 * (W - 1)) == 0).all()  # bits past V are 0


def test_handle_refusals_and_lifetime(synth_model):
    from smplpp_amd import _lib, contact, model_io

    verts, faces0, s = _mesh("ico42")
    for kw in (dict(geo_min=-0.1), dict(geo_min=INF), dict(geo_min=float("nan"))):
        with pytest.raises(_lib.SmplppError):
            contact.SelfContact(s, rest=verts, **kw)
    bad = verts.copy()
    bad[3, 1] = np.nan
    with pytest.raises(_lib.SmplppError):
        contact.SelfContact(s, rest=bad, geo_min=0.2)
    import ctypes as C

    bare, h = _BareModel(8), C.c_void_p(5)
    assert _lib.load().smplpp_self_contact_create(bare.handle, np.zeros((8, 3), f32).ctypes.data, 0.2, C.byref(h)) == 1 and not h.value
    assert _lib.load().smplpp_self_contact_create(s.handle, None, 0.2, C.byref(h)) == 1 and not h.value
    bare.close()
    # the handle outlives its model
    s2 = _smpl(model_io.tiny_model(len(verts), faces=GO.model_faces(faces0)))
    sc = contact.SelfContact(s2, rest=verts, geo_min=0.5)
    want = contact.SelfContact(s, rest=verts, geo_min=0.5)
    del s2
    gc.collect()
    fr = _dev(_frames(verts, 3))
    a, b = sc.search(fr), want.search(fr)
    assert _same(a[0], _host(b[0])) and _same(a[1], _host(b[1]))


# ---------------------------------------------------------------------------------------------------- 3. the search
def _normals(frame, faces0):
    """Area-weighted vertex normals in numpy (any normals would do: they are inputs to both sides)."""
    a, b, c = frame[faces0[:, 0]], frame[faces0[:, 1]], frame[faces0[:, 2]]
    fn = np.cross(b - a, c - a)
    out = np.zeros_like(frame)
    for k in range(3):
        np.add.at(out, faces0[:, k], fn)
    return out.astype(f32)


def _search_frames(verts, seed):
    """Folded (flattened along z: the two sides of the mesh nearly touch), folded and jittered, and a coarse lattice (ties)."""
    rng = np.random.default_rng(seed)
    flat = verts * np.array([1.0, 1.0, 0.03], f32)
    return np.stack([flat, (flat + rng.normal(0, 0.004, verts.shape)).astype(f32), np.round(verts * 4).astype(f32)]).astype(f32)


def _search_want(frames, mask, normals, cos_min, cap):
    res = [GO.search(frames[i], mask, None if normals is None else normals[i], cos_min, cap) for i in range(len(frames))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


@pytest.fixture(scope="module")
def search_case():
    """name -> (handle, its mask, frames [3,V,3] with a NaN vertex, normals [3,V,3] with a NaN and a zero row), once per mesh."""
    from smplpp_amd import contact

    made = {}

    def get(name):
        if name not in made:
            verts, faces0, s = _mesh(name)
            sc = contact.SelfContact(s, rest=verts, geo_min=1.0)
            fr = _search_frames(verts, 21)
            fr[1, 7, 2] = np.nan
            nrm = np.stack([_normals(np.nan_to_num(x), faces0) for x in fr])
            nrm[0, 11], nrm[1, 13, 0], nrm[2, 17] = 0.0, np.nan, np.inf
            made[name] = (sc, sc.mask(), fr, nrm)
        return made[name]

    return get


SEARCH_MESHES = ["torus1023", "torus1024", "torus1025", "ico642", "torus511", "torus512", "torus32", "torus33", "ico42"]


@pytest.mark.parametrize("name", SEARCH_MESHES)
def test_search_bits(name, search_case):
    """Without and with normals, without a cap, under a cap equal to an attained distance and under a tight one; n = 3 and the
    middle frame alone; device and host space.  The mask of the restatement is the handle's own, which test_mask_bits pins."""
    sc, mask, fr, nrm = search_case(name)
    V = fr.shape[1]
    assert (sc_chunks(3, V) > 1) == (V >= 2 * SC_MIN_CHUNK) and (sc_chunks(1, V) > 1) == (V >= 2 * SC_MIN_CHUNK)  # the split: from 512 on
    free_i, free_d = _search_want(fr, mask, None, 0.0, INF)
    assert (free_i[0] >= 0).all() and (free_i[1, 7] == -1) and free_d[1, 7] == 0  # the NaN vertex has no partner ...
    assert not (free_i[1] == 7).any()                                              # ... and is nobody's
    attained = float(np.sort(free_d[0])[V // 2])
    dfr, dn = _dev(fr), _dev(nrm)
    for normals, cos_min, cap in ((None, 0.0, None), (None, 0.0, attained), (nrm, 0.3, None), (nrm, 0.0, attained), (nrm, 1.0, None),
                                  (None, 0.0, float(free_d[0].min()) * 0.5)):
        wi, wd = _search_want(fr, mask, normals, cos_min, INF if cap is None else cap)
        dnn = None if normals is None else dn
        i3, d3, m3 = sc.search(dfr, dnn, cos_min, max_sqdist=cap)
        assert _same(i3, wi) and _same(d3, wd) and _same(m3, wi >= 0), (name, normals is not None, cos_min, cap)
        i1, d1, _ = sc.search(dfr[1:2].contiguous(), None if dnn is None else dnn[1:2].contiguous(), cos_min, max_sqdist=cap)
        assert _same(i1, wi[1:2]) and _same(d1, wd[1:2])
        ih, dh, _ = sc.search(fr, normals, cos_min, max_sqdist=cap)
        assert _same(ih, wi) and _same(dh, wd)
        if normals is not None:
            assert wi[0, 11] == -1 and wi[1, 13] == -1 and wi[2, 17] == -1  # a zero, a NaN, an inf normal match nothing


def test_search_cap_at_an_attained_distance(search_case):
    """The squared cap passed as it is: d <= max_sqdist keeps the vertices at exactly that distance; the next float below drops them."""
    from smplpp_amd import _lib

    sc, mask, fr, _ = search_case("torus1025")
    V = fr.shape[1]
    free_i, free_d = _search_want(fr[:1], mask, None, 0.0, INF)
    cap = np.sort(free_d[0])[V // 2]
    below = np.nextafter(cap, f32(0))
    v = _dev(fr[:1])
    for c in (cap, below):
        wi, wd = _search_want(fr[:1], mask, None, 0.0, float(c))
        oi, od = torch.empty((1, V), dtype=torch.int64, device="cuda"), torch.empty((1, V), device="cuda")
        assert _lib.load().smplpp_self_contact(sc.handle, 1, v.data_ptr(), None, 0.0, float(c), oi.data_ptr(), od.data_ptr(), _lib.DEVICE, None) == 0
        assert _same(oi, wi) and _same(od, wd)
    assert (wd == cap).sum() == 0 and (free_d[0] == cap).sum() > 0


@pytest.mark.parametrize("name,n", [("ico642", 2048), ("torus1025", 1024)])
def test_search_unsplit_path(name, n, search_case):
    """Enough frames that the candidates are not split: one chunk of V >= 512 candidates, and at 1025 a second LDS tile.  The frames
    repeat three distinct ones, so the restatement runs three times."""
    sc, mask, fr, nrm = search_case(name)
    V = fr.shape[1]
    assert sc_chunks(n, V) == 1 and sc_chunks(3, V) > 1 and (name != "torus1025" or V > SC_TILE)
    wi, wd = _search_want(fr, mask, nrm, 0.2, INF)
    rep = np.arange(n) % 3
    i, d, _ = sc.search(_dev(fr[rep]), _dev(nrm[rep]), 0.2, None)
    assert _same(i, wi[rep]) and _same(d, wd[rep])


def test_search_guards_repeat_and_refusals(search_case):
    from smplpp_amd import _lib

    Lb, D = _lib.load(), _lib.DEVICE
    sc, mask, fr, nrm = search_case("torus1023")
    n, V = fr.shape[:2]
    wi, wd = _search_want(fr, mask, nrm, 0.1, INF)
    G = 64
    oi = torch.full((n * V + 2 * G,), 9, dtype=torch.int64, device="cuda")
    od = torch.full((n * V + 2 * G,), FILL, device="cuda")
    v, nn = _dev(fr), _dev(nrm)
    for turn in range(2):
        assert Lb.smplpp_self_contact(sc.handle, n, v.data_ptr(), nn.data_ptr(), 0.1, INF, oi.data_ptr() + 8 * G, od.data_ptr() + 4 * G, D, None) == 0
        torch.cuda.synchronize()
        assert _same(oi[G:-G].reshape(n, V), wi) and _same(od[G:-G].reshape(n, V), wd), turn
        assert (oi[:G] == 9).all() and (oi[-G:] == 9).all() and (od[:G] == FILL).all() and (od[-G:] == FILL).all(), turn
    oi.fill_(9), od.fill_(FILL)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def fwd(h=sc.handle, n_=n, v_=v, cm=0.1, cap=INF, i=oi, d=od, space=D):
        return Lb.smplpp_self_contact(h, n_, P(v_), P(nn), cm, cap, P(i), P(d), space, None)

    g, gv = torch.ones((n, V), device="cuda"), torch.full((n, V, 3), FILL, device="cuda")
    ix = _dev(wi)

    def bwd(h=sc.handle, n_=n, v_=v, i=ix, g_=g, o=gv, acc=0, space=D):
        return Lb.smplpp_self_contact_vjp(h, n_, P(v_), P(i), P(g_), P(o), acc, space, None)

    refused = [fwd(**kw) for kw in (dict(h=None), dict(n_=0), dict(v_=None), dict(i=None), dict(d=None), dict(cm=-0.1), dict(cm=1.5),
                                    dict(cm=float("nan")), dict(cap=-1.0), dict(cap=float("nan")), dict(space=3), dict(n_=2 ** 21))]
    refused += [bwd(**kw) for kw in (dict(h=None), dict(n_=0), dict(v_=None), dict(i=None), dict(g_=None), dict(o=None), dict(acc=2),
                                     dict(space=3), dict(n_=2 ** 21))]
    hi = wi.copy()
    hi[0, 0] = V  # a host-space partner outside [-1, V)
    hg, ho = np.ones((n, V), f32), np.full((n, V, 3), FILL, f32)
    refused.append(Lb.smplpp_self_contact_vjp(sc.handle, n, fr.ctypes.data, hi.ctypes.data, hg.ctypes.data, ho.ctypes.data, 0, _lib.HOST, None))
    torch.cuda.synchronize()
    assert all(rc == 1 for rc in refused), refused
    assert (oi == 9).all() and (od == FILL).all() and (gv == FILL).all() and (ho == FILL).all()


def _fold(rest):
    """The template's upper half (y > -0.36) rotated by 175 degrees about the x axis through (0, -0.36, 0.11): bent double at the hips."""
    v = rest.astype(np.float64).copy()
    up = v[:, 1] > -0.36
    a = np.deg2rad(175.0)
    c, s = np.cos(a), np.sin(a)
    p = v[up] - np.array([0, -0.36, 0.11])
    y, z = p[:, 1].copy(), p[:, 2].copy()
    p[:, 1], p[:, 2] = c * y - s * z, s * y + c * z
    v[up] = p + np.array([0, -0.36, 0.11])
    return v.astype(f32)


def test_search_on_the_folded_synthetic_body(synth_model):
    from smplpp_amd import contact

    s = _smpl(synth_model)
    rest = np.ascontiguousarray(synth_model["vertices_template"], f32)
    sc = contact.SelfContact(s, geo_min=0.3)
    fr = np.stack([_fold(rest), rest])
    cap = float(f32(0.1) * f32(0.1))
    wi, wd = _search_want(fr, sc.mask(), None, 0.0, cap)
    share = (wi[0] >= 0).mean()
    print("folded: %.3f of the vertices have a partner within 10 cm (%.3f unfolded)" % (share, (wi[1] >= 0).mean()))
    assert 0.2 <= share <= 0.8
    i, d, m = sc.search(_dev(fr), max_dist=0.1)
    assert _same(i, wi) and _same(d, wd) and _same(m, wi >= 0)
    nrm = _normals(fr[0], synth_model["face_indices"].astype(np.int64) - 1)[None]
    wn, wdn = _search_want(fr[:1], sc.mask(), nrm, 0.5, cap)
    i, d, _ = sc.search(_dev(fr[:1]), _dev(nrm), 0.5, 0.1)
    assert 0 < (wn >= 0).sum() < (wi[0] >= 0).sum() and _same(i, wn) and _same(d, wdn)  # opposing normals: fewer partners


# ---------------------------------------------------------------------------------------------------- 4. the backward pass
@pytest.mark.parametrize("name", ["torus1025", "ico42"])
def test_vjp_equals_the_two_existing_calls(name, search_case):
    """accumulate 0 and 1, rows of -1, zero cotangents, device and host space."""
    from smplpp_amd import _lib

    Lb, D = _lib.load(), _lib.DEVICE
    verts, faces0, s = _mesh(name)
    sc, mask, fr, nrm = search_case(name)
    n, V = fr.shape[:2]
    index, _, _ = sc.search(_dev(fr), _dev(nrm), 0.3, None)
    ih = _host(index)
    assert (ih == -1).any() and (ih >= 0).any()
    rng = np.random.default_rng(31)
    g = rng.standard_normal((n, V)).astype(f32)
    g[:, ::7] = 0.0
    v, dg = _dev(fr), _dev(g)
    for acc in (0, 1):
        start = rng.standard_normal((n, V, 3)).astype(f32)
        want, got = _dev(start), _dev(start)
        assert Lb.smplpp_mesh_point_distance_vjp(s.handle, n, v.data_ptr(), V, v.data_ptr(), index.data_ptr(), dg.data_ptr(), want.data_ptr(), None,
                                                 acc, D, None) == 0
        assert Lb.smplpp_mesh_point_distance_vjp(s.handle, n, v.data_ptr(), V, v.data_ptr(), index.data_ptr(), dg.data_ptr(), None, want.data_ptr(),
                                                 1, D, None) == 0
        assert Lb.smplpp_self_contact_vjp(sc.handle, n, v.data_ptr(), index.data_ptr(), dg.data_ptr(), got.data_ptr(), acc, D, None) == 0
        torch.cuda.synchronize()
        wh = _host(want)
        live = np.isfinite(fr).all(2)  # (the NaN vertex: its own row and its partner's hold NaN in both)
        assert np.abs(wh[live & (ih >= 0) & (g != 0)]).max() > 0
        assert np.ascontiguousarray(_host(got)).tobytes() == np.ascontiguousarray(wh).tobytes(), (name, acc)
        # the binding, in both spaces
        if acc == 0:
            assert np.ascontiguousarray(_host(sc.searchBackward(v, index, dg))).tobytes() == wh.tobytes()
            assert np.ascontiguousarray(sc.searchBackward(fr, ih, g)).tobytes() == wh.tobytes()
        else:
            o = start.copy()
            assert sc.searchBackward(fr, ih, g, out=o) is o and o.tobytes() == wh.tobytes()


def test_chain_from_theta_and_beta(synth_model):
    """theta, beta -> FK -> search -> sum w sqdist at n = 2: the gradient per block within max(4 x the error of an fp32 autograd of
    the same graph, 1e-5 relative) of float64 autograd at the same partners.  The distances between vertices of one body do not change
    under a rigid motion, so the true gradient to the root translation (theta row 0) and the root rotation (row 1) is zero and a
    relative error is not defined there (float64 autograd leaves 3.5e-9 of the largest entry, fp32 1.4e-6): those two blocks are held to the same bar in
    absolute terms, against the largest entry of the float64 gradient to theta, and the 23 other joints are judged per block."""
    from smplpp_amd import contact, model_io

    s = _smpl(synth_model)
    sc = contact.SelfContact(s, geo_min=0.3)
    n, V = 2, s.vertex_num
    beta, theta = model_io.synthetic_inputs(n, seed=91)
    w = np.random.default_rng(92).uniform(0.5, 1.5, (n, V)).astype(f32)
    dev = torch.device("cuda")
    b, t = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (beta, theta))
    verts, _ = s.forward_differentiable(b, t)
    index, matched, sq = sc.search_differentiable(verts, max_dist=0.25)
    assert sq.requires_grad and not index.requires_grad and not matched.requires_grad
    (sq * torch.from_numpy(w).to(dev)).sum().backward()
    ih = _host(index)
    assert 0.05 < (ih >= 0).mean() < 1.0

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        args = [torch.tensor(a, dtype=dtype, requires_grad=True) for a in (beta, theta)]
        vv = FK.fk(m, args[0], args[1])["verts"]
        partner = vv[torch.arange(n)[:, None], torch.as_tensor(np.maximum(ih, 0))]
        d = ((vv - partner) ** 2).sum(-1)
        (torch.where(torch.as_tensor(ih >= 0), d, torch.zeros_like(d)) * torch.tensor(w, dtype=dtype)).sum().backward()
        return [a.grad.double().numpy() for a in args]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    tg = _host(t.grad)
    for got, want, low, name, axes in ((b.grad, r64[0], r32[0], "beta", (1,)), (tg[:, 2:], r64[1][:, 2:], r32[1][:, 2:], "theta", VB.THETA)):
        e, e32 = VB.block_error(_host(got), want, axes), VB.block_error(low, want, axes)
        print("chain %s: %.3g per block (fp32 autograd %.3g)" % (name, e, e32))
        assert e <= max(4 * e32, 1e-5), (name, e, e32)
    scale = np.abs(r64[1]).max()
    e, e32 = np.abs(tg[:, :2] - r64[1][:, :2]).max() / scale, np.abs(r32[1][:, :2] - r64[1][:, :2]).max() / scale
    print("chain rigid motion: %.3g of the largest entry (fp32 autograd %.3g; float64 itself %.3g)" % (e, e32, np.abs(r64[1][:, :2]).max() / scale))
    # (the float64 graph's own gradient there is what its Rodrigues formula leaves of the invariance: 3.5e-9 of the largest entry, measured)
    assert np.abs(r64[1][:, :2]).max() <= 1e-7 * scale and e <= max(4 * e32, 1e-5), (e, e32)


# ---------------------------------------------------------------------------------------------------- 5. C++ shim
def test_self_contact_cpp_shim(tmp_path):
    from smplpp_amd import contact, model_io

    exe = str(tmp_path / "self_contact_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "self_contact_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    v, faces0 = GO.icosphere(2)
    model = model_io.tiny_model(len(v), seed=9, faces=GO.model_faces(faces0))
    model["vertices_template"] = (0.5 * v).astype(model["vertices_template"].dtype)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    # the shim's inputs, restated
    n, V = 2, len(v)
    beta = (np.arange(n * 10, dtype=f32).reshape(n, 10) % 7 - 3) * f32(0.1)
    theta = ((np.arange(n * 75, dtype=f32).reshape(n, 25, 3) % 11) - 5) * f32(0.05)
    s = _smpl(model)
    out = s.launch(beta, theta)
    verts, rest = out["verts"], out["rest"]
    geo = s.meshGeodesic(verts, [[0], [V // 2, V - 1], []], max_dist=1.5)
    assert np.isfinite(geo[:, :2]).any() and np.isinf(geo[:, 2]).all()
    sc = contact.SelfContact(s, rest=rest[0], geo_min=0.6)
    assert 0 < sc.far_pairs < V * (V - 1) // 2
    ai, ad, _ = sc.search(verts)
    bi, bd, bm = sc.search(verts, rest, 0.1, max_sqdist=1.0)
    assert (ai >= 0).all() and bm.sum() > 0
    g = ((np.arange(n * V, dtype=f32).reshape(n, V) % 5) - 2) * f32(0.5)
    ones = np.ones((n, V, 3), f32)
    parts = [geo, np.array([sc.far_pairs, sc.words_per_row], np.int64), sc.mask().astype(np.int64), ai, ad, bi, bd, sc.searchBackward(verts, ai, g),
             sc.searchBackward(verts, ai, g, out=ones)]
    want = b"".join(np.ascontiguousarray(a).tobytes() for a in parts)
    assert len(raw) == len(want) and raw == want
