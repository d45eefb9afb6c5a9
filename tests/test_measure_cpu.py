"""Body measurements without a GPU: the rule of tests/measure_oracle.py on hand cases (the octahedron cut through its equator under
every relabelling, a plane through one vertex, one containing a face, one that misses, the negated plane), on closed_mesh spheres
(the volume does not depend on center; area and volume approach the sphere's), on dead data; its closed-form backward pass against
float64 autograd of the torch definition; the host table builder (smplpp_amd/csrc/measure_tables.h) as a stand-alone program built
with the address and undefined-behaviour sanitizers; the ABI."""
import ctypes as C
import functools
import heapq
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_oracle as MO  # noqa: E402
import test_ray_cast_cpu as RCPU  # noqa: E402  (closed_mesh, the octahedron, _header_args)
import vjp_blocks as VB  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
OCT_V, OCT_F = RCPU.OCT_V, RCPU.OCT_F
Z0 = np.array([[[0, 0, 1, 0]]], f64)  # the plane z = 0, one frame, one section


@functools.lru_cache(maxsize=None)
def sphere(F):
    """test_ray_cast_cpu.closed_mesh(F), face for face, with a heap in place of its scan of every face per split (18 s at F = 2048):
    the largest face goes next, the earliest in list order among equals."""
    v = [p for p in OCT_V.astype(f64)]
    area = lambda t: np.linalg.norm(np.cross(v[t[1]] - v[t[0]], v[t[2]] - v[t[0]]))  # noqa: E731
    heap = [(-area(t), i, tuple(int(x) for x in t)) for i, t in enumerate(OCT_F)]
    heapq.heapify(heap)
    seq = itertools.count(len(heap))  # the order of insertion: the list order of closed_mesh
    while len(heap) < F:
        _, _, (a, b, c) = heapq.heappop(heap)
        m = v[a] + v[b] + v[c]
        v.append(m / np.linalg.norm(m))
        k = len(v) - 1
        for t in ((a, b, k), (b, c, k), (c, a, k)):
            heapq.heappush(heap, (-area(t), next(seq), t))
    assert len(heap) == F
    return np.array(v).astype(f32), np.array([t for _, _, t in sorted(heap, key=lambda h: h[1])], np.int64)


@functools.lru_cache(maxsize=None)
def subdivided(levels):
    """The octahedron with every face split in four at its edge midpoints `levels` times, the vertices on the unit sphere: 8 * 4^levels
    faces, outward, and, unlike closed_mesh, with edges that shrink, so its area and volume converge to the sphere's."""
    v, f = [tuple(p) for p in OCT_V.astype(f64)], [tuple(int(x) for x in t) for t in OCT_F]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = np.add(v[a], v[b])
                v.append(tuple(p / np.linalg.norm(p)))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, f64), np.array(f, np.int64)


def whole(v, f, planes, dtype, **kw):
    """One region of all faces, every plane of planes [1,S,4] on it."""
    S = 0 if planes is None else np.shape(planes)[1]
    return MO.measure(np.asarray(v)[None], f, [np.arange(len(f))], [0] * S, planes, dtype=dtype, **kw)


def relabelled_octahedra():
    """The octahedron under the relabellings of the vertices and rolls of the stored corners that test_ray_cast_cpu uses."""
    rng = np.random.default_rng(3)
    for trial in range(12):
        perm = rng.permutation(6) if trial else np.arange(6)
        v = np.empty_like(OCT_V)
        v[perm] = OCT_V
        yield trial, v, np.stack([np.roll(perm[t], rng.integers(0, 3)) for t in OCT_F])


# ------------------------------------------------------------------------------------------------ hand cases
def test_octahedron_through_its_equator_is_counted_once():
    for trial, v, f in relabelled_octahedra():
        for dtype in (f32, f64):
            r = whole(v, f, Z0, dtype)
            assert r["section"].dtype == dtype and r["section"][0, 0] == dtype(4) * np.sqrt(dtype(2)), (trial, dtype, r["section"])
            assert r["crossings"][0, 0] == 4
            assert r["volume"][0, 0] == dtype(8) / dtype(6) and abs(r["area"][0, 0] - 4 * np.sqrt(3)) < 1e-6


def test_plane_through_one_vertex_only():
    for trial, v, f in relabelled_octahedra():
        top = whole(v, f, np.array([[[0, 0, 1, 1]]], f64), f32)  # the apex is on it and counts as above: its four faces, length 0
        assert top["crossings"][0, 0] == 4 and top["section"][0, 0] == 0
        bottom = whole(v, f, np.array([[[0, 0, 1, -1]]], f64), f32)  # everything is above
        assert bottom["crossings"][0, 0] == 0 and bottom["section"][0, 0] == 0
        # a supporting plane along the edge from +x to the apex: {s >= 0} is that edge alone, and BOTH its faces lie below it, so its
        # contour runs along the edge twice; the two other faces of each end are crossed with length 0
        slant = whole(v, f, np.array([[[1, 0, 1, 1]]], f64), f32)
        assert slant["crossings"][0, 0] == 6 and slant["section"][0, 0] == f32(2) * np.sqrt(f32(2))


def test_plane_containing_a_whole_face():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, -1]], f32)  # the base lies in z = 0, the apex below it
    f = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int64)  # outward
    for roll in range(3):
        r = whole(v, np.roll(f, roll, 1), Z0, f32)
        assert r["crossings"][0, 0] == 3  # the base itself is not crossed: its border comes from the three faces below
        assert r["section"][0, 0] == (f32(1) + f32(1)) + np.sqrt(f32(2))
    up = v * f32([1, 1, -1])  # the apex above: nothing is below the plane
    r = whole(up, f[:, ::-1], Z0, f32)
    assert r["crossings"][0, 0] == 0 and r["section"][0, 0] == 0


def test_plane_that_misses_and_the_negated_plane():
    v, f = sphere(128)
    v = (v.astype(f64) * [1.0, 0.8, 1.2] + 0.01 * np.random.default_rng(1).standard_normal(v.shape)).astype(f32)
    miss = whole(v, f, np.array([[[0, 0, 1, 5]]], f64), f32)
    assert miss["crossings"][0, 0] == 0 and miss["section"][0, 0] == 0
    pl = np.array([[[0.3, 0.2, 1.0, 0.1], [1.0, -0.5, 0.25, -0.2]]], f64)
    a, b = whole(v, f, pl, f64), whole(v, f, -pl, f64)
    s = ((v.astype(f64)[:, None, :] * pl[0, :, :3]).sum(-1) - pl[0, :, 3])
    assert (s != 0).all()  # no vertex on either plane
    assert (a["crossings"] == b["crossings"]).all() and (a["crossings"] >= 8).all()
    assert np.allclose(a["section"], b["section"], rtol=1e-12, atol=0)
    # the ellipse the plane z = 0.1 cuts from the ellipsoid is approached from inside
    flat = whole(v, f, np.array([[[0, 0, 1, 0.1]]], f64), f64)["section"][0, 0]
    assert 0.85 * 2 * np.pi * 0.9 < flat < 2 * np.pi * 1.0


# ------------------------------------------------------------------------------------------------ spheres
def test_sphere_is_closed_mesh():
    for F in (8, 128, 512):
        v, f = RCPU.closed_mesh(F)
        assert np.array_equal(sphere(F)[0], v) and np.array_equal(sphere(F)[1], f)


def test_sphere_volume_does_not_depend_on_center_and_converges():
    """On closed_mesh(F), F = 8, 128, 2048: the float64 volume does not depend on center, and it grows towards 4 pi / 3 from below.
    closed_mesh only ever splits a face at its centroid, so its first edges never shrink and it does not converge to the sphere: the
    volume stalls at 3.4338 and the area, 6.93 on the octahedron, passes 4 pi = 12.57 (14.88 at F = 128, 16.42 at 2048: the faces fold
    into creases along the old edges).  The convergence of both is therefore asked of the octahedron split at its edge midpoints, at
    the same three face counts 8, 128 = 8 * 4^2 and 2048 = 8 * 4^4, where both errors must fall monotonically and at second order (16-fold per two levels; asked as 12-fold)."""
    rng = np.random.default_rng(5)
    vol = []
    for F in (8, 128, 2048):
        v, f = sphere(F)
        v = v.astype(f64) + [2.5, -0.3, 0.7]
        base = whole(v, f, None, f64)
        for _ in range(3):
            c = rng.normal(0, 3.0, (1, 3))
            moved = whole(v, f, None, f64, center=c)
            assert abs(moved["volume"][0, 0] - base["volume"][0, 0]) <= 1e-12 * abs(base["volume"][0, 0]), (F, c)
            assert abs(moved["area"][0, 0] - base["area"][0, 0]) <= 1e-12 * base["area"][0, 0]
        vol.append(base["volume"][0, 0])
    assert vol[0] < vol[1] < vol[2] < 4 * np.pi / 3
    ev, ea = [], []
    for levels in (0, 2, 4):
        v, f = subdivided(levels)
        assert len(f) == (8, 128, 2048)[levels // 2]
        r = whole(v, f, None, f64, center=np.array([[0.3, -0.2, 0.1]]))
        ev.append(4 * np.pi / 3 - r["volume"][0, 0]), ea.append(4 * np.pi - r["area"][0, 0])
    print("volume short of 4 pi / 3 by", ev, "area short of 4 pi by", ea)
    assert ev[0] > ev[1] > ev[2] > 0 and ea[0] > ea[1] > ea[2] > 0  # monotonically, from below
    assert ev[2] < ev[1] / 12 and ea[2] < ea[1] / 12  # second order in the edge length, which halves per level: 16-fold, asked as 12


def test_float32_form_against_float64_form():
    v, f = sphere(2048)
    v = (0.3 * v.astype(f64) + [0.4, 2.4, -0.5]).astype(f32)
    pl = np.array([[[0, 0, 1, -0.45], [0.2, 1, 0.1, 2.45]]], f64)
    c = np.array([[0.4, 2.4, -0.5]], f64)
    lo, hi = whole(v, f, pl, f32, center=c), whole(v, f, pl, f64, center=c)
    assert (lo["crossings"] == hi["crossings"]).all() and (hi["crossings"] > 32).all()
    for k in ("area", "volume", "section"):
        assert np.abs(lo[k] - hi[k]).max() <= 2e-6 * np.abs(hi[k]).max(), k
    raw = whole(v, f, None, f32)["volume"][0, 0]  # without a centre the cones reach 2.5 m to the origin and cancel
    assert abs(raw - hi["volume"][0, 0]) > 4 * abs(lo["volume"][0, 0] - hi["volume"][0, 0])


# ------------------------------------------------------------------------------------------------ dead data
def test_dead_data():
    v, f = sphere(128)
    v = v.astype(f64) * 0.5
    regions = [np.arange(len(f)), np.zeros(0, np.int64), np.arange(0, len(f), 2)]
    sections = [0, 0, 2, 0, 0]
    pl = np.tile(np.array([0.1, 0.2, 1.0, 0.05]), (1, 5, 1))
    pl[0, 1, 2], pl[0, 3, 3], pl[0, 4, :3] = np.nan, np.inf, 0.0
    bad = 7
    vn = v.copy()
    vn[bad, 1] = np.nan
    kept = [np.array([k for k in r if bad not in f[k]], np.int64) for r in regions]
    for dtype in (f32, f64):
        got = MO.measure(vn[None], f, regions, sections, pl, dtype=dtype)
        assert all(np.isfinite(got[k]).all() for k in got)
        assert (got["area"][0, 1], got["volume"][0, 1]) == (0, 0)  # the empty region
        for s in (1, 3, 4):  # a NaN entry, an infinite offset, a zero normal
            assert got["section"][0, s] == 0 and got["crossings"][0, s] == 0
        ref = MO.measure(v[None], f, kept, sections, pl, dtype=f64)  # the faces of the NaN vertex left out of the lists
        assert (got["crossings"] == ref["crossings"]).all() and got["crossings"][0, 0] > got["crossings"][0, 2] > 0
        for k in ("area", "volume", "section"):
            assert np.allclose(got[k], ref[k], rtol=1e-12 if dtype is f64 else 1e-5, atol=0), k
        g = MO.measure_vjp(vn[None], f, regions, sections, pl, grad_area=np.ones((1, 3)), grad_volume=np.ones((1, 3)),
                           grad_section=np.ones((1, 5)), dtype=dtype)
        assert np.isfinite(g["verts"]).all() and np.isfinite(g["planes"]).all()
        assert (g["verts"][0, bad] == 0).all() and (g["planes"][0, [1, 3, 4]] == 0).all() and (g["planes"][0, [0, 2]] != 0).all()
        gref = MO.measure_vjp(v[None], f, kept, sections, pl, grad_area=np.ones((1, 3)), grad_volume=np.ones((1, 3)),
                              grad_section=np.ones((1, 5)), dtype=f64)
        assert VB.block_error(g["verts"], gref["verts"], (2,)) < (1e-9 if dtype is f64 else 1e-3)


# ------------------------------------------------------------------------------------------------ the backward pass
def _vjp_case(n, shared, seed):
    v0, f = sphere(128)
    rng = np.random.default_rng(seed)
    v = np.stack([v0.astype(f64) * rng.uniform(0.4, 0.6, 3) + rng.normal(0, 0.01, v0.shape) + rng.normal(0, 1.0, 3) for _ in range(n)])
    cen = v.mean(1)
    perm = rng.permutation(len(f))
    regions = [perm, np.zeros(0, np.int64), np.sort(perm[:70])]
    sections = [0, 2, 0]
    nrm = rng.normal(0, 1, (n, 3, 3))
    pl = np.concatenate([nrm, (nrm * (cen[:, None] + rng.normal(0, 0.05, (n, 3, 3)))).sum(-1, keepdims=True)], -1)
    if shared:  # one set of planes for every frame: through the mean centre, which every body covers
        v = v - cen[:, None] + rng.normal(0, 0.02, (n, 1, 3))
        cen = v.mean(1)
        pl = np.concatenate([nrm[:1], (nrm[:1] * rng.normal(0, 0.05, (1, 3, 3))).sum(-1, keepdims=True)], -1)
    w = dict(grad_area=rng.normal(0, 1, (n, 3)), grad_volume=rng.normal(0, 1, (n, 3)), grad_section=rng.normal(0, 1, (n, 3)))
    w["grad_area"][0, 0] = 0.0  # a zero cotangent contributes nothing
    return v, f, regions, sections, pl, cen, w


@pytest.mark.parametrize("n,shared", [(2, False), (33, True)])
def test_closed_form_vjp_equals_float64_autograd(n, shared):
    v, f, regions, sections, pl, cen, w = _vjp_case(n, shared, 11 + n)
    fw = MO.measure(v, f, regions, sections, pl, center=cen, dtype=f64)
    assert (fw["crossings"] >= 6).all()
    tv, tp = torch.tensor(v, requires_grad=True), torch.tensor(pl, requires_grad=True)
    a, vol, sec = MO.measure_torch(tv, f, regions, sections, tp, torch.tensor(cen))
    for k, x in (("area", a), ("volume", vol), ("section", sec)):
        assert np.allclose(x.detach().numpy(), fw[k], rtol=1e-12, atol=1e-15), k
    ((a * torch.tensor(w["grad_area"])).sum() + (vol * torch.tensor(w["grad_volume"])).sum() + (sec * torch.tensor(w["grad_section"])).sum()).backward()
    got = MO.measure_vjp(v, f, regions, sections, pl, center=cen, dtype=f64, **w)
    assert got["planes"].shape == pl.shape
    ev, ep = VB.block_error(got["verts"], tv.grad.numpy(), (2,)), VB.block_error(got["planes"], tp.grad.numpy(), (2,))
    print("closed form against float64 autograd (n = %d, shared = %s): verts %.3g, planes %.3g per block" % (n, shared, ev, ep))
    assert ev <= 1e-9 and ep <= 1e-9
    assert np.abs(tp.grad.numpy()).min() > 0
    # the float32 form of the same rule stays within fp32 of it
    lo = MO.measure_vjp(v.astype(f32), f, regions, sections, pl.astype(f32), center=cen.astype(f32), dtype=f32,
                        **{k: a.astype(f32) for k, a in w.items()})
    assert lo["verts"].dtype == f32 and lo["planes"].dtype == f32


# ------------------------------------------------------------------------------------------------ the table builder
def _table_cases():
    rng = np.random.default_rng(21)
    F = 300
    perm = rng.permutation(F)
    good = dict(F=F, regions=[perm, np.zeros(0, np.int64), np.sort(perm[:77]), perm[40:41]], sections=[2, 0, 0, 3, 2])
    cases = {"good": good, "no_sections": dict(F=5, regions=[np.array([4, 0])], sections=[]),
             "R_max": dict(F=256, regions=[np.array([r]) for r in range(256)], sections=list(range(256)))}
    bad = lambda **kw: dict(good, **kw)  # noqa: E731
    cases.update({
        "id_high": bad(regions=[np.array([0, F])]), "id_low": bad(regions=[np.array([-1])], sections=[]),
        "duplicate": bad(regions=[np.arange(5), np.array([3, 9, 3])], sections=[]), "section_high": bad(sections=[0, 4]),
        "section_low": bad(sections=[-1]), "R_zero": dict(F=F, regions=[], sections=[], claim=dict(R=0)),
        "R_over": bad(claim=dict(R=257)), "S_over": bad(claim=dict(S=257)), "S_negative": bad(claim=dict(S=-1)),
        "ptr_decreasing": bad(ptr=[0, 5, 3, 9, 9]), "ptr_start": bad(ptr=[1, 300, 300, 377, 378])})
    return cases


REFUSED = {"id_high": "face id", "id_low": "face id", "duplicate": "twice", "section_high": "section_region", "section_low": "section_region",
           "R_zero": "R must", "R_over": "R must", "S_over": "S must", "S_negative": "S must", "ptr_decreasing": "non-decreasing",
           "ptr_start": "region_ptr[0]"}


def _write_case(path, c):
    ptr = c.get("ptr", np.cumsum([0] + [len(r) for r in c["regions"]]))
    face = np.concatenate([np.asarray(r, np.int64) for r in c["regions"]] + [np.zeros(0, np.int64)])
    claim = dict(R=len(c["regions"]), S=len(c["sections"]))
    claim.update(c.get("claim", {}))
    with open(path, "wb") as f:
        f.write(np.array([c["F"], claim["R"], claim["S"], len(ptr), len(face)], np.int64).tobytes())
        f.write(np.asarray(ptr, np.int64).tobytes() + face.tobytes())
        f.write(np.asarray((list(c["sections"]) + [0] * 300)[:max(claim["S"], 0)], np.int64).tobytes())


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    from test_keypoints_cpu import read_tables

    d = tmp_path_factory.mktemp("measure_tables")
    exe = str(d / "measure_tables_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "measure_tables_dump.cpp"), "-o", exe])
    out = {}
    for name, c in _table_cases().items():
        _write_case(str(d / (name + ".in")), c)
        p = subprocess.run([exe, str(d / (name + ".in")), str(d / (name + ".out"))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=120)
        assert p.returncode == 0 and not p.stdout, (name, p.stdout)  # a sanitizer report is a failure
        out[name] = (c, read_tables(str(d / (name + ".out"))))
    return out


def test_table_header_is_plain_cpp():
    path = os.path.join(ROOT, "smplpp_amd", "csrc", "measure_tables.h")
    src = open(path).read()
    assert "hip_runtime" not in src and "__device__" not in src and "__global__" not in src
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True,
                   input='#include "%s"\n' % path)


@pytest.mark.parametrize("name", ["good", "no_sections", "R_max"])
def test_tables_equal_the_python_restatement(dumped, name):
    c, t = dumped[name]
    want = MO.tables(c["F"], c["regions"], c["sections"])
    assert "refusal" not in t and set(t) == set(want)
    for k, a in want.items():
        assert np.array_equal(np.frombuffer(t[k], a.dtype), a), k
    if name == "good":  # a face of two regions is held by both, ascending; a region's sections ascend
        ptr, reg = np.frombuffer(t["facePtr"], np.int32), np.frombuffer(t["faceRegion"], np.int32)
        assert max(np.diff(ptr)) == 3 and all((np.diff(reg[ptr[i]:ptr[i + 1]]) > 0).all() for i in range(c["F"]))
        assert np.frombuffer(t["secId"], np.int32).tolist() == [1, 2, 0, 4, 3]


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_table_refusals(dumped, name):
    c, t = dumped[name]
    assert set(t) == {"refusal"} and REFUSED[name] in t["refusal"].decode(), t
    if "claim" not in c and "ptr" not in c:
        assert isinstance(MO.tables(c["F"], c["regions"], c["sections"]), str)


# ------------------------------------------------------------------------------------------------ the surface
NAMES = ("smplpp_measure_create", "smplpp_measure_destroy", "smplpp_measure_info", "smplpp_measure", "smplpp_measure_vjp")


def test_measure_declared_exported_bound():
    from smplpp_amd import _lib

    L = _lib.load()
    for name in NAMES:
        assert name in _lib.declared_symbols()
        fn = getattr(L, name)  # exported
        args = RCPU._header_args(name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args) and fn.restype is C.c_int, (name, args)
        for a, t in zip(args, fn.argtypes):
            scalar = {"int64_t": C.c_int64, "int": C.c_int, "float": C.c_float}
            if "*" not in a:
                assert t is scalar[a.split()[0]], (name, a)
            else:
                assert t in (C.c_void_p, _lib.i64p) or t._type_ is C.c_void_p, (name, a)
    assert RCPU._header_args("smplpp_measure")[1:6] == ["int64_t n", "const float * verts", "const float * center", "const float * planes",
                                                        "int64_t plane_frames"]
    assert RCPU._header_args("smplpp_measure_vjp")[6:13] == ["const float * grad_area", "const float * grad_volume", "const float * grad_section",
                                                             "float * grad_verts", "float * grad_planes", "int accumulate", "int space"]
    # no handle: refused before anything touches a device
    buf = np.zeros(64, f32)
    p = buf.ctypes.data
    h = C.c_void_p(5)
    assert L.smplpp_measure_create(None, 1, p, p, 0, None, C.byref(h)) == 1 and b"smplpp_measure_create" in L.smplpp_last_error()
    assert L.smplpp_measure(None, 1, p, None, None, 1, p, p, None, None, 0, None) == 1 and b"smplpp_measure" in L.smplpp_last_error()
    assert L.smplpp_measure_vjp(None, 1, p, None, None, 1, p, p, None, p, None, 0, 0, None) == 1
    assert L.smplpp_measure_info(None, None, None, None) == 1 and L.smplpp_measure_destroy(None) == 0
    assert (buf == 0).all()


def test_python_helpers():
    from smplpp_amd import measure, model_io

    m = model_io.synthetic_model()
    faces = m["face_indices"].astype(np.int64) - 1
    groups = [list(range(24)), [0, 3, 6, 9], [1, 4], [16, 18, 20, 22]]
    regions = measure.regions_by_joint(m, groups)
    assert np.array_equal(regions[0], np.arange(len(faces)))
    dom = np.argmax(m["weights"], 1)
    for g, r in zip(groups, regions):
        assert len(r) > 0 and (np.diff(r) > 0).all() and np.isin(dom[faces[r]], g).all()
        assert not np.isin(dom[faces[np.setdiff1d(np.arange(len(faces)), r)]], g).all(1).any()
    p, nrm = torch.randn(2, 5, 3, dtype=torch.float64, requires_grad=True), torch.randn(2, 5, 3, dtype=torch.float64, requires_grad=True)
    pl = measure.plane_through(p, nrm)
    assert pl.shape == (2, 5, 4) and torch.equal(pl[..., :3], nrm) and torch.allclose(pl[..., 3], (p * nrm).sum(-1))
    pl.sum().backward()
    assert torch.allclose(p.grad, nrm) and torch.allclose(nrm.grad, 1 + p)
