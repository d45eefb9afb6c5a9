"""The host tables of model creation (smplpp_amd/csrc/model_tables.h) without a GPU.  tests/cpp/model_tables_dump.cpp, built here
with the address and undefined-behaviour sanitizers, runs every table builder on a model file written from numpy and writes the
tables out; a sanitizer report ends it with a non-zero status.  Each case is checked twice: (a) against what defines each table,
restated here in numpy, and (b) against tests/golden/model_tables.json, the element count and SHA-256 of every table as the
one-function smplpp_model_create computed them before the builders were split out of it (hashed from a copy of that function's host
blocks whose uploads were replaced by dumps).  The digests are data: they are never regenerated from the code under test."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from smplpp_amd import model_io

NJ, CT_LEV, CT_OFF, TREE_DMAX, MAXADJ, MAXADJ_WIDE = 24, 12, 52, 12, 12, 16  # smplpp_amd/csrc/layout.h
CT_P_J, CT_P_ZERO = NJ * 9, NJ * 9 + NJ * 3
TREE_LVL, TREE_LVLJ, TREE_SIZE = NJ, NJ + TREE_DMAX + 1, NJ + TREE_DMAX + 1 + NJ
DTYPES = {"wIdx": np.uint8, "wVal": np.float32, "wSum": np.float32, "sB": np.float32, "sG": np.float32, "faceRing": np.uint16,
          "faceMap": np.uint8, "forms": "S1", "refusal": "S1"}  # every other table: int32
BAD_TREE = b"Cannot set kinematic tree: parent(i) must precede i"
BAD_FACE = b"face_indices must be 1-based vertex ids"
BAD_MODEL = b"Cannot initialize a SMPL model!"


def _fan(model, n):
    """Vertex 0 in n faces (a fan over vertices 1..n+1), every other vertex in a strip of at most 3."""
    V = model["vertices_template"].shape[0]
    fan = [[0, 1 + i, 2 + i] for i in range(n)]
    strip = [[k, k + 1, k + 2] for k in range(n + 1, V - 2)]
    model["face_indices"] = np.array(fan + strip, np.int32) + 1
    return model


def _tree(model, parent_of):
    for i in range(1, NJ):
        model["kinematic_tree"][0, i] = parent_of(i)
    return model


def _eight(model):
    """1..4 more joints per vertex with small weights (as tests/test_fk_gpu.py::test_fk_eight_weights_per_vertex)."""
    rng = np.random.default_rng(5)
    w = model["weights"].astype(np.float64)
    for v in range(w.shape[0]):
        extra = rng.choice(np.where(w[v] == 0)[0], size=int(rng.integers(1, 5)), replace=False)
        w[v, extra] = rng.uniform(0.01, 0.1, len(extra))
    w /= w.sum(axis=1, keepdims=True)
    model["weights"] = w.astype(np.float32)
    return model


def _nine_groups():
    """V = 513: nine vertex groups, the last of one vertex; groups 0..2 on joints 0..15 only, 3..4 on joints 16..23 only, the rest
    mixed, at most 4 weights per vertex."""
    model = model_io.tiny_model(513, seed=11)
    w = model["weights"].astype(np.float64)
    w[: 3 * 64, 16:] = 0
    w[3 * 64 : 5 * 64, :16] = 0
    keep = np.argsort(-w, axis=1, kind="stable")[:, :4]
    sp = np.zeros_like(w)
    np.put_along_axis(sp, keep, np.take_along_axis(w, keep, axis=1), axis=1)
    model["weights"] = (sp / sp.sum(axis=1, keepdims=True)).astype(np.float32)
    return model


def _big():
    """V = 65536 (one more than a ring entry holds) with a handful of faces; no bases (the scales are not computed)."""
    rng = np.random.default_rng(3)
    w = np.zeros((65536, NJ), np.float32)
    cols = rng.integers(0, NJ, (65536, 3))
    np.put_along_axis(w, cols, rng.uniform(0.1, 1.0, (65536, 3)).astype(np.float32), axis=1)
    faces = np.array([[1, 2, 3], [3, 2, 65536], [65536, 65535, 1], [70, 7000, 700]], np.int32)
    return {"weights": w, "face_indices": faces, "kinematic_tree": model_io.KINEMATIC_TREE.copy()}


def _bad(key, edit):
    model = model_io.tiny_model(61, seed=7)
    edit(model[key])
    return model


def _zero_bases():
    model = model_io.tiny_model(61, seed=7)
    for k in ("pose_blend_shapes", "shape_blend_shapes", "vertices_template"):
        model[k][:] = 0
    return model


def _set(index, value):
    def edit(a):
        a[index] = value

    return edit


CASES = {
    "synth": model_io.synthetic_model,
    "dense": lambda: model_io.tiny_model(61, seed=7),
    "eight": lambda: _eight(model_io.synthetic_model()),
    "nine_groups": _nine_groups,
    "chain_tree": lambda: _tree(model_io.tiny_model(61, seed=7), lambda i: i - 1),
    "star_tree": lambda: _tree(model_io.tiny_model(61, seed=7), lambda i: 0),
    "fan13": lambda: _fan(model_io.tiny_model(61, seed=7), 13),
    "fan20": lambda: _fan(model_io.tiny_model(61, seed=7), 20),
    "big": _big,
    "bad_tree": lambda: _bad("kinematic_tree", _set((0, 5), 7)),
    "bad_face_zero": lambda: _bad("face_indices", _set((3, 1), 0)),
    "bad_face_high": lambda: _bad("face_indices", _set((3, 1), 62)),
    "zero_bases": _zero_bases,
}
#        maxw, nvg, nlev, chain_fast, madj, ring tables
EXPECT = {
    "synth": (4, 108, 9, 1, 12, True),
    "dense": (24, 1, 9, 1, 12, True),
    "eight": (8, 108, 9, 1, 12, True),
    "nine_groups": (4, 9, 9, 1, None, True),
    "chain_tree": (24, 1, 24, 0, 12, True),
    "star_tree": (24, 1, 2, 0, 12, True),
    "fan13": (24, 1, 9, 1, 16, True),
    "fan20": (24, 1, 9, 1, 16, True),
    "big": (4, 1024, 9, 1, 12, False),
}
REFUSED = {"bad_tree": BAD_TREE, "bad_face_zero": BAD_FACE, "bad_face_high": BAD_FACE, "zero_bases": BAD_MODEL}


def write_model(path, model):
    """The dump program's input (tests/cpp/model_tables_dump.cpp)."""
    w = np.ascontiguousarray(model["weights"], np.float32)
    faces = np.ascontiguousarray(model["face_indices"], np.int32)
    scales = "pose_blend_shapes" in model
    with open(path, "wb") as f:
        f.write(np.array([w.shape[0], faces.shape[0], int(scales)], np.int64).tobytes())
        f.write(w.tobytes())
        f.write(np.ascontiguousarray(model["kinematic_tree"], np.int64)[0].tobytes())
        f.write(faces.tobytes())
        if scales:
            for k in ("pose_blend_shapes", "shape_blend_shapes", "vertices_template"):
                f.write(np.ascontiguousarray(model[k], np.float32).tobytes())


def read_tables(path):
    """name -> (element size, count, bytes)."""
    raw, out, p = open(path, "rb").read(), {}, 0
    while p < len(raw):
        name = raw[p : p + 16].rstrip(b"\0").decode()
        es, n = (int(x) for x in np.frombuffer(raw, np.int64, 2, p + 16))
        out[name] = (es, n, raw[p + 32 : p + 32 + es * n])
        p += 32 + es * n
    assert p == len(raw)
    return out


def digests(tables):
    return {k: {"count": n, "sha256": hashlib.sha256(b).hexdigest()} for k, (_, n, b) in tables.items()}


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("model_tables") / "model_tables_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "model_tables_dump.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "model_tables.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module", params=list(CASES))
def case(request, dump_exe, tmp_path_factory):
    """(name, model, raw tables, tables as arrays) of one case; the program runs once per case."""
    d = tmp_path_factory.mktemp(request.param)
    model = CASES[request.param]()
    write_model(str(d / "model.bin"), model)
    r = subprocess.run([dump_exe, str(d / "model.bin"), str(d / "tables.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0 and not r.stdout, r.stdout  # a sanitizer report is a failure
    raw = read_tables(str(d / "tables.bin"))
    t = {k: np.frombuffer(b, DTYPES.get(k, np.int32)) for k, (_, _, b) in raw.items()}
    assert all(len(t[k]) == raw[k][1] for k in raw)
    return request.param, model, raw, t


def test_headers_are_plain_cpp():
    for h in ("layout.h", "model_tables.h"):
        src = open(os.path.join(ROOT, "smplpp_amd", "csrc", h)).read()
        assert "hip_runtime" not in src and "__device__" not in src and "__global__" not in src
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True,
                       input='#include "%s"\n' % os.path.join(ROOT, "smplpp_amd", "csrc", h))


def test_tables_equal_the_one_function_creation(case, golden):
    name, _, raw, _ = case
    assert digests(raw) == golden[name]


def test_refusals(case):
    name, _, _, t = case
    if name in REFUSED:
        assert t["refusal"].tobytes() == REFUSED[name] and list(t)[-1] == "refusal"
        assert "perm" not in t and ("wSum" in t) == (name == "zero_bases")  # the bases are looked at after tree and faces
    else:
        assert "refusal" not in t
    # the texts are the library's
    src = open(os.path.join(ROOT, "smplpp_amd", "csrc", "model_tables.h")).read()
    assert all(src.count('"%s"' % s.decode()) == 1 for s in (BAD_TREE, BAD_FACE, BAD_MODEL))


def test_expected_branches(case):
    name, model, _, t = case
    if name in REFUSED:
        return
    maxw, nvg, nlev, fast, madj, rings = EXPECT[name]
    V, F = model["weights"].shape[0], model["face_indices"].shape[0]
    assert (t["maxw"][0], len(t["flags"]), t["nlev"][0], t["chain_fast"][0]) == (maxw, nvg, nlev, fast)
    assert nvg == -(-V // 64)
    if madj is not None:
        assert t["madj"][0] == madj
    mr = 3 * (int(t["madj"][0]) + 1) + 1
    assert (len(t["faceRing"]), len(t["faceMap"])) == ((F * (mr + 1), F * 9 * int(t["madj"][0])) if rings else (0, 0))
    deg = np.diff(t["adjOff"]).max()
    assert {"fan13": 13, "fan20": 20}.get(name, deg) == deg and t["madj"][0] == (MAXADJ_WIDE if rings and deg > MAXADJ else MAXADJ)
    # forms under SMPLPP_SKIN unset, e, h, b, v: e holds 4 weights per vertex and b 8, a model with more takes the next form
    want = {4: b"eheehhbbvv", 8: b"bhbbhhbbvv", 24: b"vhvvhhvvvv"}[maxw]
    assert t["forms"].tobytes() == want


def test_skin_weight_tables(case):
    name, model, _, t = case
    if name in REFUSED and name != "zero_bases":
        return
    W = model["weights"]
    V, maxw = W.shape[0], int(t["maxw"][0])
    nz = int((W != 0).sum(axis=1).max())
    assert maxw == (4 if nz <= 4 else 8 if nz <= 8 else 24)
    vpad = -(-V // 32) * 32
    idx, val, wsum = t["wIdx"].reshape(vpad, maxw), t["wVal"].reshape(vpad, maxw), t["wSum"]
    assert len(wsum) == vpad and (idx[V:] == 0).all() and (val[V:] == 0).all() and (wsum[V:] == 1).all()
    back = np.zeros((V, NJ), np.float32)
    # (a dense table lists every joint once; a compacted one its non-zeros in ascending joint order, then zeros on joint 0)
    np.add.at(back, (np.repeat(np.arange(V), maxw), idx[:V].reshape(-1).astype(np.int64)), val[:V].reshape(-1))
    assert back.tobytes() == W.tobytes()
    live = val[:V] != 0
    assert maxw == NJ or ((np.diff(idx[:V].astype(int), axis=1) > 0) | ~live[:, 1:]).all()
    assert maxw == NJ or (live[:, :-1] | ~live[:, 1:]).all()  # the non-zeros come first
    s = np.zeros(V, np.float32)
    for j in range(NJ):
        s = s + W[:, j]
    assert wsum[:V].tobytes() == s.tobytes()


def test_h_scales(case):
    name, model, _, t = case
    if name in REFUSED or "pose_blend_shapes" not in model:
        assert "sB" not in t
        return
    tmax = np.abs(model["vertices_template"]).max()
    bmax = max(np.abs(model["pose_blend_shapes"]).max(), np.abs(model["shape_blend_shapes"]).max(), tmax)
    for s, bound in ((t["sB"][0], bmax), (t["sG"][0], max(16 * float(tmax), 1.0))):
        assert np.frexp(s)[0] == 0.5 and s * bound <= 32768 < 2 * s * bound  # the largest power of two that keeps the bound in range


def test_h_vertex_groups(case):
    name, model, _, t = case
    if name in REFUSED:
        return
    W = model["weights"]
    V = W.shape[0]
    nvg = -(-V // 64)
    perm, flags = t["perm"].reshape(nvg, 64), t["flags"]
    assert np.array_equal(np.sort(perm[perm >= 0]), np.arange(V))
    first = perm[:, 0]
    assert (first >= 0).all() and (first % 64 == 0).all()
    want = first[:, None] + np.arange(64)
    assert np.array_equal(perm, np.where(want < V, want, -1))  # 64 consecutive vertices, -1 past the last vertex
    # slice x of the eight is groups [x nvg / 8, (x + 1) nvg / 8) of the new order; the original groups are dealt to the slices in
    # turn, a full slice passing its turn on
    bounds = [(x * nvg) >> 3 for x in range(9)]
    dealt, x = [[] for _ in range(8)], 0
    for g in range(nvg):
        while len(dealt[x]) >= bounds[x + 1] - bounds[x]:
            x = (x + 1) % 8
        dealt[x].append(g)
        x = (x + 1) % 8
    for x in range(8):
        assert sorted(first[bounds[x] : bounds[x + 1]] // 64) == dealt[x] and len(dealt[x]) == ((x + 1) * nvg >> 3) - (x * nvg >> 3)
    lo, hi = (W[:, :16] != 0).any(axis=1), (W[:, 16:] != 0).any(axis=1)
    bits = np.where(hi, np.where(lo, 3, 2), 1)  # (a vertex without weights counts as joints 0..15)
    for g in range(nvg):
        vs = perm[g][perm[g] >= 0]
        assert flags[g] == np.bitwise_or.reduce(bits[vs])
    # inside a slice each class keeps its original order, at evenly spaced ranks: the k-th of a class's n groups sorts by (k + 1/2) / n
    for x in range(8):
        f, o = flags[bounds[x] : bounds[x + 1]], first[bounds[x] : bounds[x + 1]]
        key = np.zeros(len(f))
        for c in (1, 2, 3):
            assert (np.diff(o[f == c]) > 0).all()
            key[f == c] = (np.arange((f == c).sum()) + 0.5) / max((f == c).sum(), 1)
        assert (np.diff(key) >= 0).all()


def _parent(model):
    p = model["kinematic_tree"][0].astype(np.int64).copy()
    p[0] = -1
    return p


def test_tree_tables(case):
    name, model, _, t = case
    if name in REFUSED:
        return
    parent = _parent(model)
    depth = np.zeros(NJ, int)
    for i in range(1, NJ):
        depth[i] = depth[parent[i]] + 1
    nlev = int(t["nlev"][0])
    assert np.array_equal(t["depth"], depth) and nlev == depth.max() + 1
    lvl = t["lvl"]
    assert len(lvl) == CT_OFF + 60 * CT_LEV * 2
    off, joints = lvl[: nlev + 1], lvl[NJ + 1 : NJ + 1 + NJ]
    assert np.array_equal(joints, np.argsort(depth, kind="stable"))  # a permutation of the joints by depth, ascending inside a level
    assert np.array_equal(off, np.searchsorted(np.sort(depth), np.arange(nlev + 1)))
    widths = np.diff(off)
    fast = nlev <= CT_LEV and widths.max() <= 5
    assert t["chain_fast"][0] == int(fast)
    # chain table: [lane = slot * 12 + entry][level][2]
    ct = lvl[CT_OFF:].reshape(60, CT_LEV, 2)
    empty = (0x00FFFF, CT_P_ZERO | (CT_P_ZERO << 10) | (1 << 20))
    slot_of = {}
    for L in range(CT_LEV):
        members = list(joints[off[L] : off[L + 1]]) if L < nlev else []
        # the levels a table that is not used still holds: those before the first level wider than 5, that level's first 5 included
        written = nlev <= CT_LEV and (fast or L <= int(np.argmax(widths > 5)))
        for q in range(5):
            for e in range(12):
                w0, w1 = (int(x) for x in ct[q * 12 + e, L])
                if not written or q >= len(members):
                    assert (w0, w1) == empty
                    continue
                i, c = int(members[q]), e % 4
                p = int(parent[i])
                slot_of[i] = q
                assert (w0 & 0xFF, (w0 >> 8) & 0xFF, w0 >> 16) == (i, p if p >= 0 else 0xFF, slot_of[p] if p >= 0 else 0)
                a = i * 9 + c if c < 3 else CT_P_J + i * 3
                b = CT_P_J + p * 3 if (c == 3 and p >= 0) else CT_P_ZERO
                assert (w1 & 0x3FF, (w1 >> 10) & 0x3FF, w1 >> 20) == (a, b, 3 if c < 3 else 1)
    # IK tree tables
    anc = t["anc"]
    assert len(anc) == TREE_SIZE
    for i in range(NJ):
        m, j = 0, i
        while j >= 0:
            m |= 1 << j
            j = int(parent[j])
        assert anc[i] == m
    shallow = np.sort(depth[depth < TREE_DMAX])
    assert np.array_equal(anc[TREE_LVL : TREE_LVL + TREE_DMAX + 1], np.searchsorted(shallow, np.arange(TREE_DMAX + 1)))
    order = np.argsort(depth, kind="stable")
    order = order[depth[order] < TREE_DMAX]
    assert np.array_equal(anc[TREE_LVLJ : TREE_LVLJ + len(order)], order) and (anc[TREE_LVLJ + len(order) :] == -1).all()


def test_adjacency_and_ring_tables(case):
    name, model, _, t = case
    if name in REFUSED:
        return
    faces = model["face_indices"].astype(np.int64) - 1
    F, V = faces.shape[0], model["weights"].shape[0]
    assert np.array_equal(t["faces"].reshape(F, 3), faces)
    off, adjf = t["adjOff"], t["adjFace"]
    assert len(off) == V + 1 and off[0] == 0 and off[V] == len(adjf)
    # per vertex: the faces that contain it, ascending, once each
    pairs = np.unique(np.stack([faces.reshape(-1), np.repeat(np.arange(F), 3)], axis=1), axis=0)
    assert np.array_equal(adjf, pairs[:, 1]) and np.array_equal(np.diff(off), np.bincount(pairs[:, 0], minlength=V))
    if not len(t["faceRing"]):
        assert V > 65535 and not len(t["faceMap"])
        return
    madj = int(t["madj"][0])
    mr = 3 * (madj + 1) + 1
    ring = t["faceRing"].reshape(F, mr + 1).astype(np.int64)
    fmap = t["faceMap"].reshape(F, 3, madj, 3).astype(np.int64)
    nr, slots = ring[:, 0], ring[:, 1:]
    assert np.array_equal(slots[:, :3], faces) and (nr >= 3).all() and (nr <= mr).all()
    live = np.arange(mr)[None, :] < nr[:, None]
    assert (slots[~live] == 0).all()
    srt = np.sort(np.where(live, slots, -1 - np.arange(mr)[None, :]), axis=1)
    assert (np.diff(srt, axis=1) != 0).all()  # the ring's entries are distinct
    # (i, a, c) -> the ring slot of corner c of the a-th adjacent face of corner i (the first madj faces of a vertex with more)
    deg = np.diff(off)
    adjpad = np.full((V, madj), -1, np.int64)
    for a in range(madj):
        has = deg > a
        adjpad[has, a] = adjf[off[:-1][has] + a]
    g = adjpad[faces]  # [F, 3, madj]
    want = faces[np.maximum(g, 0)]  # [F, 3, madj, 3]
    got = np.take_along_axis(slots, fmap.reshape(F, -1), axis=1).reshape(F, 3, madj, 3)
    ok = got == want
    if (nr == mr).any():  # (random faces can fill a ring: what it could not take maps to slot 0)
        held = ((slots[:, None, None, None, :] == want[..., None]) & live[:, None, None, None, :]).any(-1)
        ok |= ~held & (nr == mr)[:, None, None, None] & (fmap == 0)
    assert ok[g >= 0].all() and (fmap[g < 0] == 0).all()
    # every ring vertex beyond the face's own comes from one of those adjacent faces
    for f in range(0, F, max(1, F // 64)):
        assert set(slots[f, : nr[f]]) <= set(faces[f]) | set(want[f][g[f] >= 0].reshape(-1))
