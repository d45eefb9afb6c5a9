"""Surface geodesics and the self-contact mask without a GPU: the two restatements of the distance rule in tests/geodesic_oracle.py
(a Dijkstra with fp32 adds, a synchronous pull relaxation) agree to the bit on every test mesh and on the synthetic body; the fp32
field against the same walk with float64 adds; the asymmetry of the fp32 sum that makes the mask's rule name the lower index; the
host edge-table builder and plan functions (smplpp_amd/csrc/edge_tables.h) as a stand-alone program built with the address and
undefined-behaviour sanitizers; filter_pairs against a loop."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geodesic_oracle as GO  # noqa: E402

from smplpp_amd import contact, model_io  # noqa: E402

MESHES = {
    "ico0": lambda: GO.icosphere(0),
    "ico1": lambda: GO.icosphere(1),
    "ico2": lambda: GO.icosphere(2),
    "ico3": lambda: GO.icosphere(3),
    "torus_7x9": lambda: GO.torus(7, 9),
    "two_spheres": lambda: GO.two_spheres(1),
    "fan": lambda: GO.fan(5),
}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def synthetic():
    m = model_io.synthetic_model()
    rest = np.ascontiguousarray(m["vertices_template"], np.float32)
    faces0 = np.asarray(m["face_indices"], np.int64) - 1
    off, adj = GO.edge_table(len(rest), faces0)
    return rest, faces0, off, adj, GO.edge_weights(rest, off, adj)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_dijkstra_equals_relaxation_on_the_meshes(name):
    verts, faces0 = MESHES[name]()
    V = len(verts)
    off, adj = GO.edge_table(V, faces0)
    w = GO.edge_weights(verts, off, adj)
    sets = [[0], [V // 2], [V - 1], [0, V // 3, V - 1], [1, 1], []]
    R, sweeps = GO.relax(V, off, adj, w, sets)
    assert sweeps <= V
    for s, srcs in enumerate(sets):
        d, hops = GO.dijkstra(V, off, adj, w, srcs)
        assert np.array_equal(_bits(d), _bits(R[s])), (name, srcs)
        assert ((hops >= 0) == np.isfinite(d)).all()
    assert np.isinf(R[5]).all()
    if name == "two_spheres":
        assert np.isinf(R[0][V * 4 // 5:]).all() and np.isfinite(R[2][V * 4 // 5:]).all()


def test_dijkstra_equals_relaxation_on_the_synthetic_body(synthetic):
    rest, _, off, adj, w = synthetic
    V = len(rest)
    srcs = [0, V // 2, V - 1]
    R, sweeps = GO.relax(V, off, adj, w, [[s] for s in srcs])
    assert 2 <= sweeps <= V
    for r, s in enumerate(srcs):
        d, _ = GO.dijkstra(V, off, adj, w, [s])
        assert np.array_equal(_bits(d), _bits(R[r])), s
        # the cap is a threshold of the uncapped field
        cap = np.float32(np.median(d))
        dc, _ = GO.dijkstra(V, off, adj, w, [s], max_dist=cap)
        assert np.array_equal(_bits(dc), _bits(np.where(d > cap, np.float32(np.inf), d)))


@pytest.mark.parametrize("name", ["ico3", "torus_7x9", "synthetic"])
def test_fp32_field_against_float64_adds(name, synthetic):
    """The same walk over the same fp32 edge lengths with float64 adds.  Each fp32 add errs by at most 2^-24 of the partial sum, which
    never exceeds the total, so along a path of h edges the two sums differ by at most h 2^-24 relative (first order); the two minima
    may run along different paths, so h is the larger of the two hop counts, and the bound asserted is h 2^-23."""
    if name == "synthetic":
        verts, _, off, adj, w = synthetic
    else:
        verts, faces0 = MESHES[name]()
        off, adj = GO.edge_table(len(verts), faces0)
        w = GO.edge_weights(verts, off, adj)
    V = len(verts)
    d32, h32 = GO.dijkstra(V, off, adj, w, [0])
    d64, h64 = GO.dijkstra(V, off, adj, w, [0], dtype=np.float64)
    assert np.isfinite(d64).all()
    hops = np.maximum(h32, h64)
    assert (np.abs(d32.astype(np.float64) - d64) <= hops * 2.0 ** -23 * d64).all()


def test_fp32_sum_is_not_symmetric_but_the_mask_is(synthetic):
    """Sources 0 and 5000 of the synthetic template: the distance one way and the other differ in the last bit, which is why far(v, u)
    names the lower index as the source."""
    rest, faces0, off, adj, w = synthetic
    V = len(rest)
    a, _ = GO.dijkstra(V, off, adj, w, [0])
    b, _ = GO.dijkstra(V, off, adj, w, [5000])
    print("0 -> 5000: %.7f   5000 -> 0: %.7f" % (a[5000], b[0]))
    assert abs(float(a[5000]) - 1.24459) < 1e-4
    ba, bb = int(_bits(a[5000:5001])[0]), int(_bits(b[0:1])[0])
    assert ba != bb and abs(ba - bb) <= 2
    # a threshold between the two values: the rule still gives one answer for the pair
    geo_min = min(a[5000], b[0])
    far, known = GO.far_matrix(rest, faces0, geo_min, sources=[0])
    assert known[0, 5000] and known[5000, 0] and far[0, 5000] == far[5000, 0] == (a[5000] > geo_min)


def test_oracle_mask_is_symmetric_with_a_zero_diagonal():
    verts, faces0 = GO.torus(4, 8)
    far, _ = GO.far_matrix(verts, faces0, 0.9)
    assert 0 < far.sum() < far.size - len(far)
    assert (far == far.T).all() and not far.diagonal().any()
    mask, pairs = GO.far_mask(verts, faces0, 0.9)
    assert mask.shape == (32, 1) and pairs == far.sum() // 2
    assert (GO.unpack_bits(mask, 32) == far).all()


# ---------------------------------------------------------------- the table builder and the plan as a stand-alone program
def _table_cases():
    tv, tf = GO.torus(5, 6)
    fv, ff = GO.fan(5)
    tet = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    return {
        "tetrahedron": (4, tet),
        "torus": (len(tv), tf),
        "fan": (len(fv), ff),
        "duplicated_face": (4, np.concatenate([tet, tet[1:2], tet[1:2, ::-1]])),
        "vertex_in_no_face": (7, tet + 2),           # vertices 0, 1 and 6 are in no face
        "repeated_corner": (4, np.array([[0, 0, 1], [1, 2, 3]])),  # (0, 0) is no edge
    }


REFUSALS = {"corner_out_of_range": (4, np.array([[0, 1, 4]])), "negative_corner": (4, np.array([[0, -1, 2]])), "no_faces": (4, np.zeros((0, 3), int))}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    from test_keypoints_cpu import read_tables

    d = tmp_path_factory.mktemp("edge_tables")
    exe = str(d / "edge_tables_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "edge_tables_dump.cpp"), "-o", exe])

    def run(name, V, faces):
        with open(str(d / (name + ".in")), "wb") as f:
            f.write(np.array([V, len(faces)], np.int64).tobytes() + np.ascontiguousarray(faces, np.int32).tobytes())
        p = subprocess.run([exe, str(d / (name + ".in")), str(d / (name + ".out"))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=120)
        assert p.returncode == 0 and not p.stdout, (name, p.stdout)  # a sanitizer report is a failure
        return read_tables(str(d / (name + ".out")))

    return exe, run


def test_table_header_is_plain_cpp():
    path = os.path.join(ROOT, "smplpp_amd", "csrc", "edge_tables.h")
    src = open(path).read()
    assert "hip_runtime" not in src and "__device__" not in src and "__global__" not in src
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True,
                   input='#include "%s"\n' % path)


@pytest.mark.parametrize("name", sorted(_table_cases()))
def test_edge_table_equals_the_numpy_builder(dump, name):
    V, faces = _table_cases()[name]
    t = dump[1](name, V, faces)
    assert "refusal" not in t
    off, adj = GO.edge_table(V, faces)
    assert np.frombuffer(t["dims"], np.int64).tolist() == [V, len(adj)]
    assert np.array_equal(np.frombuffer(t["off"], np.int32), off)
    assert np.array_equal(np.frombuffer(t["adj"], np.int32), adj)
    assert np.array_equal(np.frombuffer(t["src"], np.int32), GO.edge_rows(off))
    # ascending, each once, no self-edges, symmetric
    for v in range(V):
        row = adj[off[v]:off[v + 1]]
        assert (np.diff(row) > 0).all() and v not in row
        assert all(v in adj[off[u]:off[u + 1]] for u in row)
    if name == "vertex_in_no_face":
        assert off[1] == off[0] == off[2] and off[7] == off[6]
    if name == "duplicated_face":
        assert np.array_equal(adj, GO.edge_table(4, _table_cases()["tetrahedron"][1])[1])


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_edge_table_refusals(dump, name):
    V, faces = REFUSALS[name]
    t = dump[1](name, V, faces)
    assert list(t) == ["refusal"] and t["refusal"]


def test_plan_functions(dump):
    """The workgroup's LDS is the field, V floats, and 16 bytes of flags: 64 KiB without the opt-in up to V = 16380, so 16384 and 16385
    both need it; refused above 32768; the loop's bound is V."""
    Vs = [1, 12, 6890, 16380, 16381, 16384, 16385, 32768, 32769, 0]
    p = subprocess.run([dump[0], "--plan"] + [str(v) for v in Vs], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stderr
    rows = {r[0]: r[1:] for r in ([int(x) for x in line.split()] for line in p.stdout.splitlines())}
    assert list(rows) == Vs
    for V in Vs[:8]:
        lds, opt_in, sweeps, words, refused = rows[V]
        assert (lds, opt_in, sweeps, words, refused) == (4 * V + 16, int(4 * V + 16 > 65536), V, (V + 31) // 32, 0)
    assert rows[16380][:2] == [65536, 0] and rows[16381][:2] == [65540, 1]
    assert rows[16384][:2] == [65552, 1] and rows[16385][:2] == [65556, 1]
    assert rows[32768][0] == 131088 <= 160 * 1024
    assert rows[32769][4] == 1 and rows[0][4] == 1


# ---------------------------------------------------------------- filter_pairs
def test_filter_pairs_against_a_loop():
    rng = np.random.default_rng(5)
    V, F = 70, 120
    far = rng.random((V, V)) < 0.8
    far = np.triu(far, 1)
    far = far | far.T
    mask = GO.pack_bits(far)
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)])
    pairs = rng.integers(0, F, (3, 40, 2))
    pairs[0, 30:] = -1
    pairs[2, 5:] = -1
    want = np.zeros(pairs.shape[:2], bool)
    for n in range(3):
        for k in range(40):
            f, g = pairs[n, k]
            want[n, k] = f >= 0 and all(far[a, b] for a in faces[f] for b in faces[g])
    assert 0 < want.sum() < (pairs[..., 0] >= 0).sum()
    got = contact.filter_pairs(pairs, faces, mask)
    assert got.dtype == bool and np.array_equal(got, want)
    assert np.array_equal(contact.filter_pairs(pairs[1], faces, mask), want[1])
    tmask = torch.from_numpy(mask.view(np.int32))
    tg = contact.filter_pairs(torch.from_numpy(pairs), faces, tmask)
    assert np.array_equal(tg.numpy(), want)
