"""The numpy oracles of the stage calls and forward mesh queries (tests/stage_oracle.py, tests/mesh_query_oracle.py) must be right
before the GPU is held to them: the float64 statements against the reference's known-answer vectors, against the C oracle on
random inputs, and against the torch restatement of the whole chain; and, on every case list of tests/test_stages_gpu.py and
tests/test_mesh_queries_gpu.py, the float32 run of the same graph, whose scaled error is the yardstick of those files' bars.
It is printed here (run with -s): that is where the yardstick's size is written down.  No GPU."""
import json
import os

import numpy as np
import pytest

import mesh_query_oracle as mq
import stage_oracle as so
from conftest import GOLDEN
from oracle import cpu

TOL = 2e-6  # tests/test_oracle_kats.py: the KATs are printed with 6 decimals


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(GOLDEN, "tester_kats.json")) as f:
        return json.load(f)


def test_float64_stages_reproduce_the_kats(kats):
    i, e = kats["blendShape"]["inputs"], kats["blendShape"]["expected"]
    rot = so.rodrigues(np.array(i["theta"], np.float32))
    bs, bp = so.blend(i["beta"], rot, i["shapeBlendBasis"], i["poseBlendBasis"])
    np.testing.assert_allclose(bs.reshape(1, 3), np.array(e["shapeBlendShape"]), atol=TOL)
    np.testing.assert_allclose(bp.reshape(1, 1, 3), np.array(e["poseBlendShape"]), atol=3 * TOL)
    np.testing.assert_allclose(rot[0, :5], np.array(e["poseRotation"]), atol=TOL)
    i, e = kats["jointRegression"]["inputs"], kats["jointRegression"]["expected"]
    rest, joints = so.joint_regression(i["templateShape"], i["jointRegressor"], i["shapeBlendShape"], i["poseBlendShape"])
    np.testing.assert_allclose(rest, np.array(e["restShape"]), atol=TOL)
    np.testing.assert_allclose(joints[0], np.array(e["joints"]), atol=2 * TOL)
    i, e = kats["worldTransformation"]["inputs"], kats["worldTransformation"]["expected"]
    out = so.world(np.array(i["kineTree"], np.int64)[0], i["joints"], i["poseRotation"])
    np.testing.assert_allclose(out[0, :5], np.array(e["transformations"]), atol=3 * TOL)
    i, e = kats["linearBlendSkinning"]["inputs"], kats["linearBlendSkinning"]["expected"]
    out = so.skinning(i["weights"], i["restShape"], i["transformations"], None)
    np.testing.assert_allclose(out, np.array(e["vertices"]), atol=TOL)


def _held(name, x, ref64, x32, factor=4):
    """x within the bar that the fp32 run x32 of the same graph sets (stage_oracle.bar); prints both figures."""
    e, e32 = so.scaled_error(x, ref64), so.scaled_error(x32, ref64)
    print("%-34s E = %.3g (%.2f x 2^-24)   fp32 oracle E = %.3g (%.2f x 2^-24)" % (name, e, e / so.EPS32, e32, e32 / so.EPS32))
    assert np.isfinite(np.asarray(x32)).all(), name
    assert e <= so.bar(e32, factor), (name, e, e32)


def test_float64_stages_agree_with_the_c_oracle():
    """V = 37, n = 3, random inputs: the C oracle's stage functions compute in fp32 (their own association), so their float
    outputs sit within fp32 rounding of the float64 statement — the bar of an fp32 evaluation, 4 x the numpy fp32 run's error."""
    rng = np.random.default_rng(47)
    n, V = 3, 37
    f32 = lambda *shape: rng.normal(0, 1, shape).astype(np.float32)
    beta, theta, S, P = f32(n, 10), f32(n, 24, 3), f32(V, 3, 10), f32(V, 3, 207)
    cbs, cbp, crot = cpu.blend_shape(beta, theta, S, P)
    out = {}
    for dt in (np.float64, np.float32):
        rot = so.rodrigues(theta, dt)
        out[dt] = (rot,) + so.blend(beta, rot, S, P, dt)
    _held("C rodrigues", cpu.rodrigues(theta), out[np.float64][0], out[np.float32][0])
    _held("C blend_shape rot", crot, out[np.float64][0], out[np.float32][0])
    _held("C blend_shape Bs", cbs, out[np.float64][1], out[np.float32][1])
    _held("C blend_shape Bp", cbp, out[np.float64][2], out[np.float32][2])
    T, Jreg = f32(V, 3), f32(24, V)
    crest, cj = cpu.joint_regression(T, Jreg, cbs, cbp)
    r64, r32 = so.joint_regression(T, Jreg, cbs, cbp), so.joint_regression(T, Jreg, cbs, cbp, np.float32)
    _held("C joint_regression rest", crest, r64[0], r32[0])
    _held("C joint_regression joints", cj, r64[1], r32[1])
    kt = so.TREES["binary"]
    cx = cpu.world_transformation(kt, cj, crot)
    _held("C world_transformation", cx, so.world(kt, cj, crot), so.world(kt, cj, crot, np.float32))
    W, root = np.abs(f32(V, 24)), f32(n, 3)
    cv = cpu.lbs(W, crest, cx, root)
    _held("C lbs", cv, so.skinning(W, crest, cx, root), so.skinning(W, crest, cx, root, np.float32))


def test_float64_chain_equals_the_torch_restatement(synth_model):
    """The four stages chained in float64 on the synthetic model against tests/fk_vjp_oracle.py::fk in float64: two independent
    statements of one definition, 1e-12 relative."""
    import torch

    import fk_vjp_oracle as fo
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(3, seed=5)
    m = fo.model_tensors(synth_model)
    ref = fo.fk(m, torch.as_tensor(beta, dtype=torch.float64), torch.as_tensor(theta, dtype=torch.float64))
    rot = so.rodrigues(theta[:, 1:])
    Bs, Bp = so.blend(beta, rot, synth_model["shape_blend_shapes"], synth_model["pose_blend_shapes"])
    rest, joints = so.joint_regression(synth_model["vertices_template"], synth_model["joint_regressor"], Bs, Bp)
    X = so.world(m["parent"], joints, rot)
    verts = so.skinning(synth_model["weights"], rest, X, theta[:, 0])
    for k, x in (("rest", rest), ("joints", joints), ("xforms", X), ("verts", verts)):
        r = ref[k].numpy()
        assert np.abs(x - r).max() <= 1e-12 * np.abs(r).max(), k


# ---- the fp32 yardstick on every case list of tests/test_stages_gpu.py
def _self_held(name, fn):
    """fn(dtype) -> tuple of arrays: the fp32 run is finite and (trivially) within the bar with the factor 4 replaced by 1."""
    r64, r32 = fn(np.float64), fn(np.float32)
    for k, (a, b) in enumerate(zip(r64, r32)):
        assert b.dtype == np.float32
        _held("%s [%d]" % (name, k), b, a, b, factor=1)


def test_fp32_yardstick_of_the_stage_cases():
    for n, V in so.BLEND_SHAPES:
        for c in (so.blend_case(n, V),) + ((so.blend_zero_case(),) if (n, V) == (1, 1) else ()):
            def run(dt, c=c):
                rot = so.rodrigues(c["theta"], dt)
                return (rot,) + so.blend(c["beta"], rot, c["S"], c["P"], dt)

            _self_held("blend n=%d V=%d" % (n, V), run)
            rot32 = so.rodrigues(c["theta"], np.float32)
            for f in c["zero_frames"]:  # what the GPU test asserts with array_equal holds for the fp32 graph too
                assert np.array_equal(rot32[f], np.tile(np.eye(3, dtype=np.float32), (24, 1, 1)))
                assert np.array_equal(so.blend(c["beta"], rot32, c["S"], c["P"], np.float32)[1][f], np.zeros((V, 3), np.float32))
    for V in so.REGRESS_V:
        c = so.regress_case(V)
        _self_held("joint regression V=%d" % V, lambda dt: so.joint_regression(c["T"], c["Jreg"], c["Bs"], c["Bp"], dt))
    for n in so.WORLD_N:
        for tree in so.TREES:
            for general in (False, True):
                c = so.world_case(n, tree, general)
                _self_held("world n=%d %s %s" % (n, tree, "general" if general else "rotations"),
                           lambda dt: (so.world(c["parent"], c["joints"], c["rot"], dt),))
    for n, V in so.SKIN_SHAPES:
        c = so.skin_case(n, V)
        for root in (c["root"], None):
            _self_held("skinning n=%d V=%d root=%s" % (n, V, root is not None),
                       lambda dt: (so.skinning(c["W"], c["rest"], c["G"], root, dt),))


def test_blend_case_carries_the_edge_angles():
    for n, V in so.BLEND_SHAPES:
        a = np.linalg.norm(so.blend_case(n, V)["theta"].astype(np.float64), axis=-1)
        assert (a == float(np.float32(np.pi))).any() and (np.abs(a - 1e-4) < 1e-9).any() and (np.abs(a - 7) < 1e-5).any()
        assert n == 1 or (a[0] == 0).all()


# ---- the fp32 yardstick on the models of tests/test_mesh_queries_gpu.py
def _models():
    from smplpp_amd import model_io

    yield "synthetic", model_io.synthetic_model()
    yield "tiny61", model_io.tiny_model(61, seed=7)
    for N in mq.FANS:
        yield "fan%d" % N, mq.double_fan_model(N)


def _mesh_yardstick(name, verts, faces, adj):
    kf, kv = mq.face_condition(verts, faces), mq.vertex_condition(verts, faces, adj)
    for what, fn, kappa, exact in (("face", lambda dt: mq.face_normals(verts, faces, None, dt), kf, mq.dead_faces(verts, faces)),
                                   ("vertex", lambda dt: mq.vertex_normals(verts, faces, adj, None, dt), kv,
                                    mq.dead_vertices(verts, faces, adj))):
        r64, r32 = fn(np.float64), fn(np.float32)
        assert r32.dtype == np.float32 and np.isfinite(r32).all()
        e32 = mq.scaled_error(r32, r64, kappa, exact)
        print("%-26s %-6s normals: fp32 oracle max err/kappa = %.3g (%.2f x 2^-24), max finite kappa = %.3g"
              % (name, what, e32, e32 / mq.EPS32, kappa[np.isfinite(kappa)].max()))
        assert e32 <= mq.bar(e32, 1)
    return kf, kv


def test_fp32_yardstick_of_the_mesh_cases():
    beta, theta = mq.posed_inputs()
    for name, md in _models():
        faces, V = mq.faces0(md), md["vertices_template"].shape[0]
        adj = mq.adjacency(faces, V)
        verts = cpu.OracleModel(md).fk(beta, theta, want=("verts",))["verts"]
        _mesh_yardstick(name, verts, faces, adj)
        f, v = mq.degenerate_targets(faces, V)
        for pair in mq.CORNER_PAIRS:
            dv = mq.collapse_face(verts, faces, f, pair)
            assert np.array_equal(mq.face_normals(dv, faces, [f], np.float32), np.zeros((3, 1, 3), np.float32))
            assert np.array_equal(mq.face_normals(dv, faces, [f]), np.zeros((3, 1, 3)))
            _mesh_yardstick("%s face %d corners %s" % (name, f, pair), dv, faces, adj)
        dv = mq.collapse_vertex_star(verts, faces, v)
        assert np.array_equal(mq.vertex_normals(dv, faces, adj, [v], np.float32), np.zeros((3, 1, 3), np.float32))
        _mesh_yardstick("%s star of vertex %d" % (name, v), dv, faces, adj)


def test_adjacency_and_id_lists():
    """adjacency() against the C oracle's table (ascending face ids, 1/deg) and the shape of the id lists."""
    md = mq.double_fan_model(70)
    faces, V = mq.faces0(md), 72
    off, fid, w = mq.adjacency(faces, V)
    o = cpu.OracleModel(md)
    for v in range(V):
        of, ow = o.get_adjacency(v)
        assert sorted(of.tolist()) == fid[off[v]:off[v + 1]].tolist()
        assert (np.diff(fid[off[v]:off[v + 1]]) > 0).all()
        assert np.array_equal(w[off[v]:off[v + 1]], np.full(len(of), np.float32(1) / np.float32(len(of)), np.float32))
    assert off[1] - off[0] == 70 and off[2] - off[1] == 4
    lists = mq.id_lists(140, seed=1)
    assert [len(x) for x in lists] == [142, 1, 127, 128, 129]
    assert sorted(lists[0][:-2].tolist()) == list(range(140)) and lists[0][-2:].tolist() == [0, 139]


def test_grid_extents_and_bounds_vertices():
    for V in (61, 1024, 1025, 2500):
        for variant in ("plain", "negative", "on_grid"):
            v = mq.bounds_vertices(V, variant)
            assert v.dtype == np.float32 and (v.argmin(axis=0) == V - 1).all()
            assert (v.argmax(axis=0) == (1024 if V == 2500 else V - 2)).all()
            lo, num = mq.grid_extents(v)
            assert lo.dtype == np.int32 and (num > 1).all()
            assert variant != "negative" or (v < 0).all()
            # losing either extreme vertex changes the grid: the interior stays at least a cell away from both
            inner = np.delete(v, [V - 1, v.argmax(axis=0)[0]], axis=0)
            ilo, inum = mq.grid_extents(inner)
            assert (ilo > lo).all() and (ilo + inum < lo + num).all()
    v = mq.bounds_vertices(61, "on_grid")
    assert np.array_equal(mq.grid_extents(v)[0], [-17, -17, -17]) and np.array_equal(mq.grid_extents(v)[1], [34, 34, 34])
