"""The mesh-side backward passes on the MI355X, held to float64 VERTEX BY VERTEX (tests/vertex_blocks.py): every (frame, vertex)
three-vector of grad_verts, every (frame, query) three-vector of grad_points and every (frame, vertex) row of grad_attr within
max(4 x the fp32 oracle's worst block of the case, 4 x 2^-24) of the ABSOLUTE SUM of the shares that enter it, a block without shares
exactly zero, no block left out; so that a vertex cannot hide in a frame's L2 norm (tests/test_vertex_blocks_cpu.py plants the error
the L2 bar of the existing tests lets through).

  a. the record gather: pointMeshDistanceBackward, pointMeshSignedDistanceBackward, meshPointDistanceBackward and
     pointMeshDistanceCompatibleBackward around the 1024-record tile and the 256-target workgroup
  b. the raster walk and gather: depthRasterBackward, rasterInterpolateBackward, silhouetteBackward on the scenes of
     tests/raster_vjp_cases.py and on `near`, the body from 0.25 m (the scene whose yardstick stays under 64 x 2^-24 with the body's
     valences in the gather; `body`'s depth and interpolation are held to four times a yardstick of 9000 x 2^-24: 2.2e-3 of a vertex's
     absolute sum), and the silhouette's pixel side on an open patch that faces the camera
  c. the normal queries: calcMeshVertexNormalsBackward (LDS with and without the opt-in, staged), calcVertexNormalBackward,
     calcNormalBackward (list forms in LDS and in the workspace)

`face`, `index`, `inside` and `bary` are the forward call's own.  Every line printed (run with -s) gives E beside the yardstick
e32, the bar and the old L2 figure.  Self-penetration, the scene term and the image term are still on their L2 bars."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vertex_blocks as B  # noqa: E402

pytestmark = pytest.mark.gpu

_handles = {}


def _handle(which):
    """One SMPL handle per mesh for the module: the body through _synth, the icosphere and the fan through _model_for."""
    from test_depth_raster_gpu import _model_for, _synth

    if which not in _handles:
        m = B.mesh(which)
        _handles[which] = _synth(m["model"]) if which == "body" else _model_for(m["V"], m["faces"])
        assert _handles[which].info()["vertex_num"] == m["V"] and _handles[which].info()["face_num"] == len(m["faces"])
    return _handles[which]


def _held(tag, got, r64, r32, base=None):
    """Every output of `got` within bar(e32) of the float64 reference, block by block; with `base` {output: array} the call added
    into it: got - base is held, the scale enlarged by |base|.  Prints every figure, then asserts."""
    bad = []
    for k, (ref, A) in r64.items():
        x = np.asarray(got[k], np.float64)
        e32 = B.figure(r32[k][0], ref, A.max(-1))[0]
        scale = A.max(-1)
        if base is not None:
            x, scale = x - base[k].astype(np.float64), (A + np.abs(base[k])).max(-1)
        E, worst = B.figure(x, ref, scale)
        print("%-58s %-6s E = %9.3g (%8.1f x 2^-24) at block %-11s fp32 oracle %8.1f x 2^-24   bar %9.3g   L2 %.2e (fp32 %.2e)"
              % (tag, k, E, E / B.EPS32, worst, e32 / B.EPS32, B.bar(e32), B.frame_l2(x, ref), B.frame_l2(r32[k][0], ref)))
        if not (np.isfinite(np.asarray(got[k])).all() and E <= B.bar(e32)):
            bad.append((tag, k, E, B.bar(e32), worst))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- a. the record gather
def _point_mesh(s, c, signed):
    """(args of the reference, the backward call) at the forward's own faces (and flags)."""
    faces = B.mesh(c["mesh"])["faces"]
    if signed:
        face, _, _, _, inside, _ = s.pointMeshSignedDistance(c["verts"], c["points"])
        call = lambda **kw: s.pointMeshSignedDistanceBackward(c["verts"], c["points"], face, inside, c["grad"], **kw)  # noqa: E731
    else:
        face, inside = s.pointMeshDistance(c["verts"], c["points"])[0], None
        call = lambda **kw: s.pointMeshDistanceBackward(c["verts"], c["points"], face, c["grad"], **kw)  # noqa: E731
    return (c["verts"], faces, c["points"], face, c["grad"]), dict(inside=inside), call


def _check_point_mesh(c, signed):
    s = _handle(c["mesh"])
    a, kw, call = _point_mesh(s, c, signed)
    gv, gp = call()
    _held(("signed " if signed else "point->mesh ") + c["name"], {"verts": gv, "points": gp}, B.point_mesh_reference(*a, **kw),
          B.point_mesh_reference(*a, dtype="float32", **kw))


def _check_mesh_point(c):
    s = _handle(c["mesh"])
    index, _ = s.meshPointDistance(c["verts"], c["points"])
    assert (index >= 0).all()
    gv, gp = s.meshPointDistanceBackward(c["verts"], c["points"], index, c["grad_mp"])
    a = (c["verts"], c["points"], index, c["grad_mp"])
    _held("mesh->point " + c["name"], {"verts": gv, "points": gp}, B.mesh_point_reference(*a), B.mesh_point_reference(*a, dtype="float32"))


@pytest.mark.parametrize("K", B.GATHER_K)
@pytest.mark.parametrize("which", B.MESHES)
@pytest.mark.parametrize("signed", [False, True], ids=["distance", "signed"])
def test_point_mesh_around_the_tile(signed, which, K):
    """One tile, a tile filled exactly, one record in a second tile, a third tile; 3, 27 and 2 target workgroups (the hub of the fan
    the first target of the second)."""
    _check_point_mesh(B.gather_case(which, K), signed)


@pytest.mark.parametrize("K", [B.GATHER_TILE, 2 * B.GATHER_TILE + 1])
@pytest.mark.parametrize("which", ["ico", "body"])
@pytest.mark.parametrize("layout", ["oneface", "silent"])
@pytest.mark.parametrize("signed", [False, True], ids=["distance", "signed"])
def test_point_mesh_layouts(signed, layout, which, K):
    """Every query over one face (a tile's records all hit the same three targets: the compaction is full); frame 1 with a zero
    cotangent on every third query."""
    c = B.gather_case(which, K, layout)
    if layout == "oneface":
        face = _handle(which).pointMeshDistance(c["verts"], c["points"])[0]
        assert (face == c["face"]).mean() > 0.9
    _check_point_mesh(c, signed)


@pytest.mark.parametrize("K", B.GATHER_K + B.POINT_K)
def test_mesh_point_around_the_tile_and_the_workgroup(K):
    """642 vertex records of the icosphere into K targets: one target, 255 to 257 of them, and the tile sizes."""
    _check_mesh_point(B.gather_case("ico", K))


@pytest.mark.parametrize("which,K,layout", [("body", 1, "generic"), ("body", B.GATHER_T + 1, "generic"),
                                            ("body", B.GATHER_TILE + 1, "silent"), ("fan", B.GATHER_T + 1, "generic"),
                                            ("ico", B.GATHER_T, "silent")])
def test_mesh_point_record_counts(which, K, layout):
    """6890 records (seven tiles, the last partial; at K = 1 all of them on one target) and 257 (one tile)."""
    _check_mesh_point(B.gather_case(which, K, layout))


@pytest.mark.parametrize("entry", ["distance", "signed", "mesh_point"])
def test_record_gather_accumulates(entry):
    """out= and grad_points=: what the call added is held to the same bar, the scale enlarged by what was there."""
    c = B.gather_case("ico", B.GATHER_TILE + 1)
    s = _handle("ico")
    rng = np.random.default_rng(5)
    base = {"verts": rng.normal(size=c["verts"].shape).astype(np.float32), "points": rng.normal(size=c["points"].shape).astype(np.float32)}
    if entry == "mesh_point":
        index, _ = s.meshPointDistance(c["verts"], c["points"])
        gv, gp = s.meshPointDistanceBackward(c["verts"], c["points"], index, c["grad_mp"], out=base["verts"].copy(),
                                             grad_points=base["points"].copy())
        a = (c["verts"], c["points"], index, c["grad_mp"])
        r64, r32 = B.mesh_point_reference(*a), B.mesh_point_reference(*a, dtype="float32")
    else:
        a, kw, call = _point_mesh(s, c, entry == "signed")
        gv, gp = call(out=base["verts"].copy(), grad_points=base["points"].copy())
        r64, r32 = B.point_mesh_reference(*a, **kw), B.point_mesh_reference(*a, dtype="float32", **kw)
    _held(entry + " out= " + c["name"], {"verts": gv, "points": gp}, r64, r32, base=base)


def test_compatible_backward_with_unmatched_queries():
    """K = 1025 with face = -1 records (a third of the query normals reversed, a tenth zero; the cap keeps a reversed query from
    the far side of the body): they contribute nothing."""
    c = B.compatible_case()
    s = _handle(c["mesh"])
    face, _, _, _, matched = s.pointMeshDistanceCompatible(c["verts"], c["points"], c["normals"], max_dist=c["max_dist"])
    assert (matched == c["matched"]).mean() > 0.95 and (face[~matched] == -1).all() and (face[matched] >= 0).all()
    gv, gp = s.pointMeshDistanceCompatibleBackward(c["verts"], c["points"], face, c["grad"])
    assert not gp[~matched].any()
    a = (c["verts"], B.mesh(c["mesh"])["faces"], c["points"], face, c["grad"])
    _held("compatible " + c["name"], {"verts": gv, "points": gp}, B.point_mesh_reference(*a), B.point_mesh_reference(*a, dtype="float32"))


# ---------------------------------------------------------------------------------------------- b. the raster walk and gather
@pytest.fixture(scope="module")
def raster():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = B.raster_case(name, on_gpu=True)
        return cache[name]

    return get


def _frames(name, x):
    """The frames held to the bar.  Frame 0 of `hand` has NaN and Inf vertices and every face refused: its gradients are exactly
    zero (asserted by the callers), and the float64 oracle is not run through it."""
    if name == "hand":
        assert (x["face"][0] < 0).all() and not np.isfinite(x["verts"][0]).all()
        return slice(1, None)
    return slice(None)


@pytest.mark.parametrize("name", B.RASTER_SCENES)
def test_depth_raster_backward(raster, name):
    s, faces, H, W, x = raster(name)
    fr = _frames(name, x)
    got = s.depthRasterBackward(x["verts"], x["camera"], H, W, x["face"], x["grad_depth"])
    assert np.isfinite(got).all() and not got[:fr.start or 0].any()
    a = (x["verts"][fr], faces, x["camera"][fr], x["face"][fr], x["grad_depth"][fr])
    r64, r32 = B.depth_reference(*a), B.depth_reference(*a, dtype="float32")
    _held("depth " + name, {"verts": got[fr]}, r64, r32)
    base = x["base_verts"]
    acc = s.depthRasterBackward(x["verts"], x["camera"], H, W, x["face"], x["grad_depth"], out=base.copy())
    _held("depth out= " + name, {"verts": acc[fr]}, r64, r32, base={"verts": base[fr]})
    assert np.array_equal(acc[:fr.start or 0], base[:fr.start or 0])  # a frame whose faces are all refused leaves what was there


@pytest.mark.parametrize("want", [("attr", "verts"), ("attr",), ("verts",)], ids=["both", "attr", "verts"])
@pytest.mark.parametrize("C", B.RASTER_C)
@pytest.mark.parametrize("name", B.RASTER_SCENES)
def test_raster_interpolate_backward(raster, name, C, want):
    s, faces, H, W, x = raster(name)
    fr = _frames(name, x)
    attr, g = x["attr_%d" % C], x["grad_image_%d" % C]
    got = s.rasterInterpolateBackward(attr, x["verts"], x["camera"], H, W, x["face"], x["bary"], g, want=want)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.isfinite(got[k]).all() and not got[k][:fr.start or 0].any(), k
    a = (attr[fr], x["verts"][fr], faces, x["camera"][fr], x["face"][fr], g[fr])
    r64, r32 = B.interpolate_reference(*a), B.interpolate_reference(*a, dtype="float32")
    _held("interpolate C=%d want=%s %s" % (C, "+".join(want), name), {k: got[k][fr] for k in want}, {k: r64[k] for k in want}, r32)
    if len(want) == 2:
        base = {"attr": x["base_attr_%d" % C], "verts": x["base_verts"]}
        acc = s.rasterInterpolateBackward(attr, x["verts"], x["camera"], H, W, x["face"], x["bary"], g,
                                          out={k: b.copy() for k, b in base.items()})
        _held("interpolate C=%d out= %s" % (C, name), {k: acc[k][fr] for k in want}, r64, r32, base={k: b[fr] for k, b in base.items()})
        for k in want:
            assert np.array_equal(acc[k][:fr.start or 0], base[k][:fr.start or 0]), k


@pytest.mark.parametrize("name", B.RASTER_SCENES)
def test_silhouette_backward(raster, name):
    """Both sides on `hand` (frame 1); on `spheres`, `near` and `body` the conditioned cotangents leave the vertex side (a source
    pixel of the pixel side is a rim pixel of the coverage, grazing on a closed surface)."""
    s, faces, H, W, x = raster(name)
    fr = _frames(name, x)
    args = (x["vert_target"], x["pix_source"], x["grad_vert_sq"], x["grad_pix_sq"])
    got = s.silhouetteBackward(x["verts"], x["camera"], H, W, x["face"], *args)
    assert np.isfinite(got).all() and not got[:fr.start or 0].any()
    a = (x["verts"][fr], faces, x["camera"][fr], H, W, x["face"][fr]) + tuple(t[fr] for t in args)
    r64, r32 = B.silhouette_reference(*a), B.silhouette_reference(*a, dtype="float32")
    _held("silhouette " + name, {"verts": got[fr]}, r64, r32)
    base = x["base_verts"]
    acc = s.silhouetteBackward(x["verts"], x["camera"], H, W, x["face"], *args, out=base.copy())
    _held("silhouette out= " + name, {"verts": acc[fr]}, r64, r32, base={"verts": base[fr]})
    assert np.array_equal(acc[:fr.start or 0], base[:fr.start or 0])


def test_silhouette_pixel_side():
    """vertex_blocks.patch_case: about 3000 live records a frame (three tiles) from mask pixels in many 256-pixel groups onto the
    patch's right rim, targets in both workgroups; alone and added into `out`."""
    from test_depth_raster_gpu import _model_for

    s, faces, H, W, x = B.patch_case(_model_for)
    live = (x["pix_source"] >= 0) & (x["grad_pix_sq"] != 0)
    assert (live.sum((1, 2)) > 2 * B.GATHER_TILE).all()
    args = (x["vert_target"], x["pix_source"], x["grad_vert_sq"], x["grad_pix_sq"])
    a = (x["verts"], faces, x["camera"], H, W, x["face"]) + args
    r64, r32 = B.silhouette_reference(*a), B.silhouette_reference(*a, dtype="float32")
    got = s.silhouetteBackward(x["verts"], x["camera"], H, W, x["face"], *args)
    _held("silhouette patch", {"verts": got}, r64, r32)
    got = s.silhouetteBackward(x["verts"], x["camera"], H, W, x["face"], x["vert_target"], x["pix_source"], None, x["grad_pix_sq"])
    _held("silhouette patch (no vertex cotangent)", {"verts": got}, r64, r32)
    acc = s.silhouetteBackward(x["verts"], x["camera"], H, W, x["face"], *args, out=x["base_verts"].copy())
    _held("silhouette patch out=", {"verts": acc}, r64, r32, base={"verts": x["base_verts"]})


# ---------------------------------------------------------------------------------------------- c. the normal queries
def _normals_call(s, c, out=None):
    if c["kind"] == "face":
        return s.calcNormalBackward(c["verts"], c["ids"], c["grad"], out=out)
    if c["kind"] == "vertex":
        return s.calcVertexNormalBackward(c["verts"], c["ids"], c["grad"], out=out)
    return s.calcMeshVertexNormalsBackward(c["verts"], c["grad"], out=out)


def _check_normals(c, tag=""):
    m = B.mesh(c["mesh"])
    got = _normals_call(_handle(c["mesh"]), c)
    a = (m["oracle"], c["kind"], c["ids"], c["verts"], c["grad"])
    r64, r32 = B.normals_reference(*a), B.normals_reference(*a, dtype="float32")
    _held("normals " + tag + c["name"], {"verts": got}, r64, r32)
    return r64, r32


@pytest.mark.parametrize("which", B.MESHES)
def test_normals_backward(which):
    """The whole mesh in LDS (the body's 82.7 KB behind the opt-in, the icosphere's 7.7 KB and the fan's 3 KB without it) and the
    list forms: a vertex list of 200 ids does not fit the 64 KB of the LDS form (the arithmetic of mesh_vjp.hip from the handle's
    own adjacency), one of 5 and the face list of 300 do; the hub of valence 16."""
    s = _handle(which)
    V = s.info()["vertex_num"]
    assert (V * 12 > 64 * 1024) == (which == "body")
    if which == "body":
        maxdeg = max(len(s.getAdjacentFaces(int(u))) for u in np.argsort(-B.mesh(which)["valence"], kind="stable")[:8])
        assert maxdeg == B.mesh(which)["valence"].max()
        assert B.list_buffer_bytes(5, maxdeg, True) <= B.LIST_LDS_BYTES < B.list_buffer_bytes(200, maxdeg, True)
        assert B.list_buffer_bytes(300, maxdeg, False) <= B.LIST_LDS_BYTES
    for c in B.normals_cases(which):
        _check_normals(c)


def test_normals_backward_staged(monkeypatch):
    """SMPLPP_NORMALS_VJP_STAGED=1 (read at every call; restored by monkeypatch): the workspace forms of the whole mesh and of a list."""
    monkeypatch.setenv("SMPLPP_NORMALS_VJP_STAGED", "1")
    _check_normals(B.normals_case("body", "mesh", 3), "staged ")
    _check_normals(B.normals_case("body", "vertex", 3, B.vertex_ids("body", 5)), "staged ")


@pytest.mark.parametrize("kind", ["mesh", "vertex", "face"])
def test_normals_backward_accumulates(kind):
    ids = {"mesh": None, "vertex": np.array([B.FAN_HUB, 0, B.FAN_HUB, 17], np.int64), "face": np.array([0, 1, 15, 40, 0], np.int64)}[kind]
    c = B.normals_case("fan", kind, 3, ids)
    m = B.mesh("fan")
    base = np.random.default_rng(9).normal(size=c["verts"].shape).astype(np.float32)
    acc = _normals_call(_handle("fan"), c, out=base.copy())
    a = (m["oracle"], kind, ids, c["verts"], c["grad"])
    _held("normals out= " + c["name"], {"verts": acc}, B.normals_reference(*a), B.normals_reference(*a, dtype="float32"),
          base={"verts": base})
