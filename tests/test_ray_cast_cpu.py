"""Ray casting without a GPU: the rule of tests/ray_cast_oracle.py on hand cases (facing, a ray exactly through a shared edge and
through a vertex, parallel and edge-on faces, the range boundaries, the equal-t tie, dead rays, a NaN face); its float32 form
against its float64 form on the synthetic mesh; the closed surface's degree on rays aimed at fp32 vertices and edge midpoints; the
closed-form backward pass against float64 autograd; the camera rays against the depth rasteriser's oracle; the ABI."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_raster_oracle as DR  # noqa: E402
import ray_cast_oracle as RC  # noqa: E402

f32, f64 = np.float32, np.float64
OCT_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
OCT_F = np.array([[4, 0, 2], [4, 2, 1], [4, 1, 3], [4, 3, 0], [5, 2, 0], [5, 1, 2], [5, 3, 1], [5, 0, 3]], np.int64)  # outward
# one triangle in the plane z = 0, counter-clockwise seen from +z (normal +z)
TRI_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)
TRI_F = np.array([[0, 1, 2]], np.int64)


def closed_mesh(F, lone=False):
    """A closed, outward-facing triangulation of the unit sphere with F faces (F even, >= 8): an octahedron whose largest face is
    split at its centroid, pushed out to the sphere, until there are F.  With `lone` one free triangle more, outside it: F + 1 faces
    (an odd count, which no closed surface has)."""
    v, f = [p for p in OCT_V.astype(f64)], [tuple(t) for t in OCT_F]
    while len(f) < F:
        area = [np.linalg.norm(np.cross(v[b] - v[a], v[c] - v[a])) for a, b, c in f]
        a, b, c = f.pop(int(np.argmax(area)))
        m = v[a] + v[b] + v[c]
        v.append(m / np.linalg.norm(m))
        k = len(v) - 1
        f += [(a, b, k), (b, c, k), (c, a, k)]
    assert len(f) == F
    if lone:
        k = len(v)
        v += [np.array([1.5, 0.1, 0.2]), np.array([1.6, 0.9, 0.1]), np.array([1.4, 0.2, 1.0])]
        f.append((k, k + 1, k + 2))
    return np.array(v).astype(f32), np.array(f, np.int64)


def sphere_rays(K, centre, seed, radius=2.5):
    """K origins on a sphere about `centre` (float32)."""
    rng = np.random.default_rng(seed)
    o = rng.standard_normal((K, 3))
    return (radius * o / np.linalg.norm(o, axis=1, keepdims=True) + centre).astype(f32)


def warped_template(model):
    """The synthetic template bent by a smooth warp: (verts [V,3] float32, faces [F,3] int64)."""
    v = model["vertices_template"].astype(f64)
    v = v + 0.04 * np.sin(3.0 * v[:, [1, 2, 0]] + 0.5)
    return v.astype(f32), model["face_indices"].astype(np.int64) - 1


def cast1(v, f, o, d, **kw):
    return RC.ray_cast_frame(v, f, np.asarray(o, f32).reshape(-1, 3), np.asarray(d, f32).reshape(-1, 3), **kw)


# ------------------------------------------------------------------------------------------------ hand cases
def test_front_and_back_under_each_facing():
    down, up = ([0.25, 0.25, 2], [0, 0, -1]), ([0.25, 0.25, -2], [0, 0, 2])  # against the normal, along it (t in units of |dir|)
    for (o, d), side, t in ((down, 0, 2.0), (up, 1, 1.0)):
        for facing in (1, 2, 3):
            r = cast1(TRI_V, TRI_F, o, d, facing=facing)
            seen = bool(facing & (1 << side))
            assert r["face"][0] == (0 if seen else -1) and r["t"][0] == (f32(t) if seen else 0)
            assert r["hits"][0].tolist() == [int(seen and side == 0), int(seen and side == 1)]
            if seen:
                assert np.allclose(r["bary"][0], [0.5, 0.25, 0.25])
            else:
                assert (r["bary"][0] == 0).all()
    flipped = cast1(TRI_V, TRI_F[:, ::-1], *down, facing=1)  # the stored winding decides, not the geometry
    assert flipped["face"][0] == -1


def test_ray_through_a_shared_edge_hits_exactly_one_face():
    v = np.array([[0, 0, 0], [1, 1, 0], [1, 0, 0.25], [0, 1, -0.5]], f32)  # the edge 0-1 is shared; the ray meets it at (0.5, 0.5, 0)
    pair = (np.array([0, 1, 3]), np.array([1, 0, 2]))  # consistently oriented
    rays = [([0.5, 0.5, 3], [0, 0, -1]), ([0.5, 0.5, -3], [0, 0, 1]), ([0.5 + 2, 0.5, 4], [-1, 0, -2]), ([3.5, 0.5, 0], [-1, 0, 0])]
    seen = 0
    for flip in (False, True):
        for r0 in range(3):
            for r1 in range(3):
                f = np.stack([np.roll(pair[0], r0), np.roll(pair[1], r1)])
                f = f[:, ::-1] if flip else f
                for o, d in rays:
                    r = cast1(v, f, o, d)
                    cov = RC.coverage(v, f, np.array([o], f32), np.array([d], f32))
                    assert len(cov[0]) == 1 and r["hits"][0].sum() == 1 and r["face"][0] in (0, 1), (flip, r0, r1, o)
                    seen += 1
    assert seen == 2 * 9 * 4


def test_ray_through_a_vertex_of_a_closed_octahedron_hits_exactly_once():
    # through two opposite vertices along an axis; into a vertex at a slant, inside a symmetry plane and off every one
    rays = [([0, 0, 5], [0, 0, -1]), ([5, 0, 0], [-1, 0, 0]), ([0, -3, 0], [0, 2, 0]), ([0.5, 0, 3], [-0.25, 0, -1]), ([0.5, 0.25, 3], [-0.25, -0.125, -1])]
    rng = np.random.default_rng(3)
    for trial in range(12):  # the vertex ids must not matter: every relabelling, every stored corner order
        perm = rng.permutation(6) if trial else np.arange(6)
        v = np.empty_like(OCT_V)
        v[perm] = OCT_V
        f = np.stack([np.roll(perm[t], rng.integers(0, 3)) for t in OCT_F])
        for o, d in rays:
            r = cast1(v, f, o, d)
            assert r["hits"][0].tolist() == [1, 1] and r["cover"][0] == 0, (trial, o, r["hits"][0])
            assert cast1(v, f, o, d, facing=1)["hits"][0].tolist() == [1, 0]
    # the apex ray enters at the apex itself
    r = cast1(OCT_V, OCT_F, [0, 0, 5], [0, 0, -1])
    assert r["t"][0] == 4 and np.abs(r["bary"][0]).max() == 1


def test_parallel_and_edge_on_faces_cover_nothing():
    for o, d in (([-1, 0.25, 0], [1, 0, 0]), ([-1, 0.25, 1], [1, 0, 0]), ([0.25, -2, 0], [0, 1, 0]), ([-1, -1, 0], [1, 1, 0])):
        r = cast1(TRI_V, TRI_F, o, d)
        assert r["face"][0] == -1 and r["hits"][0].sum() == 0 and r["cover"][0] == 0


def test_range_boundaries():
    o, d = [0.25, 0.25, 2], [0, 0, -1]  # t = 2 exactly
    assert cast1(TRI_V, TRI_F, o, d, t_max=2.0)["face"][0] == 0  # t = t_max is accepted
    assert cast1(TRI_V, TRI_F, o, d, t_min=2.0)["face"][0] == -1  # t = t_min is dropped
    assert cast1(TRI_V, TRI_F, o, d, t_min=np.nextafter(f32(2), f32(0)))["face"][0] == 0
    assert cast1(TRI_V, TRI_F, o, d, t_max=np.nextafter(f32(2), f32(0)))["face"][0] == -1
    assert cast1(TRI_V, TRI_F, [0.25, 0.25, -2], [0, 0, -1])["face"][0] == -1  # behind the origin
    assert cast1(TRI_V, TRI_F, [0.25, 0.25, 0], [0, 0, -1])["face"][0] == -1  # t = 0 is never a hit


def test_equal_t_goes_to_the_lowest_face():
    v = np.concatenate([TRI_V, TRI_V + f32([0, 0, 1])])
    f = np.array([[3, 4, 5], [0, 1, 2], [0, 1, 2], [2, 0, 1]], np.int64)
    r = cast1(v, f, [0.25, 0.25, -2], [0, 0, 1], facing=3)
    assert r["face"][0] == 1 and r["t"][0] == 2 and r["hits"][0].tolist() == [0, 4]


def test_dead_rays_and_a_nan_face():
    v, f = closed_mesh(8)
    o = np.tile(f32([0.1, 0.2, 3]), (8, 1))
    d = np.tile(f32([0, 0, -1]), (8, 1))
    o[1, 0], o[2, 1], d[3, 2], d[4, 0], d[5] = np.nan, np.inf, np.nan, -np.inf, 0
    r = RC.ray_cast_frame(v, f, o, d)
    for k in range(1, 6):
        assert r["face"][k] == -1 and r["t"][k] == 0 and (r["bary"][k] == 0).all() and (r["hits"][k] == 0).all(), k
    for k in (0, 6, 7):
        assert r["face"][k] == r["face"][0] >= 0 and r["hits"][k].tolist() == [1, 1]
    vn = v.copy()
    vn[4, 1] = np.nan  # the faces of the top vertex cover nothing; the others are as they were
    rn = RC.ray_cast_frame(vn, f, o, d)
    assert rn["hits"][0].tolist() == [0, 1] and (OCT_F[rn["face"][0]] != 4).all()
    assert rn["t"][0].tobytes() == cast1(v, f, o[0], d[0], facing=2)["t"][0].tobytes()


# ------------------------------------------------------------------------------------------------ the synthetic mesh
@pytest.fixture(scope="module")
def synth_cast(synth_model):
    """3000 rays from a 2.5 m sphere aimed at random surface points of the warped template, cast in float32 and in float64."""
    v, f = warped_template(synth_model)
    K = 3000
    rng = np.random.default_rng(11)
    fid = rng.integers(0, len(f), K)
    w = rng.dirichlet([1, 1, 1], K)
    target = (v[f[fid]].astype(f64) * w[:, :, None]).sum(1)
    o = sphere_rays(K, v.mean(0), 12)
    d = (target - o).astype(f32)
    return dict(v=v, f=f, o=o, d=d, r32=RC.ray_cast_frame(v, f, o, d), r64=RC.ray_cast_frame(v, f, o, d, dtype=f64))


def test_float32_rule_against_float64_on_the_synthetic_mesh(synth_cast):
    c = synth_cast
    r32, r64, v, f = c["r32"], c["r64"], c["v"], c["f"]
    assert (r64["face"] >= 0).all() and (r32["cover"] == 0).all() and (r64["cover"] == 0).all()
    sure = np.abs(r64["bary"]).min(1) >= 1e-4
    left_out = 1.0 - sure.mean()
    print("left out by the 1e-4 margin: %.3f %%; faces that differ inside it: %d" % (100 * left_out, (r32["face"] != r64["face"])[sure].sum()))
    assert left_out <= 0.01
    assert (r32["face"] == r64["face"])[sure].all()
    same = r32["face"] == r64["face"]
    # what a textbook fp32 intersection gets wrong on the same hits: the bar is 4 x its worst error over the rays, or 1e-5
    tri = v[f[r64["face"]]]
    mt, mu, mv = RC.moller_trumbore(tri, c["o"], c["d"])
    mt_t = np.abs(mt.astype(f64) - r64["t"]) / r64["t"]
    mt_b = np.abs(np.stack([(f32(1) - mu) - mv, mu, mv], 1).astype(f64) - r64["bary"]).max(1)
    e_t = (np.abs(r32["t"].astype(f64) - r64["t"]) / r64["t"])[same]
    e_b = np.abs(r32["bary"].astype(f64) - r64["bary"]).max(1)[same]
    print("t: %.3g relative (Moller-Trumbore %.3g); bary: %.3g (Moller-Trumbore %.3g)" % (e_t.max(), mt_t.max(), e_b.max(), mt_b.max()))
    assert e_t.max() <= max(4 * mt_t.max(), 1e-5)
    assert e_b.max() <= max(4 * mt_b.max(), 1e-5)


@pytest.mark.parametrize("aim", ["vertices", "edge midpoints"])
def test_degree_and_misses_on_rays_aimed_at_vertices_and_edges(synth_model, aim):
    v, f = warped_template(synth_model)
    K = 1000
    rng = np.random.default_rng(21 if aim == "vertices" else 22)
    if aim == "vertices":
        vid = rng.integers(0, len(v), K)
        target = v[vid]
        around = [np.nonzero((f == i).any(1))[0] for i in vid]  # the faces around each target
    else:
        t = f[rng.integers(0, len(f), K)]
        e = rng.integers(0, 3, K)
        p, q = t[np.arange(K), e], t[np.arange(K), (e + 1) % 3]
        target = ((v[p] + v[q]) * f32(0.5)).astype(f32)
        around = [np.nonzero((f == i).any(1) & (f == j).any(1))[0] for i, j in zip(p, q)]
    o = sphere_rays(K, v.mean(0), 23)
    d = (target - o).astype(f32)
    r32 = RC.ray_cast_frame(v, f, o, d)
    # the closed surface's degree: as many covering faces of one sign as of the other, for every ray, before the range test
    assert (r32["cover"] == 0).all()
    assert (r32["hits"][:, 0] == r32["hits"][:, 1]).all()  # (every range is positive here: the origins are outside)
    r64 = RC.ray_cast_frame(v, f, o, d, dtype=f64)
    # silhouette grazes.  The faces float64 finds covering, as the measure is stated, and the faces around the target: the ray passes
    # within rounding of the target, so each of those covers it in one arithmetic or the other, and a ray that MISSES in float64
    # has no covering face left to show that it grazed.  A ray is left out when one of these faces is edge-on to it
    # (|n.d| / (|n||d|) < 1e-3) or when the faces around its target face both ways: the target is on the silhouette, where
    # which side of it the ray passes is decided inside the last bit of dir.  (On the covering faces alone the two miss sets
    # differed on 9 of 1000 vertex rays and 1 of 1000 edge rays, every one aimed at a silhouette vertex or edge.)
    rays, ids, _, _ = RC.coverage(v, f, o, d, dtype=f64)
    rays, ids = np.concatenate([rays, np.repeat(np.arange(K), [len(a) for a in around])]), np.concatenate([ids] + around)
    p = RC.plane(v[f[ids]].astype(f64), o[rays].astype(f64), d[rays].astype(f64), f64)
    cosine = p["nd"] / (np.linalg.norm(p["n"], axis=1) * np.linalg.norm(d[rays].astype(f64), axis=1))
    graze = np.zeros(K, bool)
    graze[rays[np.abs(cosine) < 1e-3]] = True
    own = np.arange(len(rays)) >= len(rays) - sum(len(a) for a in around)
    front, back = np.zeros(K, bool), np.zeros(K, bool)
    front[rays[own & (cosine < 0)]] = True
    back[rays[own & (cosine > 0)]] = True
    graze |= front & back
    miss32, miss64 = r32["face"] < 0, r64["face"] < 0
    print("%s: %d of %d rays left out as silhouette grazes (%.2f %%); float32 misses %d, float64 misses %d; they differ outside the grazes on %d"
          % (aim, graze.sum(), K, 100 * graze.mean(), miss32.sum(), miss64.sum(), (miss32 != miss64)[~graze].sum()))
    assert graze.mean() <= 0.05
    assert (miss32 == miss64)[~graze].all()


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("shared", [False, True])
def test_closed_form_vjp_against_float64_autograd(shared):
    v0, f = closed_mesh(64)
    n, K = 35, 40  # (two tiles of frames for the shared sum)
    rng = np.random.default_rng(5)
    v = v0[None].astype(f64) * (1 + 0.1 * rng.standard_normal((n, 1, 1))) + 0.01 * rng.standard_normal((n, len(v0), 3))
    rf = 1 if shared else n
    o = np.stack([sphere_rays(K, 0.0, 6 + i, radius=3.0) for i in range(rf)]).astype(f64)
    d = 0.3 * rng.standard_normal((rf, K, 3)) - o
    d[:, 3] = 4 * o[:, 3]  # misses: no face, no gradient
    fwd = RC.ray_cast(v, f, o, d, dtype=f64)
    assert (fwd["face"][:, 3] == -1).all() and (fwd["face"] >= 0).mean() > 0.8
    g = rng.standard_normal((n, K))
    got = RC.ray_cast_vjp(v, f, o, d, fwd["face"], g, dtype=f64)
    tv, to, td = (torch.tensor(a, requires_grad=True) for a in (v, o, d))
    hit = torch.tensor(fwd["face"] >= 0)
    ids = torch.tensor(f[np.maximum(fwd["face"], 0)])  # [n,K,3]
    corners = tv[torch.arange(n)[:, None, None], ids]  # [n,K,3,3]
    a, b, c = corners[:, :, 0], corners[:, :, 1], corners[:, :, 2]
    nrm = torch.linalg.cross(b - a, c - a)
    t = (nrm * (a - to)).sum(-1) / (nrm * td).sum(-1)
    assert np.allclose(t.detach().numpy()[fwd["face"] >= 0], fwd["t"][fwd["face"] >= 0], rtol=1e-12)
    (torch.where(hit, t, torch.zeros_like(t)) * torch.tensor(g)).sum().backward()
    for name, ref in (("verts", tv.grad), ("origin", to.grad), ("dir", td.grad)):
        ref = ref.numpy()
        err = np.abs(got[name] - ref).max() / max(1.0, np.abs(ref).max())
        print("%s: %.3g" % (name, err))
        assert got[name].shape == ref.shape and err <= 1e-9, name


def test_tile_sum_order():
    x = np.random.default_rng(0).standard_normal((70, 5)).astype(f32)
    ref = (x[:32].cumsum(0, dtype=f32)[-1] + x[32:64].cumsum(0, dtype=f32)[-1]) + x[64:].cumsum(0, dtype=f32)[-1]
    assert RC.tile_sum(x).tobytes() == ref.tobytes()


# ------------------------------------------------------------------------------------------------ against the rasteriser
def test_camera_rays_against_the_depth_rasteriser():
    from smplpp_amd.smpl import camera_rays

    H = W = 64
    v, f = DR.two_spheres(3, (0.0, 0.0, 0.0), (0.35, 0.2, 0.9), radius=0.5)
    v = v.astype(f32)
    cam = DR.look_at_camera((0.1, 0.05, 0.3), 2.6, 0.4, H, W)
    ras = DR.raster(v, f, cam, H, W, near=0.05)
    o, d = camera_rays(cam, H, W)
    assert o.dtype == f32 and o.shape == (1, H * W, 3) and d.shape == (1, H * W, 3)
    o64, d64 = RC.camera_rays(cam, H, W)
    assert np.array_equal(o, o64.astype(f32)) and np.array_equal(d, d64.astype(f32))
    r = RC.ray_cast_frame(v, f, o[0], d[0], t_min=0.05)
    face, depth = r["face"].reshape(H, W), r["t"].reshape(H, W)
    inner = (ras["face"] >= 0) & (ras["bary"].min(2) > 0.02)
    agree = (face == ras["face"])[inner]
    rel = np.abs(depth.astype(f64) - ras["depth"])[inner][agree] / ras["depth"][inner][agree]
    print("pixels well inside a face: %d; the same face on %.2f %%; depth within %.3g relative there" % (inner.sum(), 100 * agree.mean(), rel.max()))
    assert inner.sum() > 500 and agree.mean() >= 0.99
    assert rel.max() <= 1e-5
    assert ((face >= 0) == (ras["face"] >= 0)).mean() >= 0.98  # the silhouettes agree but for the snap's fringe


# ------------------------------------------------------------------------------------------------ ABI
def _header_args(name):
    from smplpp_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_ray_cast_declared_exported_bound():
    from smplpp_amd import _lib

    L = _lib.load()
    for name in ("smplpp_ray_cast", "smplpp_ray_cast_vjp"):
        assert name in _lib.declared_symbols()
        fn = getattr(L, name)  # exported
        args = _header_args(name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(args) and fn.restype is C.c_int, (name, args)
        for a, t in zip(args, fn.argtypes):
            scalar = {"int64_t": C.c_int64, "int": C.c_int, "float": C.c_float}
            want = C.c_void_p if "*" in a else scalar[a.split()[0]]
            assert t is want, (name, a)
    assert _header_args("smplpp_ray_cast")[3:10] == ["int64_t ray_frames", "int64_t K", "const float * origin", "const float * dir", "float t_min",
                                                     "float t_max", "int facing"]
    assert _header_args("smplpp_ray_cast_vjp")[7:12] == ["const int64_t * face", "const float * grad_t", "float * grad_verts",
                                                         "float * grad_origin", "float * grad_dir"]
    # no model: refused before anything touches a device
    buf = np.zeros(64, f32)
    p = buf.ctypes.data
    assert L.smplpp_ray_cast(None, 1, p, 1, 1, p, p, 0.0, 1.0, 3, p, p, None, None, 0, None) == 1 and b"smplpp_ray_cast" in L.smplpp_last_error()
    assert L.smplpp_ray_cast_vjp(None, 1, p, 1, 1, p, p, p, p, p, None, None, 0, 0, None) == 1 and b"smplpp_ray_cast_vjp" in L.smplpp_last_error()
    assert (buf == 0).all()
