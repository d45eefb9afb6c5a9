"""The depth rasteriser's numpy oracle without a GPU: hand cases of the rule (top-left ownership, skipped faces, clipping to the
image, the depth tie, zero area); the oracle against an unsnapped float64 rasterisation of the synthetic body; vertex visibility
on two spheres; the backward formula against float64 autograd and finite differences; and the library's two entry points, exported
and refusing calls without a model."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_raster_oracle as DR  # noqa: E402
from distance_cases import _rel  # noqa: E402

# identity camera with u = x / z, v = y / z: at z = 1 a vertex sits at pixel coordinates (x, y)
UNIT = DR.pinhole(np.eye(3), np.zeros(3), 1.0, 1.0, 0.0, 0.0)


def _plane(xy, z=1.0):
    return np.array([[x * z, y * z, z] for x, y in xy], np.float32)


def test_top_left_rule_owns_every_pixel_once():
    # a square whose outer edges and diagonal pass through pixel centres: centres 0.5 .. 4.5 on both axes
    v = _plane([(0.5, 0.5), (4.5, 0.5), (4.5, 4.5), (0.5, 4.5)])
    for tris in ([[0, 1, 2], [0, 2, 3]], [[2, 1, 0], [0, 2, 3]], [[0, 1, 3], [1, 2, 3]], [[3, 1, 0], [3, 2, 1]]):
        one = [DR.raster(v, [t], UNIT, 6, 6)["face"] >= 0 for t in tris]
        both = DR.raster(v, tris, UNIT, 6, 6)
        assert not (one[0] & one[1]).any()
        want = np.zeros((6, 6), bool)
        want[0:4, 0:4] = True  # top and left edges in, bottom and right edges out
        assert np.array_equal(one[0] | one[1], want) and np.array_equal(both["face"] >= 0, want)
        assert np.array_equal(both["face"] == 0, one[0]) and np.array_equal(both["face"] == 1, one[1])
        assert both["culled"] == 0 and both["visible"].all()
        assert np.array_equal(both["depth"][want], np.ones(16, np.float32)) and (both["depth"][~want] == 0).all()
        assert np.allclose(both["bary"][want].sum(-1), 1, atol=1e-6) and (both["bary"][~want] == 0).all()


def test_skipped_faces_are_counted():
    good = _plane([(0.2, 0.3), (5.1, 0.4), (2.2, 5.3)])
    behind = _plane([(0.2, 0.3), (5.1, 0.4), (2.2, 5.3)], 0.01)
    straddle = good.copy()
    straddle[1] = (0.0, 0.0, 0.05)  # exactly at near: refused
    band = good.copy()
    band[2, 0] = 40000.0
    nan = good.copy()
    nan[0, 1] = np.nan
    inf = good.copy()
    inf[2, 2] = np.inf
    alone = DR.raster(good, [[0, 1, 2]], UNIT, 6, 6)
    assert (alone["face"] >= 0).sum() > 5
    for bad in (behind, straddle, band, nan, inf):
        r = DR.raster(bad, [[0, 1, 2]], UNIT, 6, 6)
        assert r["culled"] == 1 and (r["face"] == -1).all() and (r["depth"] == 0).all() and not r["visible"].any()
    v = np.concatenate([behind, straddle, good, band, nan, inf])
    r = DR.raster(v, np.arange(18).reshape(6, 3), UNIT, 6, 6)
    assert r["culled"] == 5
    assert np.array_equal(r["face"] >= 0, alone["face"] >= 0) and (r["face"][r["face"] >= 0] == 2).all()
    assert r["depth"].tobytes() == alone["depth"].tobytes() and r["bary"].tobytes() == alone["bary"].tobytes()
    assert r["visible"].tolist() == [0] * 6 + [1] * 3 + [0] * 9


def test_triangle_partly_outside_the_image():
    v = _plane([(-3.2, -2.1), (7.3, 1.2), (1.1, 9.7)], 2.0)
    r = DR.raster(v, [[0, 1, 2]], UNIT, 6, 6)
    q = DR.raster64(v, [[0, 1, 2]], UNIT, 6, 6)
    assert np.array_equal(r["face"], q["face"]) and r["culled"] == 0
    cov = r["face"] >= 0
    assert 10 < cov.sum() < 36 and cov[0, 0] and not cov[5, 5]
    assert np.abs(r["depth"][cov] - 2.0).max() < 1e-5
    # a larger image holds the same pixels and more
    big = DR.raster(v + np.float32([6, 6, 0]), [[0, 1, 2]], UNIT, 16, 16)["face"] >= 0
    assert np.array_equal(big[3:9, 3:9], cov) and big.sum() > cov.sum()


def test_equal_depth_goes_to_the_lowest_face_id():
    t = _plane([(0.2, 0.3), (5.1, 0.4), (2.2, 5.3)], 1.5)
    v = np.concatenate([t, t])  # two faces on the same three positions: equal depth bits on every pixel
    a = DR.raster(v, [[0, 1, 2], [3, 4, 5]], UNIT, 6, 6)
    b = DR.raster(v, [[3, 4, 5], [0, 1, 2]], UNIT, 6, 6)
    cov = a["face"] >= 0
    assert cov.sum() > 5 and np.array_equal(cov, b["face"] >= 0)
    assert (a["face"][cov] == 0).all() and (b["face"][cov] == 0).all()
    assert a["visible"].tolist() == [1, 1, 1, 0, 0, 0] and b["visible"].tolist() == [0, 0, 0, 1, 1, 1]
    assert a["depth"].tobytes() == b["depth"].tobytes()
    # a nearer face wins whatever its id
    near = np.concatenate([t, _plane([(0.2, 0.3), (5.1, 0.4), (2.2, 5.3)], 1.2)])
    r = DR.raster(near, [[0, 1, 2], [3, 4, 5]], UNIT, 6, 6)
    assert (r["face"][r["face"] >= 0] == 1).all() and r["visible"].tolist() == [0, 0, 0, 1, 1, 1]


def test_zero_area_covers_nothing():
    line = _plane([(0.5, 0.5), (2.5, 2.5), (4.5, 4.5)])  # through pixel centres
    tiny = _plane([(1.5, 1.5), (1.501, 1.5), (1.5, 1.501)])  # true area > 0, snapped area 0
    for v in (line, tiny):
        r = DR.raster(v, [[0, 1, 2]], UNIT, 6, 6)
        assert (r["face"] == -1).all() and r["culled"] == 0 and not r["visible"].any()
    # a face with a repeated vertex
    r = DR.raster(_plane([(0.5, 0.5), (4.5, 0.5), (4.5, 4.5)]), [[0, 1, 1]], UNIT, 6, 6)
    assert (r["face"] == -1).all()


# ---------------------------------------------------------------------------------------------------- against float64
def _posed(synth_model, n, seed):
    from oracle import cpu

    rng = np.random.default_rng(seed)
    theta = np.zeros((n, 25, 3), np.float32)
    theta[1:, 1:] = rng.normal(0, 0.3, (n - 1, 24, 3))  # frame 0: the rest pose
    return cpu.OracleModel(synth_model).fk(np.zeros((n, 10), np.float32), theta)["verts"]


@pytest.fixture(scope="module")
def posed(synth_model):
    return _posed(synth_model, 3, 17)


@pytest.fixture(scope="module")
def faces(synth_model):
    return synth_model["face_indices"].astype(np.int64) - 1


@pytest.mark.parametrize("H", [128, 256])
@pytest.mark.parametrize("yaw", [0.0, 0.7])
def test_oracle_against_unsnapped_float64(posed, faces, H, yaw):
    for k, v in enumerate(posed):
        cam = DR.look_at_camera((v.min(0) + v.max(0)) / 2, 2.5, yaw, H, H)
        r, q = DR.raster(v, faces, cam, H, H), DR.raster64(v, faces, cam, H, H)
        cov = r["face"] >= 0
        assert cov.sum() >= 0.1 * H * H, (k, cov.sum())
        differ = int((r["face"] != q["face"]).sum())
        print("frame %d H %d yaw %.1f: covered %d, face differs %d (%.3f %%)" % (k, H, yaw, cov.sum(), differ, 100.0 * differ / cov.sum()))
        assert differ <= 0.01 * cov.sum(), (k, differ, cov.sum())
        assert not (DR.holes(cov) & ~DR.holes(q["face"] >= 0)).any(), k
        same = (r["face"] == q["face"]) & cov
        fi = np.where(same, r["face"], -1)
        pix, d32, b32 = DR.ray_plane(torch.tensor(v, dtype=torch.float32), faces, cam, fi)
        assert np.array_equal(pix.numpy(), np.nonzero(same.ravel())[0])
        d64, b64 = q["depth"][same], q["bary"][same]
        for name, got, f32, want in (("depth", r["depth"][same], d32.numpy(), d64), ("bary", r["bary"][same], b32.numpy(), b64)):
            err, bar = _rel(got, want), max(4 * _rel(f32, want), 1e-5)
            print("  %s: rel %.3g, fp32 torch %.3g" % (name, err, _rel(f32, want)))
            assert err <= bar, (k, name, err, bar)
        assert r["culled"] == 0


def test_visibility_on_two_spheres():
    H = W = 160
    cam = DR.pinhole(np.eye(3), np.zeros(3), 150.0, 150.0, W / 2, H / 2)
    centres = {"behind": (0.0, 0.0, 5.0), "beside": (1.15, 0.1, 3.2)}
    for name, c1 in centres.items():
        v, f = DR.two_spheres(2, (0.0, 0.0, 3.0), c1)
        half = len(v) // 2
        r = DR.raster(v, f, cam, H, W)
        vis = r["visible"].astype(bool)
        want = np.zeros(len(v), bool)
        want[f[np.unique(r["face"][r["face"] >= 0])].ravel()] = True
        assert np.array_equal(vis, want)
        # facing: the outward normal of a sphere's vertex against the ray from the camera to it
        c = np.where(np.arange(len(v))[:, None] < half, np.float64([0, 0, 3.0]), np.float64(c1))
        cosang = ((v - c) * v).sum(1) / (np.linalg.norm(v - c, axis=1) * np.linalg.norm(v, axis=1))
        assert vis[:half][cosang[:half] < -0.3].all() and not vis[:half][cosang[:half] > 0.3].any()
        if name == "behind":
            assert not vis[half:].any()
        else:
            assert vis[half:][cosang[half:] < -0.3].all() and not vis[half:][cosang[half:] > 0.3].any()
            assert 0.2 < vis[half:].mean() < 0.6


def test_backward_formula_against_autograd_and_finite_differences(posed, faces):
    H = W = 64
    v = posed[1].astype(np.float64)
    cam = DR.look_at_camera((v.min(0) + v.max(0)) / 2, 2.5, 0.4, H, W)
    fi = DR.raster(v, faces, cam, H, W)["face"]
    rng = np.random.default_rng(2)
    g = rng.normal(size=(H, W))
    g[rng.random((H, W)) < 1 / 3] = 0.0
    an = DR.vjp(v, faces, cam, fi, g, np.float64)
    ag = DR.vjp_autograd(v, faces, cam, fi, g, torch.float64)
    assert np.abs(ag).max() > 0 and _rel(an, ag) < 1e-10, _rel(an, ag)
    live = np.nonzero((fi >= 0) & (g != 0))
    gt = torch.tensor(g).reshape(-1)

    def loss(vv):
        pix, depth, _ = DR.ray_plane(torch.tensor(vv), faces, cam, np.where(g != 0, fi, -1))
        return float((depth * gt[pix]).sum())

    for k in rng.choice(len(live[0]), 5, replace=False):
        for vtx in faces[fi[live[0][k], live[1][k]]]:
            for x in range(3):
                h = 1e-6
                vp, vm = v.copy(), v.copy()
                vp[vtx, x] += h
                vm[vtx, x] -= h
                fd = (loss(vp) - loss(vm)) / (2 * h)
                assert abs(fd - an[vtx, x]) <= 1e-5 * max(1.0, abs(an[vtx, x])), (vtx, x, fd, an[vtx, x])
    # the float32 evaluation of the formula is an fp32-accurate version of the same numbers
    assert _rel(DR.vjp(v, faces, cam, fi, g, np.float32), ag) < 1e-3


def test_library_entry_points_refuse_bad_calls_without_a_gpu():
    """The two entry points are exported with their ctypes signatures and refuse a call without a model before touching a device."""
    import __graft_entry__ as g

    g.build()
    from smplpp_amd import _lib, smpl
    from smplpp_amd.smpl import SMPL, _ptr

    L = _lib.load()
    for name in ("smplpp_depth_raster", "smplpp_depth_raster_vjp"):
        assert getattr(L, name).argtypes is not None, name
    for name in ("depthRaster", "depthRasterBackward", "depth_raster_differentiable"):
        assert callable(getattr(SMPL, name)), name
    cam = smpl.pinhole_camera(np.eye(3), [0, 0, 2.5], 140.0, 141.0, 64.0, 48.0, n=3)
    assert cam.shape == (3, 16) and cam.dtype == np.float32
    assert np.array_equal(cam[2], DR.pinhole(np.eye(3), [0, 0, 2.5], 140.0, 141.0, 64.0, 48.0))
    v = np.zeros((1, 3, 3), np.float32)
    face, depth = np.zeros((1, 4, 4), np.int64), np.zeros((1, 4, 4), np.float32)
    calls = ((L.smplpp_depth_raster, (None, 1, _ptr(v), _ptr(cam), 4, 4, 0.05, _ptr(face), _ptr(depth), None, None, None, _lib.HOST, None)),
             (L.smplpp_depth_raster_vjp, (None, 1, _ptr(v), _ptr(cam), 4, 4, _ptr(face), _ptr(depth), _ptr(v), 0, _lib.HOST, None)))
    for fn, args in calls:
        with pytest.raises(_lib.SmplppError):
            _lib.check(fn(*args))
