"""The silhouette term's numpy oracle without a GPU: the feature transform (brute force with the key rule) and its separable two-pass
form against an independent brute force on odd sizes, empty, full and single-pixel masks and masks built to tie; scipy's Euclidean
distance transform where it is installed; the per-vertex pixel choice of the float32 rule against float64; the restated loss against
the residuals and its analytic gradient against finite differences; and the library's three entry points, exported and refusing calls
without a model."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_raster_oracle as DR  # noqa: E402
import silhouette_oracle as SO  # noqa: E402


def _masks():
    """name -> mask [H,W] uint8."""
    rng = np.random.default_rng(11)
    out = {}
    for H, W in ((1, 1), (1, 9), (9, 1), (7, 13), (64, 64)):
        for density in (0.02, 0.1, 0.5):
            out["random %dx%d %.2f" % (H, W, density)] = (rng.random((H, W)) < density).astype(np.uint8)
    out["empty"] = np.zeros((7, 13), np.uint8)
    out["full"] = np.ones((7, 13), np.uint8)
    out["one pixel at 1x1"] = np.ones((1, 1), np.uint8)
    single = np.zeros((9, 11), np.uint8)
    single[6, 2] = 200  # any nonzero byte is set
    out["single"] = single
    for name, pts in (("tie in a row", ((4, 2), (4, 8))), ("tie in a column", ((1, 5), (7, 5))), ("tie on a diagonal", ((1, 2), (7, 8))),
                      ("tie on the other diagonal", ((1, 8), (7, 2))), ("four-way tie", ((4, 2), (4, 8), (1, 5), (7, 5)))):
        m = np.zeros((9, 11), np.uint8)
        for p in pts:
            m[p] = 1
        out[name] = m
    return out


MASKS = _masks()


def test_feature_transform_against_independent_brute_force():
    for name, m in MASKS.items():
        n0, d0 = SO.feature_transform_loops(m)
        n1, d1 = SO.feature_transform(m)
        assert n1.dtype == np.int64 and d1.dtype == np.int32
        assert np.array_equal(d0, d1) and np.array_equal(n0, n1), name
    # the cases by hand: nothing set, everything set, and the lowest linear index on a tie
    n, d = SO.feature_transform(MASKS["empty"])
    assert (n == -1).all() and (d == 0).all()
    n, d = SO.feature_transform(MASKS["full"])
    assert np.array_equal(n.ravel(), np.arange(7 * 13)) and (d == 0).all()
    n, d = SO.feature_transform(MASKS["single"])
    assert (n == 6 * 11 + 2).all() and d[0, 0] == 36 + 4 and d[6, 2] == 0
    W = 11
    n, d = SO.feature_transform(MASKS["tie in a row"])
    assert n[4, 5] == 4 * W + 2 and d[4, 5] == 9 and n[0, 5] == 4 * W + 2 and n[4, 6] == 4 * W + 8
    n, d = SO.feature_transform(MASKS["tie in a column"])
    assert n[4, 5] == 1 * W + 5 and d[4, 5] == 9 and n[4, 0] == 1 * W + 5 and n[5, 5] == 7 * W + 5
    n, d = SO.feature_transform(MASKS["tie on a diagonal"])
    assert n[4, 5] == 1 * W + 2 and d[4, 5] == 18
    n, d = SO.feature_transform(MASKS["tie on the other diagonal"])
    assert n[4, 5] == 1 * W + 8 and d[4, 5] == 18
    n, d = SO.feature_transform(MASKS["four-way tie"])
    assert n[4, 5] == 1 * W + 5 and d[4, 5] == 9


def test_scipy_distance_transform_agrees():
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, m in MASKS.items():
        if not m.any():
            continue
        _, d = SO.feature_transform(m)
        edt = ndimage.distance_transform_edt(m == 0)
        assert np.array_equal(np.rint(edt ** 2).astype(np.int64), d.astype(np.int64)), name


def test_separable_form_equals_brute_force():
    for name, m in MASKS.items():
        n0, d0 = SO.feature_transform(m)
        n1, d1 = SO.feature_transform_separable(m)
        assert np.array_equal(d0, d1) and np.array_equal(n0, n1), name
    # the column pass names the upper pixel on a tie
    col = SO.column_pass(MASKS["tie in a column"])
    assert col[4, 5] == 1 and col[5, 5] == 7 and (col[:, 0] == -1).all()


# ---------------------------------------------------------------------------------------------------- against float64
def _posed(synth_model, n, seed):
    from oracle import cpu

    rng = np.random.default_rng(seed)
    theta = np.zeros((n, 25, 3), np.float32)
    theta[:, 1:] = rng.normal(0, 0.3, (n, 24, 3))
    return cpu.OracleModel(synth_model).fk(np.zeros((n, 10), np.float32), theta)["verts"]


@pytest.fixture(scope="module")
def faces(synth_model):
    return synth_model["face_indices"].astype(np.int64) - 1


@pytest.mark.parametrize("seed", [17, 23])
@pytest.mark.parametrize("H", [128, 256])
def test_vertex_pixel_choice_against_float64(synth_model, seed, H):
    """The float32 rule and a float64 projection choose the same pixel for every vertex whose float64 u and v lie more than 1e-4 px
    from an integer; at most 0.5 % of the vertices may be left out."""
    for v in _posed(synth_model, 3, seed):
        cam = DR.look_at_camera((v.min(0) + v.max(0)) / 2, 2.5, 0.3, H, H)
        u32, v32, ok = SO.project(v, cam, 0.05)
        u64, v64, _ = SO.project(v, cam, 0.05, np.float64)
        assert ok.all()
        near_int = (np.abs(u64 - np.rint(u64)) <= 1e-4) | (np.abs(v64 - np.rint(v64)) <= 1e-4)
        print("H %d seed %d: %d of %d vertices within 1e-4 px of an integer (%.3f %%)" % (H, seed, near_int.sum(), len(v), 100.0 * near_int.mean()))
        assert near_int.mean() <= 0.005
        i32, j32 = SO.vertex_pixels(u32, v32, H, H)
        i64, j64 = SO.vertex_pixels(u64, v64, H, H)
        assert np.array_equal(i32[~near_int], i64[~near_int]) and np.array_equal(j32[~near_int], j64[~near_int])


def _scene(synth_model, faces, H, W):
    """The body, and a mask rendered from a displaced pose."""
    v = _posed(synth_model, 2, 5)
    body, other = v[0], v[1] + np.float32([0.07, 0.02, 0.0])
    cam = DR.look_at_camera((body.min(0) + body.max(0)) / 2, 2.5, 0.2, H, W)
    face = DR.raster(body, faces, cam, H, W)["face"]
    mask = (DR.raster(other, faces, cam, H, W)["face"] >= 0).astype(np.uint8)
    return body, cam, face, mask


def test_residuals_and_loss_agree(synth_model, faces):
    H, W = 96, 128
    body, cam, face, mask = _scene(synth_model, faces, H, W)
    r = SO.silhouette(body, cam, H, W, face, mask)
    outside = r["vert_target"] >= 0
    uncovered = r["pix_source"] >= 0
    assert 0.02 < outside.mean() < 0.9 and uncovered.sum() > 20
    assert np.array_equal(uncovered, (mask != 0) & (face < 0)) and (r["pix_sq"][uncovered] >= 1).all() and (r["pix_sq"][~uncovered] == 0).all()
    assert (mask.ravel()[r["vert_target"][outside]] != 0).all() and (face.ravel()[r["pix_source"][uncovered]] >= 0).all()
    # the restated loss with cotangents of 1 is the sum of the residuals (the pixel half up to the rounding of beta)
    v = torch.tensor(body.astype(np.float64))
    lv = float(SO.loss(v, faces, cam, H, W, face, r["vert_target"], None, np.ones(len(body)), None))
    lp = float(SO.loss(v, faces, cam, H, W, face, None, r["pix_source"], None, np.ones((H, W))))
    assert abs(lv - r["vert_sq"].astype(np.float64).sum()) <= 1e-4 * lv
    assert abs(lp - r["pix_sq"].astype(np.float64).sum()) <= 1e-4 * lp
    # frames that give nothing: an empty mask, no coverage
    e = SO.silhouette(body, cam, H, W, face, np.zeros_like(mask))
    assert (e["vert_target"] == -1).all() and (e["vert_sq"] == 0).all() and (e["pix_source"] == -1).all()
    e = SO.silhouette(body, cam, H, W, np.full_like(face, -1), mask)
    assert (e["pix_source"] == -1).all() and (e["pix_sq"] == 0).all() and (e["vert_target"] >= 0).any()


def test_loss_gradient_against_finite_differences(synth_model, faces):
    H, W = 96, 128
    body, cam, face, mask = _scene(synth_model, faces, H, W)
    r = SO.silhouette(body, cam, H, W, face, mask)
    rng = np.random.default_rng(3)
    gv, gp = rng.normal(size=len(body)), rng.normal(size=(H, W))
    gv[rng.random(len(body)) < 1 / 3] = 0.0
    gp[rng.random((H, W)) < 1 / 3] = 0.0
    args = (faces, cam, H, W, face, r["vert_target"], r["pix_source"], gv, gp)
    an = SO.vjp_autograd(body, *args)
    assert np.abs(an).max() > 0

    x0 = body.astype(np.float64)

    def value(x):  # beta stays where the gradient was taken
        return float(SO.loss(torch.tensor(x), *args, at=x0))

    for _ in range(4):
        d = rng.normal(size=x0.shape)
        h = 1e-6
        fd = (value(x0 + h * d) - value(x0 - h * d)) / (2 * h)
        assert abs(fd - (an * d).sum()) <= 1e-5 * max(1.0, abs(fd)), (fd, (an * d).sum())


def test_library_entry_points_refuse_bad_calls_without_a_gpu():
    """The three entry points are exported with their ctypes signatures and refuse a call without a model before touching a device."""
    import __graft_entry__ as g

    g.build()
    from smplpp_amd import _lib
    from smplpp_amd.smpl import SMPL, _ptr

    L = _lib.load()
    for name in ("smplpp_mask_distance_transform", "smplpp_silhouette", "smplpp_silhouette_vjp"):
        assert getattr(L, name).argtypes is not None, name
    for name in ("maskDistanceTransform", "silhouette", "silhouetteBackward", "silhouette_differentiable"):
        assert callable(getattr(SMPL, name)), name
    cam = DR.pinhole(np.eye(3), [0, 0, 2.5], 140.0, 141.0, 2.0, 2.0)[None]
    v = np.zeros((1, 3, 3), np.float32)
    face, mask = np.zeros((1, 4, 4), np.int64), np.ones((1, 4, 4), np.uint8)
    near_, sq = np.zeros((1, 4, 4), np.int64), np.zeros((1, 4, 4), np.int32)
    vt, vs = np.zeros((1, 3), np.int64), np.zeros((1, 3), np.float32)
    calls = ((L.smplpp_mask_distance_transform, (None, 1, _ptr(mask), 4, 4, _ptr(near_), _ptr(sq), _lib.HOST, None)),
             (L.smplpp_silhouette, (None, 1, _ptr(v), _ptr(cam), 4, 4, 0.05, _ptr(face), _ptr(mask), _ptr(vt), _ptr(vs), None, None, _lib.HOST,
                                    None)),
             (L.smplpp_silhouette_vjp, (None, 1, _ptr(v), _ptr(cam), 4, 4, 0.05, _ptr(face), _ptr(vt), None, _ptr(vs), None, _ptr(v), 0,
                                        _lib.HOST, None)))
    for fn, args in calls:
        with pytest.raises(_lib.SmplppError):
            _lib.check(fn(*args))
