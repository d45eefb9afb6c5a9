"""The raster attribute interpolation's oracle without a GPU: the closed-form backward of the header against float64 autograd of the
forward's definition (hand cases, two spheres, C = 1 and 3, both gradients); the float32 forward against the float64 one; and the
refusals of the Python wrappers and of the library's entry points that need no device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_raster_oracle as DR  # noqa: E402
import raster_interpolate_oracle as RI  # noqa: E402
from distance_cases import _rel  # noqa: E402

UNIT = DR.pinhole(np.eye(3), np.zeros(3), 1.0, 1.0, 0.0, 0.0)


def _plane(xy, z=1.0):
    return np.array([[x * z, y * z, z] for x, y in xy], np.float32)


def _hand_cases():
    """(verts, faces, cam, H, W): the 6 x 6 scenes of the rasteriser's hand cases, tilted out of the image plane so that the
    barycentrics depend on every coordinate."""
    sq = _plane([(0.5, 0.5), (4.5, 0.5), (4.5, 4.5), (0.5, 4.5)])
    sq[:, 2] += np.float32([0.0, 0.2, 0.5, 0.1])
    sq[:, :2] *= sq[:, 2:3]
    for tris in ([[0, 1, 2], [0, 2, 3]], [[2, 1, 0], [0, 2, 3]], [[0, 1, 3], [1, 2, 3]], [[3, 1, 0], [3, 2, 1]]):
        yield sq, np.array(tris), UNIT, 6, 6
    t = _plane([(0.2, 0.3), (5.1, 0.4), (2.2, 5.3)], 1.5)
    v = np.concatenate([t, t, _plane([(0.6, 0.7), (3.1, 0.9), (1.2, 3.3)], 1.2), _plane([(-3.2, -2.1), (7.3, 1.2), (1.1, 9.7)], 2.0)])
    v[:, 2] += np.linspace(0, 0.3, len(v)).astype(np.float32)
    yield v, np.arange(12).reshape(4, 3), UNIT, 6, 6


def _spheres():
    H = W = 160
    cam = DR.pinhole(np.eye(3), np.zeros(3), 150.0, 150.0, W / 2, H / 2)
    v, f = DR.two_spheres(2, (0.0, 0.0, 3.0), (1.15, 0.1, 3.2))
    return v.astype(np.float32), f, cam, H, W


def _cotangent(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.normal(size=shape)
    g[rng.random(shape[:-1]) < 1 / 3] = 0.0
    return g


@pytest.mark.parametrize("C", [1, 3])
def test_closed_form_backward_equals_float64_autograd(C):
    for k, (v, f, cam, H, W) in enumerate(list(_hand_cases()) + [_spheres()]):
        r = DR.raster(v, f, cam, H, W)
        assert (r["face"] >= 0).sum() > 5
        rng = np.random.default_rng(10 + k)
        attr = rng.normal(size=(len(v), C))
        g = _cotangent((H, W, C), 20 + k)
        ga, gv = RI.vjp(attr, v, f, cam, r["face"], g, np.float64)
        ra, rv = RI.vjp_autograd(attr, v, f, cam, r["face"], g, torch.float64)
        assert np.abs(ra).max() > 0 and np.abs(rv).max() > 0
        print("case %d C %d: grad_attr rel %.3g, grad_verts rel %.3g" % (k, C, _rel(ga, ra), _rel(gv, rv)))
        assert _rel(ga, ra) <= 1e-9 and _rel(gv, rv) <= 1e-9, (k, _rel(ga, ra), _rel(gv, rv))


def test_float32_forward_within_rounding_of_float64():
    """Three products and two sums per element: |error| <= 3 eps32 sum_i |beta_i A_i| (eps32 = 2^-24, the rounding of beta and A to
    float32 included), and background is +0."""
    for k, (v, f, cam, H, W) in enumerate(list(_hand_cases()) + [_spheres()]):
        r = DR.raster(v, f, cam, H, W)
        attr = np.random.default_rng(k).normal(size=(len(v), 4)).astype(np.float32)
        attr[~r["visible"].astype(bool)] = np.nan  # vertices no visible face uses
        got = RI.interpolate(attr, f, r["face"], r["bary"])
        want = RI.interpolate(attr, f, r["face"], r["bary"], np.float64)
        cov = r["face"] >= 0
        tri = f[r["face"][cov]]
        mag = (np.abs(r["bary"][cov].astype(np.float64))[:, :, None] * np.abs(attr[tri].astype(np.float64))).sum(1)
        assert got.dtype == np.float32 and np.isfinite(got).all()
        assert (np.abs(got[cov] - want[cov]) <= 3 * 2.0 ** -24 * mag).all()
        assert (got[~cov].view(np.uint32) == 0).all()


def test_wrappers_and_entry_points_refuse_bad_calls_without_a_gpu():
    import __graft_entry__ as g

    g.build()
    from smplpp_amd import _lib
    from smplpp_amd.smpl import SMPL, _ptr

    L = _lib.load()
    for name in ("smplpp_raster_interpolate", "smplpp_raster_interpolate_vjp"):
        assert getattr(L, name).argtypes is not None, name
    for name in ("rasterInterpolate", "rasterInterpolateBackward", "raster_interpolate_differentiable", "normal_map_differentiable"):
        assert callable(getattr(SMPL, name)), name
    s = SMPL()
    s.vertex_num, s.face_num = 5, 2  # the shape checks come before the handle is asked for
    n, H, W, C = 2, 4, 3, 3
    attr, verts = np.zeros((n, 5, C), np.float32), np.zeros((n, 5, 3), np.float32)
    face, bary, gi = np.zeros((n, H, W), np.int64), np.zeros((n, H, W, 3), np.float32), np.zeros((n, H, W, C), np.float32)
    cam = np.tile(UNIT, (n, 1))
    fwd_bad = (dict(attr=attr[:, :4]), dict(attr=attr[0]), dict(attr=np.zeros((n, 5, 33), np.float32)), dict(attr=np.zeros((n, 5, 0), np.float32)),
               dict(bary=bary[:1]), dict(bary=bary[..., :2]), dict(bary=bary[:, :, 0]), dict(face=face[:, :2]),
               dict(attr=torch.zeros(n, 5, C)))
    for kw in fwd_bad:
        a = dict(attr=attr, face=face, bary=bary)
        a.update(kw)
        with pytest.raises(_lib.SmplppError) as e:
            s.rasterInterpolate(**a)
        assert e.value.code == 1, kw
    bwd_bad = (dict(attr=attr[:, :4]), dict(verts=verts[:, :4]), dict(H=5), dict(W=0), dict(grad_image=gi[..., :2]), dict(grad_image=gi[:1]),
               dict(camera=cam[:, :15]), dict(face=face[:1]), dict(want=()), dict(want=("attr", "camera")),
               dict(out={"attr": np.zeros((n, 5, C), np.float32)}), dict(want=("verts",), out={"verts": np.zeros((n, 5, 3), np.float64)}),
               dict(want=("verts",), out={"attr": np.zeros((n, 5, C), np.float32)}))
    for kw in bwd_bad:
        a = dict(attr=attr, verts=verts, camera=cam, H=H, W=W, face=face, bary=bary, grad_image=gi)
        a.update(kw)
        with pytest.raises(_lib.SmplppError) as e:
            s.rasterInterpolateBackward(**a)
        assert e.value.code == 1, kw
    # well-formed calls pass every check and stop at the missing model
    for call in (lambda: s.rasterInterpolate(attr, face, bary), lambda: s.rasterInterpolateBackward(attr, verts, cam, H, W, face, bary, gi),
                 lambda: s.rasterInterpolateBackward(attr, verts, UNIT, H, W, face, bary, gi, want=("verts",), out={"verts": verts.copy()})):
        with pytest.raises(_lib.SmplppError) as e:
            call()
        assert e.value.code == 4
    # the entry points refuse a call without a model before touching a device
    img = np.zeros((n, H, W, C), np.float32)
    calls = ((L.smplpp_raster_interpolate, (None, n, _ptr(attr), C, H, W, _ptr(face), _ptr(bary), _ptr(img), _lib.HOST, None)),
             (L.smplpp_raster_interpolate_vjp, (None, n, _ptr(attr), C, _ptr(verts), _ptr(cam), H, W, 0.05, _ptr(face), _ptr(bary), _ptr(gi),
                                                _ptr(attr), _ptr(verts), 0, _lib.HOST, None)))
    for fn, args in calls:
        with pytest.raises(_lib.SmplppError):
            _lib.check(fn(*args))
