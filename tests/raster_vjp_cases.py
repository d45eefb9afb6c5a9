"""The cases whose backward bits tests/golden/raster_vjp_bits.json pins (depthRasterBackward, rasterInterpolateBackward,
silhouetteBackward), built from fixed seeds: the smallest shapes at which the face walk, its lane tree, the channel chunks and the
vertex gather can each go wrong.

  hand     two 6 x 6 frames, six faces on their own vertices: every face of frame 0 refused; in frame 1 a depth tie, zero areas and a
           face far larger than the image (a box clipped on all four sides).  n F = 12: a last workgroup that is almost empty.
  spheres  two frames of two spheres at 160 x 160: boxes tens of pixels wide (every lane takes several strides), and in frame 1 the
           nearer sphere occludes, so a box holds pixels that name other faces.
  body     three posed frames of the synthetic body at 96 x 128: boxes smaller than the 8 lanes of a face (idle lanes enter the
           tree), the valences of the V = 6890 mesh through the gather, and n F no multiple of 32.

inputs() gives every array a case feeds the backward passes (the rasteriser's face and bary among them), outputs() every gradient;
digest() is the SHA-256 of an array's little-endian bytes.  tools/record_raster_vjp_bits.py wrote the golden file from these,
tests/test_raster_vjp_bits_gpu.py recomputes and compares."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_raster_oracle as DR  # noqa: E402
from test_depth_raster_gpu import UNIT, _cams, _model_for, _plane, _synth  # noqa: E402

NAMES = ("hand", "spheres", "body")
CHANNELS = (1, 3, 4, 5, 32)  # 5: a chunk of 4 and a chunk of 1; 32: eight walks
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raster_vjp_bits.json")


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()).hexdigest()


def scene(name, synth_model=None):
    """(handle, verts [n,V,3], cameras [n,16], H, W) of the case."""
    if name == "hand":
        good = _plane([(0.2, 0.3), (5.1, 0.4), (2.2, 5.3)])
        behind = _plane([(0.2, 0.3), (5.1, 0.4), (2.2, 5.3)], 0.01)
        straddle, band, nan, inf = good.copy(), good.copy(), good.copy(), good.copy()
        straddle[1] = (0.0, 0.0, 0.05)
        band[2, 0] = 40000.0
        nan[0, 1] = np.nan
        inf[2, 2] = np.inf
        t = _plane([(0.2, 0.3), (5.1, 0.4), (2.2, 5.3)], 1.5)
        f1 = np.concatenate([t, t, _plane([(0.6, 0.7), (3.1, 0.9), (1.2, 3.3)], 1.2), _plane([(0.5, 0.5), (2.5, 2.5), (4.5, 4.5)]),
                             _plane([(1.5, 1.5), (1.501, 1.5), (1.5, 1.501)]), _plane([(-3.2, -2.1), (7.3, 1.2), (1.1, 9.7)], 2.0)])
        f0 = np.concatenate([behind, straddle, behind, band, nan, inf])
        return _model_for(18, np.arange(18).reshape(6, 3)), np.stack([f0, f1]).astype(np.float32), np.stack([UNIT, UNIT]), 6, 6
    if name == "spheres":
        H = W = 160
        cam = DR.pinhole(np.eye(3), np.zeros(3), 150.0, 150.0, W / 2, H / 2)
        va, f = DR.two_spheres(2, (0.0, 0.0, 3.0), (0.0, 0.0, 5.0))
        vb, _ = DR.two_spheres(2, (0.0, 0.0, 3.0), (1.15, 0.1, 3.2))
        return _model_for(len(va), f), np.stack([va, vb]).astype(np.float32), np.stack([cam, cam]), H, W
    assert name == "body"
    H, W = 96, 128
    s = _synth(synth_model)
    theta = np.zeros((3, 25, 3), np.float32)
    theta[1:, 1:] = np.random.default_rng(17).normal(0, 0.3, (2, 24, 3))
    v = s.launch(np.zeros((3, 10), np.float32), theta, want=("verts",))["verts"]
    return s, v, _cams(v, H, W, ((2.5, 0.1), (2.0, 0.4), (2.7, -0.3))), H, W


def _cotangent(rng, shape):
    """Normal, with one pixel in three (every channel of it) exactly zero."""
    g = rng.normal(size=shape).astype(np.float32)
    g[rng.random(shape[:3]) < 1.0 / 3.0] = 0.0
    return g


def inputs(name, s, v, cams, H, W):
    """Every array the case's backward calls read, by name."""
    n, V = v.shape[:2]
    seed = 1000 * (1 + NAMES.index(name))
    cams = np.ascontiguousarray(cams, np.float32)
    r = s.depthRaster(v, cams, H, W)
    x = {"verts": v, "camera": cams, "face": r["face"], "bary": r["bary"],
         "grad_depth": _cotangent(np.random.default_rng(seed), (n, H, W)),
         "base_verts": np.random.default_rng(seed + 1).normal(size=(n, V, 3)).astype(np.float32)}
    for C in CHANNELS:
        rng = np.random.default_rng(seed + 10 * C)
        x["attr_%d" % C] = rng.normal(size=(n, V, C)).astype(np.float32)
        x["grad_image_%d" % C] = _cotangent(rng, (n, H, W, C))
        x["base_attr_%d" % C] = rng.normal(size=(n, V, C)).astype(np.float32)
    if name == "body":  # the silhouette against the coverage moved eight pixels to the right
        mask = np.zeros((n, H, W), np.uint8)
        mask[:, :, 8:] = r["face"][:, :, :-8] >= 0
        sil = s.silhouette(v, cams, H, W, mask, face=r["face"], want=("vert_target", "pix_source"))
        rng = np.random.default_rng(seed + 2)
        x.update(mask=mask, vert_target=sil["vert_target"], pix_source=sil["pix_source"],
                 grad_vert_sq=rng.normal(size=(n, V)).astype(np.float32), grad_pix_sq=_cotangent(rng, (n, H, W)))
    return x


def outputs(s, x, H, W, to=np.copy, back=np.asarray):
    """Every gradient of the case, by name.  `to` carries an input to the space of the call (a fresh copy each time, so an `out`
    array is never the fixture), `back` an output to numpy."""
    v, cam, face, bary = to(x["verts"]), to(x["camera"]), to(x["face"]), to(x["bary"])
    y = {"depth": back(s.depthRasterBackward(v, cam, H, W, face, to(x["grad_depth"]))),
         "depth_out": back(s.depthRasterBackward(v, cam, H, W, face, to(x["grad_depth"]), out=to(x["base_verts"])))}
    for C in CHANNELS:
        attr, g = to(x["attr_%d" % C]), to(x["grad_image_%d" % C])
        for tag, kw in (("both", {}), ("only", {"want": ("attr",)}), ("only", {"want": ("verts",)}),
                        ("out", {"out": {"attr": to(x["base_attr_%d" % C]), "verts": to(x["base_verts"])}})):
            for k, a in s.rasterInterpolateBackward(attr, v, cam, H, W, face, bary, g, **kw).items():
                y["interp_%d_%s_%s" % (C, tag, k)] = back(a)
    if "mask" in x:
        y["silhouette"] = back(s.silhouetteBackward(v, cam, H, W, face, to(x["vert_target"]), to(x["pix_source"]), to(x["grad_vert_sq"]),
                                                    to(x["grad_pix_sq"])))
    return y
