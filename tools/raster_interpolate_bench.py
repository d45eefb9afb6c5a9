"""Timing of the raster attribute interpolation and its backward pass (smplpp_raster_interpolate, smplpp_raster_interpolate_vjp) on
one MI355X, synthetic 6890-vertex model (13776 faces), C = 3.

At each (n, H, W) of SIZES (the depth rasteriser's), on frames posed and viewed as tools/depth_raster_bench.py poses and views them,
with attr = the posed vertices and face, bary from one smplpp_depth_raster call, microseconds per call of
  - the forward,
  - the backward with both outputs, with grad_attr alone and with grad_verts alone (accumulate 0, normal cotangents),
next to
  - the forward's byte floor: n H W (8 face + 12 bary + 4 C image) + n V 4 C (the attribute table once) bytes at 8 TB/s, and the
    ratio time / floor,
  - smplpp_depth_raster_vjp on the same frames, faces and GPU (cotangents of 1): the same walk over the faces' boxes with three
    sums per lane in place of nine (grad_verts) or 3 C (grad_attr); this change does not touch that kernel,
  - the same rule written in torch on the same GPU, what a user would have written: the forward as a gather of the three corner
    rows and a weighted sum; the backward as autograd of that gather (index_add_ into attr) for grad_attr, and autograd through the
    rasteriser's barycentric formula for grad_verts (the time includes that graph's forward).  Reported with its relative
    difference from the library's results,
  - covered pixels per frame (mean): the workload.
Device pointers, torch's current stream; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls
between HIP events, after `--warmup` untimed calls.  Prints one JSON line and writes it to --out.

    python tools/raster_interpolate_bench.py [--steps 20] [--warmup 3] [--reps 3] [--no-torch] [--out profiles/raster_interpolate_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from depth_raster_bench import PEAK, SIZES, _time, cameras  # noqa: E402

C = 3


def torch_interpolate(attr, verts, faces, cam, face, bary=None):
    """One frame in torch: attr [V,C], verts [V,3], faces [F,3], cam [16], face [H,W] -> image [H,W,C].  With `bary` [H,W,3] the
    weights are data; without, they are the rasteriser's formula on verts (differentiable)."""
    import torch

    H, W = face.shape
    pix = torch.nonzero(face.reshape(-1) >= 0)[:, 0]
    tri = faces[face.reshape(-1)[pix]]
    if bary is None:
        xc = verts @ cam[:9].reshape(3, 3).T + cam[9:12]
        a, b, c = xc[tri[:, 0]], xc[tri[:, 1]], xc[tri[:, 2]]
        i, j = (pix % W).float(), torch.div(pix, W, rounding_mode="floor").float()
        d = torch.stack([(i + 0.5 - cam[14]) / cam[12], (j + 0.5 - cam[15]) / cam[13], torch.ones_like(i)], 1)
        e1, e2 = b - a, c - a
        n = torch.linalg.cross(e1, e2)
        w = ((n * a).sum(1) / (n * d).sum(1))[:, None] * d - a
        nn = (n * n).sum(1)
        bb = (torch.linalg.cross(w, e2) * n).sum(1) / nn
        bc = (torch.linalg.cross(e1, w) * n).sum(1) / nn
        beta = torch.stack([1 - bb - bc, bb, bc], 1)
    else:
        beta = bary.reshape(-1, 3)[pix]
    out = torch.zeros(H * W, attr.shape[1], device=attr.device)
    out[pix] = (beta[:, :, None] * attr[tri]).sum(1)
    return out.reshape(H, W, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_interpolate_bench.json"))
    a = ap.parse_args()
    import torch

    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    model = model_io.synthetic_model()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    faces = torch.from_numpy(model["face_indices"].astype(np.int64) - 1).cuda()
    rng = np.random.default_rng(0)
    res = {"model": "synthetic", "faces": int(s.face_num), "vertices": int(s.vertex_num), "near": 0.05, "C": C, "bytes_per_second": PEAK,
           "sizes": []}
    rel = lambda x, y: float((x - y).norm() / y.norm().clamp(min=1e-30))  # noqa: E731
    for n, H, W in SIZES:
        theta = np.zeros((n, 25, 3), np.float32)
        theta[:, 1:] = rng.normal(0, 0.3, (n, 24, 3))
        v, _ = s.forward_differentiable(torch.zeros(n, 10, device="cuda"), torch.from_numpy(theta).cuda())
        v = v.detach().contiguous()
        cam = torch.from_numpy(cameras(v.cpu().numpy(), H, W)).cuda()
        r = s.depthRaster(v, cam, H, W, want=("bary",))
        face, bary, attr = r["face"], r["bary"], v
        g = torch.from_numpy(rng.normal(size=(n, H, W, C)).astype(np.float32)).cuda()
        g1 = torch.ones(n, H, W, device="cuda")
        gv = torch.empty_like(v)
        back = lambda want: s.rasterInterpolateBackward(attr, v, cam, H, W, face, bary, g, want=want)  # noqa: E731
        floor = (n * H * W * (8 + 12 + 4 * C) + n * s.vertex_num * 4 * C) / PEAK * 1e6
        row = {"n": n, "H": H, "W": W, "covered_px": round(float((face >= 0).sum(dim=(1, 2)).float().mean()), 1),
               "forward_us": _time(lambda: s.rasterInterpolate(attr, face, bary), a.steps, a.warmup, a.reps),
               "forward_floor_us": round(floor, 2),
               "backward_us": _time(lambda: back(("attr", "verts")), a.steps, a.warmup, a.reps),
               "backward_attr_only_us": _time(lambda: back(("attr",)), a.steps, a.warmup, a.reps),
               "backward_verts_only_us": _time(lambda: back(("verts",)), a.steps, a.warmup, a.reps),
               "depth_raster_vjp_us": _time(lambda: s.depthRasterBackward(v, cam, H, W, face, g1, out=gv.zero_()), a.steps, a.warmup, a.reps)}
        row["forward_over_floor"] = round(row["forward_us"] / floor, 1)
        for k in ("backward", "backward_attr_only", "backward_verts_only"):
            row[k + "_over_depth_raster_vjp"] = round(row[k + "_us"] / row["depth_raster_vjp_us"], 2)
        if not a.no_torch:
            lib_image, lib_grad = s.rasterInterpolate(attr, face, bary), back(("attr", "verts"))

            def fwd_torch():
                return torch.stack([torch_interpolate(attr[i], v[i], faces, cam[i], face[i], bary[i]) for i in range(n)])

            def bwd_torch():
                ta, tv = attr.clone().requires_grad_(True), v.clone().requires_grad_(True)
                loss = 0
                for i in range(n):
                    loss = loss + (torch_interpolate(ta[i], tv[i], faces, cam[i], face[i]) * g[i]).sum()
                return torch.autograd.grad(loss, (ta, tv))

            ta, tv = bwd_torch()
            row["torch_forward_rel_diff"] = rel(fwd_torch(), lib_image)
            row["torch_grad_attr_rel_diff"], row["torch_grad_verts_rel_diff"] = rel(ta, lib_grad["attr"]), rel(tv, lib_grad["verts"])
            row["torch_forward_us"] = _time(fwd_torch, max(1, a.steps // 10), 1, a.reps)
            row["torch_backward_us"] = _time(bwd_torch, max(1, a.steps // 10), 1, a.reps)
            row["torch_forward_over_forward"] = round(row["torch_forward_us"] / row["forward_us"], 1)
            row["torch_backward_over_backward"] = round(row["torch_backward_us"] / row["backward_us"], 1)
        res["sizes"].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
