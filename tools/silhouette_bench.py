"""Timing of the silhouette term (smplpp_mask_distance_transform, smplpp_silhouette, smplpp_silhouette_vjp) on one MI355X, synthetic
6890-vertex model (13776 faces).

At each (n, H, W) of SIZES (the depth rasteriser's), on frames posed as tools/depth_raster_bench.py poses them, with the target mask
the coverage of the same frames with the root moved 5 cm sideways and N(0, 0.05^2) added to the pose, microseconds per call of
  - the transform of the mask (both outputs),
  - the forward given `face` (all four outputs), and the smplpp_depth_raster call (face and depth alone) that produces `face`, in
    the same run: the forward walks no triangles and is expected to cost less,
  - the backward (grad_verts, accumulate 0) with cotangents of 1 on both residual sets,
next to
  - the byte floor of each call's inputs and outputs at 8 TB/s and the ratio time / floor: n H W (1 mask + 8 nearest + 4 sqdist) for
    the transform; n H W (8 face + 1 mask + 8 pix_source + 4 pix_sq) + n V (12 verts + 8 vert_target + 4 vert_sq) for the forward;
    n H W (8 face + 8 pix_source + 4 cotangent) + n V (12 verts + 8 vert_target + 4 cotangent + 12 grad_verts) for the backward,
  - the same rule in torch on the same GPU: the transform as a brute-force minimum of the 64-bit keys over all set pixels per block
    of rows (what a user would have written; the count of pixels whose result differs from the library's is reported), the
    backward as autograd of the fixed-correspondence loss,
  - uncovered mask pixels and vertices outside the mask per frame (means): the workload.
Device pointers, torch's current stream; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls
between HIP events, after `--warmup` untimed calls.  Prints one JSON line and writes it to --out.

    python tools/silhouette_bench.py [--steps 20] [--warmup 3] [--reps 3] [--no-torch] [--out profiles/silhouette_bench.json]
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


def torch_transform(mask, block=1 << 27):
    """The key rule in torch, one frame: mask [H,W] bool on the device -> (nearest [H,W] int64, sqdist [H,W] int64)."""
    import torch

    H, W = mask.shape
    q = torch.nonzero(mask.reshape(-1))[:, 0]
    qi, qj = q % W, torch.div(q, W, rounding_mode="floor")
    i = torch.arange(W, device=mask.device)
    rows = max(1, block // max(1, W * len(q)))  # rows per block: about `block` keys at a time
    out = []
    for j0 in range(0, H, rows):
        j = torch.arange(j0, min(H, j0 + rows), device=mask.device)
        d2 = (i[None, :, None] - qi[None, None, :]) ** 2 + (j[:, None, None] - qj[None, None, :]) ** 2
        out.append(((d2 << 32) | q[None, None, :]).min(-1).values)
    key = torch.cat(out)
    return key & 0xFFFFFFFF, key >> 32


def torch_loss(verts, faces, cam, H, W, face, vt, ps):
    """sum(vert_sq) + sum(pix_sq) at fixed correspondences, one frame, differentiable in verts."""
    import torch

    R, t = cam[:9].reshape(3, 3), cam[9:12]
    xc = verts @ R.T + t

    def pi(x):
        return torch.stack([cam[12] * x[:, 0] / x[:, 2] + cam[14], cam[13] * x[:, 1] / x[:, 2] + cam[15]], 1)

    k = torch.nonzero(vt >= 0)[:, 0]
    ctr = torch.stack([(vt[k] % W).float() + 0.5, torch.div(vt[k], W, rounding_mode="floor").float() + 0.5], 1)
    total = ((pi(xc[k]) - ctr) ** 2).sum()
    q = torch.nonzero(ps.reshape(-1) >= 0)[:, 0]
    s = ps.reshape(-1)[q]
    tri = faces[face.reshape(-1)[s]]
    a, b, c = xc[tri[:, 0]], xc[tri[:, 1]], xc[tri[:, 2]]
    with torch.no_grad():
        d = torch.stack([((s % W).float() + 0.5 - cam[14]) / cam[12], (torch.div(s, W, rounding_mode="floor").float() + 0.5 - cam[15]) / cam[13],
                         torch.ones(len(s), device=verts.device)], 1)
        e1, e2 = b - a, c - a
        nrm = torch.linalg.cross(e1, e2)
        w = ((nrm * a).sum(1) / (nrm * d).sum(1))[:, None] * d - a
        nn = (nrm * nrm).sum(1)
        bb, bc = (torch.linalg.cross(w, e2) * nrm).sum(1) / nn, (torch.linalg.cross(e1, w) * nrm).sum(1) / nn
    y = (1 - bb - bc)[:, None] * a + bb[:, None] * b + bc[:, None] * c
    cq = torch.stack([(q % W).float() + 0.5, torch.div(q, W, rounding_mode="floor").float() + 0.5], 1)
    return total + ((pi(y) - cq) ** 2).sum()


def floors(n, H, W, V):
    px, vx = n * H * W, n * V
    return {"transform": px * 13 / PEAK * 1e6, "forward": (px * 21 + vx * 24) / PEAK * 1e6, "backward": (px * 20 + vx * 36) / PEAK * 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "silhouette_bench.json"))
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
    res = {"model": "synthetic", "faces": int(s.face_num), "vertices": int(s.vertex_num), "near": 0.05, "bytes_per_second": PEAK, "sizes": []}
    for n, H, W in SIZES:
        theta = np.zeros((n, 25, 3), np.float32)
        theta[:, 1:] = rng.normal(0, 0.3, (n, 24, 3))
        moved = theta + rng.normal(0, 0.05, theta.shape).astype(np.float32)
        moved[:, 0] = (0.05, 0.0, 0.0)
        zero = torch.zeros(n, 10, device="cuda")
        v = s.forward_differentiable(zero, torch.from_numpy(theta).cuda())[0].detach().contiguous()
        vm = s.forward_differentiable(zero, torch.from_numpy(moved).cuda())[0].detach().contiguous()
        cam = torch.from_numpy(cameras(v.cpu().numpy(), H, W)).cuda()
        mask = (s.depthRaster(vm, cam, H, W, want=())["face"] >= 0).to(torch.uint8)
        face = s.depthRaster(v, cam, H, W, want=())["face"]
        r = s.silhouette(v, cam, H, W, mask, face=face)
        gs, gp = torch.ones_like(r["vert_sq"]), torch.ones_like(r["pix_sq"])
        gv = torch.empty_like(v)
        fl = floors(n, H, W, s.vertex_num)
        row = {"n": n, "H": H, "W": W,
               "uncovered_mask_px": round(float((r["pix_source"] >= 0).sum(dim=(1, 2)).float().mean()), 1),
               "vertices_outside_mask": round(float((r["vert_target"] >= 0).sum(1).float().mean()), 1),
               "transform_us": _time(lambda: s.maskDistanceTransform(mask), a.steps, a.warmup, a.reps),
               "forward_us": _time(lambda: s.silhouette(v, cam, H, W, mask, face=face), a.steps, a.warmup, a.reps),
               "depth_raster_face_depth_only_us": _time(lambda: s.depthRaster(v, cam, H, W, want=()), a.steps, a.warmup, a.reps),
               "backward_us": _time(lambda: s.silhouetteBackward(v, cam, H, W, face, r["vert_target"], r["pix_source"], gs, gp, out=gv.zero_()),
                                    a.steps, a.warmup, a.reps)}
        row["forward_over_depth_raster"] = round(row["forward_us"] / row["depth_raster_face_depth_only_us"], 2)
        for k in ("transform", "forward", "backward"):
            row[k + "_floor_us"] = round(fl[k], 2)
            row[k + "_over_floor"] = round(row[k + "_us"] / fl[k], 1)
        if not a.no_torch:
            lib = s.maskDistanceTransform(mask)

            def transform_in_torch():
                return [torch_transform(mask[i] != 0) for i in range(n)]

            tt = transform_in_torch()
            row["torch_transform_differs_px"] = int(sum(((tt[i][0] != lib[0][i]) | (tt[i][1] != lib[1][i])).sum() for i in range(n)))
            row["torch_transform_us"] = _time(transform_in_torch, max(1, a.steps // 10), 1, a.reps)

            def backward_in_torch():
                vv = v.clone().requires_grad_(True)
                sum(torch_loss(vv[i], faces, cam[i], H, W, face[i], r["vert_target"][i], r["pix_source"][i]) for i in range(n)).backward()
                return vv.grad

            ref = backward_in_torch()
            lib_g = s.silhouetteBackward(v, cam, H, W, face, r["vert_target"], r["pix_source"], gs, gp)
            row["torch_backward_rel_diff"] = float((ref - lib_g).norm() / ref.norm())
            row["torch_backward_us"] = _time(backward_in_torch, max(1, a.steps // 10), 1, a.reps)
        res["sizes"].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
