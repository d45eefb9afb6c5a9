"""Timing of the depth rasteriser and its backward pass (smplpp_depth_raster, smplpp_depth_raster_vjp) on one MI355X, synthetic
6890-vertex model (13776 faces).

At each (n, H, W) of SIZES, on frames posed with beta = 0, theta rows 1..24 ~ N(0, 0.3^2), no root translation, a camera 2.5 m in
front of each frame's bounding-box centre with f = 1.1 H, microseconds per call of
  - the forward with every output (face, depth, bary, visible, culled) and with face and depth alone,
  - the backward (grad_verts, accumulate 0) at the forward's faces, cotangents of 1,
next to
  - the byte floor each is to be read against: n H W (8 key write + 8 key read + 8 face + 4 depth [+ 12 bary]) + n V (12 read + 1
    visible) bytes for the forward, n H W (8 face + 4 cotangent) + n V (12 read + 12 write) for the backward, at 8 TB/s, and the
    ratio time / floor,
  - the same rule written in torch on the same GPU (candidates from the faces' bounding boxes, one scatter-min of the 64-bit keys
    per frame): what a user would have written.  Reported, with the count of pixels whose face differs from the library's,
  - covered pixels, visible vertices and culled faces per frame (means): the workload.
Device pointers, torch's current stream; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls
between HIP events, after `--warmup` untimed calls.  Prints one JSON line and writes it to --out.

    python tools/depth_raster_bench.py [--steps 20] [--warmup 3] [--reps 3] [--no-torch] [--out profiles/depth_raster_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((16, 512, 512), (64, 256, 256), (256, 128, 128), (1, 1024, 1024))
PEAK = 8e12  # bytes per second, the roofline of the README


def _time(fn, steps, warmup, reps):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / steps)
    return round(float(np.median(out)), 2)


def cameras(verts, H, W):
    """One camera per frame, 2.5 m in front of the bounding-box centre, y down, f = 1.1 H: [n,16] float32."""
    from smplpp_amd.smpl import pinhole_camera

    R = np.diag([1.0, -1.0, -1.0])
    ctr = (verts.min(1) + verts.max(1)) / 2
    t = -ctr @ R.T + np.array([0.0, 0.0, 2.5])
    return pinhole_camera(R, t, 1.1 * H, 1.1 * H, W / 2, H / 2, n=len(verts))


def torch_raster(verts, faces, cam, H, W, near=0.05):
    """The rule of smplpp_depth_raster in torch, one frame: verts [V,3], faces [F,3] int64, cam [16] on one device -> (face [H,W]
    int64, depth [H,W])."""
    import torch

    R, t = cam[:9].reshape(3, 3), cam[9:12]
    xc = torch.stack([((R[k, 0] * verts[:, 0] + R[k, 1] * verts[:, 1]) + R[k, 2] * verts[:, 2]) + t[k] for k in range(3)], 1)
    su = torch.round(((cam[12] * xc[:, 0]) / xc[:, 2] + cam[14]) * 256)
    sv = torch.round(((cam[13] * xc[:, 1]) / xc[:, 2] + cam[15]) * 256)
    ok = torch.isfinite(xc).all(1) & (xc[:, 2] > near) & (su.abs() <= 2.0 ** 23) & (sv.abs() <= 2.0 ** 23)
    x = torch.where(ok, su, torch.zeros_like(su)).long()[faces]
    y = torch.where(ok, sv, torch.zeros_like(sv)).long()[faces]
    A2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    i0, i1 = ((x.min(1).values + 127) >> 8).clamp(min=0), ((x.max(1).values - 128) >> 8).clamp(max=W - 1)
    j0, j1 = ((y.min(1).values + 127) >> 8).clamp(min=0), ((y.max(1).values - 128) >> 8).clamp(max=H - 1)
    live = torch.nonzero(ok[faces].all(1) & (A2 != 0) & (i0 <= i1) & (j0 <= j1))[:, 0]
    w = (i1 - i0 + 1)[live]
    area = w * (j1 - j0 + 1)[live]
    k = torch.repeat_interleave(torch.arange(len(live), device=verts.device), area)
    r = torch.arange(int(area.sum()), device=verts.device) - torch.repeat_interleave(torch.cumsum(area, 0) - area, area)
    f = live[k]
    i, j = i0[f] + r % w[k], j0[f] + torch.div(r, w[k], rounding_mode="floor")
    px, py = i * 256 + 128, j * 256 + 128
    s = torch.sign(A2)[f]
    inside = torch.ones_like(f, dtype=torch.bool)
    for e in range(3):
        p, q = (e + 1) % 3, (e + 2) % 3
        ex, ey = s * (x[f, q] - x[f, p]), s * (y[f, q] - y[f, p])
        E = ex * (py - y[f, p]) - ey * (px - x[f, p])
        inside &= (E > 0) | ((E == 0) & ((ey < 0) | ((ey == 0) & (ex > 0))))
    f, i, j = f[inside], i[inside], j[inside]
    a, b, c = xc[faces[f, 0]], xc[faces[f, 1]], xc[faces[f, 2]]
    e1, e2 = b - a, c - a
    n = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                     e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    dx, dy = ((i.float() + 0.5) - cam[14]) / cam[12], ((j.float() + 0.5) - cam[15]) / cam[13]
    depth = ((n[:, 0] * a[:, 0] + n[:, 1] * a[:, 1]) + n[:, 2] * a[:, 2]) / ((n[:, 0] * dx + n[:, 1] * dy) + n[:, 2])
    keep = (depth > near) & torch.isfinite(depth)
    key = (depth[keep].view(torch.int32).long() << 32) | f[keep]
    best = torch.full((H * W,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=verts.device)
    best.scatter_reduce_(0, (j * W + i)[keep], key, "amin")
    hit = best != torch.iinfo(torch.int64).max
    face = torch.where(hit, best & 0xFFFFFFFF, torch.full_like(best, -1))
    z = torch.where(hit, (best >> 32).int().view(torch.float32), torch.zeros(H * W, device=verts.device))
    return face.reshape(H, W), z.reshape(H, W)


def floors(n, H, W, V):
    px, vx = n * H * W, n * V
    return {"forward_all": (px * 40 + vx * 13) / PEAK * 1e6, "forward_min": (px * 28 + vx * 12) / PEAK * 1e6,
            "backward": (px * 12 + vx * 24) / PEAK * 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_raster_bench.json"))
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
        v, _ = s.forward_differentiable(torch.zeros(n, 10, device="cuda"), torch.from_numpy(theta).cuda())
        v = v.detach().contiguous()
        cam = torch.from_numpy(cameras(v.cpu().numpy(), H, W)).cuda()
        r = s.depthRaster(v, cam, H, W)
        g = torch.ones_like(r["depth"])
        gv = torch.empty_like(v)
        fl = floors(n, H, W, s.vertex_num)
        row = {"n": n, "H": H, "W": W,
               "covered_px": round(float((r["face"] >= 0).sum(dim=(1, 2)).float().mean()), 1),
               "visible_vertices": round(float(r["visible"].sum(1).float().mean()), 1),
               "culled_faces": round(float(r["culled"].float().mean()), 1),
               "forward_us": _time(lambda: s.depthRaster(v, cam, H, W), a.steps, a.warmup, a.reps),
               "forward_face_depth_only_us": _time(lambda: s.depthRaster(v, cam, H, W, want=()), a.steps, a.warmup, a.reps),
               "backward_us": _time(lambda: s.depthRasterBackward(v, cam, H, W, r["face"], g, out=gv.zero_()), a.steps, a.warmup, a.reps)}
        row["forward_floor_us"] = round(fl["forward_all"], 2)
        row["forward_over_floor"] = round(row["forward_us"] / fl["forward_all"], 1)
        row["forward_face_depth_only_floor_us"] = round(fl["forward_min"], 2)
        row["backward_floor_us"] = round(fl["backward"], 2)
        row["backward_over_floor"] = round(row["backward_us"] / fl["backward"], 1)
        if not a.no_torch:
            def in_torch():
                return [torch_raster(v[i], faces, cam[i], H, W) for i in range(n)]

            ft = torch.stack([o[0] for o in in_torch()])
            row["torch_face_differs_px"] = int((ft != r["face"]).sum())
            row["torch_forward_us"] = _time(in_torch, max(1, a.steps // 10), 1, a.reps)
        res["sizes"].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
