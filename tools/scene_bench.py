"""Timing of the scene term (smplpp_volume_sample, smplpp_scene_term, smplpp_scene_term_vjp) on one MI355X, in both storage layouts.

The points are the K = 6890 vertices of n posed synthetic bodies; the grid is a sphere field of 128^3 or 256^3 nodes whose spacing makes
a body span about 80 voxels per axis.  Two more rows take the first K = 512 vertices on the 128^3 grid: the 256-thread form of the frame sum
(64 < K <= 1024), which whole meshes do not reach.  Every call goes through the bare C entry point with device pointers, in `--reps` blocks of
`--steps` back-to-back calls between HIP events after `--warmup` blocks.  Reported per (grid, n) and call, for each layout:
  - us: the median block, microseconds per call, with the least and the greatest block;
  - floor_us and over_floor: the bytes the call must move (a point's 12 bytes and its cell's 32, outputs written once) at 8 TB/s;
and once per (grid, n):
  - torch_us: torch.nn.functional.grid_sample(align_corners=True) with the same energy, autograd for the backward;
  - fk_us: the smplpp_fk call that makes the vertices.
Prints one JSON line and writes it to --out.

    python tools/scene_bench.py [--steps 50] [--warmup 2] [--reps 5] [--out profiles/scene_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from depth_raster_bench import PEAK  # noqa: E402
from lbfgs_bench import blocks  # noqa: E402

from smplpp_amd import _lib, model_io  # noqa: E402
from smplpp_amd.smpl import SMPL, _stream  # noqa: E402

GRIDS, BATCHES, SPAN, RHO = (128, 256), (1, 16, 256, 1024), 80, 0.05
PART_K, PART_GRID, PART_BATCHES = 512, 128, (1, 256)


def timed(fn, a):
    for _ in range(a.warmup):
        blocks(lambda k: fn(), a.steps, 1)
    return blocks(lambda k: fn(), a.steps, a.reps)


def bodies(s, n):
    """(beta, theta, verts [n,K,3]) on the device, and the time of the smplpp_fk call that makes them."""
    import torch

    rng = np.random.default_rng(n)
    beta = torch.from_numpy(rng.normal(0, 1, (n, 10)).astype(np.float32)).cuda()
    theta = np.zeros((n, 25, 3), np.float32)
    theta[:, 1:] = rng.normal(0, 0.2, (n, 24, 3))
    theta = torch.from_numpy(theta).cuda()
    verts, joints = torch.empty(n, s.vertex_num, 3, device="cuda"), torch.empty(n, 24, 3, device="cuda")
    lib, st = _lib.load(), _stream()
    fk = lambda: _lib.check(lib.smplpp_fk(s.handle, n, beta.data_ptr(), theta.data_ptr(), verts.data_ptr(), joints.data_ptr(), None, None,  # noqa: E731
                                          _lib.DEVICE, st))
    fk()
    return verts, fk


def row(s, G, n, volumes, geometry, a, K=None):
    """K: the first K vertices of every body only (fk_us stays the whole call's)."""
    import torch
    import torch.nn.functional as F

    verts, fk = bodies(s, n)
    if K is not None:
        verts = verts[:, :K].contiguous()
    K = verts.shape[1]
    origin, h, field = geometry
    w_con = torch.zeros(K, device="cuda")
    w_con[::20] = 1.0
    energy, value, grad, valid = torch.empty(n, device="cuda"), torch.empty(n, K, device="cuda"), torch.empty(n, K, 3, device="cuda"), \
        torch.empty(n, K, dtype=torch.uint8, device="cuda")
    ge, gp = torch.ones(n, device="cuda"), torch.empty(n, K, 3, device="cuda")
    lib, st, dev, p = _lib.load(), _stream(), _lib.DEVICE, lambda t: t.data_ptr()
    pts = n * K
    nbytes = {"term": pts * 44 + 4 * K + 4 * n, "sample": pts * (44 + 4 + 12 + 1), "term_vjp": pts * (44 + 12) + 4 * K + 4 * n}
    out = {"grid": G, "n": n, "K": K, "fk_us": timed(fk, a)["median"]}
    for layout, vol in volumes.items():
        hnd = vol.handle
        calls = {
            "term": lambda: _lib.check(lib.smplpp_scene_term(hnd, n, K, p(verts), None, p(w_con), RHO, p(energy), None, None, None, dev, st)),
            "sample": lambda: _lib.check(lib.smplpp_volume_sample(hnd, n, K, p(verts), p(value), p(grad), p(valid), dev, st)),
            "term_vjp": lambda: _lib.check(lib.smplpp_scene_term_vjp(hnd, n, K, p(verts), None, p(w_con), RHO, p(ge), None, None, p(gp), 0, dev, st)),
        }
        for name, fn in calls.items():
            t = timed(fn, a)
            floor = nbytes[name] / PEAK * 1e6
            out.setdefault(name, {})[layout] = {"us": t["median"], "us_least": t["least"], "us_greatest": t["greatest"], "bytes": nbytes[name],
                                                "floor_us": round(floor, 3), "over_floor": round(t["median"] / floor, 1)}
        out["valid_share"] = round(float(valid.float().mean()), 4)
    # the same mathematics in torch
    o_t, h_t = torch.tensor(origin, device="cuda"), torch.tensor(h, device="cuda")
    top = torch.tensor([G - 1.0] * 3, device="cuda")
    vol5 = field.reshape(1, 1, G, G, G)

    def t_sample(v):
        norm = 2.0 * ((v - o_t) / h_t) / top - 1.0
        return F.grid_sample(vol5, norm.reshape(1, n, K, 1, 3), mode="bilinear", padding_mode="zeros", align_corners=True).reshape(n, K)

    def t_term(v):
        sv = t_sample(v)
        q = sv * sv
        return (torch.where(sv < 0, q, torch.zeros_like(q)) + w_con * ((RHO * RHO * q) / (RHO * RHO + q))).sum(1)

    def t_vjp():
        v = verts.detach().requires_grad_(True)
        (t_term(v) * ge).sum().backward()
        return v.grad

    def t_sample_all():
        v = verts.detach().requires_grad_(True)
        sv = t_sample(v)
        sv.sum().backward()
        return sv, v.grad

    with torch.no_grad():
        out["term"]["torch_us"] = timed(lambda: t_term(verts), a)["median"]
    out["sample"]["torch_us"] = timed(t_sample_all, a)["median"]
    out["term_vjp"]["torch_us"] = timed(t_vjp, a)["median"]
    return out


def main():
    import torch

    from smplpp_amd.scene import Volume

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_bench.json"))
    a = ap.parse_args()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model_io.synthetic_model())
    verts, _ = bodies(s, 16)
    lo, hi = verts.amin((0, 1)).cpu().numpy(), verts.amax((0, 1)).cpu().numpy()
    rows, layouts = [], {}
    for G in GRIDS:
        h = np.full(3, float((hi - lo).max()) / SPAN, np.float32)
        origin = (0.5 * (lo + hi) - 0.5 * (G - 1) * h).astype(np.float32)
        ax = [torch.arange(G, device="cuda") * float(h[c]) + float(origin[c]) for c in range(3)]
        zz, yy, xx = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        c0 = 0.5 * (lo + hi) + np.array([0.3, -0.2, 0.1])
        field = (((xx - float(c0[0])) ** 2 + (yy - float(c0[1])) ** 2 + (zz - float(c0[2])) ** 2).sqrt() - 0.6).contiguous()
        volumes = {}
        for layout in ("linear", "cells"):
            os.environ["SMPLPP_VOLUME_LAYOUT"] = layout
            volumes[layout] = Volume("cuda:0", field, origin, h)
            del os.environ["SMPLPP_VOLUME_LAYOUT"]
            assert volumes[layout].layout == layout
        default = Volume("cuda:0", None, origin, h, shape=(G, G, G)).layout
        layouts[str(G)] = default
        for n in BATCHES:
            rows.append(row(s, G, n, volumes, (origin, h, field), a))
        if G == PART_GRID:
            for n in PART_BATCHES:
                rows.append(row(s, G, n, volumes, (origin, h, field), a, PART_K))
    res = {"bytes_per_second": PEAK, "steps": a.steps, "reps": a.reps, "body_span_voxels": SPAN, "default_layout": layouts, "rows": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
