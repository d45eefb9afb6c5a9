"""Timing of the bound points (smplpp_skin_points, smplpp_unskin_points and their vector-Jacobian products) on one MI355X, synthetic
6890-vertex model.

At (n, K) = (16, 4096), (64, 1024), (1, 16384), (256, 6890) with a cloud per frame, and one shared cloud of 65536 points over 64 frames,
microseconds per call of
  - the forward (out only) and the backward (every gradient: points, world, joints and, for dense weights, weights), skinning and
    unskinning, under dense weights [1,K,24] shared by the frames and under a face binding [1,K],
next to
  - the byte floor of each call at 8 TB/s: the arrays it must read and write once (points, the binding, world, joints, out; for the
    backward grad_out and every gradient as well), and the ratio time / floor,
  - the same mathematics in float32 torch on the same GPU, what a user would have written: the blend by einsum over the dense weights,
    torch.linalg.solve for the inverse, autograd for the gradients (the time includes that graph's forward).  Reported with its
    relative difference from the library's results.
Device pointers, torch's current stream; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls between
HIP events, after `--warmup` untimed calls.  Prints one JSON line and writes it to --out.

    python tools/skin_points_bench.py [--steps 20] [--warmup 3] [--reps 3] [--no-torch] [--out profiles/skin_points_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from depth_raster_bench import PEAK, _time  # noqa: E402

CASES = ((16, 4096, False), (64, 1024, False), (1, 16384, False), (256, 6890, False), (64, 65536, True))  # (n, K, one shared cloud)


def torch_blend(world, joints, w):
    import torch

    A = world[..., :3]
    G = torch.cat([A, (world[..., 3] - torch.einsum("njab,njb->nja", A, joints))[..., None]], -1)
    return torch.einsum("kj,njab->nkab", w / w.sum(-1, keepdim=True), G)


def torch_forward(world, joints, points, w, unskin):
    import torch

    T = torch_blend(world, joints, w[0])
    p = points.expand(world.shape[0], -1, -1)
    if unskin:
        return torch.linalg.solve(T[..., :3], (p - T[..., 3])[..., None])[..., 0]
    return (T[..., :3] @ p[..., None])[..., 0] + T[..., 3]


def floors(n, K, pf, binding):
    """(forward, backward) bytes moved once."""
    bind = K * (96 if binding == "weights" else 20)
    common = pf * K * 12 + bind + n * 24 * 60
    fwd = common + n * K * 12
    bwd = common + n * K * 12 + pf * K * 12 + n * 24 * 60 + (K * 96 if binding == "weights" else 0)
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skin_points_bench.json"))
    a = ap.parse_args()
    import torch

    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    model = model_io.synthetic_model()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    faces = model["face_indices"].astype(np.int64) - 1
    vt = model["vertices_template"].astype(np.float64)
    W = model["weights"].astype(np.float32)
    rng = np.random.default_rng(0)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    rel = lambda x, y: float((x - y).norm() / y.norm().clamp(min=1e-30))  # noqa: E731
    res = {"model": "synthetic", "bytes_per_second": PEAK, "cases": []}
    for n, K, shared in CASES:
        beta = rng.standard_normal((n, 10)).astype(np.float32)
        theta = (rng.standard_normal((n, 25, 3)) * 0.3).astype(np.float32)
        sk = s.skeleton(dev(beta), dev(theta), want=("world", "joints"))
        world, joints = sk["world"], sk["joints"]
        pf = 1 if shared else n
        face = rng.integers(0, len(faces), (1, K))
        bary = rng.dirichlet(np.ones(3), (1, K)).astype(np.float32)
        rest = np.einsum("fkc,fkcx->fkx", bary, vt[faces[face]])
        x = dev((rest + rng.normal(0, 0.02, (pf, K, 3))).astype(np.float32))
        w = dev(np.einsum("fkc,fkcj->fkj", bary, W[faces[face]]).astype(np.float32))  # the dense weights of the same binding
        g = dev(rng.standard_normal((n, K, 3)).astype(np.float32))
        bindings = {"weights": dict(weights=w), "face": dict(face=dev(face), bary=dev(bary))}
        row = {"n": n, "K": K, "point_frames": pf}
        for unskin in (False, True):
            fwd_fn = s.unskinPoints if unskin else s.skinPoints
            bwd_fn = s.unskinPointsBackward if unskin else s.skinPointsBackward
            pts = x if not unskin else (s.skinPoints(world, joints, x, weights=w, want=())[0] if not shared else
                                        s.skinPoints(world, joints, x, weights=w, want=())[0][:1].contiguous())
            for binding, kw in bindings.items():
                f_floor, b_floor = (round(b / PEAK * 1e6, 2) for b in floors(n, K, pf, binding))
                r = {"forward_us": _time(lambda: fwd_fn(world, joints, pts, want=(), **kw), a.steps, a.warmup, a.reps),
                     "backward_us": _time(lambda: bwd_fn(world, joints, pts, g, **kw), a.steps, a.warmup, a.reps),
                     "forward_floor_us": f_floor, "backward_floor_us": b_floor}
                r["forward_over_floor"] = round(r["forward_us"] / f_floor, 1)
                r["backward_over_floor"] = round(r["backward_us"] / b_floor, 1)
                if binding == "weights" and not a.no_torch:
                    def bwd_torch():
                        leaves = [t.clone().requires_grad_(True) for t in (world, joints, pts, w)]
                        return torch.autograd.grad((torch_forward(*leaves, unskin) * g).sum(), leaves)

                    r["torch_forward_rel_diff"] = rel(torch_forward(world, joints, pts, w, unskin), fwd_fn(world, joints, pts, want=(), **kw)[0])
                    mine, theirs = bwd_fn(world, joints, pts, g, **kw), bwd_torch()
                    r["torch_backward_rel_diff"] = {k: rel(t, mine[k]) for k, t in zip(("world", "joints", "points", "weights"), theirs)}
                    del mine, theirs
                    r["torch_forward_us"] = _time(lambda: torch_forward(world, joints, pts, w, unskin), max(1, a.steps // 4), 1, a.reps)
                    r["torch_backward_us"] = _time(bwd_torch, max(1, a.steps // 4), 1, a.reps)
                    r["torch_forward_over_forward"] = round(r["torch_forward_us"] / r["forward_us"], 1)
                    r["torch_backward_over_backward"] = round(r["torch_backward_us"] / r["backward_us"], 1)
                row[("unskin_" if unskin else "skin_") + binding] = r
        res["cases"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
