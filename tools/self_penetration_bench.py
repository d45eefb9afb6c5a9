"""Timing of self-intersection detection and the self-penetration energy (smplpp_self_intersections, smplpp_self_penetration and
its VJP) on one MI355X, synthetic 6890-vertex model (13776 faces).

At each n of SIZES, on frames posed with beta = 0, theta rows 1..24 ~ N(0, 0.3^2) and no root translation, microseconds per call of
  - the detection alone (pairs and count),
  - the forward (detection and the pair energies, sigma = 2),
  - the backward (grad_verts, accumulate 0) at the forward's pairs,
with the pair counts per frame (min / mean / max).  Device pointers, torch's current stream, max_pairs = 32768; each figure is the
median over `--reps` timed blocks of `--steps` back-to-back calls between HIP events, after `--warmup` untimed calls.  Prints one
JSON line and writes it to --out.

    python tools/self_penetration_bench.py [--steps 20] [--warmup 3] [--reps 3] [--out profiles/self_penetration_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (1, 16, 256)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_penetration_bench.json"))
    a = ap.parse_args()
    import torch

    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model_io.synthetic_model())
    rng = np.random.default_rng(0)
    res = {"model": "synthetic", "faces": int(s.face_num), "sigma": 2.0, "max_pairs": 32768, "sizes": []}
    for n in map(int, a.sizes.split(",")):
        theta = np.zeros((n, 25, 3), np.float32)
        theta[:, 1:] = rng.normal(0, 0.3, (n, 24, 3))
        v, _ = s.forward_differentiable(torch.zeros(n, 10, device="cuda"), torch.from_numpy(theta).cuda())
        v = v.detach().contiguous()
        pairs, count, e = s.selfPenetration(v, check=False)
        g = torch.ones_like(e)
        gv = torch.empty_like(v)
        c = count.cpu().numpy()
        row = {"n": n, "pairs_min": int(c.min()), "pairs_mean": round(float(c.mean()), 1), "pairs_max": int(c.max()),
               "detect_us": _time(lambda: s.selfIntersections(v, check=False), a.steps, a.warmup, a.reps),
               "forward_us": _time(lambda: s.selfPenetration(v, check=False), a.steps, a.warmup, a.reps),
               "backward_us": _time(lambda: s.selfPenetrationBackward(v, pairs, count, g, out=gv.zero_()), a.steps, a.warmup, a.reps)}
        res["sizes"].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
