"""Timing of the pose priors (smplpp_pose_prior, smplpp_pose_prior_vjp) on one MI355X: the mixture of tests/pose_prior_oracle.py's
synthetic_gmm(8, 69, 5) with limits, on the body pose of a theta buffer (M = 8, D = 69, ld = 75).

At n = 1, 16, 1024 and 16384 frames, microseconds per call of
  - the forward with all four outputs (energy, component, residual, limit_energy; preallocated),
  - the backward with all three cotangents and the forward's components (accumulate = 0, preallocated),
next to
  - the byte floor of each call at 8 TB/s, computed from shapes: the forward reads 4 D bytes of pose per frame and writes 4 D + 16; the
    backward reads 8 D + 16 and writes 4 D; both read the tables once (the forward the transposed image, the backward both); and the
    ratio time / floor,
  - the same maths in torch on the same GPU in the same run, what a user would have written: an einsum over all components, a min and
    a gather, elementwise limits, with autograd for the backward (that time includes the graph's forward), reported with its relative
    difference from the library's results.
Device pointers, torch's current stream; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls between
HIP events, after `--warmup` untimed calls.  `--flagship-branch` / `--flagship-parent` take the JSON line bench.py printed on this
branch and on its parent commit (one line per run); their headline fields are recorded.  Prints one JSON line and writes it to --out.

    python tools/pose_prior_bench.py [--steps 20] [--warmup 3] [--reps 3] [--no-torch] [--out profiles/pose_prior_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from depth_raster_bench import PEAK, _time  # noqa: E402

import pose_prior_oracle as PO  # noqa: E402
from smplpp_amd import _lib  # noqa: E402
from smplpp_amd.smpl import _ptr, _stream  # noqa: E402

SIZES = (1, 16, 1024, 16384)
M, D, LD, OFF = 8, 69, 75, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--flagship-branch", default=None, help="file holding bench.py's JSON line on this branch")
    ap.add_argument("--flagship-parent", default=None, help="file holding bench.py's JSON line on the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_prior_bench.json"))
    a = ap.parse_args()
    import torch

    from smplpp_amd.priors import PosePrior

    p = PO.prior(M, D, seed=5)
    prior = PosePrior("cuda:0", p["mean"], p["mat"], p["offset"], p["lo"], p["hi"], p["weight"])
    tt = {k: v.cuda() for k, v in PO.tensors(p, torch.float32).items()}
    lib = _lib.load()
    us = lambda b: round(b / PEAK * 1e6, 5)  # noqa: E731
    rel = lambda x, y: float((x - y).norm() / y.norm().clamp(min=1e-30))  # noqa: E731
    t = lambda fn, torch_side=False: _time(fn, max(1, a.steps // 4) if torch_side else a.steps, 1 if torch_side else a.warmup, a.reps)  # noqa: E731
    rng = np.random.default_rng(0)
    tables = 4 * (M * D * D + M * D + M + 3 * D)
    res = {"components": M, "dim": D, "ld": LD, "bytes_per_second": PEAK, "sizes": []}
    for n in SIZES:
        theta = torch.from_numpy(rng.normal(0, 0.3, (n, 25, 3)).astype(np.float32)).cuda()
        e, c, r, le = (torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, D, device="cuda"),
                       torch.empty(n, device="cuda"))
        ge, gr, gl = torch.randn(n, device="cuda"), torch.randn(n, D, device="cuda"), torch.randn(n, device="cuda")
        gt = torch.zeros(n, 25, 3, device="cuda")
        pose, gpose = _ptr(theta) + 4 * OFF, _ptr(gt) + 4 * OFF

        def fwd():
            _lib.check(lib.smplpp_pose_prior(prior.handle, n, pose, LD, _ptr(e), _ptr(c), _ptr(r), _ptr(le), _lib.DEVICE, _stream()))

        def bwd():
            _lib.check(lib.smplpp_pose_prior_vjp(prior.handle, n, pose, LD, _ptr(c), _ptr(ge), _ptr(gr), _ptr(gl), gpose, 0, _lib.DEVICE, _stream()))

        fwd()
        row = {"n": n, "forward_us": t(fwd), "backward_us": t(bwd), "forward_floor_us": us(n * (8 * D + 16) + tables),
               "backward_floor_us": us(n * (12 * D + 16) + tables + 4 * M * D * D)}
        if not a.no_torch:
            def fwd_torch(x=None):
                body = (theta if x is None else x).reshape(n, LD)[:, OFF:]
                ea, y = PO.mixture_t(tt, body)
                best = ea.detach().argmin(1)
                i = torch.arange(n, device="cuda")
                return ea[i, best], best, y[i, best], PO.limit_t(tt, body)

            def bwd_torch():
                x = theta.clone().requires_grad_(True)
                ee, _, yy, ll = fwd_torch(x)
                return torch.autograd.grad((ee * ge).sum() + (yy * gr).sum() + (ll * gl).sum(), x)[0]

            bwd()
            te = fwd_torch()
            row["torch_energy_rel_diff"], row["torch_components_differ"] = rel(te[0], e), int((te[1] != c).sum())
            row["torch_limit_energy_rel_diff"], row["torch_grad_rel_diff"] = rel(te[3], le), rel(bwd_torch(), gt)
            row["torch_forward_us"], row["torch_backward_us"] = t(fwd_torch, True), t(bwd_torch, True)
        for kind in ("forward", "backward"):
            row[kind + "_over_floor"] = round(row[kind + "_us"] / max(row[kind + "_floor_us"], 1e-9), 1)
            if "torch_" + kind + "_us" in row:
                row["torch_%s_over_%s" % (kind, kind)] = round(row["torch_" + kind + "_us"] / row[kind + "_us"], 1)
        res["sizes"].append(row)
    for key, path in (("flagship_branch", a.flagship_branch), ("flagship_parent", a.flagship_parent)):
        if path:
            lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
            res[key] = [{"value": r["value"], "unit": r["unit"], "ms_per_step": r["ms_per_step"], "steps": r["steps"], "warmup": r["warmup"],
                         "sustained_value": r.get("sustained", {}).get("value")} for r in map(json.loads, lines)]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
