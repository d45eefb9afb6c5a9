"""Timing of the L-BFGS step on problems that span groups of rows (smplpp_lbfgs_create_grouped) on one MI355X.

For each (P, rows, D, m) of SHAPES, P problems of N = rows * D unknowns, a diagonal quadratic per problem (curvatures log-uniform in
[1, 1e4], tol_grad = 0) is first optimised once with the energies and gradients computed by torch, and every f and g of that run is
kept on the device.  Then the optimiser is reset and the run is REPLAYED from the kept arrays, as tools/lbfgs_bench.py does: the same
branches, no evaluation, no host work besides the call through the C entry point with device pointers.  The first m + 3 calls fill the
history and are not timed; then `--reps` blocks of `--steps` back-to-back calls between HIP events.  Reported per shape:
  - step_us: the grouped handle, x [P rows, D] with groups of `rows` rows: the median block, microseconds per call, with the least and
    the greatest block, and the share of the timed problem-calls that took the accepted path;
  - ungrouped_step_us: a handle from smplpp_lbfgs_create on the same unknowns as x [P, rows D] (one wavefront per problem, the
    64-partial rule: its own recorded run and replay), in the same session;
  - floor_us and over_floor: the byte floor of an accepted call at 8 TB/s, 4 (2 m N + 6 N) bytes per problem, and time over it;
  - torch_step_us: the same mathematics written batched in torch (tools/lbfgs_bench.py: TorchLBFGS) on [P, N].
Prints one JSON line and writes it to --out.

    python tools/lbfgs_wide_bench.py [--steps 20] [--warmup 3] [--reps 5] [--no-torch] [--out profiles/lbfgs_wide_bench.json]
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
from lbfgs_bench import TorchLBFGS, blocks  # noqa: E402

from smplpp_amd import _lib  # noqa: E402
from smplpp_amd.smpl import _stream  # noqa: E402

SHAPES = ((1, 1, 20670, 10), (1, 300, 75, 10), (16, 300, 75, 10), (256, 16, 75, 10))


def replayed(P, N, m, a, lam, c, rows=None, D=None):
    """Record a run of P problems of N unknowns and time its replay: with groups of `rows` rows of D when given, else on a handle without
    groups over x [P, N].  Returns (times, accepted share, stopped problems, F, G)."""
    import torch

    from smplpp_amd.optim import BatchedLBFGS

    fill, calls = m + 3, m + 3 + a.steps * a.reps
    x = torch.zeros(P, N, device="cuda")
    if rows is None:
        opt, ld = BatchedLBFGS(x, history=m, tol_grad=0.0), N
    else:
        opt, ld = BatchedLBFGS(x.view(P * rows, D), history=m, groups=[rows] * P, tol_grad=0.0), D
    F, G = torch.empty(calls, P, device="cuda"), torch.empty(calls, P, N, device="cuda")
    for k in range(calls):  # the run, recorded
        e = x - c
        G[k] = lam * e
        F[k] = 0.5 * (G[k] * e).sum(1)
        opt.step_with(F[k], G[k].view(-1, ld))
    end = {k: v.cpu().numpy() for k, v in opt.state().items()}
    x_end = x.clone()

    lib, h, xp, stream = _lib.load(), opt.handle, x.data_ptr(), _stream()
    fp, gp = [F.data_ptr() + 4 * P * k for k in range(calls)], [G.data_ptr() + 4 * P * N * k for k in range(calls)]

    def call(k):  # (the bare ABI call: the Python class's argument checks are not part of what is timed)
        _lib.check(lib.smplpp_lbfgs_step(h, xp, ld, fp[k], gp[k], ld, _lib.DEVICE, stream))

    def replay():
        opt.reset()
        x.zero_()
        for k in range(fill):
            call(k)
        before = opt.state(("iterations",))["iterations"].clone()
        return blocks(lambda k: call(fill + k), a.steps, a.reps), before

    for _ in range(a.warmup):
        replay()
    t, before = replay()
    after = {k: v.cpu().numpy() for k, v in opt.state().items()}
    if not (torch.equal(x, x_end) and all(np.array_equal(after[k], end[k], equal_nan=True) for k in end)):
        raise SystemExit("the replay of (%d, %d, %d) did not reproduce the recorded run" % (P, N, m))
    share = round(float((after["iterations"] - before.cpu().numpy()).sum()) / (P * a.steps * a.reps), 3)
    return t, share, int((after["status"] != 0).sum()), F, G


def shape_row(P, rows, D, m, a):
    import torch

    N = rows * D
    rng = np.random.default_rng(P + N + m)
    lam = torch.from_numpy(np.exp(rng.uniform(0, np.log(1e4), (P, N))).astype(np.float32)).cuda()
    c = torch.from_numpy(rng.normal(0, 1, (P, N)).astype(np.float32)).cuda()
    t, share, stopped, F, G = replayed(P, N, m, a, lam, c, rows, D)
    floor = P * 4 * (2 * m * N + 6 * N) / PEAK * 1e6
    row = {"P": P, "rows": rows, "D": D, "m": m, "N": N, "step_us": t["median"], "step_us_least": t["least"], "step_us_greatest": t["greatest"],
           "accepted_share": share, "stopped_problems": stopped, "floor_us": round(floor, 4), "over_floor": round(t["median"] / floor, 1)}
    if not a.no_torch:
        fill = m + 3

        def torch_run():
            ref, xt = TorchLBFGS(P, N, m), torch.zeros(P, N, device="cuda")
            for k in range(fill):
                ref.step(xt, F[k], G[k])
            return blocks(lambda k: ref.step(xt, F[fill + k], G[fill + k]), max(1, a.steps // 4), a.reps)

        torch_run()
        tt = torch_run()
        row.update(torch_step_us=tt["median"], torch_step_us_least=tt["least"], torch_step_us_greatest=tt["greatest"],
                   torch_over_step=round(tt["median"] / t["median"], 1))
    del F, G
    tu, share_u, stopped_u, _, _ = replayed(P, N, m, a, lam, c)
    row.update(ungrouped_step_us=tu["median"], ungrouped_step_us_least=tu["least"], ungrouped_step_us_greatest=tu["greatest"],
               ungrouped_accepted_share=share_u, ungrouped_stopped_problems=stopped_u, ungrouped_over_step=round(tu["median"] / t["median"], 1))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbfgs_wide_bench.json"))
    a = ap.parse_args()
    res = {"bytes_per_second": PEAK, "steps": a.steps, "reps": a.reps, "lds_threshold_N": 32768,
           "shapes": [shape_row(P, rows, D, m, a) for P, rows, D, m in SHAPES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
