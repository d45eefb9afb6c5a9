"""Timing of the sequence terms (smplpp_sequence_split / _merge / _sum / _smoothness / _smoothness_vjp) on one MI355X.

For each (P, T, K, C) of SHAPES: P problems of T frames and one shared row each in a buffer [P (T + 1), 75], points x [F, K, C].  Every
call goes through the bare C entry point with device pointers (the Python class's argument checks are not part of what is timed), in
`--reps` blocks of `--steps` back-to-back calls between HIP events after `--warmup` blocks.  Reported per shape and call:
  - us: the median block, microseconds per call, with the least and the greatest block;
  - floor_us and over_floor: the bytes the call must move (inputs read once, outputs written once) at 8 TB/s, and time over it;
  - torch_us: the same mathematics in torch on the same GPU (index_select / index_add for split / merge / sum, slices for the term).
Then one evaluation (energies and their gradient) of the two-sequence fit of tests/test_lbfgs_groups_gpu.py section 7, with that file's
torch glue and with these calls.  Prints one JSON line and writes it to --out.

    python tools/sequence_bench.py [--steps 50] [--warmup 2] [--reps 5] [--no-fit] [--out profiles/sequence_bench.json]
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

from smplpp_amd import _lib  # noqa: E402
from smplpp_amd.smpl import _stream  # noqa: E402

# (16, 64, 512, 3): the 256-thread form of the frame sum (64 < K <= 1024), which the other shapes do not reach
SHAPES = ((1, 300, 24, 3), (16, 300, 24, 3), (256, 16, 24, 3), (4, 64, 6890, 3), (16, 64, 512, 3))
D, C_S = 75, 10


def timed(fn, a):
    for _ in range(a.warmup):
        blocks(lambda k: fn(), a.steps, 1)
    return blocks(lambda k: fn(), a.steps, a.reps)


def shape_row(P, T, K, C, a):
    import torch

    from smplpp_amd.sequence import SequenceLayout

    seq = SequenceLayout("cuda:0", [T + 1] * P, 1)
    F, n = seq.frames, seq.rows
    g = torch.Generator(device="cuda").manual_seed(P + T + K)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    rows, frames, shared, grad_rows = rnd(n, D), torch.empty(F, D, device="cuda"), torch.empty(F, C_S, device="cuda"), torch.empty(n, D, device="cuda")
    gf, gs, fv, pv = rnd(F, D), rnd(F, C_S), rnd(F), torch.empty(P, device="cuda")
    x, fe, gfe, gx = rnd(F, K, C), torch.empty(F, device="cuda"), rnd(F), torch.empty(F, K, C, device="cuda")
    lib, h, st, dev = _lib.load(), seq.handle, _stream(), _lib.DEVICE
    p = lambda t: t.data_ptr()  # noqa: E731
    calls = {
        "split": (lambda: _lib.check(lib.smplpp_sequence_split(h, p(rows), D, 0, D, p(frames), C_S, p(shared), dev, st)), 4 * (F * D + P * C_S + F * (D + C_S))),
        "merge": (lambda: _lib.check(lib.smplpp_sequence_merge(h, p(gf), 0, D, p(gs), C_S, p(grad_rows), D, D, 0, dev, st)), 4 * (F * (D + C_S) + n * D)),
        "sum": (lambda: _lib.check(lib.smplpp_sequence_sum(h, p(fv), 1.0, p(pv), 0, dev, st)), 4 * (F + P)),
        "smoothness": (lambda: _lib.check(lib.smplpp_sequence_smoothness(h, p(x), K * C, K, C, 1, None, 0.0, p(fe), None, dev, st)), 4 * (F * K * C + F)),
        "smoothness_vjp": (lambda: _lib.check(lib.smplpp_sequence_smoothness_vjp(h, p(x), K * C, K, C, 1, None, 0.0, p(gfe), None, p(gx), 0, dev, st)),
                           4 * (2 * F * K * C + F)),
    }
    # the same mathematics in torch
    row_of = torch.from_numpy(np.concatenate([np.arange(T) + q * (T + 1) for q in range(P)])).cuda()
    shared_row = torch.from_numpy(np.repeat(np.arange(P) * (T + 1) + T, T)).cuda()
    problem_of = torch.from_numpy(np.repeat(np.arange(P), T)).cuda()
    inside = torch.from_numpy(np.tile(np.arange(T) < T - 1, P)).cuda()[:-1].float()  # the pairs (f, f + 1) of one problem

    def t_merge():
        out = torch.zeros(n, D, device="cuda")
        out.index_copy_(0, row_of, gf)
        out[:, :C_S].index_add_(0, shared_row, gs)
        return out

    def t_smooth(v):
        return ((v[1:] - v[:-1]).pow(2).sum((1, 2)) * inside)

    def t_smooth_vjp():
        v = x.detach().requires_grad_(True)
        (t_smooth(v) * gfe[:-1]).sum().backward()
        return v.grad

    torch_calls = {"split": lambda: (rows.index_select(0, row_of), rows.index_select(0, shared_row)[:, :C_S].contiguous()), "merge": t_merge,
                   "sum": lambda: torch.zeros(P, device="cuda").index_add_(0, problem_of, fv), "smoothness": lambda: t_smooth(x),
                   "smoothness_vjp": t_smooth_vjp}
    row = {"P": P, "T": T, "K": K, "C": C, "frames": F}
    for name, (fn, nbytes) in calls.items():
        t, tt = timed(fn, a), timed(torch_calls[name], a)
        floor = nbytes / PEAK * 1e6
        row[name] = {"us": t["median"], "us_least": t["least"], "us_greatest": t["greatest"], "bytes": nbytes, "floor_us": round(floor, 4),
                     "over_floor": round(t["median"] / floor, 1), "torch_us": tt["median"], "torch_over": round(tt["median"] / t["median"], 1)}
    return row


def fit_row(a):
    """One evaluation (closure and backward) of the section-7 sequence fit with the torch glue of test_lbfgs_groups_gpu and with these calls."""
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_lbfgs_groups_gpu as TG
    import test_pose_prior_gpu as TP
    from smplpp_amd import model_io
    from smplpp_amd import smpl as S
    from smplpp_amd.landmarks import Landmarks
    from smplpp_amd.priors import PosePrior
    from smplpp_amd.sequence import SequenceLayout
    from smplpp_amd.smpl import SMPL

    model = model_io.synthetic_model()
    fs = TG.seq_setup(model)
    n = fs["n"]
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    lm = Landmarks(s, *fs["reg"])
    prior = PosePrior("cuda:0", fs["prior"]["mean"], fs["prior"]["mat"], fs["prior"]["offset"])
    dev = torch.device("cuda:0")
    cam32, target32 = torch.from_numpy(fs["cam"]).to(dev), fs["target64"].float().to(dev)
    buf = (0.1 * torch.randn(sum(TG.SEQ_GROUPS), 75, device=dev)).requires_grad_(True)
    seq = SequenceLayout("cuda:0", TG.SEQ_GROUPS, 1)

    def frame_terms(theta, beta):
        verts, joints = s.forward_differentiable(beta, theta)
        _, e, _ = S.project_points_differentiable(lm.forward_differentiable(verts, joints), cam32, target32, TP.FIT_RHO, TP.NEAR)
        return e.mean(1) + TP.FIT_PRIOR * prior.forward_differentiable(theta)[0], joints

    def glue():
        theta, beta, shared = TG.seq_layout(buf)
        frames, joints = frame_terms(theta, beta)
        return TG.seq_energy(frames, joints, shared)

    def native():
        theta, beta = seq.split_differentiable(buf, 0, 75, 10)
        frames, joints = frame_terms(theta.reshape(n, 25, 3), beta)
        shared = torch.stack([beta[0], beta[n - 1]])
        return seq.sum_differentiable(frames + TG.SEQ_VELOCITY * seq.smoothness_differentiable(joints, 1)) + TG.SEQ_BETA * shared.pow(2).sum(1)

    def evaluation(closure):
        buf.grad = None
        closure().sum().backward()

    out = {}
    for name, closure in (("torch_glue", glue), ("native_glue", native)):
        t = timed(lambda: evaluation(closure), a)
        out[name + "_us"], out[name + "_us_least"], out[name + "_us_greatest"] = t["median"], t["least"], t["greatest"]
    out["torch_over_native"] = round(out["torch_glue_us"] / out["native_glue_us"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_bench.json"))
    a = ap.parse_args()
    res = {"bytes_per_second": PEAK, "steps": a.steps, "reps": a.reps, "shapes": [shape_row(P, T, K, C, a) for P, T, K, C in SHAPES]}
    if not a.no_fit:
        res["sequence_fit_evaluation"] = fit_row(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
