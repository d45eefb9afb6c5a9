"""Timing of the batched L-BFGS step (smplpp_lbfgs_step) on one MI355X.

For each (n, D, m) of SHAPES, a diagonal quadratic per frame (curvatures log-uniform in [1, 1e4], tol_grad = 0) is first optimised
once with the energies and gradients computed by torch, and every f and g of that run is kept on the device.  Then the optimiser is
reset and the run is REPLAYED from the kept arrays: the replay takes the same branches (the rule is deterministic), costs no evaluation
and no host work besides the call, and is what is timed.  The first m + 3 calls fill the history and are not timed; then `--reps`
blocks of `--steps` back-to-back calls between HIP events.  Reported per shape:
  - step_us: the median block, microseconds per call, with the least and the greatest block (the spread);
  - accepted_share: the share of the timed frame-calls that took the accepted path, two-loop recursion over a full history included
    (the others were line-search rejections, which move three vectors and no history);
  - floor_us and over_floor: the byte floor of an accepted call at 8 TB/s, computed from shapes, 4 (2 m D + 6 D) bytes a frame (the
    history read once, and six vectors: x read and written, g, x0, g0, d), and time over it;
  - torch_step_us: the same mathematics written batched in torch on the same GPU in the same run (masked over frames, no host
    synchronisation, its own trajectory from the same replayed inputs), and its ratio to step_us.
Then the step's share of one evaluation of the single-view fit of tests/test_pose_prior_gpu.fit_setup (SMPL forward and backward,
landmarks, projection, pose prior, then the step; D = 75, m = 10) at n = 4 and n = 1024 (the four frames tiled): BatchedLBFGS.step
on the closure against the closure's forward and backward alone, both through torch.autograd, 1 - the ratio of the two.
Prints one JSON line and writes it to --out.

    python tools/lbfgs_bench.py [--steps 20] [--warmup 3] [--reps 5] [--no-torch] [--no-fit] [--out profiles/lbfgs_bench.json]
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
from depth_raster_bench import PEAK  # noqa: E402

from smplpp_amd import _lib  # noqa: E402
from smplpp_amd.smpl import _stream  # noqa: E402

SHAPES = ((1, 72, 10), (16, 101, 10), (1024, 72, 10), (1024, 72, 32), (16384, 72, 10), (1, 20670, 10))


def blocks(fn, steps, reps):
    """Microseconds per call of `reps` blocks of `steps` calls fn(k), k counting on across the blocks."""
    import torch

    out, k = [], 0
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn(k)
            k += 1
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / steps)
    return dict(median=round(float(np.median(out)), 2), least=round(min(out), 2), greatest=round(max(out), 2))


class TorchLBFGS:
    """The rule of smplpp_lbfgs_step written batched in torch: every frame its own history (newest first), step and line search, by
    masks over the frames; nothing is read back.  The same mathematics, not the same rounding."""

    def __init__(self, n, D, m, c1=1e-4, curv_eps=1e-10, max_ls=20, device="cuda"):
        import torch

        z = lambda *s: torch.zeros(*s, device=device)  # noqa: E731
        self.m, self.c1, self.eps, self.max_ls = m, c1, curv_eps, max_ls
        self.x0, self.g0, self.d, self.S, self.Y = z(n, D), z(n, D), z(n, D), z(n, m, D), z(n, m, D)
        self.f0, self.t, self.gtd, self.gamma, self.sy, self.valid = z(n), z(n), z(n), torch.ones(n, device=device), torch.ones(n, m, device=device), z(n, m)
        self.ls, self.status, self.first = z(n), z(n), True

    def step(self, x, f, g):
        import torch

        if self.first:
            self.first = False
            self.x0, self.f0, self.g0, self.d = x.clone(), f.clone(), g.clone(), -g
            self.t = (1 / g.abs().sum(1)).clamp(max=1.0)
            self.gtd = (g * self.d).sum(1)
            x.copy_(self.x0 + self.t[:, None] * self.d)
            return
        run = self.status == 0
        acc = run & torch.isfinite(f) & torch.isfinite(g).all(1) & (f <= self.f0 + self.c1 * self.t * self.gtd)
        rej = run & ~acc
        # rejected
        ls = self.ls + rej
        den = 2 * ((f - self.f0) - self.gtd * self.t)
        tq = (-(self.gtd * self.t * self.t) / den).clamp(min=0).minimum(0.5 * self.t).maximum(0.1 * self.t)
        tn = torch.where(torch.isfinite(f) & (den > 0), tq, 0.5 * self.t)
        out = rej & (ls > self.max_ls)
        # accepted
        s, y = x - self.x0, g - self.g0
        sy, yy = (s * y).sum(1), (y * y).sum(1)
        push = acc & (yy > 0) & (sy > self.eps * yy)
        p3, p2 = push[:, None, None], push[:, None]
        self.S = torch.where(p3, torch.cat([s[:, None], self.S[:, :-1]], 1), self.S)
        self.Y = torch.where(p3, torch.cat([y[:, None], self.Y[:, :-1]], 1), self.Y)
        self.sy = torch.where(p2, torch.cat([sy[:, None], self.sy[:, :-1]], 1), self.sy)
        self.valid = torch.where(p2, torch.cat([torch.ones_like(sy)[:, None], self.valid[:, :-1]], 1), self.valid)
        self.gamma = torch.where(push, sy / yy.clamp(min=1e-30), self.gamma)
        q, alpha = g.clone(), []
        for i in range(self.m):
            a = self.valid[:, i] * (self.S[:, i] * q).sum(1) / self.sy[:, i]
            alpha.append(a)
            q = q - a[:, None] * self.Y[:, i]
        r = torch.where(self.valid[:, :1] > 0, self.gamma[:, None] * q, q)
        for i in range(self.m - 1, -1, -1):
            b = self.valid[:, i] * (self.Y[:, i] * r).sum(1) / self.sy[:, i]
            r = r + (alpha[i] - b)[:, None] * self.S[:, i]
        d = -r
        gtd = (g * d).sum(1)
        bad = acc & ~(gtd < 0)
        self.valid = torch.where(bad[:, None], torch.zeros_like(self.valid), self.valid)
        d, gtd = torch.where(bad[:, None], -g, d), torch.where(bad, -(g * g).sum(1), gtd)
        a2 = acc[:, None]
        self.x0, self.g0, self.f0 = torch.where(a2, x, self.x0), torch.where(a2, g, self.g0), torch.where(acc, f, self.f0)
        self.d, self.gtd = torch.where(a2, d, self.d), torch.where(acc, gtd, self.gtd)
        self.t = torch.where(acc, torch.ones_like(f), torch.where(rej, tn, self.t))
        self.ls = torch.where(acc, torch.zeros_like(ls), ls)
        self.status = torch.where(out, torch.full_like(ls, 3), self.status)
        nxt = torch.where(out[:, None], self.x0, self.x0 + self.t[:, None] * self.d)
        x.copy_(torch.where(run[:, None], nxt, x))


def shape_row(n, D, m, a):
    import torch

    from smplpp_amd.optim import BatchedLBFGS

    rng = np.random.default_rng(n + D + m)
    lam = torch.from_numpy(np.exp(rng.uniform(0, np.log(1e4), (n, D))).astype(np.float32)).cuda()
    c = torch.from_numpy(rng.normal(0, 1, (n, D)).astype(np.float32)).cuda()
    fill, calls = m + 3, m + 3 + a.steps * a.reps
    x = torch.zeros(n, D, device="cuda")
    opt = BatchedLBFGS(x, history=m, tol_grad=0.0)
    F, G = torch.empty(calls, n, device="cuda"), torch.empty(calls, n, D, device="cuda")
    for k in range(calls):  # the run, recorded
        e = x - c
        G[k] = lam * e
        F[k] = 0.5 * (G[k] * e).sum(1)
        opt.step_with(F[k], G[k])
    end = {k: v.cpu().numpy() for k, v in opt.state().items()}
    x_end = x.clone()

    lib, h, xp, stream = _lib.load(), opt.handle, x.data_ptr(), _stream()
    fp, gp = [F.data_ptr() + 4 * n * k for k in range(calls)], [G.data_ptr() + 4 * n * D * k for k in range(calls)]

    def call(k):  # (the bare ABI call: the Python class's argument checks are not part of what is timed)
        _lib.check(lib.smplpp_lbfgs_step(h, xp, D, fp[k], gp[k], D, _lib.DEVICE, stream))

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
        raise SystemExit("the replay of (%d, %d, %d) did not reproduce the recorded run" % (n, D, m))
    floor = n * 4 * (2 * m * D + 6 * D) / PEAK * 1e6
    row = {"n": n, "D": D, "m": m, "step_us": t["median"], "step_us_least": t["least"], "step_us_greatest": t["greatest"],
           "accepted_share": round(float((after["iterations"] - before.cpu().numpy()).sum()) / (n * a.steps * a.reps), 3),
           "stopped_frames": int((after["status"] != 0).sum()), "floor_us": round(floor, 4), "over_floor": round(t["median"] / floor, 1)}
    if not a.no_torch:
        def torch_run():
            ref, xt = TorchLBFGS(n, D, m), torch.zeros(n, D, device="cuda")
            for k in range(fill):
                ref.step(xt, F[k], G[k])
            return blocks(lambda k: ref.step(xt, F[fill + k], G[fill + k]), max(1, a.steps // 4), a.reps)

        torch_run()
        tt = torch_run()
        row.update(torch_step_us=tt["median"], torch_step_us_least=tt["least"], torch_step_us_greatest=tt["greatest"],
                   torch_over_step=round(tt["median"] / t["median"], 1))
    return row


def fit_rows(a):
    """The step's share of one evaluation of the single-view fit, n = 4 and the four frames tiled to n = 1024."""
    import torch

    import test_pose_prior_gpu as TP
    from smplpp_amd import model_io
    from smplpp_amd import smpl as S
    from smplpp_amd.landmarks import Landmarks
    from smplpp_amd.optim import BatchedLBFGS
    from smplpp_amd.priors import PosePrior
    from smplpp_amd.smpl import SMPL

    model = model_io.synthetic_model()
    fs = TP.fit_setup(model)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    lm = Landmarks(s, *fs["reg"])
    p = fs["prior"]
    prior = PosePrior("cuda:0", p["mean"], p["mat"], p["offset"])
    rows = []
    for n in (4, 1024):
        rep = n // 4
        target, cam, beta = fs["target64"].float().cuda().repeat(rep, 1, 1), torch.from_numpy(fs["cam"]).cuda().repeat(rep, 1), torch.zeros(n, 10, device="cuda")
        theta = torch.zeros(n, 25, 3, device="cuda", requires_grad=True)

        def closure():
            verts, joints = s.forward_differentiable(beta, theta)
            _, e, _ = S.project_points_differentiable(lm.forward_differentiable(verts, joints), cam, target, TP.FIT_RHO, TP.NEAR)
            return e.mean(1) + TP.FIT_PRIOR * prior.forward_differentiable(theta)[0]

        opt = BatchedLBFGS(theta.view(n, 75), history=10, tol_grad=0.0)
        for _ in range(13 + a.warmup):
            opt.step(closure)
        whole = blocks(lambda k: opt.step(closure), a.steps, a.reps)

        def evaluation_only(k):
            theta.grad = None
            closure().sum().backward()

        alone = blocks(evaluation_only, a.steps, a.reps)
        rows.append({"n": n, "evaluation_and_step_us": whole["median"], "evaluation_and_step_us_least": whole["least"],
                     "evaluation_and_step_us_greatest": whole["greatest"], "evaluation_only_us": alone["median"],
                     "evaluation_only_us_least": alone["least"], "evaluation_only_us_greatest": alone["greatest"],
                     "step_share": round(max(0.0, 1 - alone["median"] / whole["median"]), 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbfgs_bench.json"))
    a = ap.parse_args()
    res = {"bytes_per_second": PEAK, "steps": a.steps, "reps": a.reps, "shapes": [shape_row(n, D, m, a) for n, D, m in SHAPES]}
    if not a.no_fit:
        res["fit"] = fit_rows(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
