"""Timing of the orientation term (smplpp_orientation_term, smplpp_orientation_term_vjp) and of the Rodrigues VJP
(smplpp_axis_angle_to_rotmat_vjp) on one MI355X, beside what a caller had before them, all in one process.

At the shapes (n, S, C) = (1024, 6, 3), (1024, 24, 3), (16384, 24, 3), (1, 24, 3), (1024, 2, 1), on frames [n,24,3,4] (the `world` of
smplpp_skeleton), with offsets, per-frame targets and shared weights, rho = 0, microseconds per call of
  - the forward (all three outputs), the backward to the frames alone (what a pose fit asks for: one launch) and the backward to
    frames, offsets and target (three launches), each beside its byte floor: the bytes the call must read and write once, at 8 TB/s;
  - the same mathematics in float32 torch on the same GPU (tests/orientation_oracle.py::definition_t): forward, and forward + autograd.
One evaluation of the IMU fit of tests/test_skeleton_cpu.py at n = 4 and n = 1024: smplpp_skeleton -> term -> term_vjp (into the
grad_world buffer) -> smplpp_skeleton_vjp, against the same four-call chain with the torch loss of that test and its autograd in the
middle.  The Rodrigues VJP at n x 24 rows against float32 autograd of tests/fk_vjp_oracle.py::rodrigues.
Device pointers through the C entry points, torch's current stream, inputs resident in HBM; each figure is the median over `--reps`
timed blocks of `--steps` back-to-back calls between HIP events, after `--warmup` untimed calls, with the spread of the blocks, (max -
min) / median.  Prints one JSON line and writes it to --out.

    python tools/orientation_bench.py [--steps 50] [--warmup 10] [--reps 5] [--out profiles/orientation_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from smplpp_amd import _lib  # noqa: E402
from smplpp_amd.smpl import _ptr, _stream  # noqa: E402

SHAPES = ((1024, 6, 3), (1024, 24, 3), (16384, 24, 3), (1, 24, 3), (1024, 2, 1))
HBM_BYTES_PER_US = 8e6  # 8 TB/s
IMU_JOINTS = [0, 7, 8, 15, 20, 21]


def _time(fn, steps, warmup, reps):
    """(median us per call, (max - min) / median over the timed blocks)."""
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
    med = float(np.median(out))
    return round(med, 2), round((max(out) - min(out)) / med, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orientation_bench.json"))
    a = ap.parse_args()
    import torch

    import orientation_oracle as OR
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    L, D = _lib.load(), _lib.DEVICE
    J = 24
    res = {"steps": a.steps, "warmup": a.warmup, "reps": a.reps, "term": [], "imu_fit_evaluation": [], "rodrigues_vjp": []}
    timed = lambda row, key, fn: row.update(dict(zip((key + "_us", key + "_spread"), _time(fn, a.steps, a.warmup, a.reps))))  # noqa: E731
    for n, S, C in SHAPES:
        frames, joint, offset, target, weight = OR.random_case(n, S, C, J=J, rs=4, seed=S, Wn=1)
        fr, of, tg, w = (torch.from_numpy(x).cuda() for x in (frames, offset, target, weight))
        jt = torch.from_numpy(joint).cuda()
        e, se, r = (torch.empty(s, device="cuda") for s in ((n,), (n, S), (n, S, 3, C)))
        ge = torch.ones(n, device="cuda")
        gf, go, gt = (torch.zeros(s, device="cuda") for s in ((n, J, 3, 4), (S, 3, C), (n, S, 3, C)))
        head = (0, n, J, 4, _ptr(fr), S, C, _ptr(jt), _ptr(of), _ptr(tg), n, _ptr(w), 1, 0.0)
        tf, to_, tt = (x.clone().requires_grad_(True) for x in (fr, of, tg))

        def forward():
            _lib.check(L.smplpp_orientation_term(*head, _ptr(e), _ptr(se), _ptr(r), D, _stream()))

        def backward_frames():
            _lib.check(L.smplpp_orientation_term_vjp(*head, _ptr(ge), None, None, _ptr(gf), None, None, 0, D, _stream()))

        def backward_all():
            _lib.check(L.smplpp_orientation_term_vjp(*head, _ptr(ge), None, None, _ptr(gf), _ptr(go), _ptr(gt), 0, D, _stream()))

        def torch_forward():
            with torch.no_grad():
                OR.definition_t(fr, jt, tg, of, w, 0.0, C)

        def torch_forward_backward():
            torch.autograd.grad(OR.definition_t(tf, jt, tt, to_, w, 0.0, C)[0].sum(), (tf, to_, tt))

        read = 4 * (n * S * 9 + S * 3 * C + n * S * 3 * C + S) + 8 * S  # the sensors' 3 x 3 blocks, offsets, targets, weights, joints
        row = {"n": n, "S": S, "C": C,
               "forward_floor_us": round((read + 4 * (n + n * S + n * S * 3 * C)) / HBM_BYTES_PER_US, 3),
               "backward_frames_floor_us": round((read + 4 * n + 4 * n * J * 9) / HBM_BYTES_PER_US, 3),
               "backward_all_floor_us": round((read + 4 * n + 4 * (n * J * 9 + S * 3 * C + n * S * 3 * C)) / HBM_BYTES_PER_US, 3)}
        for key, fn in (("forward", forward), ("backward_frames", backward_frames), ("backward_all", backward_all),
                        ("torch_forward", torch_forward), ("torch_forward_backward", torch_forward_backward), ("forward_again", forward)):
            timed(row, key, fn)
        row["forward_rerun_ratio"] = round(row["forward_again_us"] / row["forward_us"], 4)
        row["torch_forward_over_forward"] = round(row["torch_forward_us"] / row["forward_us"], 2)
        row["torch_pair_over_pair"] = round(row["torch_forward_backward_us"] / (row["forward_us"] + row["backward_all_us"]), 2)
        res["term"].append(row)

    # one evaluation of the IMU fit
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model_io.synthetic_model())
    h = s.handle
    for n in (4, 1024):
        beta, theta = (torch.from_numpy(x).cuda() for x in model_io.synthetic_inputs(n, seed=n))
        world, posed = torch.empty((n, J, 3, 4), device="cuda"), torch.empty((n, J, 3), device="cuda")
        gw, gp = torch.zeros((n, J, 3, 4), device="cuda"), torch.zeros((n, J, 3), device="cuda")
        gb, gth = torch.empty((n, 10), device="cuda"), torch.empty((n, 25, 3), device="cuda")
        jt = torch.tensor(IMU_JOINTS, device="cuda")
        S = len(IMU_JOINTS)
        T = torch.from_numpy(OR.random_case(n, S, 3, seed=3)[3]).cuda()
        root = torch.zeros((n, 3), device="cuda")
        e, ge = torch.empty(n, device="cuda"), torch.ones(n, device="cuda")
        head = (0, n, J, 4, _ptr(world), S, 3, _ptr(jt), None, _ptr(T), n, None, 1, 0.0)

        def skeleton():
            _lib.check(L.smplpp_skeleton(h, n, _ptr(beta), _ptr(theta), _ptr(world), _ptr(posed), None, D, _stream()))

        def skeleton_vjp(gw_, gp_):
            _lib.check(L.smplpp_skeleton_vjp(h, n, _ptr(beta), _ptr(theta), _ptr(gw_), _ptr(gp_), None, _ptr(gb), _ptr(gth), 0, D, _stream()))

        def library():
            skeleton()
            _lib.check(L.smplpp_orientation_term(*head, _ptr(e), None, None, D, _stream()))
            # (stored, not added: every joint's 3 x 3 is written, and column 3 of the zeroed buffer is never touched)
            _lib.check(L.smplpp_orientation_term_vjp(*head, _ptr(ge), None, None, _ptr(gw), None, None, 0, D, _stream()))
            gp[:, 0] = 2 * (posed[:, 0] - root)
            skeleton_vjp(gw, gp)

        def torch_loss():
            skeleton()
            w_, p_ = world.detach().requires_grad_(True), posed.detach().requires_grad_(True)
            loss = ((w_[:, IMU_JOINTS, :, :3] - T) ** 2).sum() + ((p_[:, 0] - root) ** 2).sum()
            g1, g2 = torch.autograd.grad(loss, (w_, p_))
            skeleton_vjp(g1.contiguous(), g2.contiguous())

        row = {"n": n}
        for key, fn in (("skeleton_alone", skeleton), ("library", library), ("torch_loss", torch_loss), ("library_again", library)):
            timed(row, key, fn)
        row["torch_loss_over_library"] = round(row["torch_loss_us"] / row["library_us"], 2)
        res["imu_fit_evaluation"].append(row)

    # the Rodrigues VJP at n x 24 rows
    for n in (4, 1024, 16384):
        rows = n * 24
        rng = np.random.default_rng(n)
        aa = torch.from_numpy((0.4 * rng.standard_normal((rows, 3))).astype(np.float32)).cuda()
        g = torch.from_numpy(rng.standard_normal((rows, 3, 3)).astype(np.float32)).cuda()
        out = torch.empty((rows, 3), device="cuda")
        ta = aa.clone().requires_grad_(True)

        def vjp():
            _lib.check(L.smplpp_axis_angle_to_rotmat_vjp(0, rows, _ptr(aa), _ptr(g), _ptr(out), 0, D, _stream()))

        def torch_autograd():
            with torch.device("cuda"):
                torch.autograd.grad((OR.rodrigues(ta) * g).sum(), (ta,))

        row = {"n": n, "rows": rows, "floor_us": round(4 * rows * 15 / HBM_BYTES_PER_US, 3)}
        for key, fn in (("vjp", vjp), ("torch_autograd", torch_autograd)):
            timed(row, key, fn)
        row["torch_over_vjp"] = round(row["torch_autograd_us"] / row["vjp_us"], 2)
        res["rodrigues_vjp"].append(row)

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
