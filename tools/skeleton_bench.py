"""Timing of the skeleton calls (smplpp_skeleton, smplpp_skeleton_rotmat and their vector-Jacobian products) on one MI355X,
synthetic 6890-vertex model, beside what a caller had before them, all in one process.

At n = 1, 16, 256, 1024 and 16384 frames, microseconds per call of
  - each of the four skeleton calls (all outputs; all three cotangents, all gradients),
  - smplpp_fk asked for `joints` and `xforms` only: the pose kernel alone, the nearest forward there was; timed twice, at the start
    and at the end of the row, to show the session's spread,
  - the workaround the skeleton calls replace for posed joints and their gradient: smplpp_fk (verts) -> smplpp_landmarks with the 24
    joint-regressor rows -> smplpp_landmarks_vjp -> smplpp_fk_vjp,
  - the oracle graph (tests/skeleton_oracle.py) in float32 torch with autograd on the same GPU, forward + backward,
each with the spread of its timed blocks, (max - min) / median.  Device pointers through the C entry points, torch's current stream,
inputs resident in HBM; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls between HIP events,
after `--warmup` untimed calls.  Prints one JSON line and writes it to --out.

    python tools/skeleton_bench.py [--steps 50] [--warmup 10] [--reps 5] [--out profiles/skeleton_bench.json]
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

SIZES = (1, 16, 256, 1024, 16384)


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


def _joint_rows(model):
    """The model's joint regressor as 24 CSR rows over the vertices."""
    J = np.asarray(model["joint_regressor"], np.float32)
    rows = [np.nonzero(J[j])[0] for j in range(24)]
    row_ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int64)
    val = np.concatenate([J[j, r] for j, r in enumerate(rows)]).astype(np.float32)
    return row_ptr, col, val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skeleton_bench.json"))
    a = ap.parse_args()
    import torch

    import skeleton_oracle as SO
    from smplpp_amd import model_io
    from smplpp_amd.landmarks import Landmarks
    from smplpp_amd.smpl import SMPL

    L, D = _lib.load(), _lib.DEVICE
    model = model_io.synthetic_model()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    V, h = s.vertex_num, s.handle
    lm = Landmarks(s, *_joint_rows(model))
    m32 = {k: (v.float().cuda() if torch.is_tensor(v) else v) for k, v in SO.model_tensors(model).items()}
    res = {"model": "synthetic", "vertices": int(V), "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "rows": []}
    for n in a.sizes:
        beta, theta = model_io.synthetic_inputs(n, seed=n)
        rng = np.random.default_rng(n)
        dev = lambda shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
        beta, theta = torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda()
        trans = theta[:, 0].contiguous()
        rot = s.axisAngleToRotmat(theta[:, 1:].contiguous())
        world, posed, joints = (torch.empty(shape, device="cuda") for shape in ((n, 24, 3, 4), (n, 24, 3), (n, 24, 3)))
        xforms = torch.empty((n, 24, 4, 4), device="cuda")
        gw, gp, gj = dev((n, 24, 3, 4)), dev((n, 24, 3)), dev((n, 24, 3))
        gb, gt, gtr, gr = (torch.empty(shape, device="cuda") for shape in ((n, 10), (n, 25, 3), (n, 3), (n, 24, 3, 3)))
        verts, rest, gv = (torch.empty((n, V, 3), device="cuda") for _ in range(3))
        points = torch.empty((n, 24, 3), device="cuda")
        tb, tt = beta.clone().requires_grad_(True), theta.clone().requires_grad_(True)

        def skeleton():
            _lib.check(L.smplpp_skeleton(h, n, _ptr(beta), _ptr(theta), _ptr(world), _ptr(posed), _ptr(joints), D, _stream()))

        def skeleton_rotmat():
            _lib.check(L.smplpp_skeleton_rotmat(h, n, _ptr(beta), _ptr(trans), _ptr(rot), _ptr(world), _ptr(posed), _ptr(joints), D, _stream()))

        def skeleton_vjp():
            _lib.check(L.smplpp_skeleton_vjp(h, n, _ptr(beta), _ptr(theta), _ptr(gw), _ptr(gp), _ptr(gj), _ptr(gb), _ptr(gt), 0, D, _stream()))

        def skeleton_rotmat_vjp():
            _lib.check(L.smplpp_skeleton_rotmat_vjp(h, n, _ptr(beta), _ptr(trans), _ptr(rot), _ptr(gw), _ptr(gp), _ptr(gj), _ptr(gb), _ptr(gtr),
                                                    _ptr(gr), 0, D, _stream()))

        def fk_pose_only():
            _lib.check(L.smplpp_fk(h, n, _ptr(beta), _ptr(theta), None, _ptr(joints), _ptr(xforms), None, D, _stream()))

        def workaround():
            _lib.check(L.smplpp_fk(h, n, _ptr(beta), _ptr(theta), _ptr(verts), _ptr(joints), None, _ptr(rest), D, _stream()))
            _lib.check(L.smplpp_landmarks(lm.handle, n, _ptr(verts), _ptr(joints), _ptr(points), D, _stream()))
            _lib.check(L.smplpp_landmarks_vjp(lm.handle, n, _ptr(gp), _ptr(gv), None, 0, D, _stream()))
            _lib.check(L.smplpp_fk_vjp(h, n, _ptr(beta), _ptr(theta), _ptr(rest), _ptr(gv), None, _ptr(gb), _ptr(gt), D, _stream()))

        def torch_graph():
            with torch.device("cuda"):  # (the oracle builds its constants on the default device)
                o = SO.skeleton(m32, tb, tt)
                loss = (o["world"] * gw).sum() + (o["posed"] * gp).sum() + (o["J"] * gj).sum()
                torch.autograd.grad(loss, (tb, tt))

        row = {"n": n}
        for key, fn in (("fk_pose_only", fk_pose_only), ("skeleton", skeleton), ("skeleton_rotmat", skeleton_rotmat),
                        ("skeleton_vjp", skeleton_vjp), ("skeleton_rotmat_vjp", skeleton_rotmat_vjp), ("workaround", workaround),
                        ("torch_graph", torch_graph), ("fk_pose_only_again", fk_pose_only)):
            row[key + "_us"], row[key + "_spread"] = _time(fn, a.steps, a.warmup, a.reps)
        row["pose_only_rerun_ratio"] = round(row["fk_pose_only_again_us"] / row["fk_pose_only_us"], 4)
        row["forward_over_pose_only"] = round(row["skeleton_us"] / row["fk_pose_only_us"], 4)
        row["backward_over_forward"] = round(row["skeleton_vjp_us"] / row["skeleton_us"], 4)
        both = row["skeleton_us"] + row["skeleton_vjp_us"]
        row["workaround_over_skeleton_pair"] = round(row["workaround_us"] / both, 2)
        row["torch_graph_over_skeleton_pair"] = round(row["torch_graph_us"] / both, 2)
        res["rows"].append(row)
        del verts, rest, gv
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
