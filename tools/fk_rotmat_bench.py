"""Timing of the rotation-matrix entry points (smplpp_fk_rotmat, smplpp_fk_rotmat_vjp) beside their axis-angle counterparts on one
MI355X, synthetic 6890-vertex model.

For the default form and SMPLPP_SKIN=h, at n = 16, 256 and 1024 frames, microseconds per call of
  - smplpp_fk_rotmat and smplpp_fk on the same body (verts, joints, xforms and rest into preallocated outputs),
  - smplpp_fk_rotmat_vjp and smplpp_fk_vjp (dL/dverts and dL/djoints in, `rest` passed),
  - the workaround the new entry point replaces: smplpp_rotmat_to_axis_angle on the [n * 24] matrices, the copy of the angles into
    theta[:, 1:] (theta's rows are 25 x 3, so the angles cannot be written in place), then smplpp_fk,
each with the spread of its timed blocks, (max - min) / median, and the ratios rotmat / axis-angle and rotmat / workaround.
Device pointers through the C entry points, torch's current stream, inputs resident in HBM; each figure is the median over `--reps`
timed blocks of `--steps` back-to-back calls between HIP events, after `--warmup` untimed calls.  The calls of one comparison are
timed in turn inside the same process.  Prints one JSON line and writes it to --out.

    python tools/fk_rotmat_bench.py [--steps 50] [--warmup 10] [--reps 7] [--out profiles/fk_rotmat_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smplpp_amd import _lib  # noqa: E402
from smplpp_amd.smpl import _ptr, _stream  # noqa: E402

SIZES = (16, 256, 1024)
FORMS = ("default", "h")


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


def _model(form):
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    old = os.environ.pop("SMPLPP_SKIN", None)
    if form != "default":
        os.environ["SMPLPP_SKIN"] = form
    try:
        s = SMPL()
        s.setDevice("cuda:0")
        s.init(model_io.synthetic_model())
    finally:
        os.environ.pop("SMPLPP_SKIN", None)
        if old is not None:
            os.environ["SMPLPP_SKIN"] = old
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fk_rotmat_bench.json"))
    a = ap.parse_args()
    import torch

    from smplpp_amd import model_io

    L = _lib.load()
    D = _lib.DEVICE
    res = {"model": "synthetic", "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "forms": {}}
    for form in FORMS:
        s = _model(form)
        V, h = s.vertex_num, s.handle
        res["vertices"] = int(V)
        rows = []
        for n in SIZES:
            beta, theta = model_io.synthetic_inputs(n, seed=n)
            rng = np.random.default_rng(n)
            beta, theta = torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda()
            trans = theta[:, 0].contiguous()
            rot = s.axisAngleToRotmat(theta[:, 1:].contiguous())
            verts, rest = torch.empty((n, V, 3), device="cuda"), torch.empty((n, V, 3), device="cuda")
            joints, xforms = torch.empty((n, 24, 3), device="cuda"), torch.empty((n, 24, 4, 4), device="cuda")
            gv = torch.from_numpy(rng.standard_normal((n, V, 3)).astype(np.float32)).cuda()
            gj = torch.from_numpy(rng.standard_normal((n, 24, 3)).astype(np.float32)).cuda()
            gb, gt, gtr, gr = (torch.empty(shape, device="cuda") for shape in ((n, 10), (n, 25, 3), (n, 3), (n, 24, 3, 3)))
            aa, theta2 = torch.empty((n * 24, 3), device="cuda"), theta.clone()

            def fk():
                _lib.check(L.smplpp_fk(h, n, _ptr(beta), _ptr(theta), _ptr(verts), _ptr(joints), _ptr(xforms), _ptr(rest), D, _stream()))

            def fk_rot():
                _lib.check(L.smplpp_fk_rotmat(h, n, _ptr(beta), _ptr(trans), _ptr(rot), _ptr(verts), _ptr(joints), _ptr(xforms), _ptr(rest),
                                              D, _stream()))

            def workaround():
                _lib.check(L.smplpp_rotmat_to_axis_angle(0, n * 24, _ptr(rot), _ptr(aa), D, _stream()))
                theta2[:, 1:] = aa.view(n, 24, 3)
                _lib.check(L.smplpp_fk(h, n, _ptr(beta), _ptr(theta2), _ptr(verts), _ptr(joints), _ptr(xforms), _ptr(rest), D, _stream()))

            def vjp():
                _lib.check(L.smplpp_fk_vjp(h, n, _ptr(beta), _ptr(theta), _ptr(rest0), _ptr(gv), _ptr(gj), _ptr(gb), _ptr(gt), D, _stream()))

            def vjp_rot():
                _lib.check(L.smplpp_fk_rotmat_vjp(h, n, _ptr(beta), _ptr(trans), _ptr(rot), _ptr(rest0), _ptr(gv), _ptr(gj), _ptr(gb), _ptr(gtr),
                                                  _ptr(gr), D, _stream()))

            fk()
            rest0 = rest.clone()
            row = {"n": n}
            for key, fn in (("fk", fk), ("fk_rotmat", fk_rot), ("workaround", workaround), ("fk_vjp", vjp), ("fk_rotmat_vjp", vjp_rot),
                            ("fk_again", fk), ("fk_vjp_again", vjp)):
                row[key + "_us"], row[key + "_spread"] = _time(fn, a.steps, a.warmup, a.reps)
            # the same call timed twice in the session: the run-to-run spread the ratios are read against
            row["forward_rerun_ratio"] = round(row["fk_again_us"] / row["fk_us"], 4)
            row["backward_rerun_ratio"] = round(row["fk_vjp_again_us"] / row["fk_vjp_us"], 4)
            row["forward_ratio"] = round(row["fk_rotmat_us"] / row["fk_us"], 4)
            row["backward_ratio"] = round(row["fk_rotmat_vjp_us"] / row["fk_vjp_us"], 4)
            row["forward_over_workaround"] = round(row["fk_rotmat_us"] / row["workaround_us"], 4)
            rows.append(row)
        res["forms"][form] = rows
        del s
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
