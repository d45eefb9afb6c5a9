"""Timing of the forward mode of FK (smplpp_fk_jvp) on one MI355X, synthetic 6890-vertex model, beside what a caller had before
it, all in one process.

At (n, T) = (1024, 1), (256, 4), (16, 85 shared), (1, 85 shared): microseconds per call of smplpp_fk_jvp with all three outputs
and the rest shape handed over, and, at (1024, 1) and (16384, 1), of the chain-only call (djoints and dworld).  Beside each:
  - the byte floor: the outputs written plus one read of the operand image BT, at 8 TB/s,
  - T x smplpp_fk (verts) on the same body, the natural yardstick (one tangent ~ one forward),
  - central differences: 2 T smplpp_fk calls and the subtraction in torch,
  - float32 torch.func.jvp of the oracle graph (tests/fk_jvp_oracle.py) on the same GPU, one call over the n T columns,
each with the spread of its timed blocks, (max - min) / median.  Device pointers through the C entry points, torch's current stream,
inputs resident in HBM; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls between HIP events,
after `--warmup` untimed calls.  Prints one JSON line and writes it to --out.

    python tools/fk_jvp_bench.py [--steps 20] [--warmup 5] [--reps 5] [--out profiles/fk_jvp_bench.json]
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

FULL = ((1024, 1, False), (256, 4, False), (16, 85, True), (1, 85, True))
CHAIN = ((1024, 1), (16384, 1))
HBM = 8e12  # bytes per second, the figure of the README's byte floors


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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fk_jvp_bench.json"))
    a = ap.parse_args()
    import torch

    import fk_jvp_oracle as JO
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    L, D = _lib.load(), _lib.DEVICE
    model = model_io.synthetic_model()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    V, h = s.vertex_num, s.handle
    m32 = {k: (v.float().cuda() if torch.is_tensor(v) else v) for k, v in JO.model_tensors(model).items()}
    bt_bytes = ((V + 31) // 32) * 32 * 3 * 224 * 4
    res = {"model": "synthetic", "vertices": int(V), "steps": a.steps, "warmup": a.warmup, "reps": a.reps, "bt_bytes": bt_bytes,
           "rows": [], "chain_only": []}

    def inputs(n, T, shared):
        beta, theta = model_io.synthetic_inputs(n, seed=n)
        rng = np.random.default_rng(n + T)
        lead = (T,) if shared else (n, T)
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        if shared and T == 85:
            eye = np.eye(85, dtype=np.float32)
            db, dth = eye[:, :10], eye[:, 10:].reshape(85, 25, 3)
        else:
            db, dth = rng.standard_normal(lead + (10,)), rng.standard_normal(lead + (25, 3))
        return dev(beta), dev(theta), dev(db), dev(dth)

    for n, T, shared in FULL:
        beta, theta, db, dth = inputs(n, T, shared)
        verts, rest, v2 = (torch.empty((n, V, 3), device="cuda") for _ in range(3))
        dv, dj, dw = (torch.empty((n, T) + t, device="cuda") for t in ((V, 3), (24, 3), (24, 3, 4)))
        _lib.check(L.smplpp_fk(h, n, _ptr(beta), _ptr(theta), _ptr(verts), None, None, _ptr(rest), D, _stream()))
        step = torch.full_like(theta, 1e-3)
        cols = lambda x: x[:, None].expand((n, T) + tuple(x.shape[1:])).reshape((-1,) + tuple(x.shape[1:])).contiguous()
        cb, cth = cols(beta), cols(theta)
        tb = (db[None].expand((n,) + tuple(db.shape)) if shared else db).reshape(n * T, 10).contiguous()
        tth = (dth[None].expand((n,) + tuple(dth.shape)) if shared else dth).reshape(n * T, 25, 3).contiguous()

        def jvp():
            _lib.check(L.smplpp_fk_jvp(h, n, T, _ptr(beta), _ptr(theta), _ptr(rest), _ptr(db), _ptr(dth), int(shared), _ptr(dv), _ptr(dj),
                                       _ptr(dw), D, _stream()))

        def fk_T():
            for _ in range(T):
                _lib.check(L.smplpp_fk(h, n, _ptr(beta), _ptr(theta), _ptr(verts), None, None, None, D, _stream()))

        def central():
            for t in range(T):
                tp, tm = theta + step, theta - step
                _lib.check(L.smplpp_fk(h, n, _ptr(beta), _ptr(tp), _ptr(verts), None, None, None, D, _stream()))
                _lib.check(L.smplpp_fk(h, n, _ptr(beta), _ptr(tm), _ptr(v2), None, None, None, D, _stream()))
                dv[:, t] = (verts - v2) * 500.0

        def torch_jvp():
            with torch.device("cuda"):  # (the oracle builds its constants on the default device)
                torch.func.jvp(lambda b_, t_: JO.O.fk(m32, b_, t_)["verts"], (cb, cth), (tb, tth))

        row = {"n": n, "T": T, "shared": shared}
        for key, fn in (("jvp", jvp), ("fk_times_T", fk_T), ("central_differences", central), ("torch_jvp", torch_jvp), ("jvp_again", jvp)):
            row[key + "_us"], row[key + "_spread"] = _time(fn, a.steps, a.warmup, a.reps)
        out_bytes = 4 * n * T * (V * 3 + 72 + 288)
        row["byte_floor_us"] = round((out_bytes + bt_bytes) / HBM * 1e6, 2)
        row["over_byte_floor"] = round(row["jvp_us"] / row["byte_floor_us"], 2)
        for key in ("fk_times_T", "central_differences", "torch_jvp"):
            row[key + "_over_jvp"] = round(row[key + "_us"] / row["jvp_us"], 2)
        row["rerun_ratio"] = round(row["jvp_again_us"] / row["jvp_us"], 4)
        res["rows"].append(row)
        del verts, rest, v2, dv, cb, cth, tb, tth
    for n, T in CHAIN:
        beta, theta, db, dth = inputs(n, T, False)
        dj, dw = (torch.empty((n, T) + t, device="cuda") for t in ((24, 3), (24, 3, 4)))
        world, joints = torch.empty((n, 24, 3, 4), device="cuda"), torch.empty((n, 24, 3), device="cuda")

        def chain():
            _lib.check(L.smplpp_fk_jvp(h, n, T, _ptr(beta), _ptr(theta), None, _ptr(db), _ptr(dth), 0, None, _ptr(dj), _ptr(dw), D, _stream()))

        def skeleton():
            _lib.check(L.smplpp_skeleton(h, n, _ptr(beta), _ptr(theta), _ptr(world), None, _ptr(joints), D, _stream()))

        row = {"n": n, "T": T}
        for key, fn in (("chain_only", chain), ("skeleton", skeleton)):
            row[key + "_us"], row[key + "_spread"] = _time(fn, a.steps, a.warmup, a.reps)
        row["byte_floor_us"] = round(4 * n * T * (72 + 288) / HBM * 1e6, 3)
        row["over_skeleton"] = round(row["chain_only_us"] / row["skeleton_us"], 2)
        res["chain_only"].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
