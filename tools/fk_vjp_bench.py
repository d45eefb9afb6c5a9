"""Timing of smplpp_fk_vjp (the FK backward pass) beside the forward step, on one MI355X.

Prints one JSON line: microseconds per smplpp_fk_vjp at n frames (default 1024) on the synthetic 6890-vertex model, with `rest`
passed and with rest = NULL (recomputed inside the call), the forward step (smplpp_fk, verts + joints) on the same device, and the
algorithmic bytes / FLOPs of the backward computed from the shapes.  Device pointers, torch's current stream; each figure is the
median over `--reps` timed blocks of `--steps` back-to-back calls between HIP events, after `--warmup` untimed calls.

    python tools/fk_vjp_bench.py [--n 1024] [--steps 50] [--warmup 10] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    return float(np.median(out)), [round(x, 2) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import SMPL, _ptr, _stream

    model = model_io.synthetic_model()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    n, V = a.n, s.vertex_num
    beta, theta = model_io.synthetic_inputs(n, seed=1)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    beta, theta = dev(beta), dev(theta)
    rng = np.random.default_rng(0)
    gv = dev(rng.standard_normal((n, V, 3)).astype(np.float32))
    verts = torch.empty((n, V, 3), device="cuda")
    joints = torch.empty((n, 24, 3), device="cuda")
    rest = torch.empty((n, V, 3), device="cuda")
    gb = torch.empty((n, 10), device="cuda")
    gt = torch.empty((n, 25, 3), device="cuda")
    L = _lib.load()
    h = s.handle
    _lib.check(L.smplpp_fk(h, n, _ptr(beta), _ptr(theta), None, None, None, _ptr(rest), _lib.DEVICE, _stream()))

    def fwd():
        _lib.check(L.smplpp_fk(h, n, _ptr(beta), _ptr(theta), _ptr(verts), _ptr(joints), None, None, _lib.DEVICE, _stream()))

    def bwd_rest():
        _lib.check(L.smplpp_fk_vjp(h, n, _ptr(beta), _ptr(theta), _ptr(rest), _ptr(gv), None, _ptr(gb), _ptr(gt), _lib.DEVICE, _stream()))

    def bwd_null():
        _lib.check(L.smplpp_fk_vjp(h, n, _ptr(beta), _ptr(theta), None, _ptr(gv), None, _ptr(gb), _ptr(gt), _lib.DEVICE, _stream()))

    t_f, r_f = _time(fwd, a.steps, a.warmup, a.reps)
    t_b, r_b = _time(bwd_rest, a.steps, a.warmup, a.reps)
    t_n, r_n = _time(bwd_null, a.steps, a.warmup, a.reps)
    K = 3 * V
    bytes_ = 2 * n * V * 3 * 4 + K * 224 * 4  # grad_verts + rest + the fp32 operand image
    flops = 2 * n * 217 * K  # the transposed blend GEMM
    print(json.dumps(dict(metric="fk_vjp_us", n=n, vertex_num=V, device=torch.cuda.get_device_name(0),
                          vjp_us_rest=round(t_b, 2), vjp_us_rest_null=round(t_n, 2), forward_us=round(t_f, 2),
                          ratio_vs_forward=round(t_b / t_f, 2), reps_us=dict(forward=r_f, vjp_rest=r_b, vjp_rest_null=r_n),
                          algorithmic_bytes=bytes_, gemm_flops=flops,
                          bytes_floor_us_at_8tbps=round(bytes_ / 8e12 * 1e6, 1),
                          gemm_floor_us_at_157tflops_fp32=round(flops / 157.3e12 * 1e6, 1),
                          steps=a.steps, warmup=a.warmup, reps=a.reps)))


if __name__ == "__main__":
    main()
