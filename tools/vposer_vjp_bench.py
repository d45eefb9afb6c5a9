"""Timing of smplpp_vposer_vjp (the VPoser decoder's backward pass) beside the decoder's forward calls, on one MI355X.

Prints one JSON line: microseconds per call at each n (default 512, configs[4]'s size, and 1024) of the VJP (its forward recompute
included), the value-only forward (smplpp_vposer_forward, jac NULL) and the Jacobian call (smplpp_vposer_forward with jac: what a
J^T g workaround needs), on the synthetic decoder, plus the backward's algorithmic FLOPs and weight bytes from the shapes.  Device
pointers, torch's current stream; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls between HIP
events, after `--warmup` untimed calls.

    python tools/vposer_vjp_bench.py [--n 512 1024] [--steps 50] [--warmup 10] [--reps 5]
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
    ap.add_argument("--n", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    from smplpp_amd import _lib
    from smplpp_amd.ik import VPoserDecoder
    from smplpp_amd.smpl import _ptr, _stream

    v = VPoserDecoder(VPoserDecoder.synthetic_params())
    L = _lib.load()
    h = v._h
    res = {}
    for n in a.n:
        rng = np.random.default_rng(n)
        z = torch.from_numpy(rng.normal(0, 1.0, (n, 32)).astype(np.float32)).cuda()
        g = torch.from_numpy(rng.standard_normal((n, 21, 3)).astype(np.float32)).cuda()
        out = torch.empty((n, 21, 3), device="cuda")
        jac = torch.empty((n, 63, 32), device="cuda")
        gz = torch.empty((n, 32), device="cuda")

        def vjp():
            _lib.check(L.smplpp_vposer_vjp(h, n, 0, _ptr(z), _ptr(g), _ptr(gz), None, _lib.DEVICE, _stream()))

        def value():
            _lib.check(L.smplpp_vposer_forward(h, n, _ptr(z), _ptr(out), None, _lib.DEVICE, _stream()))

        def jacobian():
            _lib.check(L.smplpp_vposer_forward(h, n, _ptr(z), _ptr(out), _ptr(jac), _lib.DEVICE, _stream()))

        t_v, r_v = _time(vjp, a.steps, a.warmup, a.reps)
        t_f, r_f = _time(value, a.steps, a.warmup, a.reps)
        t_j, r_j = _time(jacobian, a.steps, a.warmup, a.reps)
        tiles = (n + 7) // 8
        res[str(n)] = dict(vjp_us=round(t_v, 2), value_forward_us=round(t_f, 2), jacobian_us=round(t_j, 2),
                           vjp_over_jacobian=round(t_v / t_j, 3), reps_us=dict(vjp=r_v, value_forward=r_f, jacobian=r_j),
                           backward_gemm_flops=2 * n * (126 * 512 + 512 * 512 + 512 * 32),
                           backward_weight_bytes_from_l2=tiles * 4 * (126 * 512 + 512 * 512 + 512 * 32))
    print(json.dumps(dict(metric="vposer_vjp_us", device=torch.cuda.get_device_name(0), frames_per_workgroup=8, by_n=res,
                          steps=a.steps, warmup=a.warmup, reps=a.reps)))


if __name__ == "__main__":
    main()
