"""Timing of smplpp_vposer_jacobian (the VPoser decoder's Jacobian in exact fp32) beside smplpp_vposer_forward with jac (the fp16x2
Jacobian kernel), alternated on one MI355X; and, where the IK solver has the exact-arithmetic mode, microseconds per IK iteration in
the default and exact modes.

Prints one JSON line.  Decoder: microseconds per call at each n, the two calls alternated block by block, on the synthetic decoder,
with the hot kernel's floor from the shapes (512 x 512 x 32 MACs per frame on v_mfma_f32_32x32x2_f32 at 157 TF).  Device pointers,
torch's current stream; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls between HIP events,
after `--warmup` untimed calls.

    python tools/vposer_jac_exact_bench.py [--n 8 64 512 1024] [--steps 50] [--warmup 10] [--reps 5] [--no-ik]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _block(fn, steps):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps


def _alternate(fns, steps, warmup, reps):
    """Median microseconds per call of each of `fns`, their timed blocks interleaved."""
    import torch

    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            out[i].append(_block(fn, steps))
    return [(float(np.median(o)), [round(x, 2) for x in o]) for o in out]


def decoder(a):
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
        out = torch.empty((n, 21, 3), device="cuda")
        jac = torch.empty((n, 63, 32), device="cuda")
        gz = torch.empty((n, 32), device="cuda")
        g = torch.zeros((n, 21, 3), device="cuda")

        def exact():
            _lib.check(L.smplpp_vposer_jacobian(h, n, 0, _ptr(z), _ptr(out), _ptr(jac), _lib.DEVICE, _stream()))

        def fp16x2():
            _lib.check(L.smplpp_vposer_forward(h, n, _ptr(z), _ptr(out), _ptr(jac), _lib.DEVICE, _stream()))

        def value():
            _lib.check(L.smplpp_vposer_forward(h, n, _ptr(z), _ptr(out), None, _lib.DEVICE, _stream()))

        def vjp():
            _lib.check(L.smplpp_vposer_vjp(h, n, 0, _ptr(z), _ptr(g), _ptr(gz), None, _lib.DEVICE, _stream()))

        (t_x, r_x), (t_j, r_j), (t_v, r_v), (t_b, r_b) = _alternate([exact, fp16x2, value, vjp], a.steps, a.warmup, a.reps)
        flops = 2 * n * 512 * 512 * 32
        res[str(n)] = dict(exact_jacobian_us=round(t_x, 2), fp16x2_jacobian_us=round(t_j, 2), value_forward_us=round(t_v, 2),
                           vjp_us=round(t_b, 2), exact_over_fp16x2=round(t_x / t_j, 3),
                           reps_us=dict(exact=r_x, fp16x2=r_j, value_forward=r_v, vjp=r_b),
                           layer1_flops=flops, layer1_floor_us_fp32_mfma=round(flops / 157.3e12 * 1e6, 2))
    return dict(by_n=res, device=torch.cuda.get_device_name(0))


def ik(a):
    """us per iteration (smplpp_ik_iterate, QP on) in both modes, blocks alternated: configs[2] (256 direct frames x 6 tasks) and
    configs[4] (512 latent frames x 6 tasks)."""
    from smplpp_amd import model_io
    from smplpp_amd.ik import IkSolver, VPoserDecoder, reference_task_faces
    from smplpp_amd.smpl import SMPL

    model = model_io.synthetic_model()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    vp = VPoserDecoder(VPoserDecoder.synthetic_params())
    K = 6
    _, faces = reference_task_faces(K)
    out = {}
    for name, n, latent in (("configs2_direct_256x6", 256, False), ("configs4_latent_512x6", 512, True)):
        rng = np.random.default_rng(n)
        theta = np.zeros((n, 44 if latent else 75), np.float32)
        if latent:
            theta[:, 6:38] = rng.normal(0, 0.5, (n, 32))
        else:
            theta[:, 3:] = rng.normal(0, 0.1, (n, 72))
        tp = rng.normal(0, 0.3, (n, K, 3)).astype(np.float32)
        row = {}
        fns = []
        for exact in (False, True):
            sol = IkSolver(s, n, K, vp if latent else None, exact=exact)
            sol.setTasks(face_idx=np.broadcast_to(faces, (n, K)).copy(), target_pos=tp)
            sol.setConfig(np.zeros((n, 10), np.float32), theta)

            def step(sol=sol):
                sol.iterate(1, enable_qp=True, sync=False)

            fns.append((("exact" if exact else "default"), sol, step))
        res = _alternate([f[2] for f in fns], a.ik_steps, a.warmup, a.reps)
        for (mode, _, _), (t, r) in zip(fns, res):
            row[mode + "_us_per_iter"] = round(t, 2)
            row[mode + "_reps_us"] = r
        row["exact_over_default"] = round(row["exact_us_per_iter"] / row["default_us_per_iter"], 3)
        out[name] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[8, 64, 512, 1024])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--ik-steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-ik", action="store_true")
    a = ap.parse_args()
    res = dict(metric="vposer_jacobian_exact_us", decoder=decoder(a), steps=a.steps, warmup=a.warmup, reps=a.reps)
    if not a.no_ik:
        res["ik"] = ik(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
