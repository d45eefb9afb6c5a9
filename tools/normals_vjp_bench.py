"""Timing of the normals' vector-Jacobian products beside the whole-mesh vertex-normal forward, on one MI355X.

Prints one JSON line: microseconds per call at each n (default 256 and 1024) on the synthetic 6890-vertex model of
  - smplpp_mesh_vertex_normals_vjp (accumulate 0 and 1; on-chip form, and the staged form via SMPLPP_NORMALS_VJP_STAGED=1),
  - smplpp_mesh_vertex_normals (the forward),
  - smplpp_vertex_normals_vjp on a K = 41-task list (the 123 vertices of 41 faces) with accumulate = 1,
with the HBM fraction on algorithmic bytes (verts, grad_normals and grad_verts once each: 3 n V 3 4 B, plus one more n V 3 4 B read
when accumulating; the forward: 2 n V 3 4 B) against 8 TB/s.  Device pointers, torch's current stream; each figure is the median
over `--reps` timed blocks of `--steps` back-to-back calls between HIP events, after `--warmup` untimed calls.

    python tools/normals_vjp_bench.py [--n 256 1024] [--steps 50] [--warmup 10] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8.0e12


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
    ap.add_argument("--n", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import SMPL, _ptr, _stream

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model_io.synthetic_model())
    V = s.vertex_num
    L = _lib.load()
    h = s.handle
    rng = np.random.default_rng(0)
    faces41 = rng.choice(s.face_num, 41, replace=False)
    ids = torch.from_numpy((s.getFaceIndex()[faces41].astype(np.int64) - 1).reshape(-1)).cuda()  # 123 vertex ids
    res = {}
    for n in a.n:
        beta, theta = model_io.synthetic_inputs(n, seed=n)
        verts = s.launch(torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda(), want=("verts",))["verts"]
        g = torch.from_numpy(rng.standard_normal((n, V, 3)).astype(np.float32)).cuda()
        gl = torch.from_numpy(rng.standard_normal((n, ids.numel(), 3)).astype(np.float32)).cuda()
        gv = torch.zeros((n, V, 3), device="cuda")
        nrm = torch.empty((n, V, 3), device="cuda")

        def mesh_vjp(acc):
            return lambda: _lib.check(L.smplpp_mesh_vertex_normals_vjp(h, n, _ptr(verts), _ptr(g), _ptr(gv), acc, _lib.DEVICE, _stream()))

        def forward():
            _lib.check(L.smplpp_mesh_vertex_normals(h, n, _ptr(verts), _ptr(nrm), _lib.DEVICE, _stream()))

        def list_vjp():
            _lib.check(L.smplpp_vertex_normals_vjp(h, n, _ptr(verts), ids.numel(), _ptr(ids), _ptr(gl), _ptr(gv), 1, _lib.DEVICE, _stream()))

        t0, r0 = _time(mesh_vjp(0), a.steps, a.warmup, a.reps)
        t1, r1 = _time(mesh_vjp(1), a.steps, a.warmup, a.reps)
        tf, rf = _time(forward, a.steps, a.warmup, a.reps)
        tl, rl = _time(list_vjp, a.steps, a.warmup, a.reps)
        os.environ["SMPLPP_NORMALS_VJP_STAGED"] = "1"
        ts, rs = _time(mesh_vjp(0), a.steps, a.warmup, a.reps)
        del os.environ["SMPLPP_NORMALS_VJP_STAGED"]
        slab = n * V * 3 * 4
        frac = lambda b, us: round(b / (us * 1e-6) / HBM_BPS, 3)
        res[str(n)] = dict(mesh_vjp_us=round(t0, 2), mesh_vjp_accumulate_us=round(t1, 2), mesh_vjp_staged_us=round(ts, 2),
                           mesh_forward_us=round(tf, 2), list123_vjp_accumulate_us=round(tl, 2),
                           mesh_vjp_over_list123=round(t1 / tl, 2),
                           algorithmic_bytes=dict(mesh_vjp=3 * slab, mesh_vjp_accumulate=4 * slab, mesh_forward=2 * slab),
                           hbm_fraction=dict(mesh_vjp=frac(3 * slab, t0), mesh_vjp_accumulate=frac(4 * slab, t1),
                                             mesh_vjp_staged=frac(3 * slab, ts), mesh_forward=frac(2 * slab, tf)),
                           reps_us=dict(mesh_vjp=r0, mesh_vjp_accumulate=r1, mesh_vjp_staged=rs, mesh_forward=rf, list123_vjp=rl))
    print(json.dumps(dict(metric="normals_vjp_us", device=torch.cuda.get_device_name(0), vertex_num=V, by_n=res, steps=a.steps,
                          warmup=a.warmup, reps=a.reps)))


if __name__ == "__main__":
    main()
