"""Timing of the mesh-to-point distance (smplpp_mesh_point_distance and its VJP) on one MI355X, synthetic 6890-vertex model.

At each (n, K) of SIZES, with K points per frame sampled on the posed surface and moved up to +-15 mm along the face normal (the
scan-like case), microseconds per call of
  - the forward (index and sqdist of the nearest point of every vertex),
  - the backward (grad_verts and grad_points, accumulate 0),
  - torch.cdist(verts, points).min(-1) on the same inputs, where its [n, V, K] matrix fits in memory (for comparison);
at (16, 4096) also one two-sided fitting step smplpp_fk -> both distances forward and backward -> smplpp_fk_vjp, against the same
step with the point-to-mesh term alone.  Device pointers, torch's current stream; each figure is the median over `--reps` timed
blocks of `--steps` back-to-back calls between HIP events, after `--warmup` untimed calls.  Prints one JSON line and writes it to
--out.

    python tools/mesh_point_distance_bench.py [--steps 20] [--warmup 3] [--reps 3] [--out profiles/mesh_point_distance_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((1, 16384), (16, 4096), (64, 1024), (256, 64))
CDIST_MAX_BYTES = 4 << 30  # the [n, V, K] fp32 matrix torch.cdist builds


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
    return round(float(np.median(out)), 2)


def _points(verts, faces, K, rng, off):
    """[n,K,3] device points on the posed surface, moved up to +-off along the face normal."""
    import torch

    n = verts.shape[0]
    fid = torch.from_numpy(rng.integers(0, len(faces), (n, K))).cuda()
    w = torch.from_numpy(rng.dirichlet(np.ones(3), (n, K)).astype(np.float32)).cuda()
    tri = verts[torch.arange(n, device="cuda")[:, None, None], faces[fid]]  # [n,K,3,3]
    nrm = torch.nn.functional.normalize(torch.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1), dim=-1)
    s = torch.from_numpy(rng.uniform(-off, off, (n, K, 1)).astype(np.float32)).cuda()
    return ((w[..., None] * tri).sum(2) + s * nrm).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_point_distance_bench.json"))
    ap.add_argument("--no-cdist", action="store_true")
    a = ap.parse_args()
    import torch

    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import SMPL, _ptr, _stream

    model = model_io.synthetic_model()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    L = _lib.load()
    V = s.vertex_num
    faces = torch.from_numpy(s.getFaceIndex().astype(np.int64) - 1).cuda()
    rng = np.random.default_rng(0)
    T = lambda fn: _time(fn, a.steps, a.warmup, a.reps)  # noqa: E731

    def fwd(verts, P, idx, sq):
        n, K = P.shape[:2]
        return lambda: _lib.check(L.smplpp_mesh_point_distance(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(idx), _ptr(sq), _lib.DEVICE,
                                                               _stream()))

    def bwd(verts, P, idx, g, gv, gp, acc=0):
        n, K = P.shape[:2]
        return lambda: _lib.check(L.smplpp_mesh_point_distance_vjp(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(idx), _ptr(g), _ptr(gv),
                                                                   _ptr(gp), acc, _lib.DEVICE, _stream()))

    res = {}
    for n, K in SIZES:
        beta, theta = model_io.synthetic_inputs(n, seed=n)
        beta, theta = torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda()
        verts = s.launch(beta, theta, want=("verts",))["verts"]
        P = _points(verts, faces, K, rng, 0.015)
        idx, sq = torch.empty((n, V), dtype=torch.int64, device="cuda"), torch.empty((n, V), device="cuda")
        r = dict(forward_us=T(fwd(verts, P, idx, sq)))
        fwd(verts, P, idx, sq)()
        g = torch.from_numpy(rng.standard_normal((n, V)).astype(np.float32)).cuda()
        gv, gp = torch.empty((n, V, 3), device="cuda"), torch.empty((n, K, 3), device="cuda")
        r["backward_us"] = T(bwd(verts, P, idx, g, gv, gp))
        r["pairs"] = n * V * K
        r["pairs_per_ns"] = round(n * V * K / (r["forward_us"] * 1e3), 2)
        if not a.no_cdist and n * V * K * 4 <= CDIST_MAX_BYTES:
            ci = torch.cdist(verts, P).min(-1).indices
            torch.cuda.synchronize()
            r["cdist_min_us"] = T(lambda: torch.cdist(verts, P).min(-1))
            r["cdist_index_mismatch"] = int((ci != idx).sum())  # the matrix form's argmin is not exact
            r["forward_speedup_vs_cdist"] = round(r["cdist_min_us"] / r["forward_us"], 2)
        if (n, K) == (16, 4096):
            joints = torch.empty((n, 24, 3), device="cuda")
            rest = torch.empty((n, V, 3), device="cuda")
            gb, gt = torch.empty((n, 10), device="cuda"), torch.empty((n, 25, 3), device="cuda")
            face, w, cl, psq = (torch.empty((n, K), dtype=torch.int64, device="cuda"), torch.empty((n, K, 3), device="cuda"),
                                torch.empty((n, K, 3), device="cuda"), torch.empty((n, K), device="cuda"))
            gs = torch.full((n, K), 1.0 / (n * K), device="cuda")
            gm = torch.full((n, V), 1.0 / (n * V), device="cuda")

            def step(two_sided):
                def run():
                    _lib.check(L.smplpp_fk(s.handle, n, _ptr(beta), _ptr(theta), _ptr(verts), _ptr(joints), None, _ptr(rest), _lib.DEVICE,
                                           _stream()))
                    _lib.check(L.smplpp_point_mesh_distance(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(face), _ptr(w), None, _ptr(psq),
                                                            _lib.DEVICE, _stream()))
                    _lib.check(L.smplpp_point_mesh_distance_vjp(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(face), _ptr(gs), _ptr(gv),
                                                                None, 0, _lib.DEVICE, _stream()))
                    if two_sided:
                        fwd(verts, P, idx, sq)()
                        bwd(verts, P, idx, gm, gv, None, acc=1)()
                    _lib.check(L.smplpp_fk_vjp(s.handle, n, _ptr(beta), _ptr(theta), _ptr(rest), _ptr(gv), None, _ptr(gb), _ptr(gt),
                                               _lib.DEVICE, _stream()))

                return run

            r["fit_step_point_to_mesh_us"] = T(step(False))
            r["fit_step_two_sided_us"] = T(step(True))
            r["two_sided_over_one_sided"] = round(r["fit_step_two_sided_us"] / r["fit_step_point_to_mesh_us"], 3)
        res["%d,%d" % (n, K)] = r
    line = json.dumps(dict(metric="mesh_point_distance_us", device=torch.cuda.get_device_name(0), vertex_num=V, by_size=res, steps=a.steps,
                           warmup=a.warmup, reps=a.reps))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
