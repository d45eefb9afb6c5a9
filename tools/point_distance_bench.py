"""Timing of the point-to-mesh distance (smplpp_point_mesh_distance and its VJP) on one MI355X, synthetic 6890-vertex model.

At each (n, K) of SIZES, with K points per frame sampled on the posed surface and moved up to +-15 mm along the face normal (the
scan-like case), microseconds per call of
  - the forward in the dispatch's form, and in each form forced (SMPLPP_POINT_DISTANCE_FORM = query | tiled, one model each),
  - smplpp_closest_points on the same inputs,
  - the backward (grad_verts and grad_points, accumulate 0);
at (16, 4096) also the forward and smplpp_closest_points with every point 0.25 m off the surface (the cull's bad case), and one
whole fitting step smplpp_fk -> distance forward -> distance VJP -> smplpp_fk_vjp; and the forward of both forms at small K (the
dispatch's crossover).  Device pointers, torch's current stream; each figure is the median over `--reps` timed blocks of `--steps`
back-to-back calls between HIP events, after `--warmup` untimed calls.  Prints one JSON line and writes it to --out.

    python tools/point_distance_bench.py [--steps 20] [--warmup 3] [--reps 3] [--out profiles/point_distance_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((1, 16384), (16, 4096), (64, 1024), (256, 64))


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


def _model(model, form):
    from smplpp_amd.smpl import SMPL

    if form:
        os.environ["SMPLPP_POINT_DISTANCE_FORM"] = form
    try:
        s = SMPL()
        s.setDevice("cuda:0")
        s.init(model)
    finally:
        os.environ.pop("SMPLPP_POINT_DISTANCE_FORM", None)
    return s


def _points(verts, faces, K, rng, off):
    """[n,K,3] device points on the posed surface, moved up to +-off (or exactly `off` when far) along the face normal."""
    import torch

    n = verts.shape[0]
    fid = torch.from_numpy(rng.integers(0, len(faces), (n, K))).cuda()
    w = torch.from_numpy(rng.dirichlet(np.ones(3), (n, K)).astype(np.float32)).cuda()
    tri = verts[torch.arange(n, device="cuda")[:, None, None], faces[fid]]  # [n,K,3,3]
    nrm = torch.nn.functional.normalize(torch.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1), dim=-1)
    s = torch.from_numpy(rng.uniform(-off, off, (n, K, 1)).astype(np.float32)).cuda() if off < 0.1 else off
    return ((w[..., None] * tri).sum(2) + s * nrm).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_distance_bench.json"))
    ap.add_argument("--no-crossover", action="store_true")
    a = ap.parse_args()
    import torch

    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import _ptr, _stream

    model = model_io.synthetic_model()
    ms = {f: _model(model, f) for f in ("", "query", "tiled")}
    s = ms[""]
    L = _lib.load()
    V = s.vertex_num
    faces = torch.from_numpy(s.getFaceIndex().astype(np.int64) - 1).cuda()
    rng = np.random.default_rng(0)
    T = lambda fn: _time(fn, a.steps, a.warmup, a.reps)  # noqa: E731

    def fwd(m, verts, P, out):
        n, K = P.shape[:2]
        return lambda: _lib.check(L.smplpp_point_mesh_distance(m.handle, n, _ptr(verts), K, _ptr(P), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                                                               _ptr(out[3]), _lib.DEVICE, _stream()))

    def cp(verts, P, out):
        n, K = P.shape[:2]
        return lambda: _lib.check(L.smplpp_closest_points(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(out[0]), _ptr(out[2]), _ptr(out[3]),
                                                          _lib.DEVICE, _stream()))

    def outs(n, K):
        return (torch.empty((n, K), dtype=torch.int64, device="cuda"), torch.empty((n, K, 3), device="cuda"),
                torch.empty((n, K, 3), device="cuda"), torch.empty((n, K), device="cuda"))

    res = {}
    for n, K in SIZES:
        beta, theta = model_io.synthetic_inputs(n, seed=n)
        beta, theta = torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda()
        verts = s.launch(beta, theta, want=("verts",))["verts"]
        P = _points(verts, faces, K, rng, 0.015)
        o = outs(n, K)
        r = dict(forward_us=T(fwd(s, verts, P, o)), forward_query_us=T(fwd(ms["query"], verts, P, o)),
                 forward_tiled_us=T(fwd(ms["tiled"], verts, P, o)), closest_points_us=T(cp(verts, P, o)))
        fwd(s, verts, P, o)()
        g = torch.from_numpy(rng.standard_normal((n, K)).astype(np.float32)).cuda()
        gv, gp = torch.empty((n, V, 3), device="cuda"), torch.empty((n, K, 3), device="cuda")
        r["backward_us"] = T(lambda: _lib.check(L.smplpp_point_mesh_distance_vjp(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(o[0]), _ptr(g),
                                                                                 _ptr(gv), _ptr(gp), 0, _lib.DEVICE, _stream())))
        r["backward_over_forward"] = round(r["backward_us"] / r["forward_us"], 3)
        r["forward_speedup_vs_closest_points"] = round(r["closest_points_us"] / r["forward_us"], 2)
        if (n, K) == (16, 4096):
            Pf = _points(verts, faces, K, rng, 0.25)
            r["far_0.25m"] = dict(forward_us=T(fwd(s, verts, Pf, o)), closest_points_us=T(cp(verts, Pf, o)))
            joints = torch.empty((n, 24, 3), device="cuda")
            rest = torch.empty((n, V, 3), device="cuda")
            gb, gt = torch.empty((n, 10), device="cuda"), torch.empty((n, 25, 3), device="cuda")
            gs = torch.full((n, K), 1.0 / (n * K), device="cuda")

            def step():
                _lib.check(L.smplpp_fk(s.handle, n, _ptr(beta), _ptr(theta), _ptr(verts), _ptr(joints), None, _ptr(rest), _lib.DEVICE,
                                       _stream()))
                fwd(s, verts, P, o)()
                _lib.check(L.smplpp_point_mesh_distance_vjp(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(o[0]), _ptr(gs), _ptr(gv), None, 0,
                                                            _lib.DEVICE, _stream()))
                _lib.check(L.smplpp_fk_vjp(s.handle, n, _ptr(beta), _ptr(theta), _ptr(rest), _ptr(gv), None, _ptr(gb), _ptr(gt),
                                           _lib.DEVICE, _stream()))

            r["fit_step_us"] = T(step)
        res["%d,%d" % (n, K)] = r
    cross = {}
    if not a.no_crossover:
        for n in (1, 16):
            beta, theta = model_io.synthetic_inputs(n, seed=7)
            verts = s.launch(torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda(), want=("verts",))["verts"]
            for K in (1, 16, 64, 128, 256, 512, 1024):
                P = _points(verts, faces, K, rng, 0.015)
                o = outs(n, K)
                cross["%d,%d" % (n, K)] = dict(query_us=T(fwd(ms["query"], verts, P, o)), tiled_us=T(fwd(ms["tiled"], verts, P, o)))
    line = json.dumps(dict(metric="point_distance_us", device=torch.cuda.get_device_name(0), vertex_num=V, face_num=s.face_num, by_size=res,
                           crossover=cross, steps=a.steps, warmup=a.warmup, reps=a.reps))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
