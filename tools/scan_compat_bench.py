"""Timing of the normal-compatible, distance-capped correspondences (smplpp_point_mesh_distance_compatible and
smplpp_mesh_point_distance_compatible) against the unfiltered smplpp_point_mesh_distance / smplpp_mesh_point_distance on the same
inputs in the same session, one MI355X, synthetic 6890-vertex model.

At each (n, K) of SIZES, K points per frame are sampled on the posed surface, moved up to +-15 mm along the face normal and given
that face's normal (the scan-like case); the mesh side uses the whole-mesh vertex normals.  Microseconds per call of the two
unfiltered forwards and, for cos_min in COS_MIN and max_dist in MAX_DIST, of the two filtered ones, with the share of matched
queries / vertices.  Device pointers, torch's current stream.  Each figure is the median over `--reps` timed blocks of `--steps`
back-to-back calls between HIP events, after `--warmup` untimed calls; within a repetition the unfiltered and the filtered calls
take turns, so a drift of the shared host falls on both.  Prints one JSON line and writes it to --out.

    python tools/scan_compat_bench.py [--steps 10] [--warmup 2] [--reps 5] [--out profiles/scan_compat_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((16, 4096), (64, 1024), (1, 16384), (256, 64))
COS_MIN = (0.0, 0.5)
MAX_DIST = (None, 0.05)  # no cap; 5 cm


def _time_alternating(fns, steps, warmup, reps):
    """Median microseconds per call of each of `fns`, their timed blocks interleaved within every repetition."""
    import torch

    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            e1.synchronize()
            out[i].append(e0.elapsed_time(e1) * 1e3 / steps)
    return [round(float(np.median(o)), 2) for o in out]


def _scan(verts, faces, K, rng, off):
    """([n,K,3] points, [n,K,3] normals) on the device: surface samples moved up to +-off along their face's unit normal."""
    import torch

    n = verts.shape[0]
    fid = torch.from_numpy(rng.integers(0, len(faces), (n, K))).cuda()
    w = torch.from_numpy(rng.dirichlet(np.ones(3), (n, K)).astype(np.float32)).cuda()
    tri = verts[torch.arange(n, device="cuda")[:, None, None], faces[fid]]  # [n,K,3,3]
    nrm = torch.nn.functional.normalize(torch.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1), dim=-1)
    s = torch.from_numpy(rng.uniform(-off, off, (n, K, 1)).astype(np.float32)).cuda()
    return ((w[..., None] * tri).sum(2) + s * nrm).contiguous(), nrm.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_compat_bench.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("scan_compat_bench: no GPU; nothing is measured without one")
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
    res = {}
    for n, K in SIZES:
        beta, theta = model_io.synthetic_inputs(n, seed=n)
        verts = s.launch(torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda(), want=("verts",))["verts"]
        P, N = _scan(verts, faces, K, rng, 0.015)
        vn = torch.empty((n, V, 3), device="cuda")
        _lib.check(L.smplpp_mesh_vertex_normals(s.handle, n, _ptr(verts), _ptr(vn), _lib.DEVICE, _stream()))
        face, w, sq = torch.empty((n, K), dtype=torch.int64, device="cuda"), torch.empty((n, K, 3), device="cuda"), torch.empty((n, K), device="cuda")
        idx, vsq = torch.empty((n, V), dtype=torch.int64, device="cuda"), torch.empty((n, V), device="cuda")

        def pm_plain():
            _lib.check(L.smplpp_point_mesh_distance(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(face), _ptr(w), None, _ptr(sq), _lib.DEVICE,
                                                    _stream()))

        def mp_plain():
            _lib.check(L.smplpp_mesh_point_distance(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(idx), _ptr(vsq), _lib.DEVICE, _stream()))

        def pm_compat(cm, cap):
            return lambda: _lib.check(L.smplpp_point_mesh_distance_compatible(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(N), cm, cap, _ptr(face),
                                                                              _ptr(w), None, _ptr(sq), _lib.DEVICE, _stream()))

        def mp_compat(cm, cap):
            return lambda: _lib.check(L.smplpp_mesh_point_distance_compatible(s.handle, n, _ptr(verts), _ptr(vn), K, _ptr(P), _ptr(N), cm, cap,
                                                                              _ptr(idx), _ptr(vsq), _lib.DEVICE, _stream()))

        cases = [(cm, md) for cm in COS_MIN for md in MAX_DIST]
        caps = [float("inf") if md is None else float(np.float32(md) * np.float32(md)) for _, md in cases]
        pm = _time_alternating([pm_plain] + [pm_compat(cm, cap) for (cm, _), cap in zip(cases, caps)], a.steps, a.warmup, a.reps)
        mp = _time_alternating([mp_plain] + [mp_compat(cm, cap) for (cm, _), cap in zip(cases, caps)], a.steps, a.warmup, a.reps)
        r = dict(point_mesh_us=pm[0], mesh_point_us=mp[0], filtered=[])
        for i, ((cm, md), cap) in enumerate(zip(cases, caps)):
            pm_compat(cm, cap)()
            mp_compat(cm, cap)()
            torch.cuda.synchronize()
            r["filtered"].append(dict(cos_min=cm, max_dist=md, point_mesh_us=pm[i + 1], point_mesh_over_plain=round(pm[i + 1] / pm[0], 3),
                                      point_mesh_matched=round(float((face >= 0).float().mean()), 4), mesh_point_us=mp[i + 1],
                                      mesh_point_over_plain=round(mp[i + 1] / mp[0], 3),
                                      mesh_point_matched=round(float((idx >= 0).float().mean()), 4)))
        res["%d,%d" % (n, K)] = r
    line = json.dumps(dict(metric="scan_compat_us", device=torch.cuda.get_device_name(0), vertex_num=V, face_num=int(len(faces)), by_size=res,
                           steps=a.steps, warmup=a.warmup, reps=a.reps))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
