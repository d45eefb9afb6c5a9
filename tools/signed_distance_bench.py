"""Timing of the batched winding numbers and the signed point-to-mesh distance (smplpp_point_mesh_winding,
smplpp_point_mesh_signed_distance and its VJP) on one MI355X, synthetic 6890-vertex model.

At each (n, K) of SIZES, with K points per frame sampled on the posed surface and moved up to +-3 cm along the face normal (so that
both sides of the surface are sampled), microseconds per call of
  - the winding forward (winding and inside),
  - the signed-distance forward (face, weights, winding, inside, signed_sqdist) and, for comparison, the point-to-mesh forward alone,
  - the signed-distance backward (grad_verts and grad_points, accumulate 0) and the point-to-mesh backward alone,
  - the same winding formula in torch on the same inputs (fp32 terms, fp64 sum per chunk of points), with its largest difference;
at (16, 4096) also one fitting step with a penetration term: smplpp_fk -> signed forward -> signed backward -> smplpp_fk_vjp.
Device pointers, torch's current stream; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls
between HIP events, after `--warmup` untimed calls (the torch formula: one block of one call).  Prints one JSON line and writes it
to --out.

    python tools/signed_distance_bench.py [--steps 20] [--warmup 3] [--reps 3] [--out profiles/signed_distance_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((1, 16384), (16, 4096), (64, 1024), (256, 64))
TORCH_CHUNK_PAIRS = 1 << 24  # (point, face) pairs per chunk of the torch formula


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


def torch_winding(verts, faces, P):
    """The winding formula in torch: fp32 terms atan2(det, den), summed in fp64 over all faces, a chunk of points at a time."""
    import torch

    n, K = P.shape[:2]
    F = faces.shape[0]
    out = torch.empty((n, K), dtype=torch.float32, device=P.device)
    kc = max(1, TORCH_CHUNK_PAIRS // F)
    for f in range(n):
        tri = verts[f][faces]  # [F,3,3]
        for k0 in range(0, K, kc):
            d = tri[None] - P[f, k0:k0 + kc, None, None, :]  # [kc,F,3,3]
            a, b, c = d[:, :, 0], d[:, :, 1], d[:, :, 2]
            la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
            det = (a * torch.cross(b, c, dim=-1)).sum(-1)
            den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
            out[f, k0:k0 + kc] = (torch.atan2(det, den).double().sum(-1) / (2 * np.pi)).float()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signed_distance_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
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
    F = faces.shape[0]
    rng = np.random.default_rng(0)
    T = lambda fn: _time(fn, a.steps, a.warmup, a.reps)  # noqa: E731
    D = _lib.DEVICE

    res = {}
    for n, K in SIZES:
        beta, theta = model_io.synthetic_inputs(n, seed=n)
        beta, theta = torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda()
        verts = s.launch(beta, theta, want=("verts",))["verts"]
        P = _points(verts, faces, K, rng, 0.03)
        e = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda")  # noqa: E731
        wn, ins, face, w, sq, psq = e(n, K), e(n, K, dt=torch.uint8), e(n, K, dt=torch.int64), e(n, K, 3), e(n, K), e(n, K)
        g = torch.from_numpy(rng.standard_normal((n, K)).astype(np.float32)).cuda()
        gv, gp = e(n, V, 3), e(n, K, 3)

        def winding():
            _lib.check(L.smplpp_point_mesh_winding(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(wn), _ptr(ins), D, _stream()))

        def signed():
            _lib.check(L.smplpp_point_mesh_signed_distance(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(face), _ptr(w), None, _ptr(wn), _ptr(ins),
                                                           _ptr(sq), D, _stream()))

        def unsigned():
            _lib.check(L.smplpp_point_mesh_distance(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(face), _ptr(w), None, _ptr(psq), D, _stream()))

        def signed_vjp():
            _lib.check(L.smplpp_point_mesh_signed_distance_vjp(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(face), _ptr(ins), _ptr(g), _ptr(gv),
                                                               _ptr(gp), 0, D, _stream()))

        def unsigned_vjp():
            _lib.check(L.smplpp_point_mesh_distance_vjp(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(face), _ptr(g), _ptr(gv), _ptr(gp), 0, D,
                                                        _stream()))

        r = dict(winding_us=T(winding), signed_forward_us=T(signed), point_mesh_forward_us=T(unsigned))
        signed()
        r["signed_backward_us"] = T(signed_vjp)
        r["point_mesh_backward_us"] = T(unsigned_vjp)
        r["pairs"] = n * K * F
        r["winding_pairs_per_ns"] = round(n * K * F / (r["winding_us"] * 1e3), 2)
        r["signed_over_sum_of_parts"] = round(r["signed_forward_us"] / (r["winding_us"] + r["point_mesh_forward_us"]), 3)
        r["inside_fraction"] = round(float(ins.float().mean()), 3)
        if not a.no_torch:
            ref = torch_winding(verts, faces, P)
            torch.cuda.synchronize()
            r["torch_winding_us"] = _time(lambda: torch_winding(verts, faces, P), 1, 0, 1)
            winding()
            r["torch_winding_max_abs_diff"] = float((ref - wn).abs().max())
            r["winding_speedup_vs_torch"] = round(r["torch_winding_us"] / r["winding_us"], 1)
        if (n, K) == (16, 4096):
            joints, rest = e(n, 24, 3), e(n, V, 3)
            gb, gt = e(n, 10), e(n, 25, 3)
            gpen = e(n, K)

            def step():
                _lib.check(L.smplpp_fk(s.handle, n, _ptr(beta), _ptr(theta), _ptr(verts), _ptr(joints), None, _ptr(rest), D, _stream()))
                signed()
                torch.where(sq < 0, torch.full_like(sq, -1.0 / (n * K)), torch.zeros_like(sq), out=gpen)  # d/ds of mean(relu(-s))
                _lib.check(L.smplpp_point_mesh_signed_distance_vjp(s.handle, n, _ptr(verts), K, _ptr(P), _ptr(face), _ptr(ins), _ptr(gpen),
                                                                   _ptr(gv), None, 0, D, _stream()))
                _lib.check(L.smplpp_fk_vjp(s.handle, n, _ptr(beta), _ptr(theta), _ptr(rest), _ptr(gv), None, _ptr(gb), _ptr(gt), D, _stream()))

            r["fit_step_penetration_us"] = T(step)
        res["%d,%d" % (n, K)] = r
    line = json.dumps(dict(metric="signed_distance_us", device=torch.cuda.get_device_name(0), vertex_num=V, face_num=F, by_size=res,
                           steps=a.steps, warmup=a.warmup, reps=a.reps))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
