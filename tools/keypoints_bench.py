"""Timing of the keypoint term (smplpp_landmarks, smplpp_landmarks_vjp, smplpp_project_points, smplpp_project_points_vjp) on one
MI355X, synthetic 6890-vertex model, the 53-row regressor of tests/keypoints_oracle.py (24 joint picks, 24 rows of 30 vertices, 5
vertex picks).

At n = 1, 16 and 1024 frames, microseconds per call of
  - the regression and its backward (both outputs, accumulate = 0, preallocated),
  - the projection with its energy (uv, energy, valid) and its backward (grad_points and grad_camera; and grad_points alone, which
    runs one thread per point instead of one wavefront per frame), at K = 53 landmarks and at K = 6890 raw vertices,
next to
  - the byte floor of each call at 8 TB/s, computed from shapes: the regression reads 12 bytes per entry and frame and writes 12 per
    landmark, its backward reads the cotangents and writes every [n,V+24,3] element, both read the tables once; the projection moves
    37 bytes per point (point, target, uv, energy, valid) and its backward 48 (point, target, two cotangents, grad_points), both
    with 64 bytes of camera row per frame each way; and the ratio time / floor,
  - the same maths in torch on the same GPU in the same run, what a user would have written: a dense [53, V+24] einsum for the
    regression and elementwise fp32 for the projection, with autograd for the backward passes (those times include the graph's
    forward), reported with its relative difference from the library's results.
Device pointers, torch's current stream; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls
between HIP events, after `--warmup` untimed calls.  Prints one JSON line and writes it to --out.

    python tools/keypoints_bench.py [--steps 20] [--warmup 3] [--reps 3] [--no-torch] [--out profiles/keypoints_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from depth_raster_bench import PEAK, _time  # noqa: E402

import keypoints_oracle as KP  # noqa: E402
from smplpp_amd import _lib  # noqa: E402
from smplpp_amd.smpl import _ptr, _stream  # noqa: E402

SIZES = (1, 16, 1024)
RHO, NEAR = 100.0, 0.05


def torch_energy(points, camera, target):
    import torch

    uv, valid = KP.project_t(points, camera, NEAR)
    return torch.where(valid[..., None], uv, torch.zeros_like(uv)), KP.energy_t(uv, valid, target, RHO), valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keypoints_bench.json"))
    a = ap.parse_args()
    import torch

    from smplpp_amd import model_io
    from smplpp_amd.landmarks import Landmarks
    from smplpp_amd.smpl import SMPL

    model = model_io.synthetic_model()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    V = s.vertex_num
    reg = KP.regressor_53(model)
    lm = Landmarks(s, *reg)
    L, nnz, S = 53, len(reg[1]), V + 24
    A = torch.from_numpy(KP.dense(reg, S).astype(np.float32)).cuda()
    lib = _lib.load()
    us = lambda b: round(b / PEAK * 1e6, 5)  # noqa: E731
    rel = lambda x, y: float((x - y).norm() / y.norm().clamp(min=1e-30))  # noqa: E731
    t = lambda fn, torch_side=False: _time(fn, max(1, a.steps // 4) if torch_side else a.steps, 1 if torch_side else a.warmup, a.reps)  # noqa: E731
    rng = np.random.default_rng(0)
    res = {"model": "synthetic", "vertices": int(V), "landmarks": L, "nnz": nnz, "bytes_per_second": PEAK, "sizes": []}
    for n in SIZES:
        beta, theta = model_io.synthetic_inputs(n, seed=n + 1)
        theta[:, 0] = 0
        fk = s.launch(torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda(), want=("verts", "joints"))
        verts, joints = fk["verts"].clone(), fk["joints"].clone()
        cam = torch.from_numpy(np.tile(np.concatenate([np.diag([1.0, -1.0, -1.0]).reshape(9), [0.0, -0.36, 2.5], [500.0, 500.0, 320.0, 240.0]]),
                                       (n, 1)).astype(np.float32)).cuda()
        points, gv, gj = torch.empty(n, L, 3, device="cuda"), torch.empty(n, V, 3, device="cuda"), torch.empty(n, 24, 3, device="cuda")
        g = torch.from_numpy(rng.normal(size=(n, L, 3)).astype(np.float32)).cuda()

        def fwd():
            _lib.check(lib.smplpp_landmarks(lm.handle, n, _ptr(verts), _ptr(joints), _ptr(points), _lib.DEVICE, _stream()))

        def bwd():
            _lib.check(lib.smplpp_landmarks_vjp(lm.handle, n, _ptr(g), _ptr(gv), _ptr(gj), 0, _lib.DEVICE, _stream()))

        row = {"n": n}
        r = {"forward_us": t(fwd), "backward_us": t(bwd), "forward_floor_us": us(12 * n * (nnz + L) + 8 * nnz + 4 * (L + 1)),
             "backward_floor_us": us(12 * n * (S + L) + 8 * nnz + 4 * (S + 1))}
        if not a.no_torch:
            def bwd_torch():
                vv, jj = verts.clone().requires_grad_(True), joints.clone().requires_grad_(True)
                return torch.autograd.grad((KP.landmarks_t(A, vv, jj) * g).sum(), (vv, jj))

            r["torch_forward_rel_diff"] = rel(KP.landmarks_t(A, verts, joints), points)
            r["torch_backward_rel_diff"] = rel(bwd_torch()[0], gv)
            r["torch_forward_us"] = t(lambda: KP.landmarks_t(A, verts, joints), True)
            r["torch_backward_us"] = t(bwd_torch, True)
        row["landmarks"] = r
        for K, pts in ((L, points.clone()), (V, verts)):
            with torch.no_grad():
                uv_true, _ = KP.project_t(pts, cam, NEAR)
            target = torch.cat([uv_true + 5 * torch.randn_like(uv_true), torch.rand(n, K, 1, device="cuda")], -1).contiguous()
            uv, e, valid = torch.empty(n, K, 2, device="cuda"), torch.empty(n, K, device="cuda"), torch.empty(n, K, dtype=torch.uint8, device="cuda")
            guv, ge = torch.randn(n, K, 2, device="cuda"), torch.randn(n, K, device="cuda")
            gp, gc = torch.empty(n, K, 3, device="cuda"), torch.empty(n, 16, device="cuda")

            def pf():
                _lib.check(lib.smplpp_project_points(0, n, K, _ptr(pts), _ptr(cam), NEAR, _ptr(target), RHO, _ptr(uv), _ptr(e), _ptr(valid),
                                                     _lib.DEVICE, _stream()))

            def pb(camera=True):
                _lib.check(lib.smplpp_project_points_vjp(0, n, K, _ptr(pts), _ptr(cam), NEAR, _ptr(target), RHO, _ptr(guv), _ptr(ge), _ptr(gp),
                                                         _ptr(gc) if camera else None, 0, _lib.DEVICE, _stream()))

            r = {"forward_us": t(pf), "backward_us": t(pb), "backward_points_only_us": t(lambda: pb(False)),
                 "forward_floor_us": us(n * (37 * K + 64)), "backward_floor_us": us(n * (48 * K + 128))}
            if not a.no_torch:
                def pb_torch():
                    pp, cc = pts.clone().requires_grad_(True), cam.clone().requires_grad_(True)
                    u, en, _ = torch_energy(pp, cc, target)
                    return torch.autograd.grad((u * guv).sum() + (en * ge).sum(), (pp, cc))

                pb()
                tg = pb_torch()
                r["torch_energy_rel_diff"] = rel(torch_energy(pts, cam, target)[1], e)
                r["torch_grad_points_rel_diff"], r["torch_grad_camera_rel_diff"] = rel(tg[0], gp), rel(tg[1], gc)
                r["torch_forward_us"] = t(lambda: torch_energy(pts, cam, target), True)
                r["torch_backward_us"] = t(pb_torch, True)
            row["project_K%d" % K] = r
        for r in (v for k, v in row.items() if k != "n"):
            for kind in ("forward", "backward"):
                r[kind + "_over_floor"] = round(r[kind + "_us"] / max(r[kind + "_floor_us"], 1e-9), 1)
                if kind + "_us" in r and "torch_" + kind + "_us" in r:
                    r["torch_%s_over_%s" % (kind, kind)] = round(r["torch_" + kind + "_us"] / r[kind + "_us"], 1)
        res["sizes"].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
