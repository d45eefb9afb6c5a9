"""Timing of the SMPL+D layer (smplpp_vertex_offsets, smplpp_vertex_offsets_vjp, smplpp_mesh_laplacian) on one MI355X, synthetic
6890-vertex model.

At n = 16, 256 and 1024 frames, with per-frame offsets [n,V,3] and with one shared field [1,V,3], microseconds per call of
  - the forward and the backward to the offsets, both into a preallocated output (the backward through the C entry point with
    accumulate = 0, since the binding's `out` means accumulate), so the two columns are like for like,
  - the Laplacian of one field [1,V,3] (what a shared D costs per step),
next to
  - the byte floor of each call at 8 TB/s: 12 n V bytes per [n,V,3] array it must move (forward: verts in, verts out, and the
    offsets when they are per frame; backward: grad_verts in, and grad_offsets out when it is per frame), and the ratio time / floor,
  - smplpp_fk (verts, joints, xforms, rest) on the same frames, GPU and run: what SMPL+D adds to a step,
  - the same rule in torch on the same GPU, what a user would have written: M = einsum over the dense weights, delta = M d / wSum,
    and autograd of it for the backward (the time includes that graph's forward).  Reported with its relative difference from
    the library's results.
Device pointers, torch's current stream; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls
between HIP events, after `--warmup` untimed calls.  Prints one JSON line and writes it to --out.

    python tools/vertex_offsets_bench.py [--steps 20] [--warmup 3] [--reps 3] [--no-torch] [--out profiles/vertex_offsets_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from depth_raster_bench import PEAK, _time  # noqa: E402

from smplpp_amd import _lib  # noqa: E402
from smplpp_amd.smpl import _ptr, _stream  # noqa: E402

SIZES = (16, 256, 1024)


def torch_forward(W, wsum, verts, xforms, d):
    import torch

    M = torch.einsum("vj,njab->nvab", W, xforms[:, :, :3, :3])
    return verts + torch.einsum("nvab,nvb->nva", M, d.expand_as(verts)) / wsum[None, :, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vertex_offsets_bench.json"))
    a = ap.parse_args()
    import torch

    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    model = model_io.synthetic_model()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    V = s.vertex_num
    W = torch.from_numpy(model["weights"].astype(np.float32)).cuda()
    wsum = W.sum(1)
    rng = np.random.default_rng(0)
    res = {"model": "synthetic", "vertices": int(V), "bytes_per_second": PEAK, "sizes": []}
    rel = lambda x, y: float((x - y).norm() / y.norm().clamp(min=1e-30))  # noqa: E731
    field = torch.from_numpy(rng.normal(0, 0.01, (1, V, 3)).astype(np.float32)).cuda()
    res["laplacian_1xVx3_us"] = _time(lambda: s.meshLaplacian(field), a.steps, a.warmup, a.reps)
    for n in SIZES:
        beta, theta = model_io.synthetic_inputs(n, seed=n)
        beta, theta = torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda()
        fk_out = {k: torch.empty(shape, device="cuda") for k, shape in
                  (("verts", (n, V, 3)), ("joints", (n, 24, 3)), ("xforms", (n, 24, 4, 4)), ("rest", (n, V, 3)))}
        fk = lambda: s.launch(beta, theta, out=fk_out)  # noqa: E731
        fk()
        verts, xforms = fk_out["verts"].clone(), fk_out["xforms"].clone()
        g = torch.from_numpy(rng.normal(size=(n, V, 3)).astype(np.float32)).cuda()
        out = torch.empty_like(verts)
        row = {"n": n, "fk_us": _time(fk, a.steps, a.warmup, a.reps)}
        for kind, d, arrays_f, arrays_b in (("per_frame", torch.from_numpy(rng.normal(0, 0.01, (n, V, 3)).astype(np.float32)).cuda(), 3, 2),
                                            ("shared", field, 2, 1)):
            shared = kind == "shared"
            go = torch.empty((1 if shared else n, V, 3), device="cuda")
            frames = go.shape[0]

            def bwd():
                _lib.check(_lib.load().smplpp_vertex_offsets_vjp(s.handle, n, _ptr(xforms), _ptr(g), frames, _ptr(go), 0, _lib.DEVICE, _stream()))

            r = {"forward_us": _time(lambda: s.vertexOffsets(verts, xforms, d, out=out), a.steps, a.warmup, a.reps),
                 "backward_us": _time(bwd, a.steps, a.warmup, a.reps),
                 "forward_floor_us": round(arrays_f * n * V * 12 / PEAK * 1e6, 2), "backward_floor_us": round(arrays_b * n * V * 12 / PEAK * 1e6, 2)}
            r["forward_over_floor"] = round(r["forward_us"] / r["forward_floor_us"], 1)
            r["backward_over_floor"] = round(r["backward_us"] / r["backward_floor_us"], 1)
            r["forward_over_fk"] = round(r["forward_us"] / row["fk_us"], 3)
            if not a.no_torch:
                def bwd_torch():
                    dd = d.clone().requires_grad_(True)
                    return torch.autograd.grad((torch_forward(W, wsum, verts, xforms, dd) * g).sum(), dd)[0]

                r["torch_forward_rel_diff"] = rel(torch_forward(W, wsum, verts, xforms, d), s.vertexOffsets(verts, xforms, d))
                r["torch_backward_rel_diff"] = rel(bwd_torch(), s.vertexOffsetsBackward(xforms, g, shared=shared))
                r["torch_forward_us"] = _time(lambda: torch_forward(W, wsum, verts, xforms, d), max(1, a.steps // 4), 1, a.reps)
                r["torch_backward_us"] = _time(bwd_torch, max(1, a.steps // 4), 1, a.reps)
                r["torch_forward_over_forward"] = round(r["torch_forward_us"] / r["forward_us"], 1)
                r["torch_backward_over_backward"] = round(r["torch_backward_us"] / r["backward_us"], 1)
            row[kind] = r
        res["sizes"].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
