"""Timing of the alignment of point sets (smplpp_align, smplpp_align_vjp) on one MI355X.

Five cases (n, K): joints (1024, 24), landmarks (1024, 53), whole meshes (1024, 6890) and (16, 6890), and one large cloud (1, 100000).
Similarity mode, per-frame targets and weights, every frame sound.  Every call goes through the bare C entry point with device pointers,
in `--reps` blocks of `--steps` back-to-back calls between HIP events after `--warmup` blocks, in one session.  Reported per case, for
the forward (every output) and the backward (the three cotangents, both gradients):
  - us: the median block, microseconds per call, with the least and the greatest block;
  - floor_us and over_floor: the bytes the call must move at 8 TB/s: source, target and weight read once, the outputs written once (for
    the backward the cotangents read once and both gradients written once).  A frame is one workgroup (a wavefront up to K = 64), which
    passes over its points three times (four in the backward): with few frames and many points the call is far above this floor;
  - torch_us: the same mathematics in torch on the same GPU: batched weighted Kabsch / Umeyama through torch.linalg.svd, and autograd
    of it for the backward.  The backward figure is forward plus backward on both sides: smplpp_align_vjp recomputes its forward, and
    autograd runs the forward it differentiates.
Prints one JSON line and writes it to --out.

    python tools/align_bench.py [--steps 50] [--warmup 2] [--reps 5] [--out profiles/align_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from depth_raster_bench import PEAK  # noqa: E402
from lbfgs_bench import blocks  # noqa: E402

from smplpp_amd import _lib  # noqa: E402
from smplpp_amd.smpl import _stream  # noqa: E402

CASES = ((1024, 24), (1024, 53), (1024, 6890), (16, 6890), (1, 100000))
MIN_GAP = 1e-3


def timed(fn, a, steps):
    for _ in range(a.warmup):
        blocks(lambda k: fn(), steps, 1)
    return blocks(lambda k: fn(), steps, a.reps)


def kabsch(x, y, w):
    """(transform pieces, aligned, energy) by the SVD definition, similarity mode."""
    import torch

    W = w.sum(1)
    cx, cy = (w[..., None] * x).sum(1) / W[:, None], (w[..., None] * y).sum(1) / W[:, None]
    xt, yt = x - cx[:, None], y - cy[:, None]
    C = torch.einsum("nk,nka,nkb->nab", w, yt, xt)
    U, sig, Vh = torch.linalg.svd(C)
    fix = torch.ones_like(sig)
    fix[:, 2] = torch.sign(torch.det(U @ Vh))
    R = U @ torch.diag_embed(fix) @ Vh
    s = (sig * fix).sum(1) / (w * (xt * xt).sum(-1)).sum(1)
    t = cy - s[:, None] * torch.einsum("nab,nb->na", R, cx)
    aligned = s[:, None, None] * torch.einsum("nab,nkb->nka", R, x) + t[:, None]
    return R, t, s, aligned, (w * ((aligned - y) ** 2).sum(-1)).sum(1)


def row(n, K, a):
    import torch

    g = torch.Generator(device="cuda").manual_seed(n + K)
    x = torch.randn(n, K, 3, device="cuda", generator=g) * torch.tensor([0.4, 0.25, 0.12], device="cuda")
    Q = torch.linalg.qr(torch.randn(n, 3, 3, device="cuda", generator=g))[0]
    Q = Q * torch.sign(torch.det(Q))[:, None, None]
    y = (1.2 * torch.einsum("nab,nkb->nka", Q, x) + 0.3 + 0.01 * torch.randn(n, K, 3, device="cuda", generator=g)).contiguous()
    w = (0.5 + torch.rand(n, K, device="cuda", generator=g)).contiguous()
    f = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    tr, al, en, pe, gap, st = f(n, 13), f(n, K, 3), f(n), f(n, K), f(n), torch.empty(n, dtype=torch.int32, device="cuda")
    gtr, gal, ge, gs, gt = torch.ones(n, 13, device="cuda"), torch.ones(n, K, 3, device="cuda"), torch.ones(n, device="cuda"), f(n, K, 3), f(n, K, 3)
    lib, stream, dev = _lib.load(), _stream(), _lib.DEVICE
    p = lambda t: t.data_ptr()  # noqa: E731
    head = (0, n, K, p(x), p(y), n, p(w), n, 1, MIN_GAP)
    calls = {"forward": lambda: _lib.check(lib.smplpp_align(*head, p(tr), p(al), p(en), p(pe), p(gap), p(st), dev, stream)),
             "backward": lambda: _lib.check(lib.smplpp_align_vjp(*head, p(gtr), p(gal), p(ge), p(gs), p(gt), 0, dev, stream))}
    pts = n * K
    nbytes = {"forward": pts * (12 + 12 + 4) + pts * (12 + 4) + n * (52 + 4 + 4 + 4), "backward": pts * (12 + 12 + 4) + pts * 12 + n * (52 + 4) + pts * 24}
    out = {"n": n, "K": K}
    for what, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        one = blocks(lambda k: fn(), 1, 1)["median"]  # a call of milliseconds gets fewer calls a block
        steps = max(2, min(a.steps, int(2e5 / max(one, 1.0))))
        t = timed(fn, a, steps)
        floor = nbytes[what] / PEAK * 1e6
        out[what] = {"us": t["median"], "us_least": t["least"], "us_greatest": t["greatest"], "bytes": nbytes[what], "floor_us": round(floor, 3),
                     "over_floor": round(t["median"] / floor, 1), "steps": steps}
    out["sound_frames"] = int((st == 0).sum())

    def t_backward():
        xs, ys = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
        R, t, s, aligned, energy = kabsch(xs, ys, w)
        loss = R.sum() + t.sum() + s.sum() + aligned.sum() + energy.sum()
        return torch.autograd.grad(loss, (xs, ys))

    with torch.no_grad():
        out["forward"]["torch_us"] = timed(lambda: kabsch(x, y, w), a, out["forward"]["steps"])["median"]
    out["backward"]["torch_us"] = timed(t_backward, a, out["backward"]["steps"])["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    a = ap.parse_args()
    res = {"bytes_per_second": PEAK, "steps": a.steps, "reps": a.reps, "with_scale": 1, "rows": [row(n, K, a) for n, K in CASES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
