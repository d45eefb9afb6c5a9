"""Timing of the image term (smplpp_image_sample, smplpp_image_term, smplpp_image_term_vjp) on one MI355X.

Four cases (n, K, C, H, W): joint heatmaps read through `channel` (1024, 24, 24, 64, 64); a photometric term on whole meshes (16, 6890, 3,
512, 512); a feature map (16, 6890, 32, 128, 128); and one texture shared by all frames, B = 1 (4, 65536, 3, 1024, 1024).  The points are
uniform over the pixel centres' rectangle.  Every call goes through the bare C entry point with device pointers, in `--reps` blocks of
`--steps` back-to-back calls between HIP events after `--warmup` blocks, in one session.  Reported per case and call (sample with
gradient, energy, grad_uv alone, grad_image alone):
  - us: the median block, microseconds per call, with the least and the greatest block;
  - floor_us and over_floor: the bytes the call must move at 8 TB/s: uv, the four taps of every sampled channel and the outputs, each once;
    for grad_image the image written once instead of per-point outputs;
  - torch_us: the same mathematics with torch.nn.functional.grid_sample(align_corners=False) on the NCHW view, autograd for the two
    gradients.
Prints one JSON line and writes it to --out.

    python tools/image_bench.py [--steps 50] [--warmup 2] [--reps 5] [--out profiles/image_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from depth_raster_bench import PEAK  # noqa: E402
from lbfgs_bench import blocks  # noqa: E402

from smplpp_amd import _lib  # noqa: E402
from smplpp_amd.smpl import _stream  # noqa: E402

RHO = 0.05
#        name              n     K      C   H     W     channel  shared image
CASES = (("heatmaps", 1024, 24, 24, 64, 64, True, False),
         ("photometric", 16, 6890, 3, 512, 512, False, False),
         ("features", 16, 6890, 32, 128, 128, False, False),
         ("shared texture", 4, 65536, 3, 1024, 1024, False, True))


def timed(fn, a, steps=None):
    steps = steps or a.steps
    for _ in range(a.warmup):
        blocks(lambda k: fn(), steps, 1)
    return blocks(lambda k: fn(), steps, a.reps)


def row(case, a):
    import torch
    import torch.nn.functional as F

    name, n, K, C, H, W, by_channel, shared = case
    B, Cs = (1 if shared else n), (1 if by_channel else C)
    g = torch.Generator(device="cuda").manual_seed(n + K)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g)  # noqa: E731
    uv = (0.5 + rnd(n, K, 2) * torch.tensor([W - 1.0, H - 1.0], device="cuda")).contiguous()
    image = rnd(B, H, W, C).contiguous()
    channel = (torch.arange(K, device="cuda") % C).to(torch.int64) if by_channel else None
    target = rnd(1, K, Cs)
    value, grad = torch.empty(n, K, Cs, device="cuda"), torch.empty(n, K, Cs, 2, device="cuda")
    valid, energy = torch.empty(n, K, dtype=torch.uint8, device="cuda"), torch.empty(n, device="cuda")
    ge, guv, gimg = torch.ones(n, device="cuda"), torch.empty(n, K, 2, device="cuda"), torch.empty(B, H, W, C, device="cuda")
    lib, st, dev = _lib.load(), _stream(), _lib.DEVICE
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    head = (0, n, K, p(uv), p(image), B, H, W, C, p(channel))
    calls = {
        "sample": lambda: _lib.check(lib.smplpp_image_sample(*head, p(value), p(grad), p(valid), dev, st)),
        "energy": lambda: _lib.check(lib.smplpp_image_term(*head, p(target), 1, None, 1, RHO, p(energy), None, None, None, dev, st)),
        "grad_uv": lambda: _lib.check(lib.smplpp_image_term_vjp(*head, p(target), 1, None, 1, RHO, p(ge), None, None, p(guv), None, 0, dev, st)),
        "grad_image": lambda: _lib.check(lib.smplpp_image_term_vjp(*head, p(target), 1, None, 1, RHO, p(ge), None, None, None, p(gimg), 0, dev, st)),
    }
    pts, read = n * K, 8 + 16 * Cs
    nbytes = {"sample": pts * (read + 12 * Cs + 1), "energy": pts * read + 4 * n, "grad_uv": pts * (read + 8) + 4 * n,
              "grad_image": pts * read + 4 * n + 4 * B * H * W * C}
    out = {"case": name, "n": n, "K": K, "C": C, "H": H, "W": W, "B": B, "channel": by_channel}
    for what, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        one = blocks(lambda k: fn(), 1, 1)["median"]  # a call of milliseconds gets fewer calls a block
        t = timed(fn, a, max(2, min(a.steps, int(2e5 / max(one, 1.0)))))
        floor = nbytes[what] / PEAK * 1e6
        out[what] = {"us": t["median"], "us_least": t["least"], "us_greatest": t["greatest"], "bytes": nbytes[what], "floor_us": round(floor, 3),
                     "over_floor": round(t["median"] / floor, 1)}
    out["valid_share"] = round(float(valid.float().mean()), 4)
    # the same mathematics in torch: grid_sample on the NCHW view (made once, outside the timing)
    nchw = image.permute(0, 3, 1, 2).contiguous()
    scale = torch.tensor([2.0 / W, 2.0 / H], device="cuda")

    def t_sample(u, im):
        norm = u * scale - 1.0
        grid = norm.reshape(1, n, K, 2) if shared else norm.reshape(n, 1, K, 2)
        s = F.grid_sample(im, grid, mode="bilinear", padding_mode="zeros", align_corners=False)  # [B, C, n or 1, K]
        s = s[0].permute(1, 2, 0) if shared else s[:, :, 0].permute(0, 2, 1)  # [n, K, C]
        return s.gather(2, channel.reshape(1, K, 1).expand(n, K, 1)) if by_channel else s

    def t_energy(u, im):
        r = t_sample(u, im) - target
        q = (r * r).sum(-1)
        return ((RHO * RHO * q) / (RHO * RHO + q)).sum(1)

    def t_grad(to_image):
        u, im = uv.detach().requires_grad_(not to_image), nchw.detach().requires_grad_(to_image)
        return torch.autograd.grad((t_energy(u, im) * ge).sum(), im if to_image else u)[0]

    def t_sample_all():
        u = uv.detach().requires_grad_(True)
        s = t_sample(u, nchw)
        return s, torch.autograd.grad(s.sum(), u)[0]

    steps = lambda what: max(2, min(a.steps, int(2e5 / max(out[what]["us"], 1.0))))  # noqa: E731
    with torch.no_grad():
        out["energy"]["torch_us"] = timed(lambda: t_energy(uv, nchw), a, steps("energy"))["median"]
    out["sample"]["torch_us"] = timed(t_sample_all, a, steps("sample"))["median"]
    out["grad_uv"]["torch_us"] = timed(lambda: t_grad(False), a, steps("grad_uv"))["median"]
    out["grad_image"]["torch_us"] = timed(lambda: t_grad(True), a, steps("grad_image"))["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_bench.json"))
    a = ap.parse_args()
    res = {"bytes_per_second": PEAK, "steps": a.steps, "reps": a.reps, "rho": RHO, "rows": [row(c, a) for c in CASES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
