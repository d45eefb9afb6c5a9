"""Timing of the scan preparation (smplpp_cloud_knn, smplpp_cloud_normals, smplpp_cloud_farthest_points) on one MI355X.

kNN and normals at (n, K) = (1, 16384), (16, 4096), (64, 1024) in self-query mode and (1, 131072) queried by a 16384-point subset, at
k = 8, 16, 32 (normals on the three self-query cases, from the lists the kNN call just wrote).  Farthest points at (1, 131072 -> 16384)
and (16, 16384 -> 4096).  Every call goes through the bare C entry point with device pointers, in `--reps` blocks of back-to-back calls
between HIP events after `--warmup` blocks, in one session; a call of milliseconds gets fewer calls a block, the sampling one.  Reported:
  - us: the median block, microseconds per call, with the least and the greatest block;
  - for kNN, pair_ns: us per (query, candidate) pair, and the clouds are in random order (the insertion chain runs about
    64 k (1 + ln(K / 64 k)) times per wavefront);
  - torch_us and ratio = torch_us / us: the same mathematics in float32 torch on the same GPU: cdist + topk (k + 1 and the first
    column dropped in self-query mode), a gather and batched torch.linalg.eigh of the 3 x 3 covariances, and for the sampling a loop of
    one distance pass, a minimum and an argmax per pick, all on the device.  The same mathematics, not the same rounding or tie order.
Prints one JSON line and writes it to --out.

    python tools/cloud_bench.py [--steps 20] [--warmup 1] [--reps 5] [--out profiles/cloud_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lbfgs_bench import blocks  # noqa: E402

from smplpp_amd import _lib  # noqa: E402
from smplpp_amd.smpl import _stream  # noqa: E402

KNN_CASES = ((1, 16384, 0), (16, 4096, 0), (64, 1024, 0), (1, 131072, 16384))  # (n, K, Q; 0: the cloud queries itself)
KS = (8, 16, 32)
FPS_CASES = ((1, 131072, 16384), (16, 16384, 4096))


def timed(fn, a, what):
    """The median of blocks of calls; `what` names the case in the progress line."""
    import torch

    fn()
    torch.cuda.synchronize()
    one = blocks(lambda k: fn(), 1, 1)["median"]
    steps = max(1, min(a.steps, int(1e5 / max(one, 1.0))))
    for _ in range(a.warmup):
        blocks(lambda k: fn(), steps, 1)
    t = blocks(lambda k: fn(), steps, a.reps if one < 2e5 else min(a.reps, 3))
    print("%-44s %12.1f us" % (what, t["median"]), file=sys.stderr, flush=True)
    return {"us": t["median"], "us_least": t["least"], "us_greatest": t["greatest"], "steps": steps}


def cloud(n, K, seed):
    """A body-sized random cloud on a bumpy ellipsoid shell, in random order."""
    import torch

    g = torch.Generator(device="cuda").manual_seed(seed)
    d = torch.randn(n, K, 3, device="cuda", generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    return (d * torch.tensor([0.8, 0.9, 0.15], device="cuda") + 0.002 * torch.randn(n, K, 3, device="cuda", generator=g)).contiguous()


def knn_rows(a):
    import torch

    lib, stream, dev = _lib.load(), _stream(), _lib.DEVICE
    rows = []
    for n, K, Q in KNN_CASES:
        p = cloud(n, K, n + K)
        q = p[:, torch.randperm(K, device="cuda")[:Q]].contiguous() + 1e-4 if Q else None
        Qn = Q or K
        for k in KS:
            index = torch.empty(n, Qn, k, dtype=torch.int32, device="cuda")
            dist, count = torch.empty(n, Qn, k, device="cuda"), torch.empty(n, Qn, dtype=torch.int32, device="cuda")
            call = lambda: _lib.check(lib.smplpp_cloud_knn(0, n, K, p.data_ptr(), Qn, q.data_ptr() if Q else None, k, float("inf"),  # noqa: E731
                                                           index.data_ptr(), dist.data_ptr(), count.data_ptr(), dev, stream))
            r = {"n": n, "K": K, "Q": Qn, "self": not Q, "k": k, "knn": timed(call, a, "knn n %d K %d Q %d k %d" % (n, K, Qn, k))}
            r["knn"]["pair_ns"] = round(r["knn"]["us"] * 1e3 / (n * Qn * K), 4)

            def t_knn():
                d = torch.cdist(q if Q else p, p)
                return d.topk(k if Q else k + 1, dim=-1, largest=False)

            with torch.no_grad():
                r["knn"]["torch_us"] = timed(t_knn, a, "  torch cdist + topk")["us"]
            r["knn"]["ratio"] = round(r["knn"]["torch_us"] / r["knn"]["us"], 2)
            if not Q:
                nrm, curv = torch.empty(n, K, 3, device="cuda"), torch.empty(n, K, device="cuda")
                status = torch.empty(n, K, dtype=torch.int32, device="cuda")
                view = torch.tensor([[0.0, 0.0, 3.0]], device="cuda")
                ncall = lambda: _lib.check(lib.smplpp_cloud_normals(0, n, K, p.data_ptr(), k, index.data_ptr(), view.data_ptr(), 1, 0.0,  # noqa: E731
                                                                    nrm.data_ptr(), curv.data_ptr(), status.data_ptr(), dev, stream))
                r["normals"] = timed(ncall, a, "normals n %d K %d k %d" % (n, K, k))
                ix = index.long()

                def t_normals():
                    nb = torch.cat([p[:, :, None], p[torch.arange(n, device="cuda")[:, None, None], ix]], 2)
                    nb = nb - nb.mean(2, keepdim=True)
                    lam, vec = torch.linalg.eigh(torch.einsum("nkma,nkmb->nkab", nb, nb))
                    v = vec[..., 0]
                    return torch.where(((view[:, None] - p) * v).sum(-1, keepdim=True) < 0, -v, v), lam[..., 0] / lam.sum(-1)

                with torch.no_grad():
                    r["normals"]["torch_us"] = timed(t_normals, a, "  torch gather + eigh")["us"]
                r["normals"]["ratio"] = round(r["normals"]["torch_us"] / r["normals"]["us"], 2)
                r["normals"]["sound_points"] = int((status == 0).sum())
            rows.append(r)
    return rows


def fps_rows(a):
    import torch

    lib, stream, dev = _lib.load(), _stream(), _lib.DEVICE
    rows = []
    for n, K, M in FPS_CASES:
        p = cloud(n, K, 7 * n + K)
        index, radius = torch.empty(n, M, dtype=torch.int32, device="cuda"), torch.empty(n, M, device="cuda")
        cover = torch.empty(n, K, device="cuda")
        call = lambda: _lib.check(lib.smplpp_cloud_farthest_points(0, n, K, p.data_ptr(), M, None, index.data_ptr(), radius.data_ptr(),  # noqa: E731
                                                                   cover.data_ptr(), dev, stream))
        r = {"n": n, "K": K, "M": M, "fps": timed(call, a, "farthest points n %d K %d M %d" % (n, K, M))}
        r["fps"]["round_us"] = round(r["fps"]["us"] / M, 3)
        rows_n = torch.arange(n, device="cuda")

        def t_fps():
            dmin = torch.full((n, K), float("inf"), device="cuda")
            cur = torch.zeros(n, dtype=torch.long, device="cuda")
            picks = torch.empty(n, M, dtype=torch.long, device="cuda")
            for i in range(M):
                picks[:, i] = cur
                dmin = torch.minimum(dmin, torch.cdist(p, p[rows_n, cur][:, None]).squeeze(-1) ** 2)
                cur = dmin.argmax(1)
            return picks, dmin

        with torch.no_grad():
            r["fps"]["torch_us"] = timed(t_fps, a, "  torch loop of cdist + argmax")["us"]
        r["fps"]["ratio"] = round(r["fps"]["torch_us"] / r["fps"]["us"], 2)
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_bench.json"))
    a = ap.parse_args()
    res = {"steps": a.steps, "reps": a.reps, "knn": knn_rows(a), "farthest_points": fps_rows(a)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
