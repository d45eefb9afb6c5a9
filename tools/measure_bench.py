"""Timing of the body measurements (smplpp_measure and smplpp_measure_vjp) on one MI355X, synthetic 6890-vertex model.

At each n of SIZES, with R = 4 regions (all faces and three parts by dominant joint) and S = 6 sections whose planes pass through
posed joints and face along the bone, microseconds per call of
  - the forward (area, volume, section, crossings; planes per frame; center = the root joint),
  - the backward (grad_verts and grad_planes for cotangents on all three outputs, accumulate 0),
  - the same mathematics in float32 torch, forward and forward + autograd backward, in the same session: the gather verts[:, faces]
    per region and a boolean crossing mask per plane.
Device pointers, torch's current stream; each figure is the median over `--reps` timed blocks of `--steps` back-to-back calls
between HIP events, after `--warmup` untimed calls (the torch rule: one block of one call after one untimed call).
`--flagship-branch` / `--flagship-parent` take the JSON line bench.py printed on this build and on the parent's library in the same
session; their headline fields are recorded.  Prints one JSON line and writes it to --out.

    python tools/measure_bench.py [--steps 20] [--warmup 3] [--reps 3] [--out profiles/measure_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (1, 16, 256, 1024)
GROUPS = [list(range(24)), [0, 3, 6, 9, 12, 13, 14, 15], [16, 18, 20, 22], [1, 4, 7, 10]]  # all, trunk, left arm, left leg
GIRTHS = [(0, 3, 6), (1, 6, 9), (2, 18, 20), (3, 4, 7), (0, 18, 20), (0, 4, 7)]  # (region, joint on the plane, joint it faces)


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


def torch_measure(verts, faces, regions, sections, planes, center):
    """(area [n,R], volume [n,R], section [n,S]) in float32 torch: what a torch user writes."""
    import torch

    area, volume, section = [], [], [None] * len(sections)
    for r, lst in enumerate(regions):
        tri = verts[:, faces[lst]]  # [n,K,3,3]
        p = tri - center[:, None, None, :]
        area.append(0.5 * torch.linalg.cross(p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 0]).norm(dim=-1).sum(1))
        volume.append((p[:, :, 0] * torch.linalg.cross(p[:, :, 1], p[:, :, 2])).sum(-1).sum(1) / 6)
        for s, reg in enumerate(sections):
            if reg != r:
                continue
            pl = planes[:, s]
            sv = (tri * pl[:, None, None, :3]).sum(-1) - pl[:, None, None, 3]
            ab = sv.detach() >= 0
            cnt = ab.sum(-1)
            on, la = (cnt == 1) | (cnt == 2), cnt == 1
            L = torch.argmax((ab == la[..., None]).to(torch.int64), -1)
            q = []
            for j in (1, 2):
                o = (L + j) % 3
                ia, ib = torch.where(la, o, L), torch.where(la, L, o)
                xa = torch.gather(tri, 2, ia[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
                xb = torch.gather(tri, 2, ib[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
                sa, sb = torch.gather(sv, 2, ia[..., None])[..., 0], torch.gather(sv, 2, ib[..., None])[..., 0]
                t = sa / torch.where(on, sa - sb, torch.ones_like(sa))
                q.append(xa + t[..., None] * (xb - xa))
            d2 = ((q[1] - q[0]) ** 2).sum(-1)
            on = on & (d2.detach() > 0)
            section[s] = torch.where(on, torch.sqrt(torch.where(on, d2, torch.ones_like(d2))), torch.zeros_like(d2)).sum(1)
    return torch.stack(area, 1), torch.stack(volume, 1), torch.stack(section, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "measure_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--flagship-branch", default=None, help="file holding bench.py's JSON line on this build")
    ap.add_argument("--flagship-parent", default=None, help="file holding bench.py's JSON line on the parent's library")
    a = ap.parse_args()
    import torch

    from smplpp_amd import _lib, model_io
    from smplpp_amd.measure import Measure, plane_through, regions_by_joint
    from smplpp_amd.smpl import SMPL, _ptr, _stream

    model = model_io.synthetic_model()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    L = _lib.load()
    V = s.vertex_num
    regions = regions_by_joint(model, GROUPS)
    sections = [g[0] for g in GIRTHS]
    ms = Measure(s, regions, sections)
    R, S = len(regions), len(sections)
    faces = torch.from_numpy(model["face_indices"].astype(np.int64) - 1).cuda()
    tregions = [torch.from_numpy(r).cuda() for r in regions]
    rng = np.random.default_rng(0)
    T = lambda fn: _time(fn, a.steps, a.warmup, a.reps)  # noqa: E731
    D = _lib.DEVICE
    e = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda")  # noqa: E731
    res = {}
    for n in SIZES:
        beta, theta = model_io.synthetic_inputs(n, seed=n)
        bd, td = torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda()
        verts = s.launch(bd, td, want=("verts",))["verts"]
        posed = s.skeleton(bd, td, want=("posed",))["posed"]
        at, to = posed[:, [g[1] for g in GIRTHS]], posed[:, [g[2] for g in GIRTHS]]
        planes = plane_through(at, to - at).contiguous()
        center = posed[:, 0].contiguous()
        area, volume, section, crossings = e(n, R), e(n, R), e(n, S), e(n, S, dt=torch.int32)
        ga, gvol, gs = (torch.from_numpy(rng.standard_normal(sh).astype(np.float32)).cuda() for sh in ((n, R), (n, R), (n, S)))
        gv, gp = e(n, V, 3), e(n, S, 4)

        def forward():
            _lib.check(L.smplpp_measure(ms.handle, n, _ptr(verts), _ptr(center), _ptr(planes), n, _ptr(area), _ptr(volume), _ptr(section),
                                        _ptr(crossings), D, _stream()))

        def backward():
            _lib.check(L.smplpp_measure_vjp(ms.handle, n, _ptr(verts), _ptr(center), _ptr(planes), n, _ptr(ga), _ptr(gvol), _ptr(gs), _ptr(gv),
                                            _ptr(gp), 0, D, _stream()))

        r = dict(forward_us=T(forward), backward_us=T(backward))
        forward()
        r["crossings_min"] = int(crossings.min())
        r["vertex_read_floor_us"] = round(12.0 * V * n / 8e12 * 1e6, 2)
        if not a.no_torch:
            tv, tp = verts.clone().requires_grad_(True), planes.clone().requires_grad_(True)

            def torch_forward():
                with torch.no_grad():
                    return torch_measure(tv, faces, tregions, sections, tp, center)

            def torch_both():
                tv.grad = tp.grad = None
                ta, tvol, ts = torch_measure(tv, faces, tregions, sections, tp, center)
                ((ta * ga).sum() + (tvol * gvol).sum() + (ts * gs).sum()).backward()

            r["torch_forward_us"] = _time(torch_forward, 1, 1, 1)
            r["torch_forward_backward_us"] = _time(torch_both, 1, 1, 1)
            ta, tvol, ts = torch_forward()
            r["volume_max_rel_diff_vs_torch"] = float(((tvol - volume).abs().max() / tvol.abs().max()))
            r["section_max_rel_diff_vs_torch"] = float(((ts - section).abs().max() / ts.abs().max()))
            r["speedup_vs_torch"] = round(r["torch_forward_backward_us"] / (r["forward_us"] + r["backward_us"]), 1)
            del tv, tp, ta, tvol, ts
            torch.cuda.empty_cache()
        res[str(n)] = r
    line = dict(metric="measure_us", device=torch.cuda.get_device_name(0), vertex_num=V, face_num=int(faces.shape[0]),
                region_faces=[len(r) for r in regions], sections=S, by_n=res, steps=a.steps, warmup=a.warmup, reps=a.reps)
    for key, path in (("flagship_branch", a.flagship_branch), ("flagship_parent", a.flagship_parent)):
        if path and os.path.exists(path):
            rows = [json.loads(x) for x in open(path).read().splitlines() if x.startswith("{")]
            line[key] = [{k: row.get(k) for k in ("metric", "value", "unit") if k in row} for row in rows]
    line = json.dumps(line)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
