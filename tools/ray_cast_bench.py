"""Timing of ray casting (smplpp_ray_cast and smplpp_ray_cast_vjp) on one MI355X, synthetic 6890-vertex model.

At each (n, K) of SIZES, with K rays per frame from a 2.5 m sphere about the body aimed at points of its posed surface, microseconds
per call of
  - the forward (face, t, bary, hits; both facings, the open range) and the forward with face and t alone,
  - the backward (grad_verts, grad_origin, grad_dir, accumulate 0) at the forward's faces,
  - smplpp_point_mesh_winding at the same (n, K), the ray origins as its points: the same loop over (query, face) pairs,
  - the same rule in float32 torch on the same rays (edge products compared as rounded, no fp64 branch), with the rays on which its
    face differs;
and for the 512 x 512 pixel rays of one frame (camera_rays), the forward against smplpp_depth_raster at (1, 512, 512) with the
pixels on which face and depth agree.  Device pointers, torch's current stream; each figure is the median over `--reps` timed blocks
of `--steps` back-to-back calls between HIP events, after `--warmup` untimed calls (the torch rule: one block of one call).  Prints
one JSON line and writes it to --out.

    python tools/ray_cast_bench.py [--steps 20] [--warmup 3] [--reps 3] [--out profiles/ray_cast_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((1, 16384), (16, 4096), (64, 1024), (256, 64))
TORCH_CHUNK_PAIRS = 1 << 23  # (ray, face) pairs per chunk of the torch rule


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


def _rays(verts, faces, K, rng):
    """(origin, dir) [n,K,3] on the device: origins on a 2.5 m sphere about each frame's centroid, aimed at points of its surface."""
    import torch

    n = verts.shape[0]
    fid = torch.from_numpy(rng.integers(0, len(faces), (n, K))).cuda()
    w = torch.from_numpy(rng.dirichlet(np.ones(3), (n, K)).astype(np.float32)).cuda()
    tri = verts[torch.arange(n, device="cuda")[:, None, None], faces[fid]]  # [n,K,3,3]
    aim = (w[..., None] * tri).sum(2)
    o = torch.from_numpy(rng.standard_normal((n, K, 3)).astype(np.float32)).cuda()
    o = 2.5 * torch.nn.functional.normalize(o, dim=-1) + verts.mean(1, keepdim=True)
    return o.contiguous(), (aim - o).contiguous()


def torch_ray_cast(verts, faces, o, d):
    """The rule in float32 torch, a chunk of rays at a time: the sheared plane, the three edge products compared as rounded (a tie
    counts for either sign: no fp64 branch), the plane range, the smallest t and then the lowest face.  (face [n,K], t [n,K])."""
    import torch

    n, K = o.shape[:2]
    F = faces.shape[0]
    face = torch.full((n, K), -1, dtype=torch.int64, device=o.device)
    t = torch.zeros((n, K), dtype=torch.float32, device=o.device)
    kc = max(1, TORCH_CHUNK_PAIRS // F)
    for f in range(n):
        v = verts[f]
        a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
        nrm = torch.cross(b - a, c - a, dim=-1)
        for k0 in range(0, K, kc):
            oo, dd = o[f, k0:k0 + kc], d[f, k0:k0 + kc]
            kz = dd.abs().argmax(1)
            idx = torch.stack([(kz + 1) % 3, (kz + 2) % 3, kz], 1)
            ds = torch.gather(dd, 1, idx)
            Sx, Sy = ds[:, 0] / ds[:, 2], ds[:, 1] / ds[:, 2]
            P = torch.gather(v[None] - oo[:, None], 2, idx[:, None, :].expand(-1, v.shape[0], -1))  # [kc,V,3] permuted
            X, Y = P[..., 0] - Sx[:, None] * P[..., 2], P[..., 1] - Sy[:, None] * P[..., 2]
            ge = torch.ones((len(oo), F), dtype=torch.bool, device=o.device)
            le = ge.clone()
            for p, q in ((0, 1), (1, 2), (2, 0)):
                m1, m2 = X[:, faces[:, p]] * Y[:, faces[:, q]], Y[:, faces[:, p]] * X[:, faces[:, q]]
                ge &= m1 >= m2
                le &= m1 <= m2
            tt = (nrm * (a[None] - oo[:, None])).sum(-1) / (nrm[None] * dd[:, None]).sum(-1)
            tt = torch.where((ge | le) & torch.isfinite(tt) & (tt > 0), tt, torch.full_like(tt, float("inf")))
            best, arg = tt.min(1)
            hit = torch.isfinite(best)
            face[f, k0:k0 + kc] = torch.where(hit, arg, torch.full_like(arg, -1))
            t[f, k0:k0 + kc] = torch.where(hit, best, torch.zeros_like(best))
    return face, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_cast_bench.json"))
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import torch

    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import SMPL, _ptr, _stream, camera_rays, pinhole_camera

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
    INF = float("inf")
    e = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda")  # noqa: E731

    def calls(n, K, verts, o, d, rf):
        face, t, bary, hits = e(n, K, dt=torch.int64), e(n, K), e(n, K, 3), e(n, K, 2, dt=torch.int32)
        g = torch.from_numpy(rng.standard_normal((n, K)).astype(np.float32)).cuda()
        gv, go, gd = e(n, V, 3), e(rf, K, 3), e(rf, K, 3)

        def forward():
            _lib.check(L.smplpp_ray_cast(s.handle, n, _ptr(verts), rf, K, _ptr(o), _ptr(d), 0.0, INF, 3, _ptr(face), _ptr(t), _ptr(bary), _ptr(hits),
                                         D, _stream()))

        def forward_bare():
            _lib.check(L.smplpp_ray_cast(s.handle, n, _ptr(verts), rf, K, _ptr(o), _ptr(d), 0.0, INF, 3, _ptr(face), _ptr(t), None, None, D,
                                         _stream()))

        def backward():
            _lib.check(L.smplpp_ray_cast_vjp(s.handle, n, _ptr(verts), rf, K, _ptr(o), _ptr(d), _ptr(face), _ptr(g), _ptr(gv), _ptr(go), _ptr(gd), 0,
                                             D, _stream()))

        return forward, forward_bare, backward, face, t

    res = {}
    for n, K in SIZES:
        beta, theta = model_io.synthetic_inputs(n, seed=n)
        verts = s.launch(torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda(), want=("verts",))["verts"]
        o, d = _rays(verts, faces, K, rng)
        forward, forward_bare, backward, face, t = calls(n, K, verts, o, d, n)
        wn, ins = e(n, K), e(n, K, dt=torch.uint8)

        def winding():
            _lib.check(L.smplpp_point_mesh_winding(s.handle, n, _ptr(verts), K, _ptr(o), _ptr(wn), _ptr(ins), D, _stream()))

        r = dict(forward_us=T(forward), forward_face_t_us=T(forward_bare))
        forward()
        r["backward_us"] = T(backward)
        r["winding_us"] = T(winding)
        r["pairs"] = n * K * F
        r["pairs_per_ns"] = round(n * K * F / (r["forward_us"] * 1e3), 2)
        r["winding_pairs_per_ns"] = round(n * K * F / (r["winding_us"] * 1e3), 2)
        r["hit_fraction"] = round(float((face >= 0).float().mean()), 4)
        if not a.no_torch:
            tf, tt = torch_ray_cast(verts, faces, o, d)
            torch.cuda.synchronize()
            r["torch_us"] = _time(lambda: torch_ray_cast(verts, faces, o, d), 1, 0, 1)
            forward()
            r["torch_faces_that_differ"] = int((tf != face).sum())
            r["speedup_vs_torch"] = round(r["torch_us"] / r["forward_us"], 1)
        res["%d,%d" % (n, K)] = r

    # the pixel rays of one frame against the rasteriser
    H = W = 512
    beta, theta = model_io.synthetic_inputs(1, seed=1)
    verts = s.launch(torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda(), want=("verts",))["verts"]
    vh = verts.cpu().numpy()
    R = np.diag([1.0, -1.0, -1.0])
    ctr = (vh.min(1) + vh.max(1)) / 2
    cam = pinhole_camera(R, -ctr @ R.T + np.array([0.0, 0.0, 2.5]), 1.1 * H, 1.1 * H, W / 2, H / 2, n=1)
    oh, dh = camera_rays(cam, H, W)
    o, d = torch.from_numpy(oh).cuda(), torch.from_numpy(dh).cuda()
    K = H * W
    forward, forward_bare, backward, face, t = calls(1, K, verts, o, d, 1)
    camd = torch.from_numpy(cam).cuda()
    rface, rdepth = e(1, H, W, dt=torch.int64), e(1, H, W)

    def raster():
        _lib.check(L.smplpp_depth_raster(s.handle, 1, _ptr(verts), _ptr(camd), H, W, 0.05, _ptr(rface), _ptr(rdepth), None, None, None, D, _stream()))

    px = dict(forward_us=T(forward), forward_face_t_us=T(forward_bare))
    forward()
    px["backward_us"] = T(backward)
    px["depth_raster_us"] = T(raster)
    px["pairs_per_ns"] = round(K * F / (px["forward_us"] * 1e3), 2)
    same = (rface.reshape(-1) == face.reshape(-1))
    covered = rface.reshape(-1) >= 0
    px["covered_pixels"] = int(covered.sum())
    px["same_face_fraction_of_covered"] = round(float(same[covered].float().mean()), 5)
    both = same & covered
    px["depth_max_rel_diff_on_same_face"] = float(((t.reshape(-1) - rdepth.reshape(-1)).abs() / rdepth.reshape(-1))[both].max())
    res["pixels 1,512x512"] = px
    line = json.dumps(dict(metric="ray_cast_us", device=torch.cuda.get_device_name(0), vertex_num=V, face_num=F, by_size=res, steps=a.steps,
                           warmup=a.warmup, reps=a.reps))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
