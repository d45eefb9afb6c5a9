"""Timing of the surface geodesics and the self-contact search (smplpp_mesh_geodesic, smplpp_self_contact_*) on one MI355X, synthetic
6890-vertex model.  Every call goes through the bare C entry point with device pointers, in `--reps` blocks of back-to-back calls
between HIP events after `--warmup` blocks, in one session.  Reported, as the median block in microseconds per call:
  - geodesic: (n, S) = (1, 1), (1, 64), (16, 16), (1, 6890) single sources on posed frames; `floor_us` is one pass over the frame's
    edge lengths and the CSR (nnz * 8 + V * 4 bytes per field) at 4 TB/s, `sweeps` the sweeps of the synchronous restatement from
    source 0 on the template (the kernel's in-place sweeps are at most as many), `scipy_us` scipy's float64 CPU Dijkstra for the same
    fields when scipy is there;
  - create: smplpp_self_contact_create at geo_min = 0.3 (a wall-clock time: the call synchronises);
  - search: n = 1, 16, 256, with and without normals and a 10 cm cap; `mpd_us` smplpp_mesh_point_distance(verts, verts) in the same
    session (the unmasked scan: the difference is the cost of the mask), `torch_us` float32 torch cdist + mask + min on the same GPU
    (n <= 16: the n V V matrix);
  - vjp: smplpp_self_contact_vjp against the two smplpp_mesh_point_distance_vjp calls it is defined by.
Prints one JSON line and writes it to --out.

    python tools/self_contact_bench.py [--steps 20] [--warmup 1] [--reps 5] [--out profiles/self_contact_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lbfgs_bench import blocks  # noqa: E402

from smplpp_amd import _lib, contact, model_io  # noqa: E402
from smplpp_amd.smpl import SMPL, _stream  # noqa: E402

GEO_CASES = ((1, 1), (1, 64), (16, 16), (1, 6890))
SEARCH_N = (1, 16, 256)
HBM_BYTES_PER_US = 4e6


def timed(fn, a, what):
    import torch

    fn()
    torch.cuda.synchronize()
    one = blocks(lambda k: fn(), 1, 1)["median"]
    steps = max(1, min(a.steps, int(1e5 / max(one, 1.0))))
    for _ in range(a.warmup):
        blocks(lambda k: fn(), steps, 1)
    t = blocks(lambda k: fn(), steps, a.reps if one < 2e5 else min(a.reps, 3))
    print("%-52s %12.1f us" % (what, t["median"]), file=sys.stderr, flush=True)
    return {"us": t["median"], "us_least": t["least"], "us_greatest": t["greatest"], "steps": steps}


def main():
    import numpy as np
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_contact_bench.json"))
    a = ap.parse_args()
    lib, dev = _lib.load(), _lib.DEVICE
    model = model_io.synthetic_model()
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    V = s.vertex_num
    faces0 = np.asarray(model["face_indices"], np.int64) - 1
    rest = np.ascontiguousarray(model["vertices_template"], np.float32)
    res = {"steps": a.steps, "reps": a.reps, "V": V}

    import geodesic_oracle as GO

    off, adj = GO.edge_table(V, faces0)
    w = GO.edge_weights(rest, off, adj)
    res["nnz"], res["sweeps_from_vertex_0"] = int(len(adj)), int(GO.relax(V, off, adj, w, [[0]])[1])
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import dijkstra
        graph = sp.csr_matrix((w.astype(np.float64), adj, off), shape=(V, V))
    except Exception:
        dijkstra = None

    def frames(n):
        beta, theta = model_io.synthetic_inputs(n, seed=3)
        return torch.from_numpy(s.launch(beta, theta)["verts"]).cuda().contiguous()

    # ---- geodesics
    res["geodesic"] = []
    for n, S in GEO_CASES:
        v = frames(n)
        src = np.linspace(0, V - 1, S).astype(np.int64)
        ptr, ids = torch.arange(S + 1, device="cuda"), torch.from_numpy(src).cuda()
        dist = torch.empty(n, S, V, device="cuda")
        call = lambda: _lib.check(lib.smplpp_mesh_geodesic(s.handle, n, v.data_ptr(), S, ptr.data_ptr(), ids.data_ptr(), float("inf"),  # noqa: E731
                                                           dist.data_ptr(), dev, _stream()))
        r = {"n": n, "S": S, **timed(call, a, "geodesic n %d S %d" % (n, S))}
        r["field_us"] = round(r["us"] / (n * S), 3)
        r["floor_us"] = round(n * S * (len(adj) * 8 + V * 4) / HBM_BYTES_PER_US, 3)
        r["ratio_to_floor"] = round(r["us"] / r["floor_us"], 1)
        if dijkstra is not None and n * S <= 256:
            t0 = time.perf_counter()
            dijkstra(graph, directed=True, indices=src)
            r["scipy_us"] = round((time.perf_counter() - t0) * 1e6 * n, 1)
        res["geodesic"].append(r)

    # ---- handle creation
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        sc = contact.SelfContact(s, geo_min=0.3)
        t.append((time.perf_counter() - t0) * 1e6)
    res["create"] = {"us": sorted(t)[1], "far_pairs": sc.far_pairs, "mask_bytes": V * sc.words_per_row * 4}
    print("create %.0f us" % res["create"]["us"], file=sys.stderr, flush=True)

    # ---- the search and its backward
    res["search"], res["vjp"] = [], []
    mask_bool = None
    for n in SEARCH_N:
        v = frames(n)
        nrm = torch.randn(n, V, 3, device="cuda")
        index, sq = torch.empty(n, V, dtype=torch.int64, device="cuda"), torch.empty(n, V, device="cuda")
        for normals, cap in ((False, float("inf")), (True, float("inf")), (False, 0.01), (True, 0.01)):
            call = lambda: _lib.check(lib.smplpp_self_contact(sc.handle, n, v.data_ptr(), nrm.data_ptr() if normals else None, 0.0, cap,  # noqa: E731
                                                              index.data_ptr(), sq.data_ptr(), dev, _stream()))
            r = {"n": n, "normals": normals, "cap": cap != float("inf"), **timed(call, a, "search n %d normals %d cap %d" % (n, normals, cap < 1))}
            r["pair_ns"] = round(r["us"] * 1e3 / (n * V * V), 5)
            res["search"].append(r)
        mpd = lambda: _lib.check(lib.smplpp_mesh_point_distance(s.handle, n, v.data_ptr(), V, v.data_ptr(), index.data_ptr(), sq.data_ptr(), dev,  # noqa: E731
                                                                _stream()))
        base = timed(mpd, a, "  mesh_point_distance(verts, verts) n %d" % n)["us"]
        for r in res["search"][-4:]:
            r["mpd_us"] = base
        if n <= 16:
            if mask_bool is None:
                mask_bool = torch.from_numpy(GO.unpack_bits(sc.mask(), V)).cuda()

            def t_search():
                d = torch.cdist(v, v)
                return torch.where(mask_bool[None], d, torch.full_like(d, float("inf"))).min(-1)

            with torch.no_grad():
                tu = timed(t_search, a, "  torch cdist + mask + min n %d" % n)["us"]
            for r in res["search"][-4:]:
                r["torch_us"] = tu
        _lib.check(lib.smplpp_self_contact(sc.handle, n, v.data_ptr(), None, 0.0, float("inf"), index.data_ptr(), sq.data_ptr(), dev, _stream()))
        g, gv = torch.randn(n, V, device="cuda"), torch.empty(n, V, 3, device="cuda")
        bwd = lambda: _lib.check(lib.smplpp_self_contact_vjp(sc.handle, n, v.data_ptr(), index.data_ptr(), g.data_ptr(), gv.data_ptr(), 0, dev,  # noqa: E731
                                                             _stream()))

        def two():
            _lib.check(lib.smplpp_mesh_point_distance_vjp(s.handle, n, v.data_ptr(), V, v.data_ptr(), index.data_ptr(), g.data_ptr(), gv.data_ptr(),
                                                          None, 0, dev, _stream()))
            _lib.check(lib.smplpp_mesh_point_distance_vjp(s.handle, n, v.data_ptr(), V, v.data_ptr(), index.data_ptr(), g.data_ptr(), None,
                                                          gv.data_ptr(), 1, dev, _stream()))

        r = {"n": n, **timed(bwd, a, "vjp n %d" % n)}
        r["two_calls_us"] = timed(two, a, "  the two mesh_point_distance_vjp calls n %d" % n)["us"]
        res["vjp"].append(r)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
