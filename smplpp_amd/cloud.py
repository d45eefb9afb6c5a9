"""Scan preparation (smplpp_cloud_knn, smplpp_cloud_normals, smplpp_cloud_farthest_points): what a raw cloud [N,K,3] needs before the
scan terms take it.  knn lists the k nearest cloud points of every query in the order (distance, index); estimate_normals turns the
self-query lists into a normal, a surface variation and a status per point; farthest_points thins a cloud to M well-spread points.  numpy
arrays are host space (the call stages and synchronises, on `device`), torch tensors device space (enqueued on torch's current stream);
every number of the three calls is produced by libsmplpp_hip.so.  The scan is data: nothing here is differentiable.

The path of a depth frame: farthest_points -> gather -> estimate_normals(viewpoint=camera centre) -> SMPL.pointMeshDistanceCompatible.
A normal of zero (status 1: fewer than two usable neighbours) is what the compatible searches leave unmatched."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check
from .smpl import _Call, _is_torch, _ptr, torch

K_MAX = 32


def _cloud(c, points, what="points"):
    if len(points.shape) != 3 or points.shape[2] != 3:
        c.refuse("expected %s of shape (N, K, 3)" % what)
    n, K = int(points.shape[0]), int(points.shape[1])
    return n, K, c.input(points, (n, K, 3))


def _dev(c, device):
    return int(c.device.index if c.dev and c.device.index is not None else device)


def _int32(c, a, shape, what):
    """An int32 array of `shape` in the call's space (converted from any integer array)."""
    if _is_torch(a):
        if not c.dev:
            c.refuse("mix of torch tensors and numpy arrays")
        a = a.detach().to(device=c.device, dtype=torch.int32).contiguous()
    else:
        a = np.ascontiguousarray(a, np.int32)
        if c.dev:
            a = torch.from_numpy(a).to(c.device)
    if tuple(a.shape) != tuple(shape):
        c.refuse("expected %s of shape %s" % (what, tuple(shape)))
    return a


def _cap(c, max_dist):
    if max_dist is None:
        return float("inf")
    if not max_dist >= 0:
        c.refuse("max_dist must not be negative")
    return float(np.float32(max_dist) * np.float32(max_dist))  # one fp32 product: the cap the kernel compares with


def knn(points, k, queries=None, max_dist=None, want=("index", "sqdist", "count"), device=0):
    """The k (1..32) nearest points of the cloud points [N,K,3] for every query of queries [N,Q,3]; None: the cloud queries itself and a
    point is not its own neighbour (smplpp_cloud_knn).  Only points within max_dist (None: no cap) are listed.  A dict of index [N,Q,k]
    int32 and sqdist [N,Q,k], ordered by (squared distance, index), and count [N,Q] int32; ranks from count on hold (-1, 0)."""
    c = _Call("knn", points, queries)
    n, K, p = _cloud(c, points)
    Q, q = K, None
    if queries is not None:
        nq, Q, q = _cloud(c, queries, "queries")
        if nq != n:
            c.refuse("points and queries differ in N")
    names = ("index", "sqdist", "count")
    if not want or any(w not in names for w in want):
        c.refuse("want must name some of " + ", ".join(names))
    k = int(k)
    if not 1 <= k <= K_MAX:
        c.refuse("k must be in 1..%d" % K_MAX)
    res = {}
    if "index" in want:
        res["index"] = c.empty((n, Q, k), "int32")
    if "sqdist" in want:
        res["sqdist"] = c.empty((n, Q, k))
    if "count" in want:
        res["count"] = c.empty((n, Q), "int32")
    check(_lib.load().smplpp_cloud_knn(_dev(c, device), n, K, _ptr(p), Q, _ptr(q), k, _cap(c, max_dist), _ptr(res.get("index")),
                                       _ptr(res.get("sqdist")), _ptr(res.get("count")), c.space, c.stream))
    return res


def normals_from_index(points, index, viewpoint=None, min_gap=0.0, want=("normal", "curvature", "status"), device=0):
    """Normal [N,K,3], curvature [N,K] (the surface variation l0 / (l0 + l1 + l2)) and status [N,K] int32 of every point of points
    [N,K,3] from its neighbour list index [N,K,k] (smplpp_cloud_normals).  viewpoint [3] or [N,3]: normals point towards it; None: the
    largest component is positive.  status 1: fewer than two usable neighbours, normal 0; status 2: l2 <= 0 or l1 - l0 < min_gap l2,
    the normal is not unique."""
    c = _Call("normals_from_index", points)
    n, K, p = _cloud(c, points)
    if len(index.shape) != 3:
        c.refuse("expected index of shape (N, K, k)")
    k = int(index.shape[2])
    ix = _int32(c, index, (n, K, k), "index")
    vp, Vn = None, 0
    if viewpoint is not None:
        if not _is_torch(viewpoint):
            viewpoint = np.ascontiguousarray(viewpoint, np.float32)
            if c.dev:
                viewpoint = torch.from_numpy(viewpoint).to(c.device)
        vp = viewpoint.reshape(-1, 3)
        Vn = int(vp.shape[0])
        vp = c.input(vp, (Vn, 3))
    names = ("normal", "curvature", "status")
    if not want or any(w not in names for w in want):
        c.refuse("want must name some of " + ", ".join(names))
    res = {}
    if "normal" in want:
        res["normal"] = c.empty((n, K, 3))
    if "curvature" in want:
        res["curvature"] = c.empty((n, K))
    if "status" in want:
        res["status"] = c.empty((n, K), "int32")
    check(_lib.load().smplpp_cloud_normals(_dev(c, device), n, K, _ptr(p), k, _ptr(ix), _ptr(vp), Vn, float(min_gap), _ptr(res.get("normal")),
                                           _ptr(res.get("curvature")), _ptr(res.get("status")), c.space, c.stream))
    return res


def estimate_normals(points, k=16, viewpoint=None, max_dist=None, min_gap=0.0, device=0):
    """knn of the cloud on itself, then normals_from_index: a dict of normal, curvature, status and the neighbour lists index, sqdist and
    count.  max_dist keeps far points out of a neighbourhood (a point left with fewer than two neighbours gets status 1)."""
    nb = knn(points, k, max_dist=max_dist, device=device)
    res = normals_from_index(points, nb["index"], viewpoint=viewpoint, min_gap=min_gap, device=device)
    res.update(nb)
    return res


def farthest_points(points, M, start=None, device=0):
    """M of the K points of every frame of points [N,K,3] by farthest-point sampling from start [N] (None: index 0)
    (smplpp_cloud_farthest_points): a dict of index [N,M] int32 (-1 once the finite points run out), radius_sq [N,M] (the pick's squared
    distance to the picks before it; inf for the first) and min_sqdist [N,K] (every point's squared distance to the sample)."""
    c = _Call("farthest_points", points)
    n, K, p = _cloud(c, points)
    M = int(M)
    if not 1 <= M <= K:
        c.refuse("M must be in 1..K")
    s = None if start is None else _int32(c, start, (n,), "start")
    res = {"index": c.empty((n, M), "int32"), "radius_sq": c.empty((n, M)), "min_sqdist": c.empty((n, K))}
    check(_lib.load().smplpp_cloud_farthest_points(_dev(c, device), n, K, _ptr(p), M, _ptr(s), _ptr(res["index"]), _ptr(res["radius_sq"]),
                                                   _ptr(res["min_sqdist"]), c.space, c.stream))
    return res


def gather(points, index):
    """points[f, index[f, m]] for points [N,K,...] and index [N,M] (numpy or torch; plain indexing).  A negative index gives NaN."""
    if _is_torch(points):
        ix = index.to(device=points.device, dtype=torch.int64) if _is_torch(index) else torch.as_tensor(np.asarray(index), device=points.device).long()
        rows = torch.arange(points.shape[0], device=points.device)[:, None]
        out = points[rows, ix.clamp(min=0)]
        bad = ix < 0
        return torch.where(bad.reshape(bad.shape + (1,) * (out.dim() - 2)), torch.full_like(out, float("nan")), out) if bool(bad.any()) else out
    ix = np.asarray(index, np.int64)
    out = np.asarray(points)[np.arange(len(points))[:, None], np.maximum(ix, 0)].copy()
    out[ix < 0] = np.nan
    return out


def statistical_outlier_mask(sqdist, count, ratio=2.0):
    """True for the points to KEEP, from knn's sqdist [N,K,k] and count [N,K] of a self-query: the mean distance to the listed neighbours
    is at most the frame's mean of that figure plus ratio standard deviations.  A point without a neighbour is dropped.  Plain array
    arithmetic on the knn output (numpy or torch)."""
    xp = torch if _is_torch(sqdist) else np
    has = count > 0
    cnt = xp.maximum(count, xp.ones_like(count))
    mean_d = (sqdist ** 0.5).sum(-1) / (cnt.to(sqdist.dtype) if xp is torch else cnt.astype(sqdist.dtype))
    w = has.to(sqdist.dtype) if xp is torch else has.astype(sqdist.dtype)
    tot = xp.maximum(w.sum(-1, keepdims=True), xp.ones_like(w[..., :1]))
    mu = (mean_d * w).sum(-1, keepdims=True) / tot
    sd = (((mean_d - mu) ** 2 * w).sum(-1, keepdims=True) / tot) ** 0.5
    return has & (mean_d <= mu + ratio * sd)
