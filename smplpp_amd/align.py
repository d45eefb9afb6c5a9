"""Rigid and similarity alignment of point sets (smplpp_align, smplpp_align_vjp): per frame the rotation R, translation t and scale s
that minimise sum_k w_k |s R x_k + t - y_k|^2 over source x [N,K,3] and target y [1 or N,K,3], in closed form (Horn's quaternion
method), with a closed-form backward to both point sets.  It is the inner step of ICP (the rigid pre-alignment of a scan or a marker
cloud before pointMeshDistance / meshPointDistance), Procrustes-aligned evaluation (pa_mpjpe), and fitting "up to a rigid motion" with
the global pose eliminated inside the objective.  numpy arrays are host space (the call stages and synchronises, on `device`), torch
tensors device space (enqueued on torch's current stream); every number is produced by libsmplpp_hip.so.

transform [N,13] holds R row-major, t and s.  R is always a proper rotation: a mirrored target gets the best rotation.  A weight of 0
(or a point that is not finite) leaves a point out of the fit; `aligned` still moves every point.  status [N] int32: bit 0 no live
point (identity), bit 1 all live source points coincide (R = I), bit 2 gap <= min_gap (the rotation is not unique: collinear points,
say).  A frame with a status bit keeps its transform constant in the backward."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import SmplppError, check
from .smpl import _Call, _is_torch, _ptr, torch

MIN_GAP = 1e-3
_OUT = {"transform": (lambda n, K: (n, 13), "float32"), "aligned": (lambda n, K: (n, K, 3), "float32"), "energy": (lambda n, K: (n,), "float32"),
        "point_error": (lambda n, K: (n, K), "float32"), "gap": (lambda n, K: (n,), "float32"), "status": (lambda n, K: (n,), "int32")}


class _Args:
    """The inputs the two calls share, checked and in the call's space."""

    def __init__(self, name, source, target, weight, with_scale, min_gap, device, *more):
        c = self.c = _Call(name, source, target, *more)
        if len(source.shape) != 3 or source.shape[2] != 3 or min(source.shape) < 1:
            c.refuse("expected source of shape (N, K, 3)")
        self.n, self.K = n, K = int(source.shape[0]), int(source.shape[1])
        self.source = c.input(source, (n, K, 3))
        self.target, self.Tn = self.rows(target, (K, 3))
        self.weight, self.Wn = self.rows(weight, (K,))
        self.with_scale, self.min_gap = int(bool(with_scale)), float(min_gap)
        self.dev = int(c.device.index if c.dev and c.device.index is not None else device)

    def rows(self, a, shape):
        """target / weight: [1 or N, ...] (a missing leading axis means shared); returns (array, leading count)."""
        c = self.c
        if a is None:
            return None, 1
        if not _is_torch(a):
            a = np.ascontiguousarray(a, np.float32)
            if c.dev:  # a host table for a device call
                a = torch.from_numpy(a).to(c.device)
        if len(a.shape) == len(shape):
            a = a.reshape((1,) + tuple(a.shape))
        lead = int(a.shape[0])
        return c.input(a, (lead,) + shape), lead

    def head(self):
        return (self.dev, self.n, self.K, _ptr(self.source), _ptr(self.target), self.Tn, _ptr(self.weight), self.Wn, self.with_scale, self.min_gap)


def align(source, target, weight=None, with_scale=False, min_gap=MIN_GAP, want=tuple(_OUT), device=0):
    """The alignment of source [N,K,3] onto target [1 or N,K,3] under weight [1 or N,K] (None: ones) (smplpp_align): a dict of transform
    [N,13], aligned [N,K,3] = s R x + t for every point, energy [N] = sum w point_error, point_error [N,K] = |aligned - target|^2 (0
    where the point is left out), gap [N] = (l1 - l2) / (l1 - l4) of the 4 x 4 problem's eigenvalues, and status [N] int32."""
    a = _Args("align", source, target, weight, with_scale, min_gap, device)
    c = a.c
    if not want or any(k not in _OUT for k in want):
        c.refuse("want must name some of " + ", ".join(_OUT))
    res = {k: c.empty(_OUT[k][0](a.n, a.K), _OUT[k][1]) for k in want}
    check(_lib.load().smplpp_align(*a.head(), *(_ptr(res.get(k)) for k in _OUT), c.space, c.stream))
    return res


def alignBackward(source, target, weight=None, with_scale=False, min_gap=MIN_GAP, grad_transform=None, grad_aligned=None, grad_energy=None,
                  want=("source", "target"), out=None, device=0):
    """Vector-Jacobian product of align (smplpp_align_vjp) for dL/dtransform [N,13] (R as nine independent entries), dL/daligned
    [N,K,3] and dL/denergy [N] (any may be None, not all): {"source": [N,K,3], "target": [N,K,3]}.  "target" is per frame; with a shared
    target the caller sums it over the frames.  `want` drops one; with `out` (a dict keyed the same way) the gradients are added into its
    arrays and it is returned."""
    acc = out is not None
    a = _Args("alignBackward", source, target, weight, with_scale, min_gap, device, grad_transform, grad_aligned, grad_energy,
              *(out.values() if acc else ()))
    c, n, K = a.c, a.n, a.K
    gtr, gal, ge = c.input(grad_transform, (n, 13)), c.input(grad_aligned, (n, K, 3)), c.input(grad_energy, (n,))
    keys = [k for k in ("source", "target") if k in (out if acc else want)]
    if not keys:
        c.refuse("source or target must be asked for")
    res = {k: c.inout(out[k], (n, K, 3)) if acc else c.empty((n, K, 3)) for k in keys}
    check(_lib.load().smplpp_align_vjp(*a.head(), _ptr(gtr), _ptr(gal), _ptr(ge), _ptr(res.get("source")), _ptr(res.get("target")), int(acc),
                                       c.space, c.stream))
    return out if acc else res


def apply(transform, points):
    """s R x + t for points [N,K,3] under transform [N,13] (numpy or torch; plain array arithmetic, differentiable in torch)."""
    R = transform[:, :9].reshape(-1, 1, 3, 3)
    moved = (R * points[:, :, None, :]).sum(-1)
    return transform[:, None, 12:13] * moved + transform[:, None, 9:12]


def mpjpe(pred, gt):
    """Mean per-joint position error [N]: the mean over K of |pred - gt| (numpy or torch)."""
    d = pred - gt
    return ((d * d).sum(-1) ** 0.5).mean(-1)


def pa_mpjpe(pred, gt, device=0):
    """MPJPE after Procrustes alignment [N]: the similarity alignment of pred [N,K,3] onto gt by smplpp_align, then the mean over K of
    sqrt(point_error)."""
    pe = align(pred, gt, with_scale=True, want=("point_error",), device=device)["point_error"]
    return (pe ** 0.5).mean(-1)


# ---------------------------------------------------------------------------------------------------- torch.autograd
def align_differentiable(source, target, weight=None, with_scale=False, min_gap=MIN_GAP):
    """(transform [N,13], aligned [N,K,3], energy [N]) of the device tensors source [N,K,3] and target [1 or N,K,3], differentiable in
    both: smplpp_align forward, smplpp_align_vjp backward, on torch's current stream.  No gradient flows to the weights."""
    if torch is None or not (_is_torch(source) and _is_torch(target)):
        raise SmplppError(1, "align_differentiable needs torch device tensors")
    return _AlignFunction.apply(source, target, weight, bool(with_scale), float(min_gap))


if torch is not None:
    class _AlignFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, source, target, weight, with_scale, min_gap):
            x, y = source.detach().contiguous(), target.detach().contiguous()
            ctx.args = (with_scale, min_gap)
            ctx.target_shape = tuple(target.shape)
            # a weight tensor is saved with the others, so that a change in place before the backward is noticed
            ctx.host_weight = None if _is_torch(weight) else weight
            ctx.save_for_backward(x, y, *((weight,) if _is_torch(weight) else ()))
            r = align(x, y, weight, with_scale, min_gap, want=("transform", "aligned", "energy"))
            return r["transform"], r["aligned"], r["energy"]

        @staticmethod
        def backward(ctx, g_transform, g_aligned, g_energy):
            want = tuple(k for k, need in zip(("source", "target"), ctx.needs_input_grad[:2]) if need)
            if not want:
                return (None,) * 5
            x, y, *w = ctx.saved_tensors
            g = alignBackward(x, y, w[0] if w else ctx.host_weight, *ctx.args, grad_transform=g_transform.contiguous(), grad_aligned=g_aligned.contiguous(),
                              grad_energy=g_energy.contiguous(), want=want)
            gt = g.get("target")
            if gt is not None and tuple(gt.shape) != ctx.target_shape:  # a shared target: the frames' gradients are summed
                gt = gt.sum(0, keepdim=len(ctx.target_shape) == 3).reshape(ctx.target_shape)
            return (g.get("source"), gt) + (None,) * 3
