"""The scene term (smplpp_volume_*, smplpp_scene_term, smplpp_scene_term_vjp): a signed-distance grid of a static scene kept on the
device, sampled at the body's points by trilinear interpolation, with a penetration energy on negative samples, a robust contact energy
that pulls chosen points to distance 0, and the gradient to the points.  numpy arrays are host space (the call stages and synchronises),
torch tensors device space (enqueued on torch's current stream); every number is produced by libsmplpp_hip.so.

A person-person term composes from what is here: sample body A's signed distance at the grid nodes, refresh the volume on the device,
and evaluate the term on body B (no gradient flows to A):

    nodes = torch.stack(torch.meshgrid(zs, ys, xs, indexing="ij"), -1).flip(-1).reshape(1, -1, 3)   # [1, Gz Gy Gx, 3], x fastest
    *_, inside, sq = smpl.pointMeshSignedDistance(verts_a, nodes)                                  # signed SQUARED distances
    vol.set((sq.sign() * sq.abs().sqrt()).reshape(Gz, Gy, Gx))                                     # one kernel, no synchronisation
    energy = vol.term_differentiable(verts_b, w_pen, None, 0.0)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SmplppError, check
from .smpl import _Call, _is_torch, _ptr, parse_device, torch

LAYOUTS = ("linear", "cells")


class Volume:
    """values [Gz,Gy,Gx]: node (i, j, k) holds values[k, j, i] and sits at origin + (i hx, j hy, k hz) in volume coordinates, which a
    world point reaches through world_to_volume ([3,4] or [12] row-major [R|t]; None: the identity).  values may be a numpy array (host
    space) or a float32 device tensor; None with `shape` = (Gz, Gy, Gx) makes a grid of zeros to be filled by set().  The storage layout
    (info()["layout"]) is chosen at creation, SMPLPP_VOLUME_LAYOUT=linear|cells forces one; no output bit depends on it."""

    def __init__(self, device, values, origin, spacing, world_to_volume=None, shape=None):
        self._h = None
        self._device = parse_device(device)
        if values is None:
            if shape is None or len(shape) != 3:
                raise SmplppError(1, "Volume: values [Gz,Gy,Gx], or shape = (Gz, Gy, Gx)")
            space, stream = _lib.HOST, None
        else:
            c = _Call("Volume", values)
            if len(values.shape) != 3:
                c.refuse("expected values of shape (Gz, Gy, Gx)")
            shape = tuple(int(s) for s in values.shape)
            values, space = c.input(values, shape), c.space
        o = (C.c_float * 3)(*np.asarray(origin, np.float32).reshape(3).tolist())
        h = (C.c_float * 3)(*np.asarray(spacing, np.float32).reshape(3).tolist())
        xf = None if world_to_volume is None else (C.c_float * 12)(*np.asarray(world_to_volume, np.float32).reshape(12).tolist())
        handle = C.c_void_p()
        check(_lib.load().smplpp_volume_create(self._device, int(shape[2]), int(shape[1]), int(shape[0]), o, h, xf, _ptr(values), space, C.byref(handle)))
        self._h = handle
        self.shape = tuple(int(s) for s in shape)
        self.layout = self.info()["layout"]

    def __del__(self):
        try:
            if self._h:
                _lib.load().smplpp_volume_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise SmplppError(4, "Volume: no volume")
        return self._h

    def info(self):
        G, o, h, xf, layout = (C.c_int64 * 3)(), (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 12)(), C.c_int()
        check(_lib.load().smplpp_volume_info(self.handle, G, o, h, xf, C.byref(layout)))
        return dict(G=tuple(G), origin=np.array(list(o), np.float32), spacing=np.array(list(h), np.float32),
                    world_to_volume=np.array(list(xf), np.float32).reshape(3, 4), layout=LAYOUTS[layout.value])

    def set(self, values):
        """New node values [Gz,Gy,Gx] (smplpp_volume_set).  A float32 device tensor: one kernel on torch's current stream, no allocation
        and no synchronisation, so a grid can be refreshed inside an optimisation loop."""
        c = _Call("set", values)
        v = c.input(values, self.shape)
        check(_lib.load().smplpp_volume_set(self.handle, _ptr(v), c.space, c.stream))
        return self

    # ------------------------------------------------------------------------------------------------ sampling and the term
    def _points(self, c, points):
        if len(points.shape) != 3 or points.shape[2] != 3 or min(points.shape) < 1:
            c.refuse("expected points of shape (N, K, 3)")
        n, K = int(points.shape[0]), int(points.shape[1])
        return n, K, c.input(points, (n, K, 3))

    def _weight(self, c, w, K):
        if w is None:
            return None
        if c.dev and not _is_torch(w):  # a host table for a device call
            w = torch.from_numpy(np.ascontiguousarray(w, np.float32).reshape(-1)).to(c.device)
        return c.input(w, (K,))

    def sample(self, points, want=("value", "gradient", "valid")):
        """The volume at world points [N,K,3] (smplpp_volume_sample): a dict of value [N,K], gradient [N,K,3] (d value / d point) and
        valid [N,K] uint8.  A point outside the grid, not finite, or in a cell with a node that is not finite gives valid 0, value 0 and
        gradient 0."""
        c = _Call("sample", points)
        n, K, p = self._points(c, points)
        shapes = {"value": ((n, K), "float32"), "gradient": ((n, K, 3), "float32"), "valid": ((n, K), "uint8")}
        if not want or any(k not in shapes for k in want):
            c.refuse("want must name some of value, gradient, valid")
        res = {k: c.empty(*shapes[k]) for k in want}
        check(_lib.load().smplpp_volume_sample(self.handle, n, K, _ptr(p), _ptr(res.get("value")), _ptr(res.get("gradient")), _ptr(res.get("valid")),
                                               c.space, c.stream))
        return res

    def term(self, points, w_pen=None, w_con=None, rho=0.0, want=("energy", "point_energy", "value", "valid")):
        """Penetration and contact of world points [N,K,3] (smplpp_scene_term): a dict of energy [N], point_energy [N,K], value [N,K]
        and valid [N,K] uint8.  With s the sample: w_pen[k] s^2 where s < 0 (w_pen None: ones), plus w_con[k] s^2 (w_con None: zeros),
        which rho > 0 makes the Geman-McClure form w_con rho^2 s^2 / (rho^2 + s^2).  A point that is not valid has energy 0."""
        c = _Call("term", points)
        n, K, p = self._points(c, points)
        wp, wc = self._weight(c, w_pen, K), self._weight(c, w_con, K)
        shapes = {"energy": ((n,), "float32"), "point_energy": ((n, K), "float32"), "value": ((n, K), "float32"), "valid": ((n, K), "uint8")}
        if not want or any(k not in shapes for k in want):
            c.refuse("want must name some of energy, point_energy, value, valid")
        res = {k: c.empty(*shapes[k]) for k in want}
        check(_lib.load().smplpp_scene_term(self.handle, n, K, _ptr(p), _ptr(wp), _ptr(wc), float(rho), _ptr(res.get("energy")),
                                            _ptr(res.get("point_energy")), _ptr(res.get("value")), _ptr(res.get("valid")), c.space, c.stream))
        return res

    def termBackward(self, points, w_pen=None, w_con=None, rho=0.0, grad_energy=None, grad_point_energy=None, grad_value=None, out=None):
        """Vector-Jacobian product of term to the points (smplpp_scene_term_vjp) for dL/denergy [N], dL/dpoint_energy [N,K] and
        dL/dvalue [N,K] (any may be None, not all).  Returns grad_points [N,K,3]; with `out` the gradient is added into it and it is
        returned."""
        acc = out is not None
        c = _Call("termBackward", points, grad_energy, grad_point_energy, grad_value, out)
        n, K, p = self._points(c, points)
        wp, wc = self._weight(c, w_pen, K), self._weight(c, w_con, K)
        ge, gpe, gv = c.input(grad_energy, (n,)), c.input(grad_point_energy, (n, K)), c.input(grad_value, (n, K))
        res = c.inout(out, (n, K, 3)) if acc else c.empty((n, K, 3))
        check(_lib.load().smplpp_scene_term_vjp(self.handle, n, K, _ptr(p), _ptr(wp), _ptr(wc), float(rho), _ptr(ge), _ptr(gpe), _ptr(gv), _ptr(res),
                                                int(acc), c.space, c.stream))
        return out if acc else res

    # ------------------------------------------------------------------------------------------------ torch.autograd
    def _need_torch(self, name, *tensors):
        if torch is None or not all(_is_torch(t) for t in tensors):
            raise SmplppError(1, "%s needs torch device tensors" % name)

    def sample_differentiable(self, points):
        """value [N,K] of the device tensor points [N,K,3], differentiable in the points: smplpp_volume_sample forward,
        smplpp_scene_term_vjp (the cotangent of value alone) backward, on torch's current stream."""
        self._need_torch("sample_differentiable", points)
        return _SampleFunction.apply(points, self)

    def term_differentiable(self, points, w_pen=None, w_con=None, rho=0.0):
        """energy [N] of the device tensor points [N,K,3] (the arguments of term), differentiable in the points: smplpp_scene_term
        forward, smplpp_scene_term_vjp backward.  It composes with SMPL.forward_differentiable, forward_rotmat_differentiable and
        forward_displaced_differentiable: their vertices are the points."""
        self._need_torch("term_differentiable", points)
        return _TermFunction.apply(points, self, w_pen, w_con, float(rho))


if torch is not None:
    class _SampleFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, points, vol):
            p = points.detach().contiguous()
            ctx.vol = vol
            ctx.save_for_backward(p)
            return vol.sample(p, want=("value",))["value"]

        @staticmethod
        def backward(ctx, grad):
            if not ctx.needs_input_grad[0]:
                return None, None
            (p,) = ctx.saved_tensors
            return ctx.vol.termBackward(p, None, None, 0.0, grad_value=grad.contiguous()), None

    class _TermFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, points, vol, w_pen, w_con, rho):
            p = points.detach().contiguous()
            ctx.vol, ctx.args = vol, (w_pen, w_con, rho)
            ctx.save_for_backward(p)
            return vol.term(p, w_pen, w_con, rho, want=("energy",))["energy"]

        @staticmethod
        def backward(ctx, grad):
            if not ctx.needs_input_grad[0]:
                return (None,) * 5
            (p,) = ctx.saved_tensors
            return (ctx.vol.termBackward(p, *ctx.args, grad_energy=grad.contiguous()),) + (None,) * 4
