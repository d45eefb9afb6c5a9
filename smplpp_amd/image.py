"""The image term (smplpp_image_sample, smplpp_image_term, smplpp_image_term_vjp): a dense channels-last image [B,H,W,C] that a network
produced (joint heatmaps, feature or colour maps, flow, a distance map) read at the unsnapped uv [N,K,2] of project_points by bilinear
interpolation, a robust squared residual against a target, and the gradient to uv AND to the image.  Pixel (row j, column i) has its
centre at (i + 0.5, j + 0.5), the rasteriser's convention.  numpy arrays are host space (the call stages and synchronises, on
`device`), torch tensors device space (enqueued on torch's current stream); every number is produced by libsmplpp_hip.so.

B is 1 (one image for every frame: a texture) or N.  With channel [K] (integers), point k reads channel channel[k] alone and the
sampled channel count Cs is 1: heatmap j for joint j.  A network's NCHW output becomes channels-last by

    image = heat.permute(0, 2, 3, 1).contiguous()

The gradient to the image makes the same call texture and appearance estimation: the image is the unknown, shared by all frames
(B = 1), and the points are the pixels' UVs from raster_interpolate.  It is a gather in ascending point index, bit-reproducible; its cost
grows with (image tiles) x (points)."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import SmplppError, check
from .smpl import _Call, _is_torch, _ptr, torch


class _Args:
    """The inputs the three calls share, checked and in the call's space."""

    def __init__(self, name, uv, image, channel, device, *more):
        c = self.c = _Call(name, uv, image, *more)
        if len(uv.shape) != 3 or uv.shape[2] != 2 or min(uv.shape) < 1:
            c.refuse("expected uv of shape (N, K, 2)")
        if len(image.shape) != 4:
            c.refuse("expected a channels-last image of shape (B, H, W, C)")
        self.n, self.K = int(uv.shape[0]), int(uv.shape[1])
        self.B, self.H, self.W, self.C = (int(s) for s in image.shape)
        self.uv, self.image = c.input(uv, (self.n, self.K, 2)), c.input(image, (self.B, self.H, self.W, self.C))
        self.channel = None if channel is None else c.ids(channel)
        if self.channel is not None and self.channel.shape != (self.K,):
            c.refuse("expected channel of shape (K,)")
        self.Cs = self.C if channel is None else 1
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
        return (self.dev, self.n, self.K, _ptr(self.uv), _ptr(self.image), self.B, self.H, self.W, self.C, _ptr(self.channel))


def sample(uv, image, channel=None, want=("value", "gradient", "valid"), device=0):
    """The image at uv [N,K,2] (smplpp_image_sample): a dict of value [N,K,Cs], gradient [N,K,Cs,2] = (d value / du, d value / dv) in
    pixels, and valid [N,K] uint8.  A point outside the pixel centres' rectangle, not finite, or in a cell with a pixel that is not
    finite (in a sampled channel) gives valid 0, value 0 and gradient 0."""
    a = _Args("sample", uv, image, channel, device)
    c, n, K, Cs = a.c, a.n, a.K, a.Cs
    shapes = {"value": ((n, K, Cs), "float32"), "gradient": ((n, K, Cs, 2), "float32"), "valid": ((n, K), "uint8")}
    if not want or any(k not in shapes for k in want):
        c.refuse("want must name some of value, gradient, valid")
    res = {k: c.empty(*shapes[k]) for k in want}
    check(_lib.load().smplpp_image_sample(*a.head(), _ptr(res.get("value")), _ptr(res.get("gradient")), _ptr(res.get("valid")), c.space, c.stream))
    return res


def term(uv, image, target=None, weight=None, rho=0.0, channel=None, want=("energy", "point_energy", "value", "valid"), device=0):
    """The squared residual of the sample against target [1 or N,K,Cs] (None: zeros) under weight [1 or N,K] (None: ones)
    (smplpp_image_term): a dict of energy [N], point_energy [N,K], value [N,K,Cs] and valid [N,K] uint8.  With q the sum of squared
    residuals over the sampled channels, point_energy = weight q, which rho > 0 makes the Geman-McClure form weight rho^2 q /
    (rho^2 + q).  A point that is not valid has energy 0; a point with weight 0 reads nothing of the image or the target."""
    a = _Args("term", uv, image, channel, device)
    c, n, K, Cs = a.c, a.n, a.K, a.Cs
    (t, Tn), (w, Wn) = a.rows(target, (K, Cs)), a.rows(weight, (K,))
    shapes = {"energy": ((n,), "float32"), "point_energy": ((n, K), "float32"), "value": ((n, K, Cs), "float32"), "valid": ((n, K), "uint8")}
    if not want or any(k not in shapes for k in want):
        c.refuse("want must name some of energy, point_energy, value, valid")
    res = {k: c.empty(*shapes[k]) for k in want}
    check(_lib.load().smplpp_image_term(*a.head(), _ptr(t), Tn, _ptr(w), Wn, float(rho), _ptr(res.get("energy")), _ptr(res.get("point_energy")),
                                        _ptr(res.get("value")), _ptr(res.get("valid")), c.space, c.stream))
    return res


def termBackward(uv, image, target=None, weight=None, rho=0.0, channel=None, grad_energy=None, grad_point_energy=None, grad_value=None,
                 want=("uv", "image"), out=None, device=0):
    """Vector-Jacobian product of term (smplpp_image_term_vjp) for dL/denergy [N], dL/dpoint_energy [N,K] and dL/dvalue [N,K,Cs] (any
    may be None, not all): {"uv": [N,K,2], "image": [B,H,W,C]}.  `want` drops one; with `out` (a dict keyed the same way) the gradients
    are added into its arrays and it is returned.  Each element of "image" is one sum in ascending point index: the same bits on every run."""
    acc = out is not None
    a = _Args("termBackward", uv, image, channel, device, grad_energy, grad_point_energy, grad_value, *(out.values() if acc else ()))
    c, n, K, Cs = a.c, a.n, a.K, a.Cs
    (t, Tn), (w, Wn) = a.rows(target, (K, Cs)), a.rows(weight, (K,))
    ge, gpe, gv = c.input(grad_energy, (n,)), c.input(grad_point_energy, (n, K)), c.input(grad_value, (n, K, Cs))
    shapes = {"uv": (n, K, 2), "image": (a.B, a.H, a.W, a.C)}
    keys = [k for k in shapes if k in (out if acc else want)]
    if not keys:
        c.refuse("uv or image must be asked for")
    res = {k: c.inout(out[k], shapes[k]) if acc else c.empty(shapes[k]) for k in keys}
    check(_lib.load().smplpp_image_term_vjp(*a.head(), _ptr(t), Tn, _ptr(w), Wn, float(rho), _ptr(ge), _ptr(gpe), _ptr(gv), _ptr(res.get("uv")),
                                            _ptr(res.get("image")), int(acc), c.space, c.stream))
    return out if acc else res


# ---------------------------------------------------------------------------------------------------- torch.autograd
def _need_torch(name, *tensors):
    if torch is None or not all(_is_torch(t) for t in tensors):
        raise SmplppError(1, "%s needs torch device tensors" % name)


def sample_differentiable(uv, image, channel=None):
    """value [N,K,Cs] of the device tensors uv [N,K,2] and image [B,H,W,C], differentiable in both: smplpp_image_sample forward,
    smplpp_image_term_vjp (the cotangent of value alone) backward, on torch's current stream.  uv may come from
    project_points_differentiable, so the chain reaches the points and the camera."""
    _need_torch("sample_differentiable", uv, image)
    return _SampleFunction.apply(uv, image, channel)


def term_differentiable(uv, image, target=None, weight=None, rho=0.0, channel=None):
    """energy [N] of the device tensors uv [N,K,2] and image [B,H,W,C] (the arguments of term), differentiable in uv and in the image:
    smplpp_image_term forward, smplpp_image_term_vjp backward.  No gradient flows to target or weight (a gradient to the target
    composes from sample_differentiable)."""
    _need_torch("term_differentiable", uv, image)
    return _TermFunction.apply(uv, image, target, weight, float(rho), channel)


if torch is not None:
    def _wanted(ctx):
        return tuple(k for k, need in zip(("uv", "image"), ctx.needs_input_grad[:2]) if need)

    class _SampleFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, uv, image, channel):
            u, im = uv.detach().contiguous(), image.detach().contiguous()
            ctx.channel = channel
            ctx.save_for_backward(u, im)
            return sample(u, im, channel, want=("value",))["value"]

        @staticmethod
        def backward(ctx, grad):
            want = _wanted(ctx)
            if not want:
                return None, None, None
            u, im = ctx.saved_tensors
            g = termBackward(u, im, None, None, 0.0, ctx.channel, grad_value=grad.contiguous(), want=want)
            return g.get("uv"), g.get("image"), None

    class _TermFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, uv, image, target, weight, rho, channel):
            u, im = uv.detach().contiguous(), image.detach().contiguous()
            ctx.args = (target, weight, rho, channel)
            ctx.save_for_backward(u, im)
            return term(u, im, target, weight, rho, channel, want=("energy",))["energy"]

        @staticmethod
        def backward(ctx, grad):
            want = _wanted(ctx)
            if not want:
                return (None,) * 6
            u, im = ctx.saved_tensors
            g = termBackward(u, im, *ctx.args, grad_energy=grad.contiguous(), want=want)
            return (g.get("uv"), g.get("image")) + (None,) * 4
