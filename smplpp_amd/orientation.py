"""The orientation term on world joint frames (smplpp_orientation_term, smplpp_orientation_term_vjp) and the vector-Jacobian product of
the Rodrigues formula (smplpp_axis_angle_to_rotmat_vjp): what consumes the orientations SMPL.skeleton returns.  Per frame and sensor s the
residual E = A O - T of the 3 x 3 block A of joint joint[s] in frames [N,J,3,4] (the `world` of skeleton, read in place) or [N,J,3,3]
(any stack of matrices), through a bone-to-sensor offset O [S,3,C], against a target T [1 or N,S,3,C]; its energy w |E|^2, or the
Geman-McClure form of it for rho > 0; the frame's energy; and the gradients to the frames, the offsets (summed over the frames: the
calibration gradient) and the target.  C = 3 compares whole orientations, where |E|^2 = 4 (1 - cos phi) for the geodesic angle phi;
C = 1 or 2 the images of bone-frame axes.  A sensor with weight 0, a joint index outside [0, J) or an entry that is not finite is dead:
+0 everywhere.  numpy arrays are host space (the call stages and synchronises, on `device`), torch tensors device space (enqueued on
torch's current stream); every number is produced by libsmplpp_hip.so.

Fitting to IMU orientations, by hand (the gradient lands in the grad_world buffer, column 3 untouched) or through autograd:

    sk = smpl.skeleton(beta, theta, want=("world",))
    e = orientation.term(sk["world"], joint, target, offset, want=("energy",))["energy"]
    gw = torch.zeros_like(sk["world"])                                                    # or the caller's grad_world, already filled
    orientation.termBackward(sk["world"], joint, target, offset, grad_energy=torch.ones_like(e), out={"frames": gw})
    g = smpl.skeletonBackward(beta, theta, grad_world=gw)                                  # {"beta", "theta"}

    world, posed, _ = smpl.skeleton_differentiable(beta, theta)
    energy, sensor_energy, _ = orientation.term_differentiable(world, joint, target, offset)   # offset.requires_grad: calibration
    (energy.sum() + ((posed[:, 0] - root) ** 2).sum()).backward()
    degrees = torch.rad2deg(orientation.geodesic_angle(sensor_energy.detach()))            # with weights of 1 and rho = 0

Chordal smoothness of the rotations of a sequence, end to end to theta (layout: a sequence.SequenceLayout over the frames):

    rot = orientation.axis_angle_to_rotmat_differentiable(theta[:, 1:])                    # [F,24,3,3]
    smooth = layout.smoothness_differentiable(rot.reshape(-1, 24, 9), order=1, K=24, C=9)   # [F], sum |R[f+1] - R[f]|^2 per frame
    smooth.sum().backward()                                                                # theta.grad through the Rodrigues VJP

A foot kept flat on the ground: one bone-frame axis per foot against a target shared by all frames (C = 1, Tn = 1):

    up = torch.tensor([[[0.], [1.], [0.]]] * 2, device=dev)                                # the feet's up axis in their bone frames [2,3,1]
    normal = torch.tensor([[[0.], [1.], [0.]]] * 2, device=dev)                            # the ground normal [2,3,1], shared
    energy, _, _ = orientation.term_differentiable(world, [7, 8], normal, up, weight=contact, C=1)   # contact [N,2]: 0 lifts a foot
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import SmplppError, check
from .smpl import _Call, _is_torch, _np32, _ptr, torch

_OUT = {"energy": lambda n, S, C: (n,), "sensor_energy": lambda n, S, C: (n, S), "residual": lambda n, S, C: (n, S, 3, C)}
_GRAD = ("frames", "offset", "target")


class _Args:
    """The inputs the two calls share, checked and in the call's space."""

    def __init__(self, name, frames, joint, target, offset, weight, rho, C, device, *more):
        c = self.c = _Call(name, frames, target, *more)
        sh = tuple(frames.shape)
        if len(sh) != 4 or sh[2] != 3 or sh[3] not in (3, 4) or min(sh) < 1:
            c.refuse("expected frames of shape (N, J, 3, 3) or (N, J, 3, 4)")
        self.n, self.J, self.rs = n, J, rs = int(sh[0]), int(sh[1]), int(sh[3])
        self.frames = c.input(frames, (n, J, 3, rs))
        self.joint = c.ids(joint)
        self.S = S = int(self.joint.shape[0])
        if C is None:
            C = int(target.shape[-1])
        self.C = C = int(C)
        if S < 1 or C not in (1, 2, 3):
            c.refuse("expected at least one sensor and C of 1, 2 or 3")
        self.target, self.Tn = self.rows(target, (S, 3, C))
        self.weight, self.Wn = self.rows(weight, (S,))
        self.offset = self.rows(offset, (S, 3, C), lead=False)[0]
        self.rho = float(rho)
        self.dev = int(c.device.index if c.dev and c.device.index is not None else device)

    def rows(self, a, shape, lead=True):
        """target / weight: [1 or N, ...] (a missing leading axis means shared); returns (array, leading count)."""
        c = self.c
        if a is None:
            return None, 1
        if not _is_torch(a):
            a = np.ascontiguousarray(a, np.float32)
            if c.dev:  # a host table for a device call
                a = torch.from_numpy(a).to(c.device)
        if not lead:
            return c.input(a, shape), 1
        if len(a.shape) == len(shape):
            a = a.reshape((1,) + tuple(a.shape))
        n = int(a.shape[0])
        return c.input(a, (n,) + shape), n

    def head(self):
        return (self.dev, self.n, self.J, self.rs, _ptr(self.frames), self.S, self.C, _ptr(self.joint), _ptr(self.offset), _ptr(self.target),
                self.Tn, _ptr(self.weight), self.Wn, self.rho)


def term(frames, joint, target, offset=None, weight=None, rho=0.0, C=None, want=tuple(_OUT), device=0):
    """The orientation term (smplpp_orientation_term) of frames [N,J,3,4] or [N,J,3,3], joint [S] (integers), target [1 or N,S,3,C] (or
    [S,3,C]: shared), offset [S,3,C] (None: the first C columns of the identity), weight [1 or N,S] or [S] (None: ones): a dict of
    energy [N], sensor_energy [N,S] and residual [N,S,3,C] = A O - T.  C defaults to the target's last axis."""
    a = _Args("term", frames, joint, target, offset, weight, rho, C, device)
    c = a.c
    if not want or any(k not in _OUT for k in want):
        c.refuse("want must name some of " + ", ".join(_OUT))
    res = {k: c.empty(_OUT[k](a.n, a.S, a.C)) for k in want}
    check(_lib.load().smplpp_orientation_term(*a.head(), *(_ptr(res.get(k)) for k in _OUT), c.space, c.stream))
    return res


def termBackward(frames, joint, target, offset=None, weight=None, rho=0.0, C=None, grad_energy=None, grad_sensor_energy=None,
                 grad_residual=None, want=_GRAD, out=None, device=0):
    """Vector-Jacobian product of term (smplpp_orientation_term_vjp) for dL/denergy [N], dL/dsensor_energy [N,S] and dL/dresidual
    [N,S,3,C] (any may be None, not all): {"frames": the shape of frames (3 x 3 entries only; column 3 of an [N,J,3,4] array is +0, or
    with `out` untouched), "offset": [S,3,C] summed over the frames, "target": the shape of the target as passed to the call (summed
    over the frames when it is shared)}.  `want` drops some; with `out` (a dict keyed the same way) the gradients are added into its
    arrays and it is returned: out={"frames": grad_world} puts the term's gradient beside what the caller already has for
    skeletonBackward."""
    acc = out is not None
    a = _Args("termBackward", frames, joint, target, offset, weight, rho, C, device, grad_energy, grad_sensor_energy, grad_residual,
              *(out.values() if acc else ()))
    c, n, S, Cc = a.c, a.n, a.S, a.C
    ge, gse, gr = c.input(grad_energy, (n,)), c.input(grad_sensor_energy, (n, S)), c.input(grad_residual, (n, S, 3, Cc))
    if ge is None and gse is None and gr is None:
        c.refuse("grad_energy, grad_sensor_energy or grad_residual must be given")
    shapes = {"frames": (n, a.J, 3, a.rs), "offset": (S, 3, Cc), "target": (a.Tn, S, 3, Cc)}
    keys = [k for k in _GRAD if k in (out if acc else want)]
    if not keys:
        c.refuse("frames, offset or target must be asked for")
    res = {}
    for k in keys:
        if acc:
            o = out[k]
            res[k] = c.inout(o.reshape(shapes[k]) if k == "target" and len(o.shape) == 3 and a.Tn == 1 else o, shapes[k])
        elif k == "frames" and a.rs == 4:  # column 3 is never written
            res[k] = torch.zeros(shapes[k], dtype=torch.float32, device=c.device) if c.dev else np.zeros(shapes[k], np.float32)
        else:
            res[k] = c.empty(shapes[k])
    check(_lib.load().smplpp_orientation_term_vjp(*a.head(), _ptr(ge), _ptr(gse), _ptr(gr), *(_ptr(res.get(k)) for k in _GRAD), int(acc),
                                                  c.space, c.stream))
    return out if acc else res


def geodesic_angle(sensor_q):
    """The angle, in radians, between the two rotations of a C = 3 sensor from its squared chordal distance q = |A O - T|^2 = 4 (1 -
    cos phi): 2 asin(min(1, sqrt(q) / (2 sqrt 2))).  sensor_energy is q at weight 1 and rho = 0.  Plain array arithmetic (numpy or
    torch), meant for reporting: no gradient is defined at 0."""
    if _is_torch(sensor_q):
        return 2.0 * torch.asin(torch.clamp(torch.sqrt(sensor_q.detach()) / (2.0 * 2.0 ** 0.5), max=1.0))
    q = np.asarray(sensor_q)
    return 2.0 * np.arcsin(np.minimum(1.0, np.sqrt(q) / (2.0 * np.sqrt(2.0))))


# ---------------------------------------------------------------------------------------------------- the Rodrigues formula and its VJP
def _aa_rows(c, aa):
    shape = tuple(aa.shape) if c.dev else np.shape(aa)
    if not shape or shape[-1] != 3 or int(np.prod(shape)) == 0:
        c.refuse("expected axis-angles of shape (..., 3)")
    rows = int(np.prod(shape[:-1]))
    return shape, rows, c.input(aa.reshape(rows, 3) if c.dev else _np32(aa).reshape(rows, 3), (rows, 3))


def axis_angle_to_rotmat(aa, device=0):
    """Axis-angles [..., 3] as rotation matrices [..., 3, 3] (smplpp_axis_angle_to_rotmat; SMPL.axisAngleToRotmat without a model)."""
    c = _Call("axis_angle_to_rotmat", aa)
    shape, rows, aa = _aa_rows(c, aa)
    dev = int(c.device.index if c.dev and c.device.index is not None else device)
    rot = c.empty((rows, 3, 3))
    check(_lib.load().smplpp_axis_angle_to_rotmat(dev, rows, _ptr(aa), _ptr(rot), c.space, c.stream))
    return rot.reshape(tuple(shape[:-1]) + (3, 3))


def axis_angle_to_rotmat_backward(aa, grad_rot, out=None, device=0):
    """dL/daa [..., 3] for dL/drot = grad_rot [..., 3, 3], nine independent entries per matrix (smplpp_axis_angle_to_rotmat_vjp): the
    derivative of the reference's Rodrigues formula that skeletonBackward and launchBackward contract with, finite at aa = 0 and at
    |aa| = pi.  With `out` [..., 3] the gradient is added into it and it is returned."""
    c = _Call("axis_angle_to_rotmat_backward", aa, grad_rot, out)
    shape, rows, aa = _aa_rows(c, aa)
    dev = int(c.device.index if c.dev and c.device.index is not None else device)
    if tuple(grad_rot.shape) != tuple(shape[:-1]) + (3, 3):
        c.refuse("expected grad_rot of shape %s" % (tuple(shape[:-1]) + (3, 3),))
    g = c.input(grad_rot.reshape(rows, 3, 3) if c.dev else _np32(grad_rot).reshape(rows, 3, 3), (rows, 3, 3))
    res = c.inout(out, tuple(shape)) if out is not None else c.empty(tuple(shape))
    check(_lib.load().smplpp_axis_angle_to_rotmat_vjp(dev, rows, _ptr(aa), _ptr(g), _ptr(res), int(out is not None), c.space, c.stream))
    return out if out is not None else res


# ---------------------------------------------------------------------------------------------------- torch.autograd
def term_differentiable(frames, joint, target, offset=None, weight=None, rho=0.0, C=3):
    """(energy [N], sensor_energy [N,S], residual [N,S,3,C]) of the device tensors frames [N,J,3,4] or [N,J,3,3], target and offset,
    differentiable in all three: smplpp_orientation_term forward, smplpp_orientation_term_vjp backward, on torch's current stream.
    frames takes skeleton_differentiable's world as it is.  No gradient flows to the weights."""
    if torch is None or not (_is_torch(frames) and _is_torch(target)):
        raise SmplppError(1, "term_differentiable needs torch device tensors")
    return _TermFunction.apply(frames, target, offset, joint, weight, float(rho), int(C))


def axis_angle_to_rotmat_differentiable(aa):
    """Rotation matrices [..., 3, 3] of the device tensor aa [..., 3], differentiable in aa: smplpp_axis_angle_to_rotmat forward,
    smplpp_axis_angle_to_rotmat_vjp backward, on torch's current stream."""
    if torch is None or not _is_torch(aa):
        raise SmplppError(1, "axis_angle_to_rotmat_differentiable needs a torch device tensor")
    return _RodriguesFunction.apply(aa)


if torch is not None:
    class _TermFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, frames, target, offset, joint, weight, rho, C):
            f, t = frames.detach().contiguous(), target.detach().contiguous()
            o = offset.detach().contiguous() if _is_torch(offset) else offset
            j = _Call("term_differentiable", f).ids(joint)
            ctx.args = (rho, C)
            ctx.target_shape = tuple(target.shape)
            ctx.host = (None if _is_torch(o) else o, None if _is_torch(weight) else weight)
            ctx.has = (_is_torch(o), _is_torch(weight))
            ctx.save_for_backward(f, t, j, *((o,) if _is_torch(o) else ()), *((weight,) if _is_torch(weight) else ()))
            ctx.set_materialize_grads(False)
            r = term(f, j, t, o, weight, rho, C)
            return r["energy"], r["sensor_energy"], r["residual"]

        @staticmethod
        def backward(ctx, g_energy, g_sensor, g_residual):
            need = dict(zip(_GRAD, (ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[1])))
            want = tuple(k for k in _GRAD if need[k])
            if not want or (g_energy is None and g_sensor is None and g_residual is None):
                return (None,) * 7
            f, t, j, *rest = ctx.saved_tensors
            o = rest.pop(0) if ctx.has[0] else ctx.host[0]
            w = rest.pop(0) if ctx.has[1] else ctx.host[1]
            cot = [None if g is None else g.contiguous() for g in (g_energy, g_sensor, g_residual)]
            g = termBackward(f, j, t, o, w, *ctx.args, grad_energy=cot[0], grad_sensor_energy=cot[1], grad_residual=cot[2], want=want)
            gt = g.get("target")
            if gt is not None:
                gt = gt.reshape(ctx.target_shape)
            return (g.get("frames"), gt, g.get("offset")) + (None,) * 4

    class _RodriguesFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, aa):
            a = aa.detach().contiguous()
            ctx.save_for_backward(a)
            return axis_angle_to_rotmat(a)

        @staticmethod
        def backward(ctx, g_rot):
            (a,) = ctx.saved_tensors
            return axis_angle_to_rotmat_backward(a, g_rot.contiguous())
