"""Pose priors for fitting theta directly (smplpp_pose_prior_create / smplpp_pose_prior / smplpp_pose_prior_vjp): a max-mixture
Gaussian prior over D pose coordinates and one-sided quadratic joint limits, the two pose terms a single-view fit pairs with the
keypoint energy.  numpy arrays are host space (the call stages and synchronises), torch tensors device space (enqueued on torch's
current stream); every number is produced by libsmplpp_hip.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SmplppError, check
from .smpl import _Call, _is_torch, _ptr, parse_device, torch

BODY_POSE_DIM = 69   # theta [25,3] without the root translation (row 0) and the root rotation (row 1)
THETA_OFFSET, THETA_LD = 6, 75


def gmm_tables(means, covars, weights):
    """(mean [M,D], mat [M,D,D], offset [M]) in float32 from a Gaussian mixture, computed in float64 on the host: mat = sqrt(1/2) L^T
    with the precision Sigma^-1 = L L^T (Cholesky), offset[m] = -log w_m + 1/2 log det Sigma_m - (the least of these over m).  Then
    |mat (x - mean)|^2 + offset is the negative log of component m's weighted density, up to a constant common to all components."""
    means, covars, weights = (np.asarray(x, np.float64) for x in (means, covars, weights))
    if means.ndim != 2 or covars.shape != means.shape + means.shape[1:] or weights.shape != means.shape[:1] or not (weights > 0).all():
        raise SmplppError(1, "gmm_tables: expected means [M,D], covars [M,D,D] and positive weights [M]")
    mat = np.stack([np.sqrt(0.5) * np.linalg.cholesky(np.linalg.inv(c)).T for c in covars])
    off = np.array([-np.log(w) + 0.5 * np.linalg.slogdet(c)[1] for w, c in zip(weights, covars)])
    return means.astype(np.float32), mat.astype(np.float32), (off - off.min()).astype(np.float32)


def smplify_limits(weight=1.0):
    """(lo, hi, limit_weight) for the 69-d body pose with the four coordinates SMPLify restrains set and every other one unlimited
    (a limit_weight of 0): the knees and elbows may not bend the wrong way.  The indices are QUOTED FROM MEMORY, not from a file
    shipped with this package: SMPLify uses indices 55, 58, 12, 15 of the 72-d pose with signs +, -, -, - in its exponential term
    exp(sign * theta), that is 52, 55, 9, 12 of the body pose; a + sign penalises positive angles (hi = 0), a - sign negative ones
    (lo = 0).  The penalty here is limit_weight times the squared excess, not SMPLify's exponential.  Check the indices against your
    model's joint order before relying on them."""
    lo, hi = np.full(BODY_POSE_DIM, -np.inf, np.float32), np.full(BODY_POSE_DIM, np.inf, np.float32)
    w = np.zeros(BODY_POSE_DIM, np.float32)
    for idx72, sign in ((55, 1), (58, -1), (12, -1), (15, -1)):
        k = idx72 - 3
        if sign > 0:
            hi[k] = 0.0
        else:
            lo[k] = 0.0
        w[k] = weight
    return lo, hi, w


class PosePrior:
    """A mixture of M components over D coordinates (mean [M,D], mat [M,D,D] with row j giving output j, offset [M]) and optional
    limits lo, hi, limit_weight [D] (all three or none; +-inf = no limit on that side).  M = 0 (empty arrays) needs limits."""

    def __init__(self, device, mean, mat, offset, lo=None, hi=None, limit_weight=None):
        self._h = None
        mean, mat, offset = (np.ascontiguousarray(x, np.float32) for x in (mean, mat, offset))
        M = int(offset.size)
        if mean.ndim != 2 or mean.shape[0] != M or mean.shape[1] < 1 or mat.shape != (M, mean.shape[1], mean.shape[1]):
            raise SmplppError(1, "PosePrior: expected mean [M,D], mat [M,D,D] and offset [M]")
        D = int(mean.shape[1])
        lim = [None if x is None else np.ascontiguousarray(x, np.float32).reshape(-1) for x in (lo, hi, limit_weight)]
        if any(x is not None and x.size != D for x in lim):
            raise SmplppError(1, "PosePrior: expected lo, hi and limit_weight of length D")
        self._device = parse_device(device)
        h = C.c_void_p()
        check(_lib.load().smplpp_pose_prior_create(self._device, M, D, _ptr(mean), _ptr(mat), _ptr(offset.reshape(-1)), *(_ptr(x) for x in lim),
                                                   C.byref(h)))
        self._h = h
        self.component_num, self.dim, self.has_limits = M, D, lim[0] is not None

    @classmethod
    def from_gmm(cls, device, means, covars, weights, lo=None, hi=None, limit_weight=None):
        """The prior of a Gaussian mixture: gmm_tables in float64 on the host, then the constructor."""
        return cls(device, *gmm_tables(means, covars, weights), lo=lo, hi=hi, limit_weight=limit_weight)

    @classmethod
    def from_limits(cls, device, lo, hi, limit_weight):
        """Limits alone (M = 0)."""
        D = np.size(lo)
        return cls(device, np.zeros((0, D), np.float32), np.zeros((0, D, D), np.float32), np.zeros(0, np.float32), lo, hi, limit_weight)

    @classmethod
    def load(cls, path, device="cuda:0", lo=None, hi=None, limit_weight=None):
        """From an .npz with `means` [M,D], `covars` [M,D,D] and `weights` [M]."""
        with np.load(path) as z:
            return cls.from_gmm(device, z["means"], z["covars"], z["weights"], lo=lo, hi=hi, limit_weight=limit_weight)

    def __del__(self):
        try:
            if self._h:
                _lib.load().smplpp_pose_prior_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise SmplppError(4, "PosePrior: no prior")
        return self._h

    def info(self):
        M, D, lim = C.c_int64(), C.c_int64(), C.c_int()
        check(_lib.load().smplpp_pose_prior_info(self.handle, C.byref(M), C.byref(D), C.byref(lim)))
        return dict(component_num=M.value, dim=D.value, has_limits=bool(lim.value))

    def _default_want(self):
        return (("energy", "component", "residual") if self.component_num else ()) + (("limit_energy",) if self.has_limits else ())

    def _rows(self, c, a, ld, offset=0):
        """(n, ld, address of coordinate 0 of frame 0) of a pose or grad_pose buffer: [n,D], or any contiguous float32 buffer whose rows
        are ld floats apart with the coordinates at `offset` within a row."""
        n = int(a.shape[0])
        if ld is None:
            if tuple(a.shape) != (n, self.dim):
                c.refuse("expected shape (N, %d)" % self.dim)
            ld = self.dim
        elif (a.numel() if c.dev else a.size) != n * ld or offset < 0 or offset + self.dim > ld:
            c.refuse("expected N rows of ld = %d floats holding %d coordinates at offset %d" % (ld, self.dim, offset))
        return n, int(ld), _ptr(a) + 4 * offset

    def _buffer(self, c, a):
        """A contiguous float32 buffer in the space of `c`, never copied when it already is one."""
        if c.dev:
            if not (a.is_cuda and a.dtype == torch.float32 and a.is_contiguous()):
                c.refuse("expected a contiguous float32 device tensor")
            return a.detach()
        if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous):
            a = np.ascontiguousarray(a, np.float32)
        return a

    def evaluate(self, pose, ld=None, want=None, out=None, offset=0):
        """A dict of energy [N], component [N] int64, residual [N,D] (the mixture) and limit_energy [N] (the limits) of pose [N,D], or
        with `ld` of a buffer of N rows of ld floats whose D coordinates start `offset` floats into each row (smplpp_pose_prior).
        `want` names the outputs (default: all the prior has); `out` may hold preallocated arrays for some of them."""
        c = _Call("evaluate", pose, *((out or {}).values()))
        pose = self._buffer(c, pose)
        n, ld, p = self._rows(c, pose, ld, offset)
        want = self._default_want() if want is None else tuple(want)
        shapes = {"energy": ((n,), "float32"), "component": ((n,), "int64"), "residual": ((n, self.dim), "float32"), "limit_energy": ((n,), "float32")}
        if not want or any(k not in shapes for k in want):
            c.refuse("want must name some of energy, component, residual, limit_energy")
        res = {}
        for k in want:
            if out is not None and k in out:
                a = out[k]
                if tuple(a.shape) != shapes[k][0] or str(a.dtype).split(".")[-1] != shapes[k][1] or not (a.is_contiguous() if c.dev else a.flags.c_contiguous):
                    c.refuse("out[%r] must be a contiguous %s array of shape %s" % (k, shapes[k][1], shapes[k][0]))
                res[k] = a
            else:
                res[k] = c.empty(*shapes[k])
        check(_lib.load().smplpp_pose_prior(self.handle, n, p, ld, _ptr(res.get("energy")), _ptr(res.get("component")), _ptr(res.get("residual")),
                                            _ptr(res.get("limit_energy")), c.space, c.stream))
        return res

    def evaluateBackward(self, pose, grad_energy=None, grad_residual=None, grad_limit_energy=None, component=None, ld=None, out=None, offset=0):
        """Vector-Jacobian product of evaluate to the pose (smplpp_pose_prior_vjp) for dL/denergy = grad_energy [N], dL/dresidual =
        grad_residual [N,D] and dL/dlimit_energy = grad_limit_energy [N] (each may be None).  `component` [N] fixes the components
        (what evaluate returned); None chooses them as evaluate does.  Returns grad_pose in the layout of pose; with `out` (the same
        layout: with ld and offset a grad_theta buffer) the gradient is added into it, D coordinates per row, and it is returned."""
        acc = out is not None
        c = _Call("evaluateBackward", pose, grad_energy, grad_residual, grad_limit_energy, out)
        pose = self._buffer(c, pose)
        n, ld, p = self._rows(c, pose, ld, offset)
        ge, gr, gl = c.input(grad_energy, (n,)), c.input(grad_residual, (n, self.dim)), c.input(grad_limit_energy, (n,))
        comp = None if component is None else c.ids(component)
        if comp is not None and len(comp) != n:
            c.refuse("expected component of shape (N,)")
        if acc:
            if tuple(out.shape) != tuple(pose.shape) or not (out.is_contiguous() and out.dtype == torch.float32 if c.dev else
                                                             isinstance(out, np.ndarray) and out.flags.c_contiguous and out.dtype == np.float32):
                c.refuse("out must be a contiguous float32 array of the shape of pose")
            res = out.detach() if c.dev else out
        elif ld == self.dim:
            res = c.empty((n, self.dim))
        else:  # the layout of pose: the floats outside the D coordinates are zeros
            res = torch.zeros_like(pose) if c.dev else np.zeros_like(pose)
        check(_lib.load().smplpp_pose_prior_vjp(self.handle, n, p, ld, _ptr(comp), _ptr(ge), _ptr(gr), _ptr(gl), _ptr(res) + 4 * offset, int(acc),
                                                c.space, c.stream))
        return out if acc else res

    def _theta(self, theta):
        if len(theta.shape) != 3 or tuple(theta.shape[1:]) != (25, 3) or self.dim != BODY_POSE_DIM:
            raise SmplppError(1, "evaluate_theta: expected theta [N,25,3] and a prior over %d coordinates" % BODY_POSE_DIM)

    def evaluate_theta(self, theta, want=None, out=None):
        """evaluate on the body pose of theta [N,25,3] (rows 2..24), read in place: offset 6, ld 75."""
        self._theta(theta)
        return self.evaluate(theta, ld=THETA_LD, want=want, out=out, offset=THETA_OFFSET)

    def evaluate_theta_backward(self, theta, grad_energy=None, grad_residual=None, grad_limit_energy=None, component=None, out=None):
        """evaluateBackward on the body pose of theta [N,25,3]: grad_theta [N,25,3] (zeros outside the body pose), or added into `out`."""
        self._theta(theta)
        return self.evaluateBackward(theta, grad_energy, grad_residual, grad_limit_energy, component, ld=THETA_LD, out=out, offset=THETA_OFFSET)

    def forward_differentiable(self, theta):
        """(energy [N], limit_energy [N]) of device theta [N,25,3] (a prior over 69 coordinates) or of a device pose [N,D],
        differentiable with torch.autograd: smplpp_pose_prior forward, smplpp_pose_prior_vjp backward with the forward's components
        (the selection is fixed per call), on torch's current stream.  A part the prior lacks is returned as zeros."""
        if torch is None or not _is_torch(theta):
            raise SmplppError(1, "forward_differentiable needs a torch device tensor")
        return _PosePriorFunction.apply(theta, self)


if torch is not None:
    class _PosePriorFunction(torch.autograd.Function):
        """smplpp_pose_prior forward / smplpp_pose_prior_vjp backward (PosePrior.forward_differentiable)."""

        @staticmethod
        def forward(ctx, theta, prior):
            x = theta.detach().contiguous()
            as_theta = x.dim() == 3
            want = (("energy", "component") if prior.component_num else ()) + (("limit_energy",) if prior.has_limits else ())
            r = prior.evaluate_theta(x, want=want) if as_theta else prior.evaluate(x, want=want)
            ctx.prior, ctx.as_theta = prior, as_theta
            ctx.save_for_backward(x, r.get("component"))
            zeros = torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
            return r.get("energy", zeros), r.get("limit_energy", zeros)

        @staticmethod
        def backward(ctx, grad_energy, grad_limit_energy):
            if not ctx.needs_input_grad[0]:
                return None, None
            p = ctx.prior
            x, component = ctx.saved_tensors
            ge = grad_energy.contiguous() if p.component_num else None
            gl = grad_limit_energy.contiguous() if p.has_limits else None
            call = p.evaluate_theta_backward if ctx.as_theta else p.evaluateBackward
            return call(x, grad_energy=ge, grad_limit_energy=gl, component=component), None
