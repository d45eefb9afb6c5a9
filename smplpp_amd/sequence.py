"""Sequence terms for fitting with a grouped BatchedLBFGS (smplpp_sequence_*): the layout of sequences inside the optimiser buffer, the
split of its rows into per-frame arrays and a shared row per problem (and its backward, which sums the shared row's gradient), the sum
of frame values into problem values, and the temporal smoothness term between consecutive frames of a problem with its backward.  numpy
arrays are host space (the call stages and synchronises), torch tensors device space (enqueued on torch's current stream); every number
is produced by libsmplpp_hip.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SmplppError, check
from .optim import _rows
from .smpl import _Call, _is_torch, _ptr, parse_device, torch


class SequenceLayout:
    """P = len(groups) problems; problem p owns groups[p] consecutive rows of the optimiser buffer, the last `shared_rows` (0 or 1) of
    which are not frames (the recipe of BatchedLBFGS: a block [T + 1, 75] whose last row carries beta).  Frames are numbered compactly
    in row order, and every frame-side array is compact [F, ...]."""

    def __init__(self, device, groups, shared_rows=0):
        self._h = None
        try:
            lens = [int(r) for r in groups]
            exact = all(r == v for r, v in zip(lens, groups))
        except (TypeError, ValueError):
            lens, exact = [], False
        if not exact:
            raise SmplppError(1, "SequenceLayout: groups must be a sequence of whole row counts")
        self._device = parse_device(device)
        start = (C.c_int64 * (len(lens) + 1))(0, *np.cumsum(lens).tolist())
        h = C.c_void_p()
        check(_lib.load().smplpp_sequence_create(self._device, len(lens), start, int(shared_rows), C.byref(h)))
        self._h = h
        i = self.info()
        self.problems, self.rows, self.frames, self.shared_rows, self.frame_start = i["problems"], i["rows"], i["frames"], i["shared_rows"], i["frame_start"]
        self.groups = lens
        self.problem_of = np.repeat(np.arange(self.problems), np.diff(self.frame_start))  # [F] the problem of a frame
        self._problem_of_dev = {}

    @classmethod
    def from_optimizer(cls, opt, shared_rows=0):
        """The layout of a BatchedLBFGS's problems (smplpp_lbfgs_groups), on its device."""
        _, start = opt.row_start()
        return cls(opt._device, np.diff(start).tolist(), shared_rows)

    def __del__(self):
        try:
            if self._h:
                _lib.load().smplpp_sequence_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise SmplppError(4, "SequenceLayout: no layout")
        return self._h

    def info(self):
        P, rows, frames, shared = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        check(_lib.load().smplpp_sequence_info(self.handle, C.byref(P), C.byref(rows), C.byref(frames), C.byref(shared), None))
        start = (C.c_int64 * (P.value + 1))()
        check(_lib.load().smplpp_sequence_info(self.handle, None, None, None, None, start))
        return dict(problems=P.value, rows=rows.value, frames=frames.value, shared_rows=shared.value, frame_start=np.array(list(start), np.int64))

    # ------------------------------------------------------------------------------------------------ buffer <-> per-frame arrays
    def _buffer(self, c, a, n, what):
        """(array, ld) of a float32 [n, D] buffer or a row-strided view of one, in the space of `c`, never copied."""
        if not c.dev and not (isinstance(a, np.ndarray) and a.dtype == np.float32):
            a = np.ascontiguousarray(a, np.float32)
        if c.dev:
            a = a.detach()
        rows, _, ld = _rows("SequenceLayout.%s" % c.name, a)
        if rows != n:
            c.refuse("expected %s with %d rows" % (what, n))
        return a, ld

    def split(self, rows, off_f=0, C_f=None, C_s=None):
        """(frames [F,C_f], shared [F,C_s]) of the optimiser buffer rows [n,D] (or a row-strided view): frames[f] = the coordinates
        [off_f, off_f + C_f) of frame f's row, shared[f] = the first C_s coordinates of the shared row of f's problem
        (smplpp_sequence_split, one launch).  C_f or C_s None leaves that output out (None is returned in its place)."""
        c = _Call("split", rows)
        rows, ld = self._buffer(c, rows, self.rows, "rows")
        if C_f is None and C_s is None:
            c.refuse("C_f or C_s must be given")
        frames = None if C_f is None else c.empty((self.frames, int(C_f)))
        shared = None if C_s is None else c.empty((self.frames, int(C_s)))
        check(_lib.load().smplpp_sequence_split(self.handle, _ptr(rows), ld, int(off_f), int(C_f or 0), _ptr(frames), int(C_s or 0), _ptr(shared),
                                                c.space, c.stream))
        return frames, shared

    def merge(self, grad_frames=None, off_f=0, grad_shared=None, D=None, out=None, accumulate=False):
        """The backward of split (smplpp_sequence_merge): grad_rows [n,D] from grad_frames [F,C_f] and grad_shared [F,C_s] (either may be
        None).  All D coordinates of every row are written: a frame row gets its slice and zeros elsewhere, a shared row the sum of
        grad_shared over the problem's frames.  With `out` ([n,D] or a row-strided view; D defaults to its width) the result is stored
        into it, or with accumulate added to it."""
        if grad_frames is None and grad_shared is None:
            raise SmplppError(1, "merge: grad_frames or grad_shared must be given")
        c = _Call("merge", grad_frames, grad_shared, out)
        C_f = 0 if grad_frames is None else int(grad_frames.shape[-1])
        C_s = 0 if grad_shared is None else int(grad_shared.shape[-1])
        gf, gs = c.input(grad_frames, (self.frames, C_f)), c.input(grad_shared, (self.frames, C_s))
        if out is None:
            if D is None or accumulate:
                c.refuse("D must be given without out, and accumulate needs out")
            out, ld = c.empty((self.rows, int(D))), int(D)
        else:
            if c.dev != _is_torch(out) or (not c.dev and not (isinstance(out, np.ndarray) and out.dtype == np.float32)):
                c.refuse("out must be a float32 array in the space of the gradients")
            n, width, ld = _rows("SequenceLayout.merge", out.detach() if c.dev else out)
            if n != self.rows:
                c.refuse("expected out with %d rows" % self.rows)
            D = width if D is None else int(D)
        check(_lib.load().smplpp_sequence_merge(self.handle, _ptr(gf), int(off_f), C_f, _ptr(gs), C_s, _ptr(out.detach() if c.dev else out), ld, int(D),
                                                int(bool(accumulate)), c.space, c.stream))
        return out

    def sum(self, frame_values, scale=1.0, out=None, accumulate=False):
        """problem_values [P] = scale * (the sum of frame_values [F] over each problem's frames) (smplpp_sequence_sum); with `out` stored
        into it, or with accumulate added to it: several terms fold into the energies of BatchedLBFGS.step_with one call each."""
        c = _Call("sum", frame_values, out)
        fv = c.input(frame_values, (self.frames,))
        if out is None:
            if accumulate:
                c.refuse("accumulate needs out")
            out = c.empty((self.problems,))
        res = c.inout(out, (self.problems,))
        check(_lib.load().smplpp_sequence_sum(self.handle, _ptr(fv), float(scale), _ptr(res), int(bool(accumulate)), c.space, c.stream))
        return out

    # ------------------------------------------------------------------------------------------------ the temporal term
    def _points(self, c, x, K, C_, offset):
        """(x as a buffer, ld, K, C, address of coordinate 0 of frame 0): x [F,K,C], or with K and C any contiguous float32 buffer of F
        equal rows whose K C coordinates start `offset` floats into each row."""
        if c.dev:
            if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
                c.refuse("expected a contiguous float32 device tensor")
            x = x.detach()
        elif not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.flags.c_contiguous):
            x = np.ascontiguousarray(x, np.float32)
        size = x.numel() if c.dev else x.size
        if K is None or C_ is None:
            if len(x.shape) != 3 or int(x.shape[0]) != self.frames or offset:
                c.refuse("expected x of shape (%d, K, C), or K, C (and offset) with a buffer of %d rows" % (self.frames, self.frames))
            K, C_ = int(x.shape[1]), int(x.shape[2])
        if int(x.shape[0]) != self.frames or size % self.frames or offset < 0 or offset + K * C_ > size // self.frames:
            c.refuse("expected %d equal rows holding K C = %d coordinates at offset %d" % (self.frames, K * C_, offset))
        return x, size // self.frames, int(K), int(C_), _ptr(x) + 4 * int(offset)

    def _weight(self, c, weight, K):
        if weight is None:
            return None
        if c.dev and not _is_torch(weight):  # a host table for device calls: checked here (device-space weights are not read on the host)
            w = np.ascontiguousarray(weight, np.float32).reshape(-1)
            if not (np.isfinite(w).all() and (w >= 0).all()):
                c.refuse("a weight is negative or not finite")
            weight = torch.from_numpy(w).to(c.device)
        return c.input(weight, (K,))

    def smoothness(self, x, order=1, weight=None, rho=0.0, K=None, C=None, offset=0, want=("frame_energy", "point_energy")):
        """The temporal term of x [F,K,C] (or, with K and C, of a buffer of F rows whose points start `offset` floats into each row:
        theta [F,25,3] with K=24, C=3, offset=3 is the rotations of a theta buffer, read in place): a dict of frame_energy [F] and
        point_energy [F,K] (smplpp_sequence_smoothness).  order 1: first differences x[f+1] - x[f]; order 2: second differences; a
        stencil never crosses a problem boundary.  weight [K] scales each point's energy; rho > 0 makes it the Geman-McClure form."""
        c = _Call("smoothness", x)
        x, ld, K, C_, p = self._points(c, x, K, C, offset)
        w = self._weight(c, weight, K)
        shapes = {"frame_energy": (self.frames,), "point_energy": (self.frames, K)}
        if not want or any(k not in shapes for k in want):
            c.refuse("want must name some of frame_energy, point_energy")
        res = {k: c.empty(shapes[k]) for k in want}
        check(_lib.load().smplpp_sequence_smoothness(self.handle, p, ld, K, C_, int(order), _ptr(w), float(rho), _ptr(res.get("frame_energy")),
                                                     _ptr(res.get("point_energy")), c.space, c.stream))
        return res

    def smoothnessBackward(self, x, grad_frame_energy=None, grad_point_energy=None, order=1, weight=None, rho=0.0, K=None, C=None, offset=0,
                           out=None):
        """Vector-Jacobian product of smoothness to x (smplpp_sequence_smoothness_vjp) for dL/dframe_energy [F] and dL/dpoint_energy
        [F,K] (either may be None).  Returns grad_x in the layout of x (zeros outside the K C coordinates); with `out` (the same
        layout) the gradient is added into it and it is returned."""
        acc = out is not None
        c = _Call("smoothnessBackward", x, grad_frame_energy, grad_point_energy, out)
        x, ld, K, C_, p = self._points(c, x, K, C, offset)
        w = self._weight(c, weight, K)
        gfe, gpe = c.input(grad_frame_energy, (self.frames,)), c.input(grad_point_energy, (self.frames, K))
        if acc:
            res = c.inout(out, tuple(x.shape))
        elif ld == K * C_:
            res = c.empty(tuple(x.shape))
        else:
            res = torch.zeros_like(x) if c.dev else np.zeros_like(x)
        check(_lib.load().smplpp_sequence_smoothness_vjp(self.handle, p, ld, K, C_, int(order), _ptr(w), float(rho), _ptr(gfe), _ptr(gpe),
                                                         _ptr(res) + 4 * int(offset), int(acc), c.space, c.stream))
        return out if acc else res

    # ------------------------------------------------------------------------------------------------ torch.autograd
    def _need_torch(self, name, *tensors):
        if torch is None or not all(_is_torch(t) for t in tensors):
            raise SmplppError(1, "%s needs torch device tensors" % name)

    def problem_of_device(self, device):
        """problem_of as an int64 tensor on `device` (made once per device)."""
        key = str(device)
        if key not in self._problem_of_dev:
            self._problem_of_dev[key] = torch.from_numpy(self.problem_of.astype(np.int64)).to(device)
        return self._problem_of_dev[key]

    def split_differentiable(self, buf, off_f=0, C_f=75, C_s=None):
        """(frames [F,C_f], shared [F,C_s]) of the device buffer buf [n,D], differentiable with torch.autograd: smplpp_sequence_split
        forward, smplpp_sequence_merge backward (every coordinate of buf's gradient is written; the shared rows' gradient is the
        fixed-order sum over their problem's frames).  Without C_s only frames is returned."""
        self._need_torch("split_differentiable", buf)
        frames, shared = _SplitFunction.apply(buf, self, int(off_f), int(C_f), None if C_s is None else int(C_s))
        return frames if C_s is None else (frames, shared)

    def sum_differentiable(self, frame_values, scale=1.0):
        """problem values [P] = scale * the per-problem sums of the device tensor frame_values [F] (smplpp_sequence_sum), differentiable:
        the backward hands scale * grad[p] to every frame of problem p."""
        self._need_torch("sum_differentiable", frame_values)
        return _SumFunction.apply(frame_values, self, float(scale))

    def smoothness_differentiable(self, x, order=1, weight=None, rho=0.0, K=None, C=None, offset=0):
        """frame_energy [F] of the device tensor x (the arguments of smoothness), differentiable in x: smplpp_sequence_smoothness
        forward, smplpp_sequence_smoothness_vjp backward, on torch's current stream."""
        self._need_torch("smoothness_differentiable", x)
        return _SmoothnessFunction.apply(x, self, int(order), weight, float(rho), K, C, int(offset))


if torch is not None:
    class _SplitFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, buf, layout, off_f, C_f, C_s):
            b = buf.detach()
            if b.dim() != 2:
                raise SmplppError(1, "split_differentiable: expected buf of shape (n, D)")
            frames, shared = layout.split(b, off_f, C_f, C_s)
            ctx.layout, ctx.off_f, ctx.D, ctx.has_shared = layout, off_f, int(b.shape[1]), C_s is not None
            if shared is None:
                shared = b.new_zeros(0)
                ctx.mark_non_differentiable(shared)
            return frames, shared

        @staticmethod
        def backward(ctx, grad_frames, grad_shared):
            if not ctx.needs_input_grad[0]:
                return None, None, None, None, None
            gs = grad_shared.contiguous() if ctx.has_shared and grad_shared is not None else None
            gf = None if grad_frames is None else grad_frames.contiguous()
            return ctx.layout.merge(gf, ctx.off_f, gs, D=ctx.D), None, None, None, None

    class _SumFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, frame_values, layout, scale):
            ctx.layout, ctx.scale = layout, scale
            return layout.sum(frame_values.detach().contiguous(), scale)

        @staticmethod
        def backward(ctx, grad):
            if not ctx.needs_input_grad[0]:
                return None, None, None
            # (a copy of one value per frame: no arithmetic beyond the one product the rule states)
            return (grad * ctx.scale).index_select(0, ctx.layout.problem_of_device(grad.device)), None, None

    class _SmoothnessFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, layout, order, weight, rho, K, C_, offset):
            xd = x.detach().contiguous()
            ctx.layout, ctx.args = layout, dict(order=order, weight=weight, rho=rho, K=K, C=C_, offset=offset)
            ctx.save_for_backward(xd)
            return layout.smoothness(xd, want=("frame_energy",), **ctx.args)["frame_energy"]

        @staticmethod
        def backward(ctx, grad):
            if not ctx.needs_input_grad[0]:
                return (None,) * 8
            (xd,) = ctx.saved_tensors
            return (ctx.layout.smoothnessBackward(xd, grad_frame_energy=grad.contiguous(), **ctx.args),) + (None,) * 7
