"""A batched L-BFGS for fitting (smplpp_lbfgs_create / smplpp_lbfgs_step / smplpp_lbfgs_state / smplpp_lbfgs_best): every frame of a
batch is its own problem, with its own history, step length, line search and status, all kept on the device.  One evaluation of the
energies is one kernel launch; nothing is read back unless asked.  numpy arrays are host space (the call stages and synchronises),
torch tensors device space (enqueued on torch's current stream); every number is produced by libsmplpp_hip.so."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SmplppError, check
from .smpl import _is_torch, _ptr, _stream, parse_device, torch

STATUS = {0: "running", 1: "gradient tolerance met", 2: "energy tolerance met", 3: "line search exhausted", 4: "not finite at the start"}
DEFAULTS = dict(c1=1e-4, tol_grad=1e-5, tol_f=0.0, max_ls=20, curv_eps=1e-10)


def _rows(name, a):
    """(n, D, ld) of a float32 [n,D] array whose rows are ld >= D floats apart with unit stride inside a row."""
    if _is_torch(a):
        ok = a.dtype == torch.float32 and a.dim() == 2 and a.numel() > 0 and (a.stride(1) == 1 or a.shape[1] == 1)
        ld = a.stride(0) if ok else 0
    else:
        ok = isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 2 and a.size > 0 and (a.strides[1] == 4 or a.shape[1] == 1) and a.strides[0] % 4 == 0
        ld = a.strides[0] // 4 if ok else 0
    if ok and a.shape[0] == 1:
        ld = max(ld, a.shape[1])
    if not ok or ld < a.shape[1]:
        raise SmplppError(1, "%s: expected a float32 [n,D] array or a view of rows at least D floats apart" % name)
    return int(a.shape[0]), int(a.shape[1]), int(ld)


class BatchedLBFGS:
    """L-BFGS over the rows of x [n,D]: a float32 CUDA tensor with requires_grad, or a row-strided view of one (theta.view(n, 75)[:, 3:]
    optimises rotation and pose inside a theta buffer), or for the host-space path a float32 numpy array.  history: pairs kept per
    frame (1..32).  Options: c1, tol_grad, tol_f, max_ls, curv_eps (smplpp_lbfgs_create).

    groups=[len_0, len_1, ...] (row counts summing to n) makes problem p the len_p consecutive rows after those of problem p - 1, with
    one history, step length, line search and status for all its len_p * D unknowns (smplpp_lbfgs_create_grouped): a sequence whose
    frames are coupled by a velocity term or share a vector.  Then step(closure) expects energies of shape (P,), state() arrays have P
    entries, and everything else works as without groups.  Sums follow the 1024-partial rule, so the numbers of a one-row problem are
    not those of the same row without groups: per-frame fits belong on a handle without groups.  The recipe for a vector shared by T
    frames: optimise a buffer [T + 1, 75] whose rows 0 .. T - 1 are theta and whose last row carries beta in its first 10 coordinates
    (groups=[T + 1]); the closure reads beta from buf[T, :10], and the unused coordinates have zero gradient and never move.
    sequence.SequenceLayout.from_optimizer(opt, shared_rows=1) gives that closure its glue natively: the split of the buffer into per-frame
    theta and beta, the smoothness term between consecutive frames and the per-problem sums, each with its backward."""

    def __init__(self, x, history=10, device=None, groups=None, **options):
        self._h = None
        bad = set(options) - set(DEFAULTS)
        if bad:
            raise SmplppError(1, "BatchedLBFGS: unknown options %s" % sorted(bad))
        self.options = dict(DEFAULTS, **options)
        self.x = x
        self.dev = _is_torch(x)
        if self.dev and not x.is_cuda:
            raise SmplppError(1, "BatchedLBFGS: expected a CUDA tensor or a numpy array")
        self.n, self.dim, self._ld = _rows("BatchedLBFGS", x.detach() if self.dev else x)
        self.history = int(history)
        self._device = parse_device(x.device if self.dev else ("cuda:0" if device is None else device))
        o = self.options
        h = C.c_void_p()
        scalars = (float(o["c1"]), float(o["tol_grad"]), float(o["tol_f"]), int(o["max_ls"]), float(o["curv_eps"]))
        self.groups, self.problems = None, self.n
        if groups is None:
            check(_lib.load().smplpp_lbfgs_create(self._device, self.n, self.dim, self.history, *scalars, C.byref(h)))
        else:
            self.groups = self._groups(groups)
            self.problems = len(self.groups)
            start = (C.c_int64 * (self.problems + 1))(0, *np.cumsum(self.groups).tolist())
            check(_lib.load().smplpp_lbfgs_create_grouped(self._device, self.n, self.dim, self.history, self.problems, start, *scalars, C.byref(h)))
        self._h = h

    def _groups(self, groups):
        """The row counts as a list of ints; what smplpp_lbfgs_create_grouped refuses is refused here, with or without a device."""
        try:
            lens = [int(r) for r in groups]
            exact = all(r == v for r, v in zip(lens, groups))
        except (TypeError, ValueError):
            lens, exact = [], False
        if not exact:
            raise SmplppError(1, "BatchedLBFGS: groups must be a sequence of whole row counts")
        if not lens:
            raise SmplppError(1, "BatchedLBFGS: P must be positive")
        if any(r <= 0 for r in lens):
            raise SmplppError(1, "BatchedLBFGS: row_start must strictly increase (every group needs a row)")
        if sum(lens) != self.n:
            raise SmplppError(1, "BatchedLBFGS: row_start[P] must be n (the groups sum to %d, x has %d rows)" % (sum(lens), self.n))
        return lens

    def row_start(self):
        """(P, row_start [P+1]) as the handle reports them (smplpp_lbfgs_groups)."""
        P = C.c_int64()
        check(_lib.load().smplpp_lbfgs_groups(self.handle, C.byref(P), None))
        start = (C.c_int64 * (P.value + 1))()
        check(_lib.load().smplpp_lbfgs_groups(self.handle, None, start))
        return P.value, list(start)

    def __del__(self):
        try:
            if self._h:
                _lib.load().smplpp_lbfgs_destroy(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def handle(self):
        if not self._h:
            raise SmplppError(4, "BatchedLBFGS: no optimiser")
        return self._h

    def _space(self):
        return (_lib.DEVICE, _stream()) if self.dev else (_lib.HOST, None)

    def info(self):
        n, D, m = C.c_int64(), C.c_int64(), C.c_int64()
        check(_lib.load().smplpp_lbfgs_info(self.handle, C.byref(n), C.byref(D), C.byref(m)))
        return dict(n=n.value, dim=D.value, history=m.value)

    def step_with(self, f, g):
        """One call of smplpp_lbfgs_step with energies f [n] ([P] with groups) and gradients g [n,D] (or a row-strided view) at the current
        x, which is overwritten in place with the next points to evaluate."""
        x = self.x.detach() if self.dev else self.x
        if _is_torch(f) != self.dev or _is_torch(g) != self.dev:
            raise SmplppError(1, "BatchedLBFGS: mix of torch tensors and numpy arrays")
        if self.dev:
            if not (f.is_cuda and g.is_cuda and f.dtype == torch.float32 and tuple(f.shape) == (self.problems,)):
                raise SmplppError(1, "BatchedLBFGS: expected float32 device energies of shape (%d,)" % self.problems)
            f = f.detach().contiguous()
        else:
            f = np.ascontiguousarray(f, np.float32)
            if f.shape != (self.problems,):
                raise SmplppError(1, "BatchedLBFGS: expected energies of shape (%d,)" % self.problems)
        gn, gD, ld_g = _rows("BatchedLBFGS: g", g)
        if (gn, gD) != (self.n, self.dim):
            raise SmplppError(1, "BatchedLBFGS: expected gradients of shape (%d, %d)" % (self.n, self.dim))
        space, stream = self._space()
        check(_lib.load().smplpp_lbfgs_step(self.handle, _ptr(x), self._ld, _ptr(f), _ptr(g), ld_g, space, stream))

    def step(self, closure):
        """One evaluation: closure() returns the per-frame energies [n] (per-problem [P] with groups) of the current x; their sum is
        back-propagated, the step is taken on x.data, x.grad and the energies, and the gradient is cleared.  Returns the energies
        (detached)."""
        if not self.dev:
            raise SmplppError(1, "BatchedLBFGS.step needs a torch tensor; use step_with(f, g) with numpy arrays")
        root = self.x if self.x.is_leaf else self.x._base
        if root is None or not root.requires_grad:
            raise SmplppError(1, "BatchedLBFGS.step: x (or the tensor it is a view of) must require a gradient")
        root.grad = None
        with torch.enable_grad():
            f = closure()
            if tuple(f.shape) != (self.problems,):
                raise SmplppError(1, "BatchedLBFGS.step: the closure must return per-frame energies of shape (%d,)" % self.problems)
            f.sum().backward()
        if root.grad is None:
            raise SmplppError(1, "BatchedLBFGS.step: the energies do not depend on x")
        g = root.grad if root is self.x else root.grad.as_strided(self.x.shape, self.x.stride(), self.x.storage_offset())
        self.step_with(f.detach().float(), g)
        root.grad = None
        return f.detach()

    def run(self, closure, max_evals, check_every=10):
        """Up to max_evals evaluations; the number of running frames is read back every check_every evaluations only, and the loop
        ends early when it is 0.  Ends with best(): x holds every frame's accepted point.  Returns state()."""
        for k in range(int(max_evals)):
            self.step(closure)
            if (k + 1) % check_every == 0 and int(self.state(("running",))["running"][0]) == 0:
                break
        self.best()
        return self.state()

    def state(self, want=("status", "iterations", "evaluations", "f_best", "step", "running")):
        """A dict of status, iterations, evaluations (int32 [n]), f_best, step (float32 [n]) and running (int64 [1]): smplpp_lbfgs_state,
        in the space of x."""
        kinds = dict(status="int32", iterations="int32", evaluations="int32", f_best="float32", step="float32", running="int64")
        if not want or any(k not in kinds for k in want):
            raise SmplppError(1, "BatchedLBFGS.state: want must name some of %s" % ", ".join(kinds))
        res = {}
        for k in want:
            shape = (1,) if k == "running" else (self.problems,)
            res[k] = torch.empty(shape, dtype=getattr(torch, kinds[k]), device=self.x.device) if self.dev else np.empty(shape, kinds[k])
        space, stream = self._space()
        check(_lib.load().smplpp_lbfgs_state(self.handle, *(_ptr(res.get(k)) for k in kinds), space, stream))
        return res

    def best(self, want_f=False):
        """Every frame's last accepted point into x (smplpp_lbfgs_best); with want_f also returns its energy [n]."""
        x = self.x.detach() if self.dev else self.x
        f = None
        if want_f:
            f = torch.empty(self.problems, dtype=torch.float32, device=x.device) if self.dev else np.empty(self.problems, np.float32)
        space, stream = self._space()
        check(_lib.load().smplpp_lbfgs_best(self.handle, _ptr(x), self._ld, _ptr(f), space, stream))
        return f

    def reset(self):
        """Every frame back to its first evaluation, with an empty history."""
        check(_lib.load().smplpp_lbfgs_reset(self.handle, self._space()[1]))
