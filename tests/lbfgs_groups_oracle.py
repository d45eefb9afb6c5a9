"""The rule of a grouped L-BFGS handle (smplpp_lbfgs_create_grouped, include/smplpp_hip.h) restated in numpy with the dtype as a parameter:
the per-frame rule of smplpp_lbfgs_step on the N = rows * D elements of a problem, with every sum by the 1024-partial rule.  In float32,
operation for operation, it is the bit reference of the library; in float64 the numerical one.  The ring arithmetic, the options and the
test functions are those of lbfgs_oracle.py; Chain couples the rows of a problem.

A problem's sums run over vectors of 1024 partials, one numpy operation per 1024 elements."""
import numpy as np

import lbfgs_oracle as LO
from lbfgs_oracle import OPTIONS, ring_push, ring_slot

_PARTS = np.arange(1024)
_TREE = (32, 16, 8, 4, 2, 1, 512, 256, 128, 64)


def sum1024(v):
    """sum_j v[j]: j to partial j mod 1024 in ascending j from +0; the partials meet by the xor tree 32, 16, 8, 4, 2, 1, 512, 256, 128, 64."""
    part = np.zeros(1024, v.dtype)
    for j0 in range(0, len(v), 1024):
        w = min(1024, len(v) - j0)
        part[:w] = part[:w] + v[j0:j0 + w]
    for s in _TREE:
        part = part + part[_PARTS ^ s]
    return part[0]


class GroupedLBFGS:
    """P problems of groups[p] consecutive rows of D coordinates each, with histories of m pairs.  step(x, f, g) consumes f [P] and g [n,D]
    at x [n,D] (n = sum(groups)) and overwrites the rows of x in place; rows of stopped problems are neither read nor written.  log[p] names
    the branch problem p took in each call it ran."""

    def __init__(self, groups, D, m, dtype=np.float32, **options):
        o = dict(OPTIONS, **options)
        self.groups = [int(r) for r in groups]
        self.row_start = np.concatenate([[0], np.cumsum(self.groups)]).astype(np.int64)
        self.P, self.n, self.D, self.m, self.dt = len(self.groups), int(self.row_start[-1]), D, m, np.dtype(dtype).type
        dt = self.dt
        self.c1, self.tol_grad, self.tol_f, self.curv_eps = (dt(np.float32(o[k])) if dt is np.float32 else dt(o[k]) for k in ("c1", "tol_grad", "tol_f", "curv_eps"))
        self.max_ls = int(o["max_ls"])
        self.reset()

    def reset(self):
        self.frames = [LO._Frame(r * self.D, self.m, self.dt) for r in self.groups]

    def rows(self, p):
        return slice(int(self.row_start[p]), int(self.row_start[p + 1]))

    # ------------------------------------------------------------------ the state, as smplpp_lbfgs_state reports it
    def state(self):
        F = self.frames
        return dict(status=np.array([a.status for a in F], np.int32), iterations=np.array([a.iterations for a in F], np.int32),
                    evaluations=np.array([a.evaluations for a in F], np.int32), f_best=np.array([a.f0 for a in F], self.dt),
                    step=np.array([a.t for a in F], self.dt), running=np.array([sum(a.status == 0 for a in F)], np.int64))

    def best(self, x, f=None):
        for p, a in enumerate(self.frames):
            if a.evaluations:
                x[self.rows(p)] = a.x0.reshape(-1, self.D)
                if f is not None:
                    f[p] = a.f0
        return x

    @property
    def log(self):
        return [a.log for a in self.frames]

    # ------------------------------------------------------------------ the rule
    def step(self, x, f, g):
        assert x.dtype == self.dt and x.shape == (self.n, self.D)
        with np.errstate(all="ignore"):
            for p, a in enumerate(self.frames):
                if a.status == 0:
                    xp = x[self.rows(p)].reshape(-1).copy()
                    self._problem(a, xp, self.dt(f[p]), np.asarray(g[self.rows(p)], self.dt).reshape(-1))
                    x[self.rows(p)] = xp.reshape(-1, self.D)

    def _problem(self, a, x, f, g):
        dt = self.dt
        fin = bool(np.isfinite(f)) and bool(np.isfinite(g).all())
        gmax = np.abs(g).max()
        if a.evaluations == 0:
            a.evaluations = 1
            a.x0, a.f0 = x.copy(), f
            if not fin:
                a.status = 4
                return a.log.append("first_nonfinite")
            if gmax <= self.tol_grad:
                a.status = 1
                return a.log.append("first_converged")
            a.g0, a.d = g.copy(), -g
            a.t = min(dt(1), dt(1) / sum1024(np.abs(g)))
            a.gtd = sum1024(g * a.d)
            x[:] = a.x0 + a.t * a.d
            a.ls = 0
            return a.log.append("first")
        a.evaluations += 1
        if not (fin and f <= a.f0 + (self.c1 * a.t) * a.gtd):
            a.ls += 1
            if a.ls > self.max_ls:
                a.status = 3
                x[:] = a.x0
                return a.log.append("exhausted")
            tn, how = dt(0.5) * a.t, "half"
            if np.isfinite(f):
                den = dt(2) * ((f - a.f0) - a.gtd * a.t)
                if den > 0:
                    lo, hi = dt(0.1) * a.t, dt(0.5) * a.t
                    tn, how = -((a.gtd * a.t) * a.t) / den, "interpolated"
                    if not tn >= lo:
                        tn, how = lo, "interpolated_low"
                    if tn > hi:
                        tn, how = hi, "interpolated_high"
            a.t = tn
            x[:] = a.x0 + a.t * a.d
            return a.log.append(how)
        s, y = x - a.x0, g - a.g0
        sy, yy = sum1024(s * y), sum1024(y * y)
        if yy > 0 and sy > self.curv_eps * yy:
            slot, a.head, a.count = ring_push(a.head, a.count, self.m)
            a.S[slot], a.Y[slot], a.sy[slot], a.gamma = s, y, sy, sy / yy
        fo = a.f0
        a.x0, a.f0, a.g0 = x.copy(), f, g.copy()
        a.iterations += 1
        if gmax <= self.tol_grad:
            a.status = 1
            return a.log.append("converged")
        if self.tol_f > 0 and fo - f <= self.tol_f * max(max(abs(fo), abs(f)), dt(1)):
            a.status = 2
            return a.log.append("flat")
        q = g.copy()
        alpha = [None] * a.count
        for i in range(a.count):
            sl = ring_slot(a.head, a.count, self.m, i)
            alpha[i] = sum1024(a.S[sl] * q) / a.sy[sl]
            q = q - alpha[i] * a.Y[sl]
        r = a.gamma * q if a.count else q
        for i in range(a.count - 1, -1, -1):
            sl = ring_slot(a.head, a.count, self.m, i)
            c = alpha[i] - sum1024(a.Y[sl] * r) / a.sy[sl]
            r = r + c * a.S[sl]
        a.d = -r
        a.gtd = sum1024(g * a.d)
        how = "accepted"
        if not a.gtd < 0:
            a.head = a.count = 0
            a.d = -g
            a.gtd = -sum1024(g * g)
            how = "accepted_dropped"
        a.t, a.ls = dt(1), 0
        x[:] = a.x0 + a.d
        a.log.append(how)


def run(opt, funcs, x, max_evals, after=None):
    """max_evals calls of opt.step on x [n,D] (changed in place) with funcs[p] evaluating problem p on its flat vector [rows * D]; stopped
    problems are not evaluated again.  after(call) runs after each call.  Returns x."""
    dt = opt.dt
    f, g = np.zeros(opt.P, dt), np.zeros_like(x)
    for call in range(max_evals):
        live = [p for p, a in enumerate(opt.frames) if a.status == 0]
        if not live:
            break
        for p in live:
            f[p], gp = funcs[p](x[opt.rows(p)].reshape(-1))
            g[opt.rows(p)] = gp.reshape(-1, opt.D)
        opt.step(x, f, g)
        if after:
            after(call)
    return x


# ---------------------------------------------------------------------------------------------------- test functions
class Chain:
    """sum_t Quadratic(D, cond, seed + t)(x_t) + lam sum_t |x_(t+1) - x_t|^2 on the flat vector of T rows of D: the frames of a sequence with
    a velocity term between consecutive ones."""

    def __init__(self, T, D, cond, lam, seed):
        self.T, self.D, self.lam = T, D, lam
        self.q = [LO.Quadratic(D, cond, seed + t) for t in range(T)]

    def __call__(self, x):
        dt = x.dtype.type
        X = x.reshape(self.T, self.D)
        with np.errstate(all="ignore"):
            f, G = dt(0), np.zeros_like(X)
            for t, q in enumerate(self.q):
                ft, G[t] = q(X[t])
                f = f + ft
            d = X[1:] - X[:-1]
            f = f + dt(self.lam) * (d * d).sum(dtype=x.dtype)
            G[1:] = G[1:] + dt(2 * self.lam) * d
            G[:-1] = G[:-1] - dt(2 * self.lam) * d
        return f, G.reshape(-1)


def ragged_batch(dtype):
    """A ragged batch at D = 4: a chain of 5 rows, the chained Rosenbrock function on 2 rows (8 unknowns), a NaN-at-start problem of 1 row and
    a 3-row quadratic that is +inf outside a ball its first steps leave.  Returns (funcs, groups, x [11,4]); the expected statuses are
    1, 1, 4, 1."""
    D = 4
    chain, easy, hard = Chain(5, D, 10, 1.0, 1), LO.Quadratic(D, 10, 1), LO.Quadratic(3 * D, 30, 2)
    hard.c = hard.c * (0.5 / np.linalg.norm(hard.c))  # the minimum is well inside the ball of radius 1
    funcs, groups = [chain, LO.Rosenbrock(), LO.NanAtStart(easy), LO.InfOutsideBall(hard, 1.0)], [5, 2, 1, 3]
    x = np.zeros((sum(groups), D), dtype)
    x[5:7] = LO.Rosenbrock.start(2 * D, dtype).reshape(2, D)
    x[8:11] = (-0.9 * hard.c / np.linalg.norm(hard.c)).reshape(3, D)  # near the rim, opposite the minimum
    return funcs, groups, x
