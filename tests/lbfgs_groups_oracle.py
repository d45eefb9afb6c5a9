"""The rule of a grouped L-BFGS handle (smplpp_lbfgs_create_grouped, include/smplpp_hip.h) restated in numpy with the dtype as a parameter:
the per-frame rule of smplpp_lbfgs_step on the N = rows * D elements of a problem, with every sum by the 1024-partial rule (sum_rules.sum1024).  In float32,
operation for operation, it is the bit reference of the library; in float64 the numerical one.  The rule itself (lbfgs_oracle.rule, called
here with sum1024), the ring arithmetic, the options and the test functions are those of lbfgs_oracle.py; Chain couples the rows of a problem.

A problem's sums run over vectors of 1024 partials, one numpy operation per 1024 elements."""
import numpy as np

import lbfgs_oracle as LO
from lbfgs_oracle import OPTIONS, ring_push, ring_slot
from sum_rules import sum1024


class GroupedLBFGS(LO.LBFGS):
    """P problems of groups[p] consecutive rows of D coordinates each, with histories of m pairs.  step(x, f, g) consumes f [P] and g [n,D]
    at x [n,D] (n = sum(groups)) and overwrites the rows of x in place; rows of stopped problems are neither read nor written.  log[p] names
    the branch problem p took in each call it ran.  Options, state() and log are those of LBFGS, one entry per problem."""

    def __init__(self, groups, D, m, dtype=np.float32, **options):
        self.groups = [int(r) for r in groups]
        self.row_start = np.concatenate([[0], np.cumsum(self.groups)]).astype(np.int64)
        self.P = len(self.groups)
        LO.LBFGS.__init__(self, int(self.row_start[-1]), D, m, dtype, **options)

    def reset(self):
        self.frames = [LO._Frame(r * self.D, self.m, self.dt) for r in self.groups]

    def rows(self, p):
        return slice(int(self.row_start[p]), int(self.row_start[p + 1]))

    def best(self, x, f=None):
        for p, a in enumerate(self.frames):
            if a.evaluations:
                x[self.rows(p)] = a.x0.reshape(-1, self.D)
                if f is not None:
                    f[p] = a.f0
        return x

    def step(self, x, f, g):
        assert x.dtype == self.dt and x.shape == (self.n, self.D)
        with np.errstate(all="ignore"):
            for p, a in enumerate(self.frames):
                if a.status == 0:
                    xp = x[self.rows(p)].reshape(-1).copy()
                    LO.rule(self, a, xp, self.dt(f[p]), np.asarray(g[self.rows(p)], self.dt).reshape(-1), sum1024)
                    x[self.rows(p)] = xp.reshape(-1, self.D)


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
