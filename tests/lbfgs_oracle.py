"""The per-frame rule of smplpp_lbfgs_step (include/smplpp_hip.h) restated in numpy with the dtype as a parameter: in float32,
operation for operation with the 64-partial sums (sum_rules.sum64), it is the bit reference of the library; in float64 it is the numerical reference.
`rule` states it once with the sum rule as a parameter; lbfgs_groups_oracle.py calls it with sum_rules.sum1024.  Also the test functions the L-BFGS tests share, each returning (f, g) in the dtype of its argument.

A frame's sums run over vectors of 64 partials, one numpy operation per 64 coordinates, so that D = 20670 is cheap."""
import numpy as np

from sum_rules import sum64

OPTIONS = dict(c1=1e-4, tol_grad=1e-5, tol_f=0.0, max_ls=20, curv_eps=1e-10)


def ring_slot(head, count, m, i):
    """The slot of the i-th newest pair."""
    return (head + count - 1 - i) % m


def ring_push(head, count, m):
    """(slot written, head, count) after a push."""
    if count < m:
        return (head + count) % m, head, count + 1
    return head, (head + 1) % m, count


def rule(o, a, x, f, g, total):
    """The rule, once: one evaluation of the problem with state `a` (a _Frame) at its flat vector x (overwritten in place) with energy
    f and gradient g, under the options of `o` (dt, m, c1, tol_grad, tol_f, curv_eps, max_ls).  total(v) is the sum rule: sum64 for the
    frames of smplpp_lbfgs_create, sum1024 for the problems of a grouped handle; nothing else differs."""
    dt = o.dt
    fin = bool(np.isfinite(f)) and bool(np.isfinite(g).all())
    gmax = np.abs(g).max()
    if a.evaluations == 0:
        a.evaluations = 1
        a.x0, a.f0 = x.copy(), f
        if not fin:
            a.status = 4
            return a.log.append("first_nonfinite")
        if gmax <= o.tol_grad:
            a.status = 1
            return a.log.append("first_converged")
        a.g0, a.d = g.copy(), -g
        a.t = min(dt(1), dt(1) / total(np.abs(g)))
        a.gtd = total(g * a.d)
        x[:] = a.x0 + a.t * a.d
        a.ls = 0
        return a.log.append("first")
    a.evaluations += 1
    if not (fin and f <= a.f0 + (o.c1 * a.t) * a.gtd):
        a.ls += 1
        if a.ls > o.max_ls:
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
    sy, yy = total(s * y), total(y * y)
    if yy > 0 and sy > o.curv_eps * yy:
        slot, a.head, a.count = ring_push(a.head, a.count, o.m)
        a.S[slot], a.Y[slot], a.sy[slot], a.gamma = s, y, sy, sy / yy
    fo = a.f0
    a.x0, a.f0, a.g0 = x.copy(), f, g.copy()
    a.iterations += 1
    if gmax <= o.tol_grad:
        a.status = 1
        return a.log.append("converged")
    if o.tol_f > 0 and fo - f <= o.tol_f * max(max(abs(fo), abs(f)), dt(1)):
        a.status = 2
        return a.log.append("flat")
    q = g.copy()
    alpha = [None] * a.count
    for i in range(a.count):
        sl = ring_slot(a.head, a.count, o.m, i)
        alpha[i] = total(a.S[sl] * q) / a.sy[sl]
        q = q - alpha[i] * a.Y[sl]
    r = a.gamma * q if a.count else q
    for i in range(a.count - 1, -1, -1):
        sl = ring_slot(a.head, a.count, o.m, i)
        c = alpha[i] - total(a.Y[sl] * r) / a.sy[sl]
        r = r + c * a.S[sl]
    a.d = -r
    a.gtd = total(g * a.d)
    how = "accepted"
    if not a.gtd < 0:
        a.head = a.count = 0
        a.d = -g
        a.gtd = -total(g * g)
        how = "accepted_dropped"
    a.t, a.ls = dt(1), 0
    x[:] = a.x0 + a.d
    a.log.append(how)


class _Frame:
    def __init__(self, D, m, dt):
        self.status = self.iterations = self.evaluations = self.ls = self.head = self.count = 0
        self.f0 = self.t = self.gtd = self.gamma = dt(0)
        self.x0 = self.g0 = self.d = None
        self.S, self.Y, self.sy = np.zeros((m, D), dt), np.zeros((m, D), dt), np.zeros(m, dt)
        self.log = []


class LBFGS:
    """n frames of D unknowns with histories of m pairs.  step(x, f, g) consumes f [n] and g [n,D] at x [n,D] and overwrites the rows of
    x in place; rows of stopped frames are not touched (nor read).  log[i] names the branch frame i took in each call it ran."""

    def __init__(self, n, D, m, dtype=np.float32, **options):
        o = dict(OPTIONS, **options)
        self.n, self.D, self.m, self.dt = n, D, m, np.dtype(dtype).type
        dt = self.dt
        self.c1, self.tol_grad, self.tol_f, self.curv_eps = (dt(np.float32(o[k])) if dt is np.float32 else dt(o[k]) for k in ("c1", "tol_grad", "tol_f", "curv_eps"))
        self.max_ls = int(o["max_ls"])
        self.reset()

    def reset(self):
        self.frames = [_Frame(self.D, self.m, self.dt) for _ in range(self.n)]

    # ------------------------------------------------------------------ the state, as smplpp_lbfgs_state reports it
    def state(self):
        F = self.frames
        return dict(status=np.array([a.status for a in F], np.int32), iterations=np.array([a.iterations for a in F], np.int32),
                    evaluations=np.array([a.evaluations for a in F], np.int32), f_best=np.array([a.f0 for a in F], self.dt),
                    step=np.array([a.t for a in F], self.dt), running=np.array([sum(a.status == 0 for a in F)], np.int64))

    def best(self, x, f=None):
        for i, a in enumerate(self.frames):
            if a.evaluations:
                x[i] = a.x0
                if f is not None:
                    f[i] = a.f0
        return x

    @property
    def log(self):
        return [a.log for a in self.frames]

    def step(self, x, f, g):
        assert x.dtype == self.dt and x.shape == (self.n, self.D)
        with np.errstate(all="ignore"):
            for i, a in enumerate(self.frames):
                if a.status == 0:
                    rule(self, a, x[i], self.dt(f[i]), np.asarray(g[i], self.dt), sum64)


def run(opt, funcs, x, max_evals, after=None):
    """max_evals calls of opt.step on x [n,D] (changed in place) with funcs[i] evaluating frame i; rows of stopped frames are not
    evaluated again.  after(call) runs after each call.  Returns x."""
    n, dt = len(funcs), opt.dt
    f, g = np.zeros(n, dt), np.zeros_like(x)
    for call in range(max_evals):
        live = [i for i, a in enumerate(opt.frames) if a.status == 0]
        if not live:
            break
        for i in live:
            f[i], g[i] = funcs[i](x[i])
        opt.step(x, f, g)
        if after:
            after(call)
    return x


# ---------------------------------------------------------------------------------------------------- test functions
class Quadratic:
    """f = 1/2 (x - c)^T A (x - c) with A = H diag(lam) H, H = I - 2 v v^T a reflection and lam log-spaced in scale [1, cond]: a prescribed
    spectrum at O(D) work per evaluation."""

    def __init__(self, D, cond, seed, scale=1.0):
        rng = np.random.default_rng(seed)
        v = rng.normal(size=D)
        self.v = v / np.linalg.norm(v)
        self.lam = scale * (np.exp(np.linspace(0.0, np.log(cond), D)) if D > 1 else np.ones(1))
        self.c = rng.normal(size=D)

    def __call__(self, x):
        dt = x.dtype.type
        v, lam, c = self.v.astype(dt), self.lam.astype(dt), self.c.astype(dt)
        with np.errstate(all="ignore"):
            e = x - c
            w = e - (dt(2) * (v @ e)) * v
            lw = lam * w
            return dt(0.5) * (w @ lw), lw - (dt(2) * (v @ lw)) * v


class SoftAbs(Quadratic):
    """f = sum_k lam_k (sqrt(1 + w_k^2) - 1) with w = H (x - c): convex and not quadratic, so that a small D does not end in a few
    exact steps."""

    def __call__(self, x):
        dt = x.dtype.type
        v, lam, c = self.v.astype(dt), self.lam.astype(dt), self.c.astype(dt)
        with np.errstate(all="ignore"):
            e = x - c
            w = e - (dt(2) * (v @ e)) * v
            r = np.sqrt(dt(1) + w * w)
            lw = lam * (w / r)
            return lam @ (r - dt(1)), lw - (dt(2) * (v @ lw)) * v


class Rosenbrock:
    """The chained Rosenbrock function: sum_i 100 (x_(i+1) - x_i^2)^2 + (1 - x_i)^2."""

    def __call__(self, x):
        dt = x.dtype.type
        with np.errstate(all="ignore"):
            a, b = x[1:] - x[:-1] * x[:-1], dt(1) - x[:-1]
            g = np.zeros_like(x)
            g[:-1] = dt(-400) * a * x[:-1] - dt(2) * b
            g[1:] = g[1:] + dt(200) * a
            return dt(100) * (a @ a) + b @ b, g

    @staticmethod
    def start(D, dtype):
        x = np.ones(D, dtype)
        x[0::2] = -1.2
        return x


class InfOutsideBall:
    """`inner` inside the ball |x| <= radius, +inf outside (where the gradient is the inner one's)."""

    def __init__(self, inner, radius):
        self.inner, self.radius = inner, radius

    def __call__(self, x):
        f, g = self.inner(x)
        return (f if x @ x <= x.dtype.type(self.radius) ** 2 else x.dtype.type(np.inf)), g


class NanGradientPast:
    """`inner`, but the gradient is NaN where sign x[0] > threshold."""

    def __init__(self, inner, threshold, sign=1.0):
        self.inner, self.threshold, self.sign = inner, threshold, sign

    def __call__(self, x):
        f, g = self.inner(x)
        return f, (g if self.sign * x[0] <= self.threshold else np.full_like(g, np.nan))


class NanAtStart:
    """NaN energy everywhere."""

    def __init__(self, inner):
        self.inner = inner

    def __call__(self, x):
        return x.dtype.type(np.nan), self.inner(x)[1]


class NeverArmijo:
    """A constant energy with a gradient that promises descent: no step, however short, satisfies the Armijo condition."""

    def __call__(self, x):
        return x.dtype.type(1), np.ones_like(x)


def mixed_batch(dtype):
    """The issue's mixed batch at D = 8: an easy quadratic, Rosenbrock, a NaN-at-start frame and a quadratic that is +inf outside a
    ball its first steps leave.  Returns (funcs, x [4,8]); the expected statuses are 1, 1, 4, 1."""
    D = 8
    easy, hard = Quadratic(D, 10, 1), Quadratic(D, 30, 2)
    hard.c = hard.c * (0.5 / np.linalg.norm(hard.c))  # the minimum is well inside the ball of radius 1
    funcs = [easy, Rosenbrock(), NanAtStart(easy), InfOutsideBall(hard, 1.0)]
    x = np.zeros((4, D), dtype)
    x[1] = Rosenbrock.start(D, dtype)
    x[3] = -0.9 * hard.c / np.linalg.norm(hard.c)  # near the rim, opposite the minimum
    return funcs, x
