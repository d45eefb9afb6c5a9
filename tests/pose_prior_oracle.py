"""The pose-prior rules (include/smplpp_hip.h: smplpp_pose_prior, smplpp_pose_prior_vjp) restated twice: in numpy float32, operation
for operation with the partial and tree orders, so that every output bit of the library can be reproduced; and in torch (any dtype)
as the plain definitions, whose float64 autograd is the oracle of the backward pass and whose float32 autograd measures what a plain
fp32 evaluation gets wrong.  Also the synthetic mixtures the tests and the benchmark share.

A prior is a dict: mean [M,D], mat [M,D,D] (row j = output j), offset [M], and lo, hi, weight [D] or None; M may be 0."""
import numpy as np
import torch

from sum_rules import sum64

f32 = np.float32


# ------------------------------------------------------------------------------------------------ priors
def synthetic_gmm(M, D, seed):
    """(means [M,D], covars [M,D,D], weights [M]) in float64: centres from N(0, 0.25^2), covariances Q diag(lambda) Q^T with Q from a
    QR of a normal matrix and lambda log-uniform in [0.02^2, 0.3^2], weights uniform in [0.5, 1.5], normalised."""
    rng = np.random.default_rng(seed)
    means = rng.normal(0, 0.25, (M, D))
    covars = np.empty((M, D, D))
    for m in range(M):
        Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
        lam = np.exp(rng.uniform(np.log(0.02 ** 2), np.log(0.3 ** 2), D))
        covars[m] = (Q * lam) @ Q.T
    w = rng.uniform(0.5, 1.5, M)
    return means, covars, w / w.sum()


def gmm_tables(means, covars, weights):
    """(mean, mat, offset) in float32 from a mixture in float64: mat = sqrt(1/2) L^T with Sigma^-1 = L L^T, offset[m] = -log w_m +
    1/2 log det Sigma_m - (the least of these)."""
    means, covars, weights = (np.asarray(x, np.float64) for x in (means, covars, weights))
    mat = np.stack([np.sqrt(0.5) * np.linalg.cholesky(np.linalg.inv(c)).T for c in covars])
    off = np.array([-np.log(w) + 0.5 * np.linalg.slogdet(c)[1] for w, c in zip(weights, covars)])
    return means.astype(f32), mat.astype(f32), (off - off.min()).astype(f32)


def prior(M, D, seed, limits=True):
    """The prior of synthetic_gmm(M, D, seed) (M = 0: limits alone), with limits that a pose from N(0, 0.3^2) crosses on both sides:
    coordinate 0 unlimited (-inf, inf), coordinate 1 (if any) without an upper limit, a zero weight on coordinate 2."""
    rng = np.random.default_rng(seed + 1000)
    if M:
        mean, mat, offset = gmm_tables(*synthetic_gmm(M, D, seed))
    else:
        mean, mat, offset = np.zeros((0, D), f32), np.zeros((0, D, D), f32), np.zeros(0, f32)
    p = dict(mean=mean, mat=mat, offset=offset, lo=None, hi=None, weight=None)
    if limits:
        lo, hi = rng.uniform(-0.4, -0.05, D).astype(f32), rng.uniform(0.05, 0.4, D).astype(f32)
        w = rng.uniform(0.5, 2.0, D).astype(f32)
        lo[0], hi[0] = -np.inf, np.inf
        if D > 1:
            hi[1] = np.inf
        if D > 2:
            w[2] = 0.0
        p.update(lo=lo, hi=hi, weight=w)
    return p


def poses(n, D, seed):
    return np.random.default_rng(seed).normal(0, 0.3, (n, D)).astype(f32)


# ------------------------------------------------------------------------------------------------ numpy float32, operation for operation
def _matvec8(A, x):
    """out[f, a] = sum_i A[a, i] x[f, i]: partial i mod 8 in ascending i from +0, then ((s0+s4)+(s2+s6)) + ((s1+s5)+(s3+s7))."""
    s = np.zeros((8, x.shape[0], A.shape[0]), f32)
    for i in range(A.shape[1]):
        s[i % 8] = s[i % 8] + A[None, :, i] * x[:, i:i + 1]
    return ((s[0] + s[4]) + (s[2] + s[6])) + ((s[1] + s[5]) + (s[3] + s[7]))


def _mixture(p, X):
    """(e [n,M], y [M,n,D]) of every component."""
    M = len(p["offset"])
    y = np.stack([_matvec8(p["mat"][m], X - p["mean"][m][None, :]) for m in range(M)])
    e = np.stack([sum64(y[m] * y[m]) + p["offset"][m] for m in range(M)], 1)
    return e, y


def _select(e):
    best, eb = np.zeros(e.shape[0], np.int64), e[:, 0].copy()
    for m in range(1, e.shape[1]):
        r = e[:, m] < eb
        eb, best = np.where(r, e[:, m], eb), np.where(r, m, best)
    return best, eb


def _limit(p, X):
    """(v [n,D], sign [n,D])."""
    a, b = X - p["hi"][None, :], p["lo"][None, :] - X
    v = np.where(a > 0, a, np.where(b > 0, b, f32(0))).astype(f32)
    return v, np.where(a > 0, 1, np.where(b > 0, -1, 0))


def forward(p, pose):
    """dict(energy [n], component [n] int64, residual [n,D]) with a mixture, limit_energy [n] with limits."""
    X = np.asarray(pose, f32)
    out = {}
    with np.errstate(all="ignore"):
        if len(p["offset"]):
            e, y = _mixture(p, X)
            best, eb = _select(e)
            out.update(energy=eb.astype(f32), component=best, residual=np.ascontiguousarray(y[best, np.arange(len(X))]))
        if p["lo"] is not None:
            v, _ = _limit(p, X)
            out["limit_energy"] = sum64(p["weight"][None, :] * (v * v))
    return out


def backward(p, pose, component=None, grad_energy=None, grad_residual=None, grad_limit_energy=None, base=None):
    """grad_pose [n,D]; a component outside [0, M) gives the mixture's part +0 (the device-space rule); a base is what accumulate = 1
    adds the finished element to."""
    X = np.asarray(pose, f32)
    n, D = X.shape
    mix, lim = grad_energy is not None or grad_residual is not None, grad_limit_energy is not None
    with np.errstate(all="ignore"):
        if mix:
            M = len(p["offset"])
            comp = forward(p, X)["component"] if component is None else np.asarray(component, np.int64)
            t = np.zeros((n, D), f32)
            for m in range(M):
                rows = np.nonzero(comp == m)[0]
                if not len(rows):
                    continue
                v = np.zeros((len(rows), D), f32)
                if grad_energy is not None:
                    g = np.asarray(grad_energy, f32)[rows]
                    y = _matvec8(p["mat"][m], X[rows] - p["mean"][m][None, :])
                    v = np.where(g[:, None] != 0, (f32(2) * g)[:, None] * y, f32(0)).astype(f32)
                if grad_residual is not None:
                    v = v + np.asarray(grad_residual, f32)[rows]
                t[rows] = _matvec8(np.ascontiguousarray(p["mat"][m].T), v)
            el = t
        if lim:
            g = np.asarray(grad_limit_energy, f32)
            v, sign = _limit(p, X)
            c = (f32(2) * g)[:, None] * p["weight"][None, :]
            u = np.where((g[:, None] != 0) & (sign > 0), c * v, np.where((g[:, None] != 0) & (sign < 0), -(c * v), f32(0))).astype(f32)
            el = t + u if mix else u
        if base is not None:
            el = np.asarray(base, f32) + el
    return np.ascontiguousarray(el, f32)


# ------------------------------------------------------------------------------------------------ torch: the definitions, any dtype
def tensors(p, dtype):
    return {k: None if v is None else torch.tensor(np.asarray(v), dtype=dtype) for k, v in p.items()}


def mixture_t(t, pose):
    """(e [n,M], y [n,M,D]): y = mat (pose - mean), e = |y|^2 + offset."""
    y = torch.einsum("mjk,nmk->nmj", t["mat"], pose[:, None, :] - t["mean"][None])
    return (y * y).sum(-1) + t["offset"][None], y


def energy_t(t, pose, component=None):
    """(energy [n], residual [n,D], component [n]) of the given components, or of the best ones."""
    e, y = mixture_t(t, pose)
    if component is None:
        component = e.detach().argmin(1)
    i = torch.arange(len(pose))
    return e[i, component], y[i, component], component


def limit_t(t, pose):
    """[n]: sum_k weight_k max(pose_k - hi_k, lo_k - pose_k, 0)^2."""
    v = torch.maximum(torch.maximum(pose - t["hi"][None], t["lo"][None] - pose), torch.zeros_like(pose))
    return (t["weight"][None] * v * v).sum(-1)
