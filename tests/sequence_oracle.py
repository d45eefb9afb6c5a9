"""The rules of the sequence terms (smplpp_sequence_*, include/smplpp_hip.h) restated in float32 numpy, operation by operation: the layout
tables, split, merge, sum and the temporal smoothness term with its vector-Jacobian product.  In float32 it is the bit reference of the
library.  energy_t is the DEFINITION of the term in torch (any dtype), for autograd in float64."""
import numpy as np

from sum_rules import sum1024

f32 = np.float32


def tables(P, row_start, shared_rows):
    """What sequence_tables.h builds: a dict of P, rows, frames, shared_rows, row_start, frame_start [P+1], problem_of [F],
    row_of [F], frame_of [rows] (-1 - p for the shared row of p), or {"refusal": why}."""
    def no(why):
        return {"refusal": why}

    if P <= 0:
        return no("P must be positive")
    if row_start is None:
        return no("row_start is NULL")
    rs = [int(r) for r in row_start]
    if rs[0] != 0:
        return no("row_start[0] must be 0")
    if any(rs[p + 1] <= rs[p] for p in range(P)):
        return no("row_start must strictly increase")
    if shared_rows not in (0, 1):
        return no("shared_rows must be 0 or 1")
    if rs[P] > 2 ** 31 - 1:
        return no("rows beyond int32 indexing")
    if any(rs[p + 1] - rs[p] - shared_rows < 1 for p in range(P)):
        return no("a problem has no frame beside its shared row")
    T = [rs[p + 1] - rs[p] - shared_rows for p in range(P)]
    frame_of = np.zeros(rs[P], np.int32)
    problem_of, row_of = [], []
    for p in range(P):
        for j in range(T[p]):
            frame_of[rs[p] + j] = len(row_of)
            problem_of.append(p), row_of.append(rs[p] + j)
        if shared_rows:
            frame_of[rs[p + 1] - 1] = -1 - p
    return dict(P=P, rows=rs[P], frames=sum(T), shared_rows=shared_rows, row_start=np.array(rs[:P + 1], np.int64),
                frame_start=np.concatenate([[0], np.cumsum(T)]).astype(np.int64), problem_of=np.array(problem_of, np.int32),
                row_of=np.array(row_of, np.int32), frame_of=frame_of)


def layout(groups, shared_rows=0):
    """tables() of row counts."""
    t = tables(len(groups), np.concatenate([[0], np.cumsum(groups)]), shared_rows)
    assert "refusal" not in t, t
    return t


def split(L, rows, off_f, C_f, C_s=None):
    """rows [n, ld] -> (frames [F, C_f], shared [F, C_s] or None)."""
    frames = rows[L["row_of"], off_f:off_f + C_f].copy()
    shared = None if C_s is None else rows[L["row_start"][L["problem_of"] + 1] - 1, :C_s].copy()
    return frames, shared


def merge(L, grad_frames, off_f, C_f, grad_shared, C_s, out, D, accumulate):
    """The elements [:, :D] of out [n, ld] written (or added into) by smplpp_sequence_merge; the rest is left alone."""
    val = np.zeros((L["rows"], D), f32)
    if grad_frames is not None:
        val[L["row_of"], off_f:off_f + C_f] = grad_frames
    if grad_shared is not None:
        for p in range(L["P"]):
            f0, f1 = L["frame_start"][p], L["frame_start"][p + 1]
            val[L["row_start"][p + 1] - 1, :C_s] = sum1024(np.asarray(grad_shared[f0:f1, :C_s], f32), axis=0)
    with np.errstate(all="ignore"):
        out[:, :D] = out[:, :D] + val if accumulate else val
    return out


def seq_sum(L, frame_values, scale, out, accumulate):
    with np.errstate(all="ignore"):
        for p in range(L["P"]):
            v = f32(scale) * sum1024(np.asarray(frame_values[L["frame_start"][p]:L["frame_start"][p + 1]], f32))
            out[p] = out[p] + v if accumulate else v
    return out


def stencils(L, order):
    """[F] bool: is there a stencil at frame f."""
    f = np.arange(L["frames"])
    lo, hi = L["frame_start"][L["problem_of"]], L["frame_start"][L["problem_of"] + 1]
    return f + 1 < hi if order == 1 else (f - 1 >= lo) & (f + 1 < hi)


def _differences(L, x, K, C, order):
    """(st [F], d [F,K,C] (+0 without a stencil), q [F,K])."""
    F, dt = L["frames"], x.dtype.type
    X = x[:, :K * C].reshape(F, K, C)
    st = stencils(L, order)
    at = np.nonzero(st)[0]
    d = np.zeros((F, K, C), dt)
    d[at] = X[at + 1] - X[at] if order == 1 else (X[at + 1] - X[at]) - (X[at] - X[at - 1])
    q = np.zeros((F, K), dt)
    for c in range(C):
        q = q + d[:, :, c] * d[:, :, c]
    return st, d, q


def smoothness(L, x, K, C, order, weight, rho):
    """x [F, ld] -> (frame_energy [F], point_energy [F,K]), in the dtype of x (float32: the bits of the library)."""
    dt = x.dtype.type
    w = np.ones(K, dt) if weight is None else np.asarray(weight, dt)
    with np.errstate(all="ignore"):
        st, d, q = _differences(L, x, K, C, order)
        if rho == 0:
            e = w[None] * q
        else:
            p2 = dt(rho) * dt(rho)
            e = w[None] * ((p2 * q) / (p2 + q))
        e = np.where(st[:, None] & (w != 0)[None], e, dt(0)).astype(dt)
        return sum1024(e, axis=1), e


def smoothness_vjp(L, x, K, C, order, weight, rho, grad_frame_energy, grad_point_energy, out, accumulate):
    """The K C coordinates of every row of out [F, ld] written (or added into) by smplpp_sequence_smoothness_vjp."""
    F = L["frames"]
    dt = x.dtype.type
    w = np.ones(K, dt) if weight is None else np.asarray(weight, dt)
    with np.errstate(all="ignore"):
        st, d, q = _differences(L, x, K, C, order)
        g = np.zeros((F, K), dt) if grad_frame_energy is None else np.broadcast_to(np.asarray(grad_frame_energy, dt)[:, None], (F, K))
        if grad_point_energy is not None:
            g = g + grad_point_energy
        live = st[:, None] & (w != 0)[None] & (g != 0)
        s = (dt(2) * g) * w[None]
        if rho != 0:
            p2 = dt(rho) * dt(rho)
            t = p2 / (p2 + q)
            s = s * (t * t)
        v = np.where(live[:, :, None], s[:, :, None] * d, dt(0)).astype(dt)
        zero = np.zeros((1, K, C), dt)
        prob = L["problem_of"]
        before = np.concatenate([zero, v[:-1]])
        before[np.concatenate([[True], prob[1:] != prob[:-1]])] = 0
        after = np.concatenate([v[1:], zero])
        after[np.concatenate([prob[1:] != prob[:-1], [True]])] = 0
        val = (before - v if order == 1 else (before + after) - (dt(2) * v)).reshape(F, K * C)
        out[:, :K * C] = out[:, :K * C] + val if accumulate else val
    return out


def energy_t(L, X, order, weight, rho):
    """The definition in torch: point energies [F,K] of X [F,K,C] (zero rows where a frame has no stencil)."""
    import torch

    F, K, _ = X.shape
    w = torch.ones(K, dtype=X.dtype, device=X.device) if weight is None else torch.as_tensor(np.asarray(weight, np.float64)).to(X.dtype).to(X.device)
    out = []
    for p in range(L["P"]):
        Xp = X[int(L["frame_start"][p]):int(L["frame_start"][p + 1])]
        T = Xp.shape[0]
        zero = torch.zeros(1, K, dtype=X.dtype, device=X.device)
        if order == 1:
            d, pad = Xp[1:] - Xp[:-1], ([], [zero])
        else:
            d, pad = Xp[2:] - 2 * Xp[1:-1] + Xp[:-2], ([zero], [zero])
        if T <= order:
            out.append(torch.zeros(T, K, dtype=X.dtype, device=X.device))
            continue
        q = (d * d).sum(-1)
        e = w * q if rho == 0 else w * (rho * rho * q) / (rho * rho + q)
        out.append(torch.cat(pad[0] + [e] + pad[1]))
    return torch.cat(out)
