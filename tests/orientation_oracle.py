"""The oracle of smplpp_orientation_term / smplpp_orientation_term_vjp and of smplpp_axis_angle_to_rotmat_vjp:

 - `term` / `term_vjp`: the rule of include/smplpp_hip.h restated in numpy operation by operation, the sums through tests/sum_rules.py;
   in float32 it gives the bits of the library, in float64 it is held to the definition;
 - `definition_t`: the definition in torch (A O - T, its squared norm, the Geman-McClure form), for float64 autograd;
 - `rodrigues`: the reference's Rodrigues formula in torch (tests/fk_rotmat_oracle.py), whose float64 autograd is the oracle of the VJP;
 - the three fits of tests/test_orientation_cpu.py and tests/test_orientation_gpu.py, written over callables so that the oracle and
   the library run the same schedule."""
import numpy as np
import torch

import fk_rotmat_oracle as RO
from sum_rules import sum1024

rodrigues = RO.rodrigues


def _prepare(frames, joint, target, offset, weight, C, dt):
    frames = np.asarray(frames, dt)
    n, J = frames.shape[:2]
    joint = np.asarray(joint, np.int64).reshape(-1)
    S = len(joint)
    inr = (joint >= 0) & (joint < J)
    A = frames[:, np.where(inr, joint, 0), :, :3]  # [n,S,3,3]
    O = np.eye(3, dtype=dt)[None, :, :C].repeat(S, 0) if offset is None else np.asarray(offset, dt).reshape(S, 3, C)
    T = np.asarray(target, dt).reshape(-1, S, 3, C)
    Tn = T.shape[0]
    T = np.broadcast_to(T, (n, S, 3, C))
    w = np.ones((1, S), dt) if weight is None else np.asarray(weight, dt).reshape(-1, S)
    w = np.broadcast_to(w, (n, S))
    fin = lambda a, ax: np.isfinite(a).all(axis=ax)
    live = (w != 0) & np.isfinite(w) & inr[None] & fin(A, (2, 3)) & fin(O, (1, 2))[None] & fin(T, (2, 3))
    z = dt(0)
    A = np.where(live[:, :, None, None], A, z)
    T = np.where(live[:, :, None, None], T, z)
    O = np.where(np.isfinite(O), O, z)
    return n, J, S, Tn, joint, inr, A, O, T, np.where(live, w, z), live


def _forward(A, O, T, live, C, dt):
    n, S = live.shape
    E = np.zeros((n, S, 3, C), dt)
    q = np.zeros((n, S), dt)
    for r in range(3):
        for c in range(C):
            m = (A[:, :, r, 0] * O[None, :, 0, c] + A[:, :, r, 1] * O[None, :, 1, c]) + A[:, :, r, 2] * O[None, :, 2, c]
            e = np.where(live, m - T[:, :, r, c], dt(0))
            E[:, :, r, c] = e
            q = q + e * e
    return E, q


def term(frames, joint, target, offset=None, weight=None, rho=0.0, C=3, dtype=np.float32):
    """(energy [n], sensor_energy [n,S], residual [n,S,3,C]) in `dtype`."""
    dt = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        n, J, S, Tn, joint, inr, A, O, T, w, live = _prepare(frames, joint, target, offset, weight, C, dt)
        E, q = _forward(A, O, T, live, C, dt)
        if rho == 0:
            se = w * q
        else:
            p2 = dt(rho) * dt(rho)
            se = w * ((p2 * q) / (p2 + q))
        se = np.where(live, se, dt(0)).astype(dt)
    return sum1024(se, axis=1), se, E


def term_vjp(frames, joint, target, offset=None, weight=None, rho=0.0, C=3, grad_energy=None, grad_sensor_energy=None, grad_residual=None,
             grad_frames=None, grad_offset=None, grad_target=None, accumulate=0, dtype=np.float32):
    """The three gradients written into (accumulate: added into) the arrays given, which are returned; None is left out.  grad_frames
    has the shape of frames (column 3 of a row_stride 4 array is never written), grad_offset [S,3,C], grad_target [Tn,S,3,C]."""
    dt = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        n, J, S, Tn, joint, inr, A, O, T, w, live = _prepare(frames, joint, target, offset, weight, C, dt)
        E, q = _forward(A, O, T, live, C, dt)
        g = (np.zeros(n, dt) if grad_energy is None else np.asarray(grad_energy, dt))[:, None] + \
            (np.zeros((n, S), dt) if grad_sensor_energy is None else np.asarray(grad_sensor_energy, dt))
        m = w
        if rho != 0:
            p2 = dt(rho) * dt(rho)
            d = p2 / (p2 + q)
            m = w * (d * d)
        k = (dt(2) * g) * m
        gr = np.zeros((n, S, 3, C), dt) if grad_residual is None else np.asarray(grad_residual, dt).reshape(n, S, 3, C)
        G = np.where(live[:, :, None, None], k[:, :, None, None] * E + gr, dt(0)).astype(dt)
        if grad_frames is not None:
            acc = np.zeros((n, J, 3, 3), dt)
            hit = np.zeros((n, J), bool)
            for s in range(S):
                if not inr[s]:
                    continue
                j = joint[s]
                v = np.zeros((n, 3, 3), dt)
                for r in range(3):
                    for kk in range(3):
                        t = G[:, s, r, 0] * O[s, kk, 0]
                        for c in range(1, C):
                            t = t + G[:, s, r, c] * O[s, kk, c]
                        v[:, r, kk] = t
                acc[:, j] = np.where(live[:, s, None, None], acc[:, j] + v, acc[:, j])
                hit[:, j] |= live[:, s]
            old = grad_frames[..., :3]
            grad_frames[..., :3] = np.where(hit[:, :, None, None], old + acc, old) if accumulate else acc
        neg = np.where(live[:, :, None, None], -G, dt(0)).astype(dt)
        if grad_target is not None:
            val = neg if Tn != 1 else sum1024(neg, axis=0)[None]  # (Tn = n = 1 is the shared form: one element through the sum)
            grad_target[...] = grad_target + val if accumulate else val
        if grad_offset is not None:
            AtG = np.zeros((n, S, 3, C), dt)
            for kk in range(3):
                for c in range(C):
                    AtG[:, :, kk, c] = (A[:, :, 0, kk] * G[:, :, 0, c] + A[:, :, 1, kk] * G[:, :, 1, c]) + A[:, :, 2, kk] * G[:, :, 2, c]
            val = sum1024(np.where(live[:, :, None, None], AtG, dt(0)).astype(dt), axis=0)
            grad_offset[...] = grad_offset + val if accumulate else val
    return grad_frames, grad_offset, grad_target


def live_mask(frames, joint, target, offset, weight, C):
    """[n,S] bool: the sensors that are not dead."""
    return _prepare(frames, joint, target, offset, weight, C, np.float64)[-1]


def definition_t(frames, joint, target, offset=None, weight=None, rho=0.0, C=3, live=None):
    """The definition in torch, in the dtype of `frames` [n,J,3,3 or 4]: (energy [n], sensor_energy [n,S], residual [n,S,3,C]).  `live`
    [n,S] bool (live_mask) switches dead sensors off; their inputs must then be finite stand-ins (clean_t)."""
    dt, dev = frames.dtype, frames.device
    joint = joint if torch.is_tensor(joint) else torch.as_tensor(np.asarray(joint, np.int64), device=dev)
    A = frames[:, joint, :, :3]
    O = torch.eye(3, dtype=dt, device=dev)[:, :C].expand(len(joint), 3, C) if offset is None else offset
    E = A @ O - target
    w = torch.ones((), dtype=dt, device=dev) if weight is None else weight.reshape(-1, len(joint))
    if live is not None:
        mask = torch.as_tensor(np.asarray(live), device=dev)
        E = torch.where(mask[:, :, None, None], E, torch.zeros((), dtype=dt, device=dev))
    q = (E * E).sum((-1, -2))
    se = w * q if rho == 0 else w * (rho * rho * q) / (rho * rho + q)
    if live is not None:
        se = torch.where(mask, se, torch.zeros((), dtype=dt, device=dev))
    else:
        se = se.expand(q.shape)
    return se.sum(1), se, E


def clean(frames, joint, target, offset, weight):
    """The inputs with every entry that is not finite, and every joint index out of range, replaced by a finite stand-in (for
    definition_t under a live mask)."""
    J = np.shape(frames)[1]
    z = lambda a: None if a is None else np.nan_to_num(np.asarray(a, np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    joint = np.asarray(joint, np.int64)
    return z(frames), np.where((joint >= 0) & (joint < J), joint, 0), z(target), z(offset), z(weight)


def definition_vjp(frames, joint, target, offset, weight, rho, C, cot, dtype=torch.float64):
    """((energy, sensor_energy, residual), (grad_frames, grad_offset, grad_target)) of the definition by autograd in `dtype`, as float64
    numpy; cot = (grad_energy, grad_sensor_energy, grad_residual), None = zero.  offset None: the gradient at the identity columns."""
    live = live_mask(frames, joint, target, offset, weight, C)
    f, j, t, o, w = clean(frames, joint, target, offset, weight)
    S = len(j)
    if o is None:
        o = np.eye(3)[None, :, :C].repeat(S, 0)
    leaf = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype, requires_grad=True)
    F, T, O = leaf(f), leaf(t), leaf(o)
    W = None if w is None else torch.tensor(w, dtype=dtype)
    out = definition_t(F, j, T, O, W, rho, C, live)
    loss = 0
    for v, g in zip(out, cot):
        if g is not None:
            loss = loss + (v * torch.tensor(np.asarray(g, np.float64), dtype=dtype).reshape(v.shape)).sum()
    gs = torch.autograd.grad(loss, (F, O, T), allow_unused=True)
    gs = tuple((torch.zeros_like(x) if g is None else g).detach().double().numpy() for g, x in zip(gs, (F, O, T)))
    return tuple(v.detach().double().numpy() for v in out), gs


def rodrigues_vjp(aa, grad_rot, dtype=torch.float64):
    """dL/daa [..., 3] by autograd of `rodrigues` in `dtype`, float64 numpy out."""
    th = torch.tensor(np.asarray(aa, np.float64), dtype=dtype, requires_grad=True)
    (g,) = torch.autograd.grad((rodrigues(th) * torch.tensor(np.asarray(grad_rot, np.float64), dtype=dtype)).sum(), (th,))
    return g.double().numpy()


def random_rotations(rng, shape, angle=None):
    """float64 rotations [*shape,3,3] about random axes; by N(0,1)-scaled axis-angles, or all by `angle` radians.  (The reference's
    formula with its 1e-8 is a rotation to 1e-8 only: the polar factor makes it one to float64.)"""
    aa = rng.standard_normal(tuple(shape) + (3,))
    if angle is not None:
        aa = angle * aa / np.linalg.norm(aa, axis=-1, keepdims=True)
    u, _, vt = np.linalg.svd(RO.rodrigues_np(aa))
    return u @ vt


def random_case(n, S, C, J=24, rs=4, seed=0, Tn=None, Wn=None, offsets=True, one_joint=False, dtype=np.float32):
    """frames [n,J,3,rs] of rotations (column 3 random), joint [S] (sensors share joints once S > J), offset, target, weight."""
    rng = np.random.default_rng(seed)
    frames = np.empty((n, J, 3, rs))
    frames[..., :3] = random_rotations(rng, (n, J))
    frames[..., 3:] = rng.standard_normal((n, J, 3, rs - 3))
    joint = np.full(S, J // 2, np.int64) if one_joint else rng.integers(0, J, S)
    offset = random_rotations(rng, (S,), 0.4)[:, :, :C] if offsets else None
    Tn, Wn = n if Tn is None else Tn, n if Wn is None else Wn
    target = random_rotations(rng, (Tn, S))[..., :C] + 0.05 * rng.standard_normal((Tn, S, 3, C))
    weight = rng.uniform(0.5, 2.0, (Wn, S))
    cast = lambda a: None if a is None else np.ascontiguousarray(a, dtype)
    return cast(frames), joint, cast(offset), cast(target), cast(weight)


def cotangents(n, S, C, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(s).astype(dtype) for s in ((n,), (n, S), (n, S, 3, C)))


# ------------------------------------------------------------------------------------------------ the three fits
FIT_STEPS, FIT_LR = 200, 0.05


def adam(params, loss_fn, steps=FIT_STEPS, lr=FIT_LR, every=25):
    """Adam on loss_fn(): (first loss, last loss after the final step, the losses at every `every`-th step)."""
    opt = torch.optim.Adam(params, lr=lr)
    track = []
    for i in range(steps):
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        opt.step()
        if i % every == 0:
            track.append(float(loss.detach()))
    with torch.no_grad():
        last = float(loss_fn())
    return track[0], last, track + [last]


def fit_passes(last, last64):
    return np.isfinite(last) and (last < 1e-6 or last <= 2 * last64)


def imu_fit(forward, term_energy, dtype, device="cpu"):
    """The IMU fit of tests/test_skeleton_cpu.py with its orientation part through the term: forward(theta) -> (world, posed);
    term_energy(frames, joint, target, offset, weight, C) -> energy [n]."""
    import test_skeleton_cpu as SK

    target = torch.as_tensor(SK.fit_target(), dtype=dtype, device=device)
    with torch.no_grad():
        world_t, posed_t = (a.clone() for a in forward(target))
    T = world_t[:, SK.IMU_JOINTS, :, :3].contiguous()
    theta = torch.zeros(SK.FIT_N, 25, 3, dtype=dtype, device=device, requires_grad=True)

    def loss():
        world, posed = forward(theta)
        return term_energy(world, SK.IMU_JOINTS, T, None, None, 3).sum() + ((posed[:, 0] - posed_t[:, 0]) ** 2).sum()

    return adam([theta], loss)


CAL_N = 8


def calibration_case():
    """theta ~ N(0, 0.3^2) [8,25,3] (default_rng(11)) and the six true offsets: rotations of 0.4 rad about random axes."""
    rng = np.random.default_rng(11)
    theta = (0.3 * rng.standard_normal((CAL_N, 25, 3))).astype(np.float32)
    return theta, random_rotations(rng, (6,), 0.4).astype(np.float32)


def calibration_fit(world, term_energy, rot6d, dtype, device="cpu"):
    """Poses fixed (world [8,24,3,4] of calibration_case's theta), the six offsets unknown: O = rot6d(x) from the identity, targets
    A O*, Adam on sum energy."""
    import test_skeleton_cpu as SK

    world = world.detach()
    O_true = torch.as_tensor(calibration_case()[1], dtype=dtype, device=device)
    with torch.no_grad():
        T = (world[:, SK.IMU_JOINTS, :, :3] @ O_true).contiguous()
    x = torch.tensor([1.0, 0, 0, 1, 0, 0], dtype=dtype, device=device).repeat(6, 1).requires_grad_(True)
    return adam([x], lambda: term_energy(world, SK.IMU_JOINTS, T, rot6d(x), None, 3).sum())


SMOOTH_T = 6


def smooth_case():
    """A sequence of six poses that moves steadily: theta[f] = a + f b, a ~ N(0, 0.2^2), b ~ N(0, 0.05^2) (default_rng(13))."""
    rng = np.random.default_rng(13)
    a, b = 0.2 * rng.standard_normal((25, 3)), 0.05 * rng.standard_normal((25, 3))
    return (a[None] + np.arange(SMOOTH_T)[:, None, None] * b[None]).astype(np.float32)


def smooth_fit(forward, term_energy, rotmat, smooth, dtype, device="cpu"):
    """One sequence of T = 6: the orientation of all 24 joints and the root position as data on frames 0 and 5 only (weight 0 in
    between), plus the chordal smoothness sum_f |R[f+1] - R[f]|^2 of the 24 local rotations: rotmat(aa [6,24,3]) -> [6,24,3,3],
    smooth(rot [6,24,9]) -> frame energies."""
    target = torch.as_tensor(smooth_case(), dtype=dtype, device=device)
    with torch.no_grad():
        world_t, posed_t = (a.clone() for a in forward(target))
    T = world_t[..., :3].contiguous()
    joints = list(range(24))
    w = torch.zeros(SMOOTH_T, 24, dtype=dtype, device=device)
    w[0], w[SMOOTH_T - 1] = 1, 1
    ends = [0, SMOOTH_T - 1]
    theta = torch.zeros(SMOOTH_T, 25, 3, dtype=dtype, device=device, requires_grad=True)

    def loss():
        world, posed = forward(theta)
        data = term_energy(world, joints, T, None, w, 3).sum() + ((posed[ends, 0] - posed_t[ends, 0]) ** 2).sum()
        return data + smooth(rotmat(theta[:, 1:]).reshape(SMOOTH_T, 24, 9)).sum()

    return adam([theta], loss)


def oracle_term_energy(frames, joint, target, offset, weight, C):
    return definition_t(frames, joint, target, offset, weight, 0.0, C)[0]


def oracle_smooth(rot):
    return ((rot[1:] - rot[:-1]) ** 2).sum((1, 2))
