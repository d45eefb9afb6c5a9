"""Plain numpy statements of the four FK stages on ARBITRARY inputs (smplpp_amd/csrc/stages.hip, the reference's BlendShape /
JointRegression / WorldTransformation / LinearBlendSkinning).  No torch, no GPU.  In float64 they are the reference the stage
calls are held to; in float32 they are "the same graph in fp32", the yardstick whose own error sizes every bar
(tests/test_stage_oracle_cpu.py prints it)."""
import numpy as np

EPS32 = 2.0 ** -24  # half an ulp of 1 in fp32


def rodrigues(theta24, dtype=np.float64):
    """[..., 3] -> [..., 3, 3], pose_math.h's rule: angle = ||theta + 1e-8|| (eps per component), axis from the RAW theta,
    R = I + K sin + K.K (1 - cos)."""
    th = np.asarray(theta24, dtype)
    a = np.sqrt(((th + dtype(1e-8)) ** 2).sum(-1, keepdims=True, dtype=dtype))
    k = th / a
    z = np.zeros_like(k[..., 0])
    K = np.stack([z, -k[..., 2], k[..., 1], k[..., 2], z, -k[..., 0], -k[..., 1], k[..., 0], z], -1).reshape(k.shape[:-1] + (3, 3))
    s, c1 = np.sin(a)[..., None], (dtype(1) - np.cos(a))[..., None]
    R = np.eye(3, dtype=dtype) + K * s + (K @ K) * c1
    assert R.dtype == dtype
    return R


def blend(beta, rot, S, P, dtype=np.float64):
    """beta [n,10], rot [n,24,3,3], S [V,3,10], P [V,3,207] -> (Bs, Bp) [n,V,3]: Bs = S.beta, Bp = P.vec(rot[1:] - I) with the 207
    coefficients joint-major, row-major."""
    beta, rot, S, P = (np.asarray(a, dtype) for a in (beta, rot, S, P))
    n = beta.shape[0]
    c = (rot[:, 1:] - np.eye(3, dtype=dtype)).reshape(n, 207)
    Bs = np.einsum("vxk,nk->nvx", S, beta)
    Bp = np.einsum("vxk,nk->nvx", P, c)
    assert Bs.dtype == dtype and Bp.dtype == dtype
    return Bs, Bp


def joint_regression(T, Jreg, Bs, Bp, dtype=np.float64):
    """T [V,3], Jreg [24,V], Bs, Bp [n,V,3] -> (rest [n,V,3], joints [n,24,3]): rest = T + Bs + Bp, joints = Jreg.(T + Bs), the
    pose blend left out."""
    T, Jreg, Bs, Bp = (np.asarray(a, dtype) for a in (T, Jreg, Bs, Bp))
    shaped = T[None] + Bs
    rest = shaped + Bp
    joints = np.einsum("jv,nvx->njx", Jreg, shaped)
    assert rest.dtype == dtype and joints.dtype == dtype
    return rest, joints


def world(parent, joints, rot, dtype=np.float64):
    """parent [24] (parent[0] ignored), joints [n,24,3], rot [n,24,3,3] ANY 3x3 matrices -> relative transforms [n,24,4,4]:
    the chain G_i = G_p.[R_i | j_i - j_p], then [A | t - A.j] with bottom row (0,0,0,1)."""
    J, R = np.asarray(joints, dtype), np.asarray(rot, dtype)
    n = J.shape[0]
    A, t = [R[:, 0]], [J[:, 0]]
    for i in range(1, 24):
        p = int(parent[i])
        A.append(A[p] @ R[:, i])
        t.append((A[p] @ (J[:, i] - J[:, p])[..., None])[..., 0] + t[p])
    A, t = np.stack(A, 1), np.stack(t, 1)
    X = np.zeros((n, 24, 4, 4), dtype)
    X[..., :3, :3] = A
    X[..., :3, 3] = t - (A @ J[..., None])[..., 0]
    X[..., 3, 3] = 1
    return X


def skinning(W, rest, G, root=None, dtype=np.float64):
    """W [V,24] (any weights), rest [n,V,3], G [n,24,4,4] FULL 4x4 matrices, root [n,3] or None -> verts [n,V,3]:
    M = sum_j w_j G_j, h = M.[rest; 1], verts = h[:3] / h[3] + root."""
    W, rest, G = (np.asarray(a, dtype) for a in (W, rest, G))
    M = np.einsum("vj,njab->nvab", W, G)
    h = np.einsum("nvab,nvb->nva", M[..., :3], rest) + M[..., 3]
    verts = h[..., :3] / h[..., 3:4]
    if root is not None:
        verts = verts + np.asarray(root, dtype)[:, None, :]
    assert verts.dtype == dtype
    return verts


def scaled_error(x, ref64):
    """E(x) = max_i |x_i - ref_i| / max_i |ref_i| over ALL elements: no element can hide in a norm."""
    ref64 = np.asarray(ref64, np.float64)
    err, scale = float(np.abs(np.asarray(x, np.float64) - ref64).max()), float(np.abs(ref64).max())
    if scale == 0:  # an all-zero reference (the pose blend of a zero frame) has no scale: equal or not
        return 0.0 if err == 0 else np.inf
    return err / scale


def bar(e32, factor=4):
    """The elementwise-max form of the project's '4x an fp32 evaluation of the same graph' rule."""
    return max(factor * e32, factor * EPS32)


# ---- the case lists of tests/test_stages_gpu.py (shared with tests/test_stage_oracle_cpu.py, which runs the fp32 oracle on them)
BLEND_SHAPES = [(1, 1), (3, 37), (2, 300)]
REGRESS_V = [1, 255, 256, 257, 700]
WORLD_N = [1, 64, 65]
SKIN_SHAPES = [(1, 1), (3, 37), (2, 300)]

SMPL_PARENT = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21], np.int64)
TREES = {
    "smpl": SMPL_PARENT,
    "chain": np.maximum(0, np.arange(24) - 1).astype(np.int64),
    "star": np.zeros(24, np.int64),
    "binary": np.maximum(0, (np.arange(24) - 1) // 2).astype(np.int64),
}


def _f32(rng, *shape):
    return rng.normal(0, 1, shape).astype(np.float32)


def blend_case(n, V):
    """Inputs of one blend case.  The theta rows carry (where the frame exists) an all-zero frame, a joint at exactly |theta| = pi
    (the fp32 pi along x), one at |theta| = 1e-4 and one at |theta| ~ 7 rad; the rest ~ N(0, 0.5)."""
    rng = np.random.default_rng(1000 + 10 * n + V)
    theta = (0.5 * _f32(rng, n, 24, 3)).astype(np.float32)
    f = n - 1  # the frame that carries the special joints (frame 0 is the zero frame when there are two or more)
    theta[f, 3] = (np.float32(np.pi), 0, 0)
    u = rng.normal(0, 1, 3)
    theta[f, 7] = (1e-4 * u / np.linalg.norm(u)).astype(np.float32)
    u = rng.normal(0, 1, 3)
    theta[f, 11] = (7.0 * u / np.linalg.norm(u)).astype(np.float32)
    if n == 1:  # one frame only: the zero frame is a case of its own (blend_zero_case)
        pass
    else:
        theta[0] = 0
    return dict(beta=_f32(rng, n, 10), theta=theta, S=_f32(rng, V, 3, 10), P=_f32(rng, V, 3, 207), zero_frames=[0] if n > 1 else [])


def blend_zero_case():
    """(n, V) = (1, 1) with the all-zero frame (the one-frame case above carries the special joints instead)."""
    c = blend_case(1, 1)
    c["theta"] = np.zeros_like(c["theta"])
    c["zero_frames"] = [0]
    return c


def regress_case(V, n=3):
    rng = np.random.default_rng(2000 + V)
    return dict(T=_f32(rng, V, 3), Jreg=_f32(rng, 24, V), Bs=_f32(rng, n, V, 3), Bp=_f32(rng, n, V, 3), Bp2=_f32(rng, n, V, 3))


def world_case(n, tree, general):
    """rot: rotations (Rodrigues of N(0,1) vectors, rounded to fp32) or general matrices I + 0.3 N(0,1)."""
    rng = np.random.default_rng(3000 + 7 * n + 2 * sorted(TREES).index(tree) + int(general))
    joints = _f32(rng, n, 24, 3)
    if general:
        rot = (np.eye(3) + 0.3 * rng.normal(0, 1, (n, 24, 3, 3))).astype(np.float32)
    else:
        rot = rodrigues(rng.normal(0, 1, (n, 24, 3))).astype(np.float32)
    return dict(parent=TREES[tree], joints=joints, rot=rot)


def skin_case(n, V):
    """Dense weights |N(0,1)| that do NOT sum to 1, transforms with a random bottom row near (0,0,0,1): the divide matters."""
    rng = np.random.default_rng(4000 + 10 * n + V)
    G = (np.eye(4) + 0.3 * rng.normal(0, 1, (n, 24, 4, 4))).astype(np.float32)
    G[..., 3, :] = (np.array([0, 0, 0, 1]) + 0.05 * rng.normal(0, 1, (n, 24, 4))).astype(np.float32)
    return dict(W=np.abs(_f32(rng, V, 24)), rest=_f32(rng, n, V, 3), G=G, root=_f32(rng, n, 3))
