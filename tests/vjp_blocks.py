"""The block-scaled bar of the backward passes smplpp_fk_vjp, smplpp_fk_rotmat_vjp and smplpp_vposer_vjp, and the cases it is
asserted on (tests/test_vjp_blocks_cpu.py runs the fp32 oracle through them, tests/test_vjp_blocks_gpu.py the kernels).

An L2 norm over a frame's dL/dtheta is owned by the root: a leaf joint's 3-vector can be wrong by 1e-3 of its own size inside a
norm that moves by 1e-5.  Here every output is cut into the blocks a caller reads as one quantity,

    output                 block
    dL/dtheta [n,25,3]     each (frame, row) 3-vector; row 0 is the root translation      THETA
    dL/dbeta  [n,10]       each frame                                                     FRAME
    rot       [n,24,3,3]   each (frame, joint) 3x3                                        ROT
    trans     [n,3]        each frame                                                     FRAME
    dL/dz     [n,32]       each frame                                                     FRAME

and E = max over blocks of (max_{i in block} |x_i - ref_i| / max_{i in block} |ref_i|) is held to bar(e32) = max(4 e32, 4 x 2^-24)
(stage_oracle.bar), e32 the E of the fp32 torch evaluation of the same oracle graph on the same case: the maximum over ALL the
case's blocks of that output, never a per-block yardstick.

numpy only at import; the `*_reference` helpers import the torch restatements (fk_vjp_oracle, fk_rotmat_oracle,
vposer_vjp_oracle) when they are called."""
import numpy as np

from stage_oracle import EPS32, bar  # noqa: F401  (bar(e32) = max(4 e32, 4 x 2^-24); restated nowhere else)

THETA, ROT = (2,), (2, 3)  # block axes of dL/dtheta [n,25,3] and rot [n,24,3,3]


def frame_axes(a):
    """Block axes that make each frame (axis 0) one block."""
    return tuple(range(1, np.ndim(a)))


def block_errors(x, ref64, block_axes):
    """Per block: max |x - ref| / max |ref|; a block whose float64 reference is all zero gives 0 if x is all zero there (either
    sign of zero), inf otherwise."""
    ref64 = np.asarray(ref64, np.float64)
    x = np.asarray(x, np.float64)
    assert x.shape == ref64.shape, (x.shape, ref64.shape)
    err = np.abs(x - ref64).max(axis=block_axes)
    scale = np.abs(ref64).max(axis=block_axes)
    bad = ~np.isfinite(err)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale == 0, np.where(np.abs(x).max(axis=block_axes) == 0, 0.0, np.inf), err / scale)
    return np.where(bad, np.inf, e)


def block_error(x, ref64, block_axes):
    """E = max over blocks of `block_errors`."""
    return float(block_errors(x, ref64, block_axes).max())


def zero_blocks(ref64, block_axes):
    """bool per block: the float64 reference is exactly zero there."""
    return np.abs(np.asarray(ref64, np.float64)).max(axis=block_axes) == 0


def l2_rel(a, b):
    """The L2 figure of the existing backward tests (test_fk_vjp_gpu.py::_rel), kept to show what it admits."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30))


# ------------------------------------------------------------------------------------------------ models
def eight_weights(synth_model):
    """The synthetic model with one to four extra small weights per vertex: at most 8 weights per vertex (MAXW = 8)."""
    md = {k: v.copy() for k, v in synth_model.items()}
    rng = np.random.default_rng(5)
    w = md["weights"].astype(np.float64)
    for v in range(w.shape[0]):
        extra = rng.choice(np.where(w[v] == 0)[0], size=int(rng.integers(1, 5)), replace=False)
        w[v, extra] = rng.uniform(0.01, 0.1, len(extra))
    w /= w.sum(axis=1, keepdims=True)
    md["weights"] = w.astype(np.float32)
    return md


MODELS = ("synth", "eight", "tiny")
MAXW = {"synth": 4, "eight": 8, "tiny": 24}
_models = {}


def model(which):
    """One of MODELS (built once; never modified): the synthetic model (6890 = 215 x 32 + 10 vertices), its eight-weight variant,
    tiny_model(61, seed=7) (dense weights, two vertex groups, the second partial)."""
    from smplpp_amd import model_io

    if which not in _models:
        _models[which] = {"synth": model_io.synthetic_model, "eight": lambda: eight_weights(model_io.synthetic_model()),
                          "tiny": lambda: model_io.tiny_model(61, seed=7)}[which]()
    return _models[which]


# ------------------------------------------------------------------------------------------------ FK cases
# A case: dict(name, model, beta [n,10], theta [n,25,3], gv [n,V,3] or None, gj [n,24,3] or None, frames (the checked ones)).
# The rotation-matrix entry point takes trans = theta[:, 0] and `rot_of(case, general)`.
VJ_FT = 32  # smplpp_amd/csrc/fk_vjp.hip: frames per workgroup of vjp_skin_kernel
DENSE_N = [1, VJ_FT - 1, VJ_FT, VJ_FT + 1, 2 * VJ_FT + 1]
KINDS = ["verts", "joints", "both"]
BIG_N, BIG_FRAMES = 1024, [0, 31, 32, 1023]
FORMS = ["e", "h", "b"]


def vjp_chunks(cus, n, V):
    """fk_vjp.hip::vjp_chunks restated: (frame tiles, chunks of vertex groups, groups per chunk) of vjp_skin_kernel's grid on a
    device with `cus` compute units.  The slab sum of vjp_chain_kernel runs over the chunks, so the bits depend on n through it."""
    VGn = (V + 31) // 32
    nft = (n + VJ_FT - 1) // VJ_FT
    want = max(1, 2 * cus // nft)
    gpc = (VGn + want - 1) // want
    gpc = max(4, (gpc + 3) // 4 * 4)
    return nft, (VGn + gpc - 1) // gpc, gpc


def dense_inputs(n, seed):
    """tests/test_fk_vjp_gpu.py::_inputs, restated: config-2 style inputs with a theta = 0 joint, a zero frame and |theta| = pi
    joints."""
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(n, seed=seed)
    rng = np.random.default_rng(seed + 100)
    theta[0, 3] = 0.0
    if n > 2:
        theta[2, 1:] = 0.0
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    theta[n - 1, 7] = (np.pi * ax[n - 1]).astype(np.float32)
    if n > 3:
        theta[1, 2:5] = (np.pi * ax[1]).astype(np.float32)
    return beta, theta


def dense_grads(V, n, seed, kind):
    """tests/test_fk_vjp_gpu.py::_grads, restated: dense N(0,1) cotangents."""
    rng = np.random.default_rng(seed)
    gv = rng.standard_normal((n, V, 3)).astype(np.float32) if kind in ("verts", "both") else None
    gj = rng.standard_normal((n, 24, 3)).astype(np.float32) if kind in ("joints", "both") else None
    return gv, gj


def _V(which):
    return model(which)["vertices_template"].shape[0]


def dense_case(n, kind, which="synth", seed=None):
    """(a): a dense cotangent.  Every frame is checked, except at n = 1024 (BIG_FRAMES)."""
    seed = n if seed is None else seed
    beta, theta = dense_inputs(n, seed)
    gv, gj = dense_grads(_V(which), n, 7 * seed, kind)
    return dict(name="dense %s n=%d %s" % (which, n, kind), model=which, beta=beta, theta=theta, gv=gv, gj=gj,
                frames=list(range(n)) if n <= DENSE_N[-1] else list(BIG_FRAMES))


def generic_pose(seed=23):
    """One (beta, theta) with generic angles: N(0, 0.4^2) rad on every joint (no zero, none near pi), a translation."""
    rng = np.random.default_rng(seed)
    beta = rng.standard_normal((1, 10)).astype(np.float32)
    theta = (0.4 * rng.standard_normal((1, 25, 3))).astype(np.float32)
    theta[0, 0] = rng.uniform(-1, 1, 3)
    return beta, theta


def row_vertices(which):
    """(b): the vertices whose Jacobian rows are taken.  The group boundaries 0, 1, 31, 32, 33, V-11, V-10, V-1 of the 32-vertex
    groups; on the synthetic model also, for each of the 24 joints, the vertex with the largest weight on it, and on every model
    the 8 vertices with the most evenly mixed weights (the smallest largest weight).  Ascending, without repeats."""
    md = model(which)
    W = np.asarray(md["weights"], np.float64)
    V = W.shape[0]
    vs = [0, 1, 31, 32, 33, V - 11, V - 10, V - 1]
    if which == "synth":
        vs += [int(W[:, j].argmax()) for j in range(24)]
    vs += [int(v) for v in np.argsort(W.max(axis=1), kind="stable")[:8]]
    return sorted(set(vs))


def rows_case(which="synth"):
    """(b): the generic pose replicated over K frames; frame k's grad_verts is one-hot at (vertex, coordinate) k, so the outputs
    are rows of the Jacobian."""
    vs = row_vertices(which)
    K, V = 3 * len(vs), _V(which)
    beta, theta = generic_pose()
    gv = np.zeros((K, V, 3), np.float32)
    for k in range(K):
        gv[k, vs[k // 3], k % 3] = 1.0
    return dict(name="rows %s K=%d" % (which, K), model=which, beta=np.repeat(beta, K, 0), theta=np.repeat(theta, K, 0), gv=gv, gj=None,
                frames=list(range(K)), row_vertex=[vs[k // 3] for k in range(K)])


def faces_case():
    """(c): n = 3, a cotangent on the three corners of the 6 end-effector faces (tests/test_fk_vjp_gpu.py::
    test_vjp_pinned_to_reference_autograd's construction: a random 3-vector per face spread by barycentric weights)."""
    from smplpp_amd.ik import reference_task_faces

    md = model("synth")
    K = 6
    _, faces = reference_task_faces(K)
    F = np.asarray(md["face_indices"], np.int64) - 1
    rng = np.random.default_rng(3)
    beta, theta = dense_inputs(3, seed=11)
    gv = np.zeros((3, _V("synth"), 3), np.float64)
    for f in range(3):
        bary = rng.dirichlet(np.ones(3), size=K)
        u = rng.standard_normal((K, 3))
        for k in range(K):
            for c in range(3):
                gv[f, F[faces[k], c]] += u[k] * bary[k, c]
    return dict(name="faces n=3", model="synth", beta=beta, theta=theta, gv=gv.astype(np.float32), gj=None, frames=[0, 1, 2])


HAND_JOINT = 22


def hand_case():
    """(c): n = 3, a N(0,1) cotangent on the vertices whose largest weight is on one hand joint."""
    md = model("synth")
    W = np.asarray(md["weights"], np.float64)
    vs = np.nonzero(W.argmax(axis=1) == HAND_JOINT)[0]
    assert len(vs) > 0
    rng = np.random.default_rng(4)
    beta, theta = dense_inputs(3, seed=12)
    gv = np.zeros((3, W.shape[0], 3), np.float32)
    gv[:, vs] = rng.standard_normal((3, len(vs), 3))
    return dict(name="hand n=3 (%d vertices)" % len(vs), model="synth", beta=beta, theta=theta, gv=gv, gj=None, frames=[0, 1, 2])


SILENT_N = 64


def silent_frames():
    """(d): every odd frame and all of frames 40-47."""
    return sorted(set(range(1, SILENT_N, 2)) | set(range(40, 48)))


def silent_case():
    """(d): n = 64, `both`; grad_verts is zero on `silent_frames()` (grad_joints is not), inside 32-frame tiles of live frames.
    `gv_full` is the dense cotangent the zeros were cut from: the live frames must have the same bits under either."""
    c = dense_case(SILENT_N, "both", seed=77)
    c["gv_full"] = c["gv"].copy()
    c["gv"][silent_frames()] = 0.0
    c["name"] = "silent n=64"
    return c


def sparse_cases():
    return [faces_case(), hand_case()]


def live(case):
    """bool [n]: the frame has a vertex cotangent (only then can dL/dtheta, rot and trans be other than zero)."""
    n = len(case["beta"])
    return np.zeros(n, bool) if case["gv"] is None else np.abs(case["gv"]).reshape(n, -1).max(axis=1) > 0


def rot_of(case, general):
    """The rotation-matrix entry point's `rot` [n,24,3,3] fp32: the float64 Rodrigues matrices of theta rounded to fp32, or (general)
    those + 0.05 N(0,1) per entry (tests/test_fk_rotmat_gpu.py::_general: not orthonormal, inside form h's range)."""
    import fk_rotmat_oracle as RO

    R = RO.rodrigues_np(case["theta"][:, 1:])
    if general:
        R = R + 0.05 * np.random.default_rng(len(case["beta"]) + 7).standard_normal(R.shape)
    return R.astype(np.float32)


def _sub(a, frames):
    return None if a is None else a[frames]


def fk_reference(case, dtype="float64", rest=None):
    """(dL/dbeta, dL/dtheta) float64 arrays over case["frames"], by autograd of fk_vjp_oracle.fk in `dtype`.  `rest` [n,V,3]: the
    rest shape the skinning backward reads is this one instead of the graph's (the yardstick of a form whose recomputed rest is
    not an fp32 quantity)."""
    import fk_vjp_oracle as O

    fr = case["frames"]
    return O.vjp(O.model_tensors(model(case["model"])), case["beta"][fr], case["theta"][fr], _sub(case["gv"], fr), _sub(case["gj"], fr),
                 dtype=getattr(O.torch, dtype), rest=_sub(rest, fr))


def rotmat_reference(case, rot, dtype="float64"):
    """(dL/dbeta, dL/dtrans, dL/drot) float64 arrays over case["frames"], by autograd of fk_rotmat_oracle.fk in `dtype`."""
    import fk_rotmat_oracle as RO

    fr = case["frames"]
    return RO.vjp(RO.model_tensors(model(case["model"])), case["beta"][fr], case["theta"][fr, 0], rot[fr], _sub(case["gv"], fr),
                  _sub(case["gj"], fr), dtype=getattr(RO.torch, dtype))


FK_OUTPUTS = (("beta", None), ("theta", THETA))          # (name, block axes; None = each frame)
ROTMAT_OUTPUTS = (("beta", None), ("trans", None), ("rot", ROT))


def axes_of(block_axes, a):
    return frame_axes(a) if block_axes is None else block_axes


# ------------------------------------------------------------------------------------------------ VPoser cases
VV_NF = 8  # smplpp_amd/csrc/vposer_vjp.hip: frames per workgroup of vposer_vjp_kernel
VPOSER_DENSE_N = [1, VV_NF - 1, VV_NF, VV_NF + 1, 64, 257]
VPOSER_LATENTS = ["zero", "unit", "0.3"]


def vposer_rows_case(latent):
    """(f): one latent (z = 0, z ~ N(0,1) or z ~ N(0, 0.3^2)) replicated over 63 frames, frame k's cotangent one-hot at (joint,
    axis) k: the whole transposed Jacobian."""
    rng = np.random.default_rng(31 + VPOSER_LATENTS.index(latent))
    z = {"zero": 0.0, "unit": 1.0, "0.3": 0.3}[latent] * rng.standard_normal((1, 32))
    return dict(name="vposer rows z=%s" % latent, z=np.repeat(z.astype(np.float32), 63, 0), g=np.eye(63, dtype=np.float32).reshape(63, 21, 3),
                frames=list(range(63)))


def vposer_dense_case(n):
    """(f): tests/test_vposer_vjp_gpu.py::test_vjp_parity's inputs."""
    rng = np.random.default_rng(n)
    z = rng.normal(0, 1.0, (n, 32)).astype(np.float32)
    z[0] = 0.0
    return dict(name="vposer dense n=%d" % n, z=z, g=rng.standard_normal((n, 21, 3)).astype(np.float32), frames=list(range(n)))


def vposer_reference(params, case, dtype="float64"):
    """dL/dz [n,32] float64 by autograd of the decoder restatement in `dtype`."""
    import vposer_vjp_oracle as VO

    dt = getattr(VO.torch, dtype)
    return VO.vjp(VO.decoder(params, dt), case["z"], case["g"], dtype=dt)[0]
