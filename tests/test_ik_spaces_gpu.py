"""Every entry point of the IK solver handle runs on one call frame (csrc/staging.h) and copies between the solver's device arrays
and the caller's with Frame::fetch / Frame::store.  Both memory spaces run the same kernels on the same inputs, only where the bytes
travel differs: solver A is driven in host space, solver B in device space (on torch's current stream), and everything that comes
back is compared bit for bit.  Shapes: n = 2 frames (a per-frame stride), K = 3 tasks (the x3, x6 and x4.D strides), the direct
(theta 75) and the latent (theta 44) layout (theta_dim, J / Jl), optimize_beta 0 and 1 for the evaluation (D)."""
import ctypes as C

import numpy as np
import pytest

import torch
pytestmark = pytest.mark.gpu

N, K = 2, 3
INVALID, STATE = 1, 4  # SMPLPP_ERR_INVALID, SMPLPP_ERR_STATE (include/smplpp_hip.h)
TASK_ARGS = ("face_idx", "vertex_weights", "target_pos", "target_normal", "pos_task_weight", "normal_task_weight", "phi_limit",
             "normal_offset")
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int64): torch.int64,
          np.dtype(np.int32): torch.int32}


def _lib():
    from smplpp_amd import _lib as L

    return L.load()


def _ok(rc):
    from smplpp_amd._lib import check

    check(rc)


class Space:
    """The caller's side of one memory space: where its arrays live, the stream it passes, how it reads a result."""

    def __init__(self, space):
        from smplpp_amd._lib import DEVICE
        from smplpp_amd.smpl import _stream

        self.space = space
        self.device = space == DEVICE
        self.stream = _stream() if self.device else None

    def put(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a).cuda() if self.device else a

    def empty(self, shape, dtype):
        """An output array, preset to what no call delivers (NaN, -1): a copy that stops short shows in _same."""
        fill = np.nan if np.dtype(dtype).kind == "f" else -1
        if self.device:
            return torch.full(shape, fill, dtype=_TORCH[np.dtype(dtype)], device="cuda")
        return np.full(shape, fill, dtype)

    def read(self, *arrays):
        if self.device:
            torch.cuda.synchronize()
        got = tuple(a.cpu().numpy() if torch.is_tensor(a) else a for a in arrays)
        return got[0] if len(got) == 1 else got


def _p(a):
    from smplpp_amd.smpl import _ptr

    return _ptr(a)


def set_config(sol, sp, beta, theta):
    b, t = sp.put(beta), sp.put(theta)
    _ok(_lib().smplpp_ik_set_config(sol._h, _p(b), _p(t), sp.space))
    sp.read()  # (the device copies b and t are read before they go)


def get_config(sol, sp):
    b, t = sp.empty((N, 10), np.float32), sp.empty((N, sol.theta_dim), np.float32)
    _ok(_lib().smplpp_ik_get_config(sol._h, _p(b), _p(t), sp.space))
    return sp.read(b, t)


def set_tasks(sol, sp, **tasks):
    args = [sp.put(tasks.get(k)) for k in TASK_ARGS]
    rc = _lib().smplpp_ik_set_tasks(sol._h, *[_p(a) for a in args], sp.space)
    sp.read()
    return rc


def get_tasks(sol, sp, inputs_only=False):
    """All five outputs; inputs_only: the faces and weights alone (the other three are the evaluation's: none before one)."""
    out = [sp.empty((N, K), np.int64), sp.empty((N, K, 3), np.float32), sp.empty((N, K, 3, 2), np.float32),
           sp.empty((N, K, 3), np.float32), sp.empty((N, K, 3), np.float32)]
    if inputs_only:
        out[2:] = [None, None, None]
    _ok(_lib().smplpp_ik_get_tasks(sol._h, *[_p(a) for a in out], sp.space))
    return sp.read(*out[:2]) if inputs_only else sp.read(*out)


def evaluate(sol, sp, optimize_beta, want_e=True, want_J=True):
    D = sol.theta_dim + 2 * K + (10 if optimize_beta else 0)
    e = sp.empty((N, 4 * K), np.float64) if want_e else None
    J = sp.empty((N, 4 * K, D), np.float64) if want_J else None
    _ok(_lib().smplpp_ik_eval(sol._h, optimize_beta, _p(e), _p(J), sp.space, sp.stream))
    return sp.read(e, J)


def iterate(sol, sp, iters, enable_qp):
    e2 = sp.empty((N,), np.float64)
    _ok(_lib().smplpp_ik_iterate(sol._h, iters, enable_qp, -1, 0, _p(e2), sp.space, sp.stream))
    return sp.read(e2)


def get_step(sol, sp):
    D = C.c_int64(-1)
    _ok(_lib().smplpp_ik_get_step(sol._h, None, C.byref(D), sp.space, sp.stream))  # x null: D alone
    x = sp.empty((N, D.value), np.float64)
    D2 = C.c_int64(-1)
    _ok(_lib().smplpp_ik_get_step(sol._h, _p(x), C.byref(D2), sp.space, sp.stream))
    assert D2.value == D.value
    return sp.read(x), D.value


def get_status(sol, sp):
    f = sp.empty((N,), np.int32)
    _ok(_lib().smplpp_ik_get_status(sol._h, _p(f), sp.space, sp.stream))
    return sp.read(f)


def get_vertices(sol, sp):
    v = sp.empty((N, sol.smpl.vertex_num, 3), np.float32)
    _ok(_lib().smplpp_ik_get_vertices(sol._h, _p(v), sp.space, sp.stream))
    return sp.read(v)


def _same(readings, what):
    """Every reading (an array or a tuple of arrays) equals the first, bit for bit, and was written to its end."""
    first = readings[0] if isinstance(readings[0], tuple) else (readings[0],)
    for a in first:
        assert np.isfinite(a).all() if a.dtype.kind == "f" else (a >= 0).all(), what
    for r in readings[1:]:
        r = r if isinstance(r, tuple) else (r,)
        assert len(r) == len(first), what
        for i, (a, b) in enumerate(zip(first, r)):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (what, i)
    return readings[0]


@pytest.fixture(scope="module")
def smpl(synth_model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    return s


@pytest.fixture(scope="module")
def vposer():
    from smplpp_amd.ik import VPoserDecoder

    return VPoserDecoder(VPoserDecoder.synthetic_params())


@pytest.fixture(scope="module")
def spaces():
    from smplpp_amd._lib import DEVICE, HOST

    return Space(HOST), Space(DEVICE)


def _inputs(theta_dim, seed):
    """A configuration and all eight task arrays, every frame and task with values of its own."""
    from smplpp_amd.ik import reference_task_faces

    rng = np.random.default_rng(seed)
    beta = rng.normal(0, 0.5, (N, 10)).astype(np.float32)
    theta = rng.normal(0, 0.05, (N, theta_dim)).astype(np.float32)
    faces = np.stack([reference_task_faces(K)[1], reference_task_faces(K)[1][::-1]]).astype(np.int64)
    vw = rng.uniform(0.1, 1.0, (N, K, 3)).astype(np.float32)
    vw /= vw.sum(-1, keepdims=True)
    tn = rng.normal(0, 1, (N, K, 3)).astype(np.float32)
    tn /= np.linalg.norm(tn, axis=-1, keepdims=True)
    tasks = dict(face_idx=faces, vertex_weights=vw, target_pos=rng.normal(0, 0.3, (N, K, 3)).astype(np.float32), target_normal=tn,
                 pos_task_weight=rng.uniform(0.5, 1.5, (N, K)), normal_task_weight=rng.uniform(0.1, 0.5, (N, K)),
                 phi_limit=rng.uniform(0.02, 0.06, (N, K)), normal_offset=rng.uniform(0.0, 0.02, (N, K)))
    return beta, theta, tasks


def _pair(smpl, vposer, layout, spaces, seed=51, **override):
    """Solver A set up in host space, solver B in device space, from the same inputs."""
    from smplpp_amd.ik import IkSolver

    vp = vposer if layout == "latent" else None
    A, B = IkSolver(smpl, N, K, vposer=vp), IkSolver(smpl, N, K, vposer=vp)
    assert A.theta_dim == (44 if vp else 75)
    beta, theta, tasks = _inputs(A.theta_dim, seed)
    tasks.update(override)
    for sol, sp in zip((A, B), spaces):
        set_config(sol, sp, beta, theta)
        _ok(set_tasks(sol, sp, **tasks))
    return A, B, beta, theta, tasks


LAYOUTS = ("direct", "latent")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_round_trips(smpl, vposer, spaces, layout):
    A, B, beta, theta, tasks = _pair(smpl, vposer, layout, spaces)
    both = [(sol, sp) for sol in (A, B) for sp in spaces]
    face, vw = _same([get_tasks(sol, sp, inputs_only=True) for sol, sp in both], "get_tasks (faces and weights as set)")
    assert np.array_equal(face, tasks["face_idx"]) and np.array_equal(vw, tasks["vertex_weights"])
    # the tangents, actual positions and normals are the evaluation's, which also restates the weights at the point it
    # differentiates at (ik_eval_kernel: calcVertexWeights with phi = 0): from here on the weights are compared between readings only
    for sol, sp in zip((A, B), spaces):
        evaluate(sol, sp, 0, want_e=False, want_J=False)
    b, t = _same([get_config(sol, sp) for sol, sp in both], "get_config")
    assert np.array_equal(b, beta) and np.array_equal(t, theta)
    face, vw, tang, apos, anrm = _same([get_tasks(sol, sp) for sol, sp in both], "get_tasks")
    assert np.array_equal(face, tasks["face_idx"])
    for a in (tang, apos, anrm):
        assert np.abs(a[1]).max() > 0


@pytest.mark.parametrize("optimize_beta", (0, 1))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_evaluation(smpl, vposer, spaces, layout, optimize_beta):
    A, B, _, _, tasks = _pair(smpl, vposer, layout, spaces)
    host, dev = spaces
    e, J = _same([evaluate(A, host, optimize_beta), evaluate(B, dev, optimize_beta)], "eval")
    assert J.shape[-1] == A.theta_dim + 2 * K + 10 * optimize_beta
    assert np.abs(e[1]).max() > 0 and np.abs(J[1]).max() > 0
    _same([get_vertices(sol, sp) for sol in (A, B) for sp in spaces], "get_vertices")
    # an output left out: the call succeeds and fills the other.  (An evaluation restates the weights at the point it
    # differentiates at: each of these starts from the weights the first one started from, and so repeats it.)
    for want_e in (False, True):
        got = []
        for sol, sp in zip((A, B), spaces):
            _ok(set_tasks(sol, sp, vertex_weights=tasks["vertex_weights"]))
            e1, J1 = evaluate(sol, sp, optimize_beta, want_e=want_e, want_J=not want_e)
            assert (e1 is None) == (not want_e) and (J1 is None) == want_e
            got.append(e1 if want_e else J1)
        assert np.array_equal(_same(got, "eval with an output left out"), e if want_e else J)


@pytest.mark.parametrize("enable_qp", (0, 1))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_iteration(smpl, vposer, spaces, layout, enable_qp):
    A, B, _, theta, _ = _pair(smpl, vposer, layout, spaces)
    host, dev = spaces
    e2 = _same([iterate(A, host, 3, enable_qp), iterate(B, dev, 3, enable_qp)], "e_sqnorm")
    assert np.isfinite(e2).all() and (e2 > 0).all()
    _, t = _same([get_config(A, host), get_config(B, dev)], "get_config")
    assert not np.array_equal(t, theta)
    (x, D) = get_step(A, host)
    (xb, Db) = get_step(B, dev)
    assert D == Db == A.theta_dim + 2 * K and x.shape == (N, D) and np.array_equal(x, xb) and np.abs(x).max() > 0
    status = _same([get_status(sol, sp) for sol in (A, B) for sp in spaces], "get_status")
    assert (status & 1 == 0).all()
    _same([get_vertices(A, host), get_vertices(B, dev)], "get_vertices")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_partial_setters(smpl, vposer, spaces, layout):
    """phi_limit alone, all zeros, locks phi (the one read-back of smplpp_ik_set_tasks, behind its one synchronisation)."""
    host, dev = spaces
    A, B, _, _, tasks = _pair(smpl, vposer, layout, spaces)
    full, _, _, _, _ = _pair(smpl, vposer, layout, spaces, phi_limit=np.zeros((N, K)))  # the same limits with all the other arrays
    steps = []
    for sol, sp in ((A, host), (B, dev), (full, host)):
        if sol is not full:
            _ok(set_tasks(sol, sp, phi_limit=np.zeros((N, K))))
        iterate(sol, sp, 1, 0)
        steps.append(get_step(sol, sp)[0])
    x = _same(steps, "step behind a phi_limit given alone")
    td = A.theta_dim
    assert x.shape == (N, td + 2 * K) and not x[:, td:].any() and np.abs(x[:, :td]).max() > 0
    # target_pos alone: the faces and weights stay
    before = get_tasks(full, host)
    _ok(set_tasks(full, host, target_pos=tasks["target_pos"] + np.float32(0.125)))
    after = get_tasks(full, host)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    e_moved, _ = evaluate(full, host, 0)
    _ok(set_tasks(full, host, target_pos=tasks["target_pos"]))
    e_back, _ = evaluate(full, host, 0)
    assert not np.array_equal(e_moved, e_back)  # (and the targets did change)


def test_refusals_keep_their_codes(smpl, synth_model, spaces):
    from smplpp_amd.ik import IkSolver

    host, _ = spaces
    L = _lib()
    sol = IkSolver(smpl, N, K)
    beta, theta, tasks = _inputs(75, 52)
    set_config(sol, host, beta, theta)
    _ok(set_tasks(sol, host, **tasks))
    v = np.empty((N, smpl.vertex_num, 3), np.float32)
    assert L.smplpp_ik_get_vertices(sol._h, _p(v), host.space, None) == STATE  # before any evaluation
    e_want, J_want = evaluate(sol, host, 0)
    assert np.isfinite(get_vertices(sol, host)).all()

    b, t, D = np.empty((N, 10), np.float32), np.empty((N, 75), np.float32), C.c_int64(0)
    face, vw = np.empty((N, K), np.int64), np.empty((N, K, 3), np.float32)
    e, J = np.empty((N, 4 * K), np.float64), np.empty((N, 4 * K, 75 + 2 * K), np.float64)
    e2, x, flags = np.empty(N, np.float64), np.empty((N, 75 + 2 * K), np.float64), np.empty(N, np.int32)
    targs = [np.ascontiguousarray(tasks[k]) for k in TASK_ARGS]
    # (iterate behind the getters: it moves the configuration their results are checked against)
    calls = [("set_config", lambda sp: L.smplpp_ik_set_config(sol._h, _p(beta), _p(theta), sp)),
             ("get_config", lambda sp: L.smplpp_ik_get_config(sol._h, _p(b), _p(t), sp)),
             ("set_tasks", lambda sp: L.smplpp_ik_set_tasks(sol._h, *[_p(a) for a in targs], sp)),
             ("get_tasks", lambda sp: L.smplpp_ik_get_tasks(sol._h, _p(face), _p(vw), None, None, None, sp)),
             ("eval", lambda sp: L.smplpp_ik_eval(sol._h, 0, _p(e), _p(J), sp, None)),
             ("get_vertices", lambda sp: L.smplpp_ik_get_vertices(sol._h, _p(v), sp, None)),
             ("get_status", lambda sp: L.smplpp_ik_get_status(sol._h, _p(flags), sp, None)),
             ("iterate", lambda sp: L.smplpp_ik_iterate(sol._h, 1, 0, -1, 0, _p(e2), sp, None)),
             ("get_step", lambda sp: L.smplpp_ik_get_step(sol._h, _p(x), C.byref(D), sp, None))]
    for name, call in calls:
        for bad in (2, -1):
            assert call(bad) == INVALID, name
            assert b"bad memory space" in L.smplpp_last_error(), name
        _ok(call(host.space))  # a valid call right behind the refusal
    assert np.array_equal(e, e_want) and np.array_equal(J, J_want) and np.array_equal(face, tasks["face_idx"])
    assert np.array_equal(b, beta) and np.array_equal(t, theta) and np.array_equal(vw, tasks["vertex_weights"])
    assert D.value == 75 + 2 * K and np.isfinite(x).all() and np.isfinite(e2).all()

    bad = tasks["face_idx"].copy()
    bad[1, 2] = len(synth_model["face_indices"])  # = F, the first id past the mesh
    assert set_tasks(sol, host, face_idx=bad) == INVALID
    assert b"face index out of range" in L.smplpp_last_error()
    _ok(set_tasks(sol, host, face_idx=tasks["face_idx"]))
    assert np.array_equal(get_tasks(sol, host)[0], tasks["face_idx"])
