"""The IK solver's exact-arithmetic mode (smplpp_ik_set_arithmetic EXACT) on the MI355X: the latent rows are the direct rows pulled
back through the exact decoder Jacobian, the loops' mesh is SMPL.launch's, no fp16x2 range limit, steps against the CPU oracle in
the direct and latent layouts (configs[4] at full size), chain and shard invariance, and mode switches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import latent_oracle as LO  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def smpl(synth_model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    return s


@pytest.fixture(scope="module")
def decoders():
    from oracle import vposer_torch as VT
    from smplpp_amd.ik import VPoserDecoder

    params = VPoserDecoder.synthetic_params()
    return VPoserDecoder(params), VT.VPoserDecoder(params)


def _latent_problem(n, K, seed):
    from smplpp_amd.ik import reference_task_faces

    _, faces = reference_task_faces(K)
    rng = np.random.default_rng(seed)
    g = np.zeros((n, 44), np.float32)
    g[:, :3] = rng.normal(0, 0.05, (n, 3))
    g[:, 3:6] = rng.normal(0, 0.2, (n, 3))
    g[:, 6:38] = rng.normal(0, 0.8, (n, 32))
    g[:, 38:] = rng.normal(0, 0.2, (n, 6))
    tp = rng.normal(0, 0.4, (n, K, 3)).astype(np.float32)
    return faces, g, tp


def _theta25(gpu, g):
    out = gpu.forward(g[:, 6:38])
    return np.stack([LO.splice(g[f], out[f]) for f in range(g.shape[0])])


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30)


def test_latent_eval_rows_are_the_direct_rows_through_the_exact_jacobian(smpl, decoders):
    from smplpp_amd.ik import IkSolver

    gpu, _ = decoders
    n, K = 16, 6
    faces, g, tp = _latent_problem(n, K, 1)
    th25 = _theta25(gpu, g)
    jz = gpu.jacobian(g[:, 6:38]).astype(np.float64)
    direct = IkSolver(smpl, n, K, exact=True)
    direct.setTasks(face_idx=faces, target_pos=tp)
    direct.setConfig(np.zeros((n, 10), np.float32), th25)
    e75, J75 = direct.eval()
    errs = {}
    for exact in (True, False):
        lat = IkSolver(smpl, n, K, vposer=gpu, exact=exact)
        lat.setTasks(face_idx=faces, target_pos=tp)
        lat.setConfig(np.zeros((n, 10), np.float32), g)
        e, J = lat.eval()
        errs[exact] = max(_rel(J[f][:, 6:38], J75[f][:, 6:69] @ jz[f]) for f in range(n))
        if exact:
            assert np.array_equal(e, e75)
            assert np.array_equal(J[:, :, :6], J75[:, :, :6]) and np.array_equal(J[:, :, 38:44], J75[:, :, 69:75])
    print("latent rows against J75 . jacobian(z): exact %.3g, default %.3g" % (errs[True], errs[False]))
    assert errs[True] <= 1e-5


def test_vertices_are_smpl_launch(smpl, decoders):
    from smplpp_amd.ik import IkSolver

    gpu, _ = decoders
    n, K = 12, 6
    faces, g, tp = _latent_problem(n, K, 2)
    rng = np.random.default_rng(2)
    beta = (rng.standard_normal((n, 10)) * 0.5).astype(np.float32)
    th25 = _theta25(gpu, g)
    for vposer, theta, th in ((None, th25, th25), (gpu, g, th25)):
        s = IkSolver(smpl, n, K, vposer=vposer, exact=True)
        s.setTasks(face_idx=faces, target_pos=tp)
        s.setConfig(beta, theta)
        s.eval()
        assert np.array_equal(s.getVertices(), smpl.launch(beta, th)["verts"]), vposer is None


def test_large_beta_keeps_range_and_status(smpl):
    from smplpp_amd.ik import IkSolver, reference_task_faces

    n, K = 4, 6
    _, faces = reference_task_faces(K)
    rng = np.random.default_rng(3)
    beta = rng.standard_normal((n, 10)).astype(np.float32)
    beta *= np.float32(2000.0) / np.linalg.norm(beta, axis=1, keepdims=True)
    theta = np.zeros((n, 25, 3), np.float32)
    theta[:, 1:] = rng.normal(0, 0.1, (n, 24, 3))
    s = IkSolver(smpl, n, K, exact=True)
    s.setTasks(face_idx=faces, target_pos=rng.normal(0, 0.4, (n, K, 3)).astype(np.float32))
    s.setConfig(beta, theta)
    s.eval()
    v = s.getVertices()
    assert np.isfinite(v).all()
    assert np.array_equal(v, smpl.launch(beta, theta)["verts"])
    assert (s.getStatus() & 8).sum() == 0


def test_direct_steps_on_ik_traj50(smpl):
    """One exact-mode iteration from each of the reference trajectory's 50 states lands within 1e-4 rad of its next state."""
    from smplpp_amd.ik import IkSolver

    g = np.load(os.path.join(GOLDEN, "ik_traj50.npz"))
    K = len(g["face_idx"])
    traj = g["traj_theta"]
    worst = {}
    for exact in (True, False):
        s = IkSolver(smpl, 50, K, exact=exact)
        s.setTasks(face_idx=g["traj_faces"][:50], vertex_weights=g["traj_weights"][:50], target_pos=g["target_pos"],
                   target_normal=g["target_normal"], phi_limit=np.zeros(K))
        s.setConfig(np.zeros((50, 10), np.float32), traj[:50])
        s.iterate(1)
        _, theta = s.getConfig()
        worst[exact] = float(np.abs(theta - traj[1:51]).max())
        if exact:
            assert (s.getTasks()["face_idx"] == g["traj_faces"][1:51]).all()
    print("ik_traj50 worst step error: exact %.3g rad, default %.3g rad" % (worst[True], worst[False]))
    assert worst[True] < 1e-4


def test_latent_steps_against_the_oracle(smpl, decoders, oracle_synth):
    """From identical state, one exact-mode step in the latent layout (box QP, prior, moving surface coordinates) and one body-stage
    step (beta optimised) against tests/latent_oracle.latent_step: the new configuration within 1e-4 (compare_states)."""
    from oracle import cpu
    from smplpp_amd.ik import IkSolver

    gpu, ref = decoders
    n, K = 4, 6
    faces, g, tp = _latent_problem(n, K, 5)
    worst = {}
    for exact in (True, False):
        for optimize_beta in (False, True):
            s = IkSolver(smpl, n, K, vposer=gpu, exact=exact)
            s.setTasks(face_idx=faces, target_pos=tp, normal_task_weight=np.zeros(K), normal_offset=np.full(K, 0.015))
            s.setConfig(np.zeros((n, 10), np.float32), g)
            s.eval(optimize_beta=optimize_beta)  # tangents and weights of the start state
            t = s.getTasks()
            s.iterate(1, enable_qp=True, optimize_beta_from=0 if optimize_beta else -1)
            beta_after, g_after = s.getConfig()
            for f in range(n):
                ts = cpu.TaskSet(t["face_idx"][f], tp[f], normal_task_weight=np.zeros(K), normal_offset=np.full(K, 0.015),
                                 vertex_weights=t["vertex_weights"][f])
                r = LO.latent_step(oracle_synth, ref, np.zeros(10), g[f], ts, enable_qp=True, optimize_beta=optimize_beta, project=False)
                d = LO.compare_states(ref, g_after[f], r["g44"])
                d = max(d + (float(np.abs(beta_after[f] - r["beta"]).max()),))
                worst[(exact, optimize_beta)] = max(worst.get((exact, optimize_beta), 0.0), d)
    print("latent steps against the oracle (motion, body): exact %.3g %.3g, default %.3g %.3g"
          % (worst[(True, False)], worst[(True, True)], worst[(False, False)], worst[(False, True)]))
    assert worst[(True, False)] < 1e-4 and worst[(True, True)] < 1e-4


def test_config4_size_exact(decoders, synth_model, oracle_synth):
    """configs[4] at its stated size in exact mode: 512 latent frames x 6 position targets x 50 iterations; sampled frames and the
    worst ones are re-synchronised with the CPU oracle at iterations 1 and 50 (within 1e-4), and the residual falls on > 90 %."""
    from oracle import cpu
    from smplpp_amd.ik import IkSolver, reference_task_faces
    from smplpp_amd.smpl import SMPL

    gpu, ref = decoders
    n, K, iters = 512, 6, 50
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    _, faces = reference_task_faces(K)
    rng = np.random.default_rng(300)
    hid = np.zeros((n, 25, 3), np.float32)
    hid[:, 1:22] = rng.normal(0, 0.15, (n, 21, 3))
    hv = s.launch(np.zeros((n, 10), np.float32), hid, want=("verts",))["verts"]
    tp = hv[:, synth_model["face_indices"][faces] - 1].mean(axis=2)
    sol = IkSolver(s, n, K, vposer=gpu, exact=True)
    sol.setTasks(face_idx=faces, target_pos=tp, phi_limit=np.zeros(K), normal_task_weight=np.zeros(K))
    sol.setConfig(np.zeros((n, 10), np.float32), np.zeros((n, 44), np.float32))
    worst = 0.0
    done = 0
    for target in (1, iters):
        if target - 1 > done:
            sol.iterate(target - 1 - done)
            done = target - 1
        _, g_before = sol.getConfig()
        t_before = sol.getTasks()
        e2 = sol.iterate(1)
        done += 1
        if target == 1:
            e2_first = e2.copy()
        _, g_after = sol.getConfig()
        for f in [0, 91, 300, 511] + [int(f) for f in np.argsort(-e2)[:3]]:
            ts = cpu.TaskSet(t_before["face_idx"][f], tp[f], phi_limit=np.zeros(K), normal_task_weight=np.zeros(K),
                             vertex_weights=t_before["vertex_weights"][f])
            r = LO.latent_step(oracle_synth, ref, np.zeros(10), g_before[f], ts, enable_qp=False, project=False)
            d = max(LO.compare_states(ref, g_after[f], r["g44"]))
            worst = max(worst, d)
            assert d < 1e-4, (target, f, d)
    print("configs[4] exact: worst step error %.3g" % worst)
    assert np.isfinite(e2).all() and (e2 < e2_first).mean() > 0.9


def test_exact_bits_do_not_depend_on_the_chains_beside(smpl, decoders):
    """A chain's trajectory is the same whether it runs among 8 chains or alone at its global index (frame_base); the device frame
    loop (solveSequence) gives the bits of the host-driven loop (iterate per frame)."""
    from smplpp_amd.ik import IkSolver

    gpu, _ = decoders
    n, K = 8, 6
    faces, g, tp = _latent_problem(n, K, 7)
    big = IkSolver(smpl, n, K, vposer=gpu, exact=True)
    big.setTasks(face_idx=faces, target_pos=tp)
    big.setConfig(np.zeros((n, 10), np.float32), g)
    big.iterate(4, enable_qp=True)
    _, gb = big.getConfig()
    for f in (0, 5):
        one = IkSolver(smpl, 1, K, vposer=gpu, frame_base=f, exact=True)
        one.setTasks(face_idx=faces, target_pos=tp[f:f + 1])
        one.setConfig(np.zeros((1, 10), np.float32), g[f:f + 1])
        one.iterate(4, enable_qp=True)
        assert np.array_equal(one.getConfig()[1], gb[f:f + 1]), f
    # the device frame loop (smplpp_ik_solve_sequence) against the host-driven loop, through MocapMotionSolver(exact=True)
    from smplpp_amd import mocap

    T, R = 6, 2
    markers = (tp[:1, None] + np.random.default_rng(8).normal(0, 0.01, (R, T, K, 3))).astype(np.float32)
    valid = np.ones((R, T, K), bool)
    valid[0, 2, :2] = False
    out = []
    for host_loop in (True, False):
        ms = mocap.MocapMotionSolver(smpl, faces, np.full((K, 3), 1 / 3, np.float32), restarts=R, vposer=gpu, exact=True)
        th, _ = ms.solve(markers, valid, np.zeros(10, np.float32), g[:R].copy(), host_loop=host_loop)
        out.append(th)
    assert np.isfinite(out[0]).all() and np.array_equal(out[0], out[1])


def test_mode_switch_and_refusals(smpl, decoders, synth_model):
    from smplpp_amd import _lib
    from smplpp_amd.ik import IkSolver

    gpu, _ = decoders
    n, K = 8, 6  # (n <= 128: the default mode's side-stream decoder schedule is on)
    faces, g, tp = _latent_problem(n, K, 9)
    beta = np.zeros((n, 10), np.float32)

    def run(s):
        s.setTasks(face_idx=faces, vertex_weights=np.full((n, K, 3), 1 / 3, np.float32), target_pos=tp)
        s.setConfig(beta, g)
        s.iterate(6, enable_qp=True)
        return s.getConfig()[1]

    fresh = run(IkSolver(smpl, n, K, vposer=gpu))
    sw = IkSolver(smpl, n, K, vposer=gpu, exact=True)
    ex = run(sw)
    sw.setExactArithmetic(False)
    assert np.array_equal(run(sw), fresh)
    assert not np.array_equal(ex, fresh)
    assert _lib.load().smplpp_ik_set_arithmetic(sw._h, 2) == 1
    assert _lib.load().smplpp_ik_set_arithmetic(sw._h, -1) == 1
    assert _lib.load().smplpp_ik_set_arithmetic(None, 1) == 1
    assert np.array_equal(run(sw), fresh)  # (a refused switch leaves the mode as it was)
    # a model created with SMPLPP_SKIN=h has no exact forward form
    from smplpp_amd.smpl import SMPL

    old = os.environ.get("SMPLPP_SKIN")
    os.environ["SMPLPP_SKIN"] = "h"
    try:
        sh = SMPL()
        sh.setDevice("cuda:0")
        sh.init(synth_model)
    finally:
        if old is None:
            del os.environ["SMPLPP_SKIN"]
        else:
            os.environ["SMPLPP_SKIN"] = old
    s = IkSolver(sh, 2, K)
    with pytest.raises(_lib.SmplppError):
        s.setExactArithmetic(True)
    s.setExactArithmetic(False)
