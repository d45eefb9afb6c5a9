"""ik_solve_kernel (smplpp_amd/csrc/ik_solve.h) against a float64 reference of the same solve, on every dispatch path.

The solve runs in fp64 on an (e, J) that smplpp_ik_eval reads back bit for bit, so its step is known to round-off: each case
evaluates twice from one state (bit for bit the same; each evaluation refreshes the vertex weights, so the state is put back
between them: see run_case), iterates once from that state (its |e|^2 must equal the evaluation's to 1e-14: the two are tied
together), and then per frame
  * the step (smplpp_ik_get_step) lies within step_bound = max(1e-12, 1e3 eps cond(A_FF)) max(1, |x|) of the reference step
    (tests/solve_ref.py: the oracle's normal equations, box QP / LLT), and every case's bound is below 1e-6;
  * the step is optimal on its own terms: its KKT residual (feasibility, free gradient, multiplier signs) is within that bound;
  * theta / beta after the update are fp32(before + fp32(x)) bit for bit, within 1 ulp of the same with the reference step, and
    in the latent layout the pass-through entries reach theta25 (the posed mesh equals a fresh solver's at that configuration);
  * status 0 (no numeric failure, bit 4 clear: every QP met its optimality test); skipped frames keep theta and beta.
The case list (solve_ref.CASES) reaches every instantiation, dual-form factorisation and row chunking the host and the kernel
choose between; tests/test_solve_ref_cpu.py proves that from solve_ref.solve_plan.

Margins, worst |x_engine - x_ref| / step_bound per path on the MI355X: see DESIGN.md §3.3 ("What the solve tests measure")."""
import os
import sys
import zlib
from math import fsum

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solve_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = {c["name"]: c for c in S.CASES}


def make_problem(c, oracle_model, ref_decoder):
    """Tasks and configuration of a case (host data only: the targets come from the CPU oracle's FK of a hidden pose, or 5 cm
    off the current surface), every frame different."""
    n, K, latent = c["n"], c["K"], c["layout"] == "latent"
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    faces = rng.integers(0, oracle_model.F, (n, K))
    beta = (0.5 * rng.standard_normal((n, 10))).astype(np.float32)
    if latent:
        from latent_oracle import splice, LATENT

        g = np.zeros((n, 44), np.float32)
        g[:, :3] = rng.normal(0, 0.05, (n, 3))
        g[:, 3:6] = rng.normal(0, 0.2, (n, 3))
        g[:, 6:38] = rng.normal(0, 0.5, (n, 32))
        g[:, 38:] = rng.normal(0, 0.2, (n, 6))
        gh = g + np.concatenate([rng.normal(0, 0.02, (n, 6)), rng.normal(0, 0.2, (n, 32)), rng.normal(0, 0.05, (n, 6))], 1).astype(np.float32)

        def th25(q):
            import torch

            with torch.no_grad():
                out = ref_decoder.forward(torch.from_numpy(np.ascontiguousarray(q[:, LATENT]))).numpy()
            return np.stack([splice(q[f], out[f].reshape(63)) for f in range(n)])

        theta, cur25, hid25 = g, th25(g), th25(gh)
    else:
        theta = np.zeros((n, 25, 3), np.float32)
        theta[:, 0] = rng.uniform(-0.5, 0.5, (n, 3))
        theta[:, 1:] = rng.normal(0, 0.25, (n, 24, 3))
        hid25 = theta + np.concatenate([rng.normal(0, 0.02, (n, 1, 3)), rng.normal(0, 0.08, (n, 24, 3))], 1).astype(np.float32)
        cur25 = theta
    bh = beta.copy()
    noise = 0.02
    if c["targets"] == "beta":  # the current pose in a shape |d beta| <= 0.5 cannot reach on several coordinates
        bh[:, :4] += rng.choice([-3.0, 3.0], (n, 4)).astype(np.float32)
        hid25, noise = cur25, 0.002
    fidx = oracle_model.m["face_indices"].astype(np.int64)[faces] - 1  # (1-based in the model)
    if c["targets"] == "off5":
        v = oracle_model.fk(beta, cur25, want=("verts",))["verts"]
        d = rng.normal(0, 1, (n, K, 3))
        off = 0.05 * d / np.linalg.norm(d, axis=2, keepdims=True)
    else:
        v = oracle_model.fk(bh, hid25, want=("verts",))["verts"]
        off = rng.normal(0, noise, (n, K, 3))
    tp = (np.stack([v[f][fidx[f]].mean(axis=1) for f in range(n)]) + off).astype(np.float32)
    pw = np.ones((n, K))
    nw = np.ones((n, K)) if c["normals"] else np.zeros((n, K))
    if c["zero"]:  # per frame: f % 3 missing markers, about half the tasks position-only
        for f in range(n):
            pw[f, rng.choice(K, f % 3, replace=False)] = 0.0
            nw[f] = rng.integers(0, 2, K)
    pl = np.full((n, K), {"live": 0.04, "tiny": 1e-4, "locked": 0.0}[c["phi"]])
    min_valid = K - 1 if c["skip"] else 0
    return dict(faces=faces, tp=tp, pw=pw, nw=nw, pl=pl, beta=beta, theta=theta, min_valid=min_valid)


def run_case(smpl, vposer, oracle_model, ref_decoder, c):
    """One case on the engine, every assertion of the module; returns the worst |x_engine - x_ref| / step_bound."""
    from smplpp_amd.ik import IkSolver

    n, K, latent, ob = c["n"], c["K"], c["layout"] == "latent", c["beta"]
    td, bd = (S.TD44 if latent else S.TD75), (S.NB if ob else 0)
    P = make_problem(c, oracle_model, ref_decoder)
    s = IkSolver(smpl, n, K, vposer=vposer if latent else None)
    s.setTasks(face_idx=P["faces"], target_pos=P["tp"], pos_task_weight=P["pw"], normal_task_weight=P["nw"], phi_limit=P["pl"])
    s.setConfig(P["beta"], P["theta"])
    # Each evaluation refreshes the tasks' vertex weights (calcVertexWeights at the current actual position, node.cpp:804), an
    # fp32 round trip that is not a fixed point (on the synthetic mesh the weights move by ~1e-5 per evaluation).  So the state is
    # put back before each evaluation: two evaluations of one state must agree bit for bit, and the iteration's own evaluation
    # then starts from that state too.
    w0 = s.getTasks()["vertex_weights"]
    e, J = s.eval(ob)
    s.setTasks(vertex_weights=w0)
    e_again, J_again = s.eval(ob)
    assert np.array_equal(e, e_again) and np.array_equal(J, J_again), "two evaluations of one state differ"
    s.setTasks(vertex_weights=w0)
    b0, t0 = s.getConfig()
    t0 = t0.reshape(n, td)
    e2 = s.iterate(1, enable_qp=c["qp"], optimize_beta_from=0 if ob else -1, min_valid=P["min_valid"])
    x = s.getStep()
    b1, t1 = s.getConfig()
    t1 = t1.reshape(n, td)
    st = s.getStatus()
    assert x.shape == (n, td + 2 * K + bd)
    assert not st.any(), st  # no numeric failure, and bit 4: every box QP met its optimality test
    skipped = (P["pw"] > 0).sum(axis=1) < P["min_valid"]
    assert skipped.any() == c["skip"]
    worst = 0.0
    for f in range(n):
        if skipped[f]:
            assert e2[f] == 0.0
            assert np.array_equal(t1[f], t0[f]) and np.array_equal(b1[f], b0[f]), f
            continue
        s2 = fsum((e[f] * e[f]).tolist())
        assert abs(e2[f] - s2) <= 1e-14 * s2, (f, e2[f], s2)
        r = S.reference_step(e[f], J[f], td, K, bd, P["pl"][f], c["qp"], prior_theta=t0[f] if latent else None)
        bound = S.step_bound(r["A"], r["free"], r["x"])
        assert bound < 1e-6, (f, bound)  # a case beyond this is ill-posed: redesign it
        dx = float(np.abs(x[f] - r["x"]).max())
        worst = max(worst, dx / bound)
        assert dx <= bound, (f, dx, bound)
        kkt = S.kkt_residual(r["A"], r["b"], r["lo"], r["hi"], x[f])
        assert kkt["worst"] <= bound, (f, kkt, bound)
        assert np.all(x[f][r["pinned"]] == 0.0)
        if c["name"].startswith("latent_dual_to_primal"):
            # enough surface coordinates bind for the free set to fall to the row count: the QP's passes end in the primal form
            nb = int((~r["free"] & ~r["pinned"]).sum())
            assert td + 2 * K + bd - nb <= 4 * K, (f, nb)
        # the update, node.cpp:945-968: fp32(theta + fp32(x)) bit for bit; within 1 ulp of the reference step's
        want = (t0[f] + x[f, :td].astype(np.float32)).astype(np.float32)
        assert np.array_equal(t1[f], want), f
        ref = (t0[f] + r["x"][:td].astype(np.float32)).astype(np.float32)
        assert np.all(np.abs(t1[f] - ref) <= np.spacing(np.maximum(np.abs(t1[f]), np.abs(ref)))), f
        if ob:
            assert np.array_equal(b1[f], (b0[f] + x[f, td + 2 * K:].astype(np.float32)).astype(np.float32)), f
        else:
            assert np.array_equal(b1[f], b0[f]), f
    if latent:  # the pass-through entries 0..5, 38..43 reached theta25: the posed mesh is a fresh solver's at (b1, t1)
        s.eval(False)
        v = s.getVertices()
        fresh = IkSolver(smpl, n, K, vposer=vposer)
        fresh.setTasks(face_idx=P["faces"])
        fresh.setConfig(b1, t1)
        fresh.eval(False)
        assert np.array_equal(v, fresh.getVertices())
    return worst


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


@pytest.fixture(scope="module")
def oracle_model(synth_model):
    from oracle import cpu

    return cpu.OracleModel(synth_model)


@pytest.mark.parametrize("name", list(CASES))
def test_ik_solve_step_vs_float64_reference(smpl, decoders, oracle_model, monkeypatch, name):
    c = CASES[name]
    for k in ("SMPLPP_IK_DBG_STOP", "SMPLPP_IK_OVERLAP", "SMPLPP_IK_EVENTS", "SMPLPP_IK_LATENT_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    if c["primal"]:
        monkeypatch.setenv("SMPLPP_IK_DBG_STOP", "9")  # read at solver creation: every pass in the primal form
    run_case(smpl, decoders[0], oracle_model, decoders[1], c)


def test_get_step_reports_its_width_and_bit_4_stays_clear_in_host_space(smpl):
    """getStep before any solve is None; D follows the last solve's beta dimension; a host-space iterate never fails on bit 4."""
    from smplpp_amd.ik import IkSolver

    K = 4
    s = IkSolver(smpl, 2, K)
    assert s.getStep() is None
    rng = np.random.default_rng(5)
    s.setTasks(face_idx=rng.integers(0, 13776, K), target_pos=rng.normal(0, 0.3, (2, K, 3)).astype(np.float32))
    s.iterate(1, enable_qp=True, optimize_beta_from=0)
    assert s.getStep().shape == (2, 75 + 2 * K + 10)
    s.iterate(1, enable_qp=True)
    assert s.getStep().shape == (2, 75 + 2 * K)
    assert not (s.getStatus() & 16).any()
