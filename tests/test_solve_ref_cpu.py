"""tests/solve_ref.py on the CPU: the KKT judge, the reference step and the host-path restatement the GPU solve tests rely on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solve_ref as S  # noqa: E402


def _spd(rng, D, rows):
    J = rng.normal(0, 1, (rows, D))
    return J.T @ J + np.diag(rng.uniform(1e-2, 1.0, D))


@pytest.mark.parametrize("seed", range(6))
def test_kkt_residual_is_zero_at_the_box_qp_optimum_and_not_elsewhere(seed):
    from oracle import cpu

    rng = np.random.default_rng(seed)
    D = int(rng.integers(8, 60))
    A = _spd(rng, D, D // 2)
    b = rng.normal(0, 3, D)
    w = rng.uniform(0.05, 0.8, D)
    lo, hi = -w, w
    lo[: D // 4], hi[: D // 4] = -np.inf, np.inf  # unbounded like theta
    lo[-2:], hi[-2:] = 0.0, 0.0  # pinned like a phi with a zero limit
    x = cpu.box_qp(A, b, lo, hi)
    r = S.kkt_residual(A, b, lo, hi, x)
    bound = S.step_bound(A, (x > lo) & (x < hi), x)
    assert r["worst"] <= bound, (r, bound)
    assert ((x <= lo) | (x >= hi))[: -2].any()  # some bound is active: the sign test is exercised
    # a perturbation of the free part, of a bound coordinate into the box, and out of the box each show
    free = np.flatnonzero((x > lo) & (x < hi))
    y = x.copy()
    y[free[0]] += 1e-6
    assert S.kkt_residual(A, b, lo, hi, y)["grad"] > 1e3 * bound
    act = np.flatnonzero(((x <= lo) | (x >= hi)) & (lo < hi))
    y = x.copy()
    y[act[0]] = 0.5 * (lo[act[0]] + hi[act[0]]) if np.isfinite(lo[act[0]]) else 0.0
    assert S.kkt_residual(A, b, lo, hi, y)["worst"] > 1e3 * bound
    y = x.copy()
    y[act[0]] += 1e-6 * np.sign(x[act[0]])
    assert S.kkt_residual(A, b, lo, hi, y)["feas"] > 5e-7
    # a bound coordinate released to the wrong side: the multiplier's sign
    y = x.copy()
    k = act[0]
    y[k] = hi[k] if x[k] <= lo[k] else lo[k]
    assert S.kkt_residual(A, b, lo, hi, y)["worst"] > 1e3 * bound


@pytest.mark.parametrize("latent", [False, True])
def test_reference_step_without_bounds_is_the_linear_solve(latent):
    rng = np.random.default_rng(4)
    td, K, bd = (44, 7, 10) if latent else (75, 5, 10)
    D = td + 2 * K + bd
    J = rng.normal(0, 0.5, (4 * K, D))
    J[:, td + 2 * K - 2: td + 2 * K] = 0.0  # the last task's phi columns: its limit is 0 below, the engine zeroes them
    e = rng.normal(0, 0.05, 4 * K)
    prior = rng.normal(0, 0.3, td).astype(np.float32) if latent else None
    pl = np.full(K, 0.04)
    pl[-1] = 0.0
    r = S.reference_step(e, J, td, K, bd, pl, enable_qp=False, prior_theta=prior)
    A = J.T @ J + np.diag(np.r_[np.full(td, 1e-3), np.full(2 * K, 1e-1), np.full(bd, 1e-3)] + e @ e)
    b = J.T @ e
    if latent:
        w = np.r_[np.zeros(6), np.full(td - 12, 1e-5), np.full(6, 1e3)]
        A[:td, :td] += np.diag(w)
        b[:td] += w * prior.astype(np.float64)
    x = np.linalg.solve(A, -b)
    assert np.abs(r["x"] - x).max() <= S.step_bound(A, np.ones(D, bool), x)
    assert np.all(r["x"][td + 2 * K - 2: td + 2 * K] == 0.0) and r["pinned"].sum() == 2
    assert np.allclose(r["A"], A, rtol=1e-14, atol=1e-14) and np.allclose(r["b"], b, rtol=1e-14, atol=1e-14)
    q = S.reference_step(e, J, td, K, bd, pl, enable_qp=True, prior_theta=prior)  # the box of node.cpp:911-929
    assert np.all(q["lo"][td + 2 * K:] == -0.5) and np.all(q["hi"][: td] == np.inf)
    assert S.kkt_residual(q["A"], q["b"], q["lo"], q["hi"], q["x"])["worst"] <= S.step_bound(q["A"], q["free"], q["x"])


def test_phi_limits_are_taken_at_fp32():
    lo, hi, pinned = S.box(75, 2, 0, [0.04, 1e-4], True)
    assert hi[75] == float(np.float32(0.04)) and hi[77] == float(np.float32(1e-4)) and not pinned.any()
    lo, hi, pinned = S.box(75, 2, 10, [0.04, 0.04], True, phi_live=False)
    assert pinned[75:79].all() and np.all(hi[79:] == 0.5)


def test_solve_plan_matches_the_documented_shapes():
    # the capture fit's motion solve: 41 markers, phi pinned, beta fixed -> 75 + 1 unknown rows, two row chunks, LLT exit
    p = S.solve_plan(41, 75, 0, True)
    assert (p["kernel"], p["m_dim"], p["chunks"], p["qp"]) == ("ntr5", 75, 2, False)
    # the 48-marker body solve with beta: all-LDS primal in ~5-row chunks
    p = S.solve_plan(48, 75, 10, False)
    assert (p["kernel"], p["first_factor"], p["chunk_rows"], p["chunks"]) == ("ntr6", "lds", 5, 39)
    assert S.solve_plan(45, 75, 10, False)["kernel"] == "ntr11"  # m_dim + 1 == 176: the last register-tiled size
    assert S.solve_plan(6, 75, 10, False)["dual_chol"] == "reg24_24"
    assert S.solve_plan(6, 75, 10, False, primal_only=True)["first_factor"] == "reg"


def test_the_gpu_case_list_reaches_every_path():
    plans = {c["name"]: (c, S.case_plan(c)) for c in S.CASES}
    assert len(plans) == len(S.CASES)
    got = set()
    for c, p in plans.values():
        lay = c["layout"]
        got.add((lay, p["kernel"]))
        got.add((lay, "first", p["first_factor"]))
        if p["kernel"] == "dual":
            got.add((lay, "chol", p["dual_chol"]))
            got.add((lay, "dual", "qp" if p["qp"] else "llt"))
        if c["primal"]:
            got.add((lay, "primal_only", "qp" if p["qp"] else "llt", p["rows"]))
        if p["dual_to_primal"] and c["phi"] == "tiny":
            got.add((lay, "dual_to_primal"))
        if c["qp"] and not p["qp"]:
            got.add((lay, "llt_exit"))
        if c["phi"] == "locked" and c["beta"] and p["qp"]:
            got.add((lay, "box_on_beta_only"))
        got.add(("chunks", min(p["chunks"], 3)))
        if p["m_dim"] + 1 in (176, 172, 178, 180, 182):
            got.add(("size", p["m_dim"] + 1, p["kernel"], p["first_factor"]))
        for k in ("zero", "skip"):
            if c[k]:
                got.add((k, p["kernel"]))
        if c["phi"] == "tiny" and c["targets"] == "beta":
            got.add(("many_bounds", p["kernel"]))
    need = {("direct", "dual"), ("direct", "ntr5"), ("direct", "ntr6"), ("direct", "ntr11"), ("direct", "first", "lds"),
            ("latent", "ntr3"), ("latent", "ntr5"), ("latent", "ntr6"), ("latent", "ntr11"), ("latent", "dual"),
            ("latent", "dual_to_primal"), ("latent", "llt_exit"), ("direct", "llt_exit"), ("direct", "box_on_beta_only"),
            ("chunks", 1), ("chunks", 2), ("chunks", 3),
            ("size", 176, "ntr11", "reg"), ("size", 172, "ntr11", "reg"), ("size", 178, "ntr6", "lds"),
            ("size", 180, "ntr6", "lds"), ("size", 182, "ntr6", "lds"),
            ("zero", "dual"), ("zero", "ntr11"), ("zero", "ntr5"), ("skip", "dual"),
            ("many_bounds", "dual"), ("many_bounds", "ntr11")}
    for ch in ("reg8", "reg16", "reg24", "reg24_24", "reg32", "lds"):
        need.add(("direct", "chol", ch))
    for mode in ("qp", "llt"):
        need.add(("direct", "dual", mode))
        need.add(("latent", "dual", mode))
    for r in (8, 16, 20, 24, 32, 44, 60):  # every dual-form size above, also through the primal form
        need.add(("direct", "primal_only", "qp", r))
    need.add(("direct", "primal_only", "llt", 8))
    need.add(("direct", "primal_only", "llt", 60))
    assert not need - got, sorted(need - got)
    # the LDS dual Cholesky covers 32 < r <= 63 from both ends of the range the case list uses
    rs = {p["rows"] for _, p in plans.values() if p["dual_chol"] == "lds"}
    assert min(rs) <= 44 and max(rs) >= 60
    # the capture shape (K = 41) is one case
    assert any(c["K"] == 41 and p["kernel"] == "ntr5" for c, p in plans.values())
