"""The IK solve of one frame (node/node.cpp:883-943) in float64 on the CPU, and the host's choice of the solve kernel's path —
test infrastructure for tests/test_ik_solve_gpu.py.

`reference_step` builds the damped normal equations with the oracle's `normal_equations` (J^T J, |e|^2 and the per-block damping
on the diagonal, the latent prior) and the box of node.cpp:911-929, and solves them with the oracle's box QP or LLT.
`kkt_residual` judges any candidate step on its own (plain numpy, no active-set solver), `step_bound` is the agreement a
backward-stable fp64 solve of that system owes, and `solve_plan` restates the host side of smplpp_ik_iterate
(smplpp_amd/csrc/ik_plan.h) so that a case list can show which instantiation, dual-form factorisation and row chunking it reaches."""
import numpy as np

from oracle import cpu

EPS = 2.220446049250313e-16
NB = 10
TD75, TD44 = 75, 44
SOLVE_LDS_MAX = 160 * 1024 - 1536  # ik_plan.h: dynamic LDS of the solve kernels


def box(theta_dim, K, beta_dim, phi_limit, enable_qp, phi_live=True):
    """(lo, hi, pinned) of node.cpp:911-929 as ik_solve_kernel sets them: theta free; |phi| <= phiLimit_ under the QP (free in
    the LLT form); |d beta| <= 0.5 under the QP; phi pinned to 0 where its limit is not > 0 or phi is not live this iteration
    (its Jacobian columns are zero: the variable leaves the system in both forms).  phi_limit [K] is rounded to fp32 first, as
    the engine stores it."""
    D = theta_dim + 2 * K + beta_dim
    pl = np.asarray(phi_limit, np.float32).astype(np.float64).reshape(K) if phi_live else np.zeros(K)
    lo, hi = np.full(D, -np.inf), np.full(D, np.inf)
    pinned = np.zeros(D, bool)
    for k in range(K):
        s = slice(theta_dim + 2 * k, theta_dim + 2 * k + 2)
        if not pl[k] > 0.0:
            lo[s], hi[s], pinned[s] = 0.0, 0.0, True
        elif enable_qp:
            lo[s], hi[s] = -pl[k], pl[k]
    if enable_qp:
        lo[theta_dim + 2 * K:], hi[theta_dim + 2 * K:] = -0.5, 0.5
    return lo, hi, pinned


def reference_step(e, J, theta_dim, K, beta_dim, phi_limit, enable_qp, prior_theta=None, phi_live=True):
    """The step x [D] of one frame from its residual e [4K] and Jacobian J [4K, D] (D = theta_dim + 2K + beta_dim), with
    prior_theta [theta_dim] (fp32) in the latent layout.  Returns dict(x, A, b, lo, hi, pinned, free) — `free` are the
    coordinates strictly inside their box at x."""
    e = np.asarray(e, np.float64)
    J = np.asarray(J, np.float64)
    D = theta_dim + 2 * K + beta_dim
    assert J.shape == (4 * K, D) and e.shape == (4 * K,)
    A, b = cpu.normal_equations(e, J, theta_dim, 2 * K, beta_dim, vposer_theta=prior_theta)
    lo, hi, pinned = box(theta_dim, K, beta_dim, phi_limit, enable_qp, phi_live)
    x = np.zeros(D)
    live = ~pinned
    As, bs = A[np.ix_(live, live)], b[live]
    if enable_qp:
        x[live] = cpu.box_qp(As, bs, lo[live], hi[live])
    else:
        x[live] = cpu.llt_solve(As, bs)
    free = live & (x > lo) & (x < hi)
    return dict(x=x, A=A, b=b, lo=lo, hi=hi, pinned=pinned, free=free)


def kkt_residual(A, b, lo, hi, x):
    """Optimality of x for min 1/2 x'Ax + b'x over lo <= x <= hi (oracle_normal_equations' convention: x = -A^-1 b unbounded),
    in units of x.  g = A x + b.  feas: the largest box violation; grad: |A_FF^-1 g_F|_inf over the free coordinates F (those
    strictly inside the box: the Newton step that would still change them); sign: the largest multiplier of the wrong sign at a
    bound (at lo g must be >= 0, at hi <= 0), divided by A_ii.  Pinned coordinates (lo == hi) carry no condition but
    feasibility.  Returns dict(feas, grad, sign, worst)."""
    A, b, x = np.asarray(A, np.float64), np.asarray(b, np.float64), np.asarray(x, np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    g = A @ x + b
    feas = float(max(0.0, np.max(lo - x), np.max(x - hi)))
    pinned = lo >= hi
    at_lo = ~pinned & (x <= lo)
    at_hi = ~pinned & (x >= hi)
    free = ~pinned & ~at_lo & ~at_hi
    grad = 0.0
    if free.any():
        grad = float(np.abs(np.linalg.solve(A[np.ix_(free, free)], g[free])).max())
    d = np.diag(A)
    wrong = np.concatenate([np.maximum(0.0, -g[at_lo]) / d[at_lo], np.maximum(0.0, g[at_hi]) / d[at_hi], [0.0]])
    sign = float(wrong.max())
    return dict(feas=feas, grad=grad, sign=sign, worst=max(feas, grad, sign))


def step_bound(A, free_set, x):
    """max(1e-12, 1e3 eps cond(A_FF)) max(1, |x|_inf): how far two backward-stable fp64 solves of the same system may lie apart."""
    free_set = np.asarray(free_set, bool)
    c = np.linalg.cond(A[np.ix_(free_set, free_set)]) if free_set.any() else 1.0
    return max(1e-12, 1e3 * EPS * c) * max(1.0, float(np.abs(x).max()))


def _dual_chol(r):
    """The dual form's factorisation of the r x r system I + J G^-1 J' (solve_dual, ik_solve.h): by (r + 7) / 8."""
    w = (r + 7) >> 3
    if w == 1:
        return "reg8"
    if w == 2:
        return "reg16"
    if w == 3:
        return "reg24_24" if r == 24 else "reg24"
    if w == 4:
        return "reg32"
    return "lds"


def solve_plan(K, theta_dim, beta_dim, phi_locked, rows_live=None, enable_qp=True, phi_live=True, primal_only=False):
    """The host's choice for one iteration of smplpp_ik_iterate, restated independently of smplpp_amd/csrc/ik_plan.h
    (solve_plan there, whose SolvePlan fields are named on the left; tests/test_ik_plan_cpu.py holds the two together row by row):

      D, rows        D = theta_dim + 2K + beta_dim, rows = 4K
      m_dim          D - 2K when phi cannot move (not live this iteration, or every limit <= 0: ik_plan.h's phi_free is false)
      qp_k           enable_qp unless phi is pinned and beta fixed (the kernel's LLT exit)
      ntr            3 / 5 / 6 / 11 tiles by m_dim + 1 <= 48 / 80 / 96 (or > 176) / 176; 6 for a dual shape: rows < theta_dim,
                     rows <= 63, D <= 192, not SMPLPP_IK_DBG_STOP=9 (`primal_only`)
      chunk_rows     what is left of SOLVE_LDS_MAX beside the fixed part, in rows of J; fewer than 4 is refusal 1 (the first
                     assertion below)
      shmem          fixed + 8 chunk_rows D
      dual_only      a dual shape whose rows all fit; one whose rows do not is refusal 2 (the second assertion)

    plus what the kernel decides from it: `kernel` the instantiation (dual / ntr3 / ntr5 / ntr6 / ntr11), `first_factor` the
    factorisation of the first pass with every non-pinned unknown free (dual, reg (register tiles) or lds (the all-LDS primal):
    ik_solve.h:1182-1205), `dual_chol` its dual-form Cholesky (by rows = 4K: zero rows still count there), `dual_to_primal`
    whether a pass of the QP can leave the dual form for the primal one as bounds bind (a primal instantiation that starts in
    the dual form), and the host's row chunking `chunk_rows` / `chunks` of J through LDS.  `rows_live` (rows of J that can be
    non-zero) is carried for the case list; the host's choice does not depend on it."""
    D, rows = theta_dim + 2 * K + beta_dim, 4 * K
    phi_free = phi_live and not phi_locked
    m_dim = D - (0 if phi_free else 2 * K)
    qp_k = bool(enable_qp and not ((not phi_free) and beta_dim == 0))
    ntr_primal = 3 if m_dim + 1 <= 48 else 5 if m_dim + 1 <= 80 else (6 if (m_dim + 1 <= 96 or m_dim + 1 > 176) else 11)
    dual_shape = rows < theta_dim and rows <= 63 and D <= 192 and not primal_only
    ntr = 6 if dual_shape else ntr_primal
    fixed = 8 * ((m_dim + 1) * (m_dim + 2) // 2 + 7 * D + 2 * rows + 128 * ntr + 4) + 4 * 2 * D
    chunk_rows = min((SOLVE_LDS_MAX - fixed) // (8 * D), rows)
    assert chunk_rows >= 4
    dual_only = dual_shape and chunk_rows >= rows
    assert dual_only or not dual_shape
    nf0 = m_dim  # every unknown that can be free is free in the first pass
    dual0 = rows < nf0 and rows <= 63 and chunk_rows >= rows and nf0 <= 192 and (dual_only or not primal_only)
    if dual0:
        first = "dual"
    else:
        first = "reg" if nf0 + 1 <= 16 * ntr else "lds"
    return dict(D=D, rows=rows, rows_live=rows if rows_live is None else int(rows_live), m_dim=m_dim, qp=qp_k,
                kernel="dual" if dual_only else "ntr%d" % ntr, ntr=ntr, first_factor=first,
                dual_chol=_dual_chol(rows) if dual0 else None,
                dual_to_primal=bool(dual0 and not dual_only and qp_k), chunk_rows=int(chunk_rows),
                chunks=-(-rows // int(chunk_rows)))


def _case(name, layout, K, beta, qp, phi="live", n=4, primal=False, zero=False, normals=True, targets="near", skip=False):
    return dict(name=name, layout=layout, K=K, beta=beta, qp=qp, phi=phi, n=n, primal=primal, zero=zero, normals=normals,
                targets=targets, skip=skip)


# The case list of tests/test_ik_solve_gpu.py.  phi: "live" (phiLimit_ 0.04, the default), "tiny" (1e-4: most surface
# coordinates bind), "locked" (0 everywhere: the solver's phi_locked).  primal: SMPLPP_IK_DBG_STOP=9 at creation (every pass in
# the primal form).  zero: missing markers and position-only tasks, different per frame.  targets: "near" (a hidden pose a little
# away, a few cm of noise), "off5" (5 cm off the surface in random directions), "beta" (a hidden shape needing |d beta| > 0.5).
# skip: min_valid above the valid-marker count of some frames.
CASES = (
    [_case("dual_k%d_%s" % (K, "qp" if qp else "llt"), "direct", K, True, qp) for K in (2, 4, 5, 6, 8, 11, 15) for qp in (False, True)]
    + [_case("dual_k6_zero", "direct", 6, True, True, zero=True, n=6),
       _case("dual_k3_llt_nobeta", "direct", 3, False, False, n=2)]
    + [_case("primal_k%d_qp" % K, "direct", K, True, True, primal=True) for K in (2, 4, 5, 6, 8, 11, 15)]
    + [_case("primal_k%d_llt" % K, "direct", K, True, False, primal=True) for K in (2, 15)]
    + [_case("ntr5_capture_k41", "direct", 41, False, True, phi="locked", normals=False),
       _case("ntr5_k16_llt", "direct", 16, False, False, phi="locked"),
       _case("ntr6_k16_beta_box", "direct", 16, True, True, phi="locked", normals=False, targets="beta"),
       _case("ntr6_k32_beta_box", "direct", 32, True, True, phi="locked", n=3),
       _case("ntr11_k16", "direct", 16, False, True),
       _case("ntr11_k45_beta", "direct", 45, True, True, n=3),
       _case("ntr11_k48_nobeta", "direct", 48, False, True, n=3),
       _case("lds_k46_beta", "direct", 46, True, True, n=3),
       _case("lds_k47_beta", "direct", 47, True, True, n=3),
       _case("lds_k48_beta", "direct", 48, True, True, n=3),
       _case("lds_k48_beta_llt", "direct", 48, True, False, n=2),
       _case("bounds_dual_k10", "direct", 10, True, True, phi="tiny", normals=False, targets="beta"),
       _case("bounds_primal_k24", "direct", 24, True, True, phi="tiny", normals=False, targets="beta"),
       _case("zero_rows_primal_k24", "direct", 24, True, True, zero=True, n=6),
       _case("zero_rows_locked_k24", "direct", 24, False, False, phi="locked", zero=True, n=6),
       _case("skip_k8", "direct", 8, True, True, zero=True, skip=True, n=6)]
    + [_case("latent_ntr3_locked_k12", "latent", 12, False, True, phi="locked"),
       _case("latent_ntr5_locked_beta_k12", "latent", 12, True, True, phi="locked"),
       _case("latent_ntr5_k16", "latent", 16, False, True),
       _case("latent_ntr6_k20", "latent", 20, False, True),
       _case("latent_ntr11_k28", "latent", 28, False, True, n=3),
       _case("latent_dual_k6_qp", "latent", 6, True, True),
       _case("latent_dual_k6_llt", "latent", 6, True, False),
       _case("latent_dual_k10", "latent", 10, False, True, zero=True, n=6),
       _case("latent_dual_to_primal_k12", "latent", 12, False, True, phi="tiny", targets="off5"),
       _case("latent_dual_to_primal_k15", "latent", 15, False, True, phi="tiny", targets="off5")]
)


def case_plan(c):
    """solve_plan of a case of CASES."""
    td = TD44 if c["layout"] == "latent" else TD75
    return solve_plan(c["K"], td, NB if c["beta"] else 0, c["phi"] == "locked", enable_qp=c["qp"], primal_only=c["primal"])
