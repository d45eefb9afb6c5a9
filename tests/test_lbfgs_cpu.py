"""The batched L-BFGS without a GPU.  (1) The entry points are declared, exported and bound, and a call without a device fails loudly.
(2) The host decisions of smplpp_amd/csrc/lbfgs_plan.h as a stand-alone program, tests/cpp/lbfgs_plan_dump.cpp, built with the address
and undefined-behaviour sanitizers: its ring arithmetic, plans and refusals equal a Python restatement over a sweep of (n, D, m).
(3) The float32 restatement of the rule (tests/lbfgs_oracle.py), the one the GPU tests hold the library to bit for bit, behaves as an
L-BFGS: it converges on quadratics and on Rosenbrock in about the evaluations of the float64 run, keeps the frames of a mixed batch
independent, and ends with the statuses the rule names."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_oracle as LO  # noqa: E402
from distance_cases import _same_bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"smplpp_lbfgs_create": 10, "smplpp_lbfgs_destroy": 1, "smplpp_lbfgs_info": 4, "smplpp_lbfgs_reset": 2, "smplpp_lbfgs_step": 8,
         "smplpp_lbfgs_state": 9, "smplpp_lbfgs_best": 6}


# ---------------------------------------------------------------------------------------------------- 1. the ABI
def test_entry_points_are_declared_exported_and_bound():
    import __graft_entry__ as g

    g.build()
    from smplpp_amd import _lib

    L = _lib.load()
    declared = _lib.declared_symbols()
    for name, nargs in NAMES.items():
        assert name in declared and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == nargs, name


def test_a_call_without_a_device_fails_loudly():
    from smplpp_amd import _lib
    from smplpp_amd.optim import BatchedLBFGS

    x = np.zeros((3, 5), np.float32)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.SmplppError):
            BatchedLBFGS(x)
    for bad in (dict(history=0), dict(history=33), dict(c1=0.0), dict(c1=float("nan")), dict(tol_grad=-1.0), dict(tol_f=float("inf")),
                dict(max_ls=0), dict(curv_eps=1.0), dict(device="cpu"), dict(line_search="wolfe")):  # refused on the host, with or without a device
        with pytest.raises(_lib.SmplppError):
            BatchedLBFGS(x, **bad)
    for bad in (np.zeros((3, 5)), np.zeros(5, np.float32), np.zeros((3, 10), np.float32)[:, ::2], torch.zeros(3, 5)):
        with pytest.raises(_lib.SmplppError):
            BatchedLBFGS(bad)


# ---------------------------------------------------------------------------------------------------- 2. the plan header
MAX31 = 2 ** 31 - 1


def plan_py(n, D, m):
    if n <= 0:
        return "n must be positive"
    if D <= 0:
        return "D must be positive"
    if not 1 <= m <= 32:
        return "m must be in [1, 32]"
    if n > MAX31 or D > MAX31 or n * D * m > MAX31:
        return "n * m * D beyond int32 indexing"
    lds = D <= 2048
    return "ok %d 256 %d %d %d %d %d %d %d" % (-(-n // 4), lds, 16 * D if lds else 0, 6 * n, 4 * n, n * m, 3 * n * D, 2 * n * m * D)


def rows_py(n, D, ld):
    if ld < D:
        return "ld must be at least D"
    return "n * ld beyond int32 indexing" if ld > MAX31 or n * ld > MAX31 else "ok"


def opts_py(c1, tol_grad, tol_f, max_ls, curv_eps):
    f = np.float32
    c1, tol_grad, tol_f, curv_eps = f(c1), f(tol_grad), f(tol_f), f(curv_eps)
    if not (np.isfinite(c1) and 0 < c1 < 1):
        return "c1 must be in (0, 1)"
    if not (np.isfinite(tol_grad) and tol_grad >= 0):
        return "tol_grad must be finite and not negative"
    if not (np.isfinite(tol_f) and tol_f >= 0):
        return "tol_f must be finite and not negative"
    if not 1 <= max_ls <= 64:
        return "max_ls must be in [1, 64]"
    return "ok" if np.isfinite(curv_eps) and 0 <= curv_eps < 1 else "curv_eps must be in [0, 1)"


def ring_py(m, ops):
    head = count = 0
    out = ""
    for op in ops:
        if op == "p":
            slot, head, count = LO.ring_push(head, count, m)
            out += str(slot)
        else:
            head = count = 0
            out += "-"
        out += ":%d:%d:" % (head, count) + "".join("%d " % LO.ring_slot(head, count, m, i) for i in range(count)) + ","
    return out


def test_ring_restatement_is_a_ring():
    """The Python restatement itself: the i-th newest pair is the pair pushed i pushes ago, and a full ring keeps the last m."""
    for m in (1, 2, 3, 10, 32):
        head = count = 0
        written = {}
        for k in range(3 * m + 2):
            slot, head, count = LO.ring_push(head, count, m)
            written[slot] = k
            assert count == min(k + 1, m)
            assert [written[LO.ring_slot(head, count, m, i)] for i in range(count)] == list(range(k, k - count, -1))


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lbfgs_plan") / "lbfgs_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "lbfgs_plan_dump.cpp"), "-o", exe])
    return exe


def test_header_is_plain_cpp():
    path = os.path.join(ROOT, "smplpp_amd", "csrc", "lbfgs_plan.h")
    src = open(path).read()
    assert "hip_runtime" not in src and "__device__" not in src and "__global__" not in src
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True,
                   input='#include "%s"\n' % path)


def test_plans_rings_and_refusals_equal_python(dump_exe, tmp_path):
    queries, want = [], []
    for n in (-1, 0, 1, 3, 4, 5, 65, 1024, 16384, 2 ** 20, 2 ** 31):
        for D in (-2, 0, 1, 63, 64, 65, 72, 128, 2048, 2049, 20670, 2 ** 31):
            for m in (-1, 0, 1, 3, 10, 32, 33):
                queries.append("plan %d %d %d" % (n, D, m))
                want.append(plan_py(n, D, m))
    for n, D, ld in ((1, 5, 4), (1, 5, 5), (3, 72, 75), (2 ** 20, 72, 2 ** 11), (2 ** 31 // 72 + 1, 72, 72), (1, 5, 2 ** 31), (29826161, 72, 72)):
        queries.append("rows %d %d %d" % (n, D, ld))
        want.append(rows_py(n, D, ld))
    good = (1e-4, 1e-5, 0.0, 20, 1e-10)
    for i, values in enumerate(((0.0, 1.0, -1e-3, "nan", "inf", 0.5), (-1.0, 0.0, "nan", "inf", 1e-3), (-1e-9, 0.0, "nan", "inf", 1e-6),
                                (0, 1, 64, 65, -3), (-1e-12, 0.0, 1.0, "nan", "inf", 0.5))):
        for v in values:
            o = list(good)
            o[i] = v
            queries.append("opts %s %s %s %s %s" % tuple(o))
            want.append(opts_py(*(float(a) if k != 3 else int(a) for k, a in enumerate(o))))
    rng = np.random.default_rng(0)
    for m in range(1, 33):
        ops = "".join(rng.choice(["p", "p", "p", "p", "p", "p", "p", "d"], 3 * m + 8))
        queries.append("ring %d %s" % (m, ops))
        want.append(ring_py(m, ops))
    q, a = tmp_path / "queries.txt", tmp_path / "answers.txt"
    q.write_text("\n".join(queries) + "\n")
    r = subprocess.run([dump_exe, str(q), str(a)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and not r.stdout, r.stdout  # a sanitizer report is a failure
    got = a.read_text().split("\n")[:-1]
    assert len(got) == len(want)
    assert {w.split(" ")[0] for w in want} >= {"ok", "n", "D", "m", "ld", "c1", "tol_grad", "tol_f", "max_ls", "curv_eps"}
    for query, g, w in zip(queries, got, want):
        assert g == w, (query, g, w)


# ---------------------------------------------------------------------------------------------------- 3. the restatement
def _solve(func, x0, dtype, m=10, budget=500, **options):
    opt = LO.LBFGS(1, len(x0), m, dtype, **options)
    x = np.asarray(x0, dtype)[None].copy()
    LO.run(opt, [func], x, budget)
    s = opt.state()
    return int(s["status"][0]), int(s["evaluations"][0]), x[0], opt


@pytest.mark.parametrize("name", ["quadratic_5_10", "quadratic_69_100", "rosenbrock_8"])
def test_float32_restatement_behaves_as_lbfgs(name):
    """Measured, evaluations in float32 / float64: quadratic (5, 10) 10 / 10, quadratic (69, 100) 58 / 58, Rosenbrock 88 / 85."""
    if name.startswith("quadratic"):
        D, cond = (int(v) for v in name.split("_")[1:])
        func, x0 = LO.Quadratic(D, cond, 7), np.zeros(D)
        x_min = func.c
    else:
        func, x0, x_min = LO.Rosenbrock(), LO.Rosenbrock.start(8, np.float64), np.ones(8)
    st32, ev32, x32, _ = _solve(func, x0, np.float32, tol_grad=1e-3)
    st64, ev64, x64, _ = _solve(func, x0, np.float64, tol_grad=1e-3)
    print("%s: %d evaluations in float32, %d in float64" % (name, ev32, ev64))
    assert st32 == 1 and st64 == 1
    assert ev32 <= 1.5 * ev64 + 5
    assert np.abs(x64 - x_min).max() < 1e-2 and np.abs(x32 - x_min).max() < 1e-2
    assert np.abs(func(x32)[1]).max() <= 1e-3


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_frames_of_a_mixed_batch_are_independent(dtype):
    funcs, x = LO.mixed_batch(dtype)
    n, D, m, budget = len(funcs), x.shape[1], 5, 300
    batch = LO.LBFGS(n, D, m, dtype, tol_grad=1e-3)
    trail = [[] for _ in range(n)]
    xb = x.copy()
    LO.run(batch, funcs, xb, budget, after=lambda call: [trail[i].append(xb[i].copy()) for i in range(n)])
    assert batch.state()["status"].tolist() == [1, 1, 4, 1] and batch.state()["running"][0] == 0
    assert _same_bits(xb[2], x[2])  # the NaN frame's x is untouched
    logs = batch.log
    assert "half" in logs[3] or any(w.startswith("interpolated") for w in logs[3])  # the ball frame was thrown back inside
    for i in range(n):
        alone = LO.LBFGS(1, D, m, dtype, tol_grad=1e-3)
        xa = x[i:i + 1].copy()
        own = []
        LO.run(alone, funcs[i:i + 1], xa, budget, after=lambda call: own.append(xa[0].copy()))
        assert alone.log[0] == logs[i]
        assert all(_same_bits(a, b) for a, b in zip(own, trail[i])) and _same_bits(xa[0], xb[i])
        sa, sb = alone.state(), batch.state()
        assert all(_same_bits(np.ascontiguousarray(sa[k][:1]), np.ascontiguousarray(sb[k][i:i + 1])) for k in sa if k != "running")


def test_tol_f_stops_a_frame_with_status_2():
    func = LO.Quadratic(12, 50, 3)
    st, ev, x, opt = _solve(func, np.zeros(12), np.float32, tol_grad=0.0, tol_f=1e-4)
    assert st == 2 and opt.log[0][-1] == "flat" and ev < 100
    st0, ev0, _, _ = _solve(func, np.zeros(12), np.float32, tol_grad=0.0, tol_f=0.0, budget=ev + 5)
    assert st0 == 0 and ev0 == ev + 5  # tol_f = 0 is off: the same run goes on


def test_a_function_that_never_satisfies_armijo_ends_with_status_3():
    x0 = np.linspace(-1, 1, 6)
    for dtype in (np.float32, np.float64):
        st, ev, x, opt = _solve(LO.NeverArmijo(), x0, dtype, max_ls=7)
        assert st == 3 and ev == 1 + 8 and opt.log[0][-1] == "exhausted" and opt.state()["iterations"][0] == 0
        assert _same_bits(x, x0.astype(dtype))  # back at x0


def test_a_gradient_that_turns_nan_is_rejected():
    """The threshold lies between the minimum's first coordinate and the largest one the free run tries on its way there."""
    inner = LO.Quadratic(6, 100, 5)
    opt = LO.LBFGS(1, 6, 10, np.float32, tol_grad=1e-3)
    x, tried = np.zeros((1, 6), np.float32), []
    LO.run(opt, [inner], x, 200, after=lambda call: tried.append(float(x[0, 0])))
    assert opt.state()["status"][0] == 1
    final = float(x[0, 0])
    sign = 1.0 if max(tried) - max(final, 0.0) >= min(final, 0.0) - min(tried) else -1.0
    beyond, inside = max(sign * t for t in tried), max(sign * final, 0.0)
    assert beyond > inside + 1e-3  # the free run overshoots on that side
    threshold = 0.5 * (beyond + inside)
    st, ev, x, opt = _solve(LO.NanGradientPast(inner, threshold, sign), np.zeros(6), np.float32, tol_grad=1e-3)
    print(opt.log[0])
    assert st == 1 and sign * x[0] <= threshold and any(w == "half" or w.startswith("interpolated") for w in opt.log[0])
