"""L-BFGS problems that span groups of rows, without a GPU.  (1) The two entry points are declared, exported and bound, a call without a
device fails loudly, and every refusal of smplpp_lbfgs_create_grouped is made on the host: by the library before it selects a device,
and by the Python class.  (2) The host decisions of smplpp_amd/csrc/lbfgs_wide_plan.h as a stand-alone program,
tests/cpp/lbfgs_wide_plan_dump.cpp, built with the address and undefined-behaviour sanitizers: offsets, sizes, launch, refusals and the
walk of a thread through a caller's rows equal a Python restatement over ragged row_start and D in {1, 72, 75, 1023, 1024, 1025}.
(3) The float32 restatement of the grouped rule (tests/lbfgs_groups_oracle.py), the one the GPU tests hold the library to bit for bit,
behaves as an L-BFGS on chains of coupled rows.  (4) The problems of a ragged batch are independent."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_groups_oracle as GO  # noqa: E402
import lbfgs_oracle as LO  # noqa: E402
from distance_cases import _same_bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"smplpp_lbfgs_create_grouped": 12, "smplpp_lbfgs_groups": 3}
GOOD = (1e-4, 1e-5, 0.0, 20, 1e-10)


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


def test_the_library_refuses_bad_groups_before_it_selects_a_device():
    from smplpp_amd import _lib

    L = _lib.load()

    def create(n, D, m, P, start, o=GOOD):
        h = C.c_void_p(7)
        arr = None if start is None else (C.c_int64 * len(start))(*start)
        rc = L.smplpp_lbfgs_create_grouped(0, n, D, m, P, arr, *o, C.byref(h))
        assert rc != 0 and h.value is None  # *out = NULL
        return rc

    for args in ((6, 5, 3, 0, [0]), (6, 5, 3, -2, [0]),  # P <= 0
                 (6, 5, 3, 2, [1, 3, 6]),                 # row_start[0] != 0
                 (6, 5, 3, 2, [0, 3, 5]), (6, 5, 3, 2, [0, 3, 7]),  # row_start[P] != n
                 (6, 5, 3, 3, [0, 3, 3, 6]), (6, 5, 3, 3, [0, 4, 3, 6]),  # not strictly increasing
                 (6, 5, 3, 2, None),                      # a NULL row_start
                 (0, 5, 3, 1, [0, 0]), (6, 0, 3, 1, [0, 6]), (6, 5, 0, 1, [0, 6]), (6, 5, 33, 1, [0, 6]), (2 ** 20, 2 ** 10, 2, 1, [0, 2 ** 20])):  # the shape
        assert create(*args) == 1, args
    for i, bad in ((0, 0.0), (1, -1.0), (2, float("nan")), (3, 0), (4, 1.0)):  # the options
        o = list(GOOD)
        o[i] = bad
        assert create(6, 5, 3, 2, [0, 3, 6], tuple(o)) == 1, (i, bad)
    assert L.smplpp_lbfgs_create_grouped(0, 6, 5, 3, 2, (C.c_int64 * 3)(0, 3, 6), *GOOD, None) == 1  # no out
    assert L.smplpp_lbfgs_groups(None, None, None) == 1


def test_a_call_without_a_device_fails_loudly():
    from smplpp_amd import _lib
    from smplpp_amd.optim import BatchedLBFGS

    x = np.zeros((6, 5), np.float32)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.SmplppError):
            BatchedLBFGS(x, groups=[2, 1, 3])
    for bad in ([], [0, 6], [3, 0, 3], [2, 2], [4, 4], [-1, 7], [1.5, 4.5], "ab", 6, [None]):  # refused on the host, with or without a device
        with pytest.raises(_lib.SmplppError):
            BatchedLBFGS(x, groups=bad)
    for bad in (dict(history=0), dict(history=33), dict(c1=0.0), dict(max_ls=0), dict(device="cpu"), dict(line_search="wolfe")):
        with pytest.raises(_lib.SmplppError):
            BatchedLBFGS(x, groups=[2, 1, 3], **bad)


# ---------------------------------------------------------------------------------------------------- 2. the plan header
MAX31 = 2 ** 31 - 1
T, LDS_N = 1024, 32768


def groups_py(n, D, m, P, start):
    if n <= 0:
        return "n must be positive"
    if D <= 0:
        return "D must be positive"
    if not 1 <= m <= 32:
        return "m must be in [1, 32]"
    if n > MAX31 or D > MAX31 or n * D * m > MAX31:
        return "n * m * D beyond int32 indexing"
    if P <= 0:
        return "P must be positive"
    if start is None:
        return "row_start is NULL"
    if start[0] != 0:
        return "row_start[0] must be 0"
    if any(start[p + 1] <= start[p] for p in range(P)):
        return "row_start must strictly increase"
    if start[P] != n:
        return "row_start[P] must be n"
    longest = max(start[p + 1] - start[p] for p in range(P)) * D
    lds = longest <= LDS_N
    out = "ok %d %d %d %d %d %d %d %d %d %d" % (P, T, lds, 4 * longest if lds else 0, 6 * P, 4 * P, P * m, 3 * n * D, 2 * n * m * D, P + 1)
    for p in range(P):
        r0, N = start[p], (start[p + 1] - start[p]) * D
        # x0, g0 and d of the problem are N contiguous floats at its first row's place in a [n, D] array; its ring is 2 m N floats after the
        # rings of the problems before it, s slots first
        out += " | %d %d %d %d %d %d" % (r0 * D, n * D + r0 * D, 2 * n * D + r0 * D, 2 * m * D * r0, m * N, (2 * m - 1) * N)
    return out


def walk_py(D, ld, t, steps):
    """Element j = t + 1024 i is coordinate j mod D of row j div D."""
    return " ".join("%d:%d" % (j % D, (j // D) * ld + j % D) for j in range(t, t + T * (steps + 1), T))


def test_offsets_restatement_tiles_the_buffers():
    """The Python restatement itself: the problems' blocks tile vec and hist without gaps or overlaps."""
    n, D, m, start = 21, 75, 10, [0, 1, 4, 18, 21]
    blocks = [[int(v) for v in b.split()] for b in groups_py(n, D, m, 4, start).split(" | ")[1:]]
    for p, (x0, g0, d, ring, y0, ylast) in enumerate(blocks):
        N = (start[p + 1] - start[p]) * D
        nxt = blocks[p + 1] if p + 1 < len(blocks) else [n * D, 2 * n * D, 3 * n * D, 2 * n * m * D]
        assert (x0 + N, g0 + N, d + N, ring + 2 * m * N) == tuple(nxt[:4]) and ring + ylast + N == nxt[3]


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lbfgs_wide_plan") / "lbfgs_wide_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "lbfgs_wide_plan_dump.cpp"), "-o", exe])
    return exe


def test_header_is_plain_cpp():
    path = os.path.join(ROOT, "smplpp_amd", "csrc", "lbfgs_wide_plan.h")
    src = open(path).read()
    assert "hip_runtime" not in src and "__device__" not in src and "__global__" not in src
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True,
                   input='#include "%s"\n' % path)


def test_plans_walks_and_refusals_equal_python(dump_exe, tmp_path):
    queries, want = [], []

    def ask(n, D, m, P, start):
        queries.append(("nogroups %d %d %d %d" % (n, D, m, P)) if start is None else "groups %d %d %d %d %s" % (n, D, m, P, " ".join(map(str, start))))
        want.append(groups_py(n, D, m, P, start))

    ragged = ([1], [1, 3, 14], [15], [14, 1], [2, 1, 2], [300, 7], [5, 1, 1, 9], [8, 1], [109, 110], [7, 5])
    for D in (1, 72, 75, 1023, 1024, 1025):
        for lens in ragged:
            start = [0] + np.cumsum(lens).tolist()
            for m in (1, 10, 32):
                ask(start[-1], D, m, len(lens), start)
    for D in (1, 2, 4, 8):  # the LDS decision at its threshold: the longest problem has 32768 elements, or one row more
        for rows in (LDS_N // D, LDS_N // D + 1):
            ask(rows + 3, D, 3, 2, [0, 3, rows + 3])
            ask(rows + 3, D, 3, 2, [0, rows, rows + 3])
    n, D, m = 18, 72, 3
    for P, start in ((0, [0]), (-1, [0]), (3, None), (3, [1, 2, 4, 18]), (3, [0, 4, 4, 18]), (3, [0, 5, 4, 18]), (3, [0, 4, 18, 18]), (3, [0, 1, 4, 17]),
                     (3, [0, 1, 4, 19]), (3, [-1, 1, 4, 18]), (1, [0, 18]), (18, list(range(19)))):
        ask(n, D, m, P, start)
    for n_, D_, m_ in ((0, 72, 3), (-1, 72, 3), (18, 0, 3), (18, 72, 0), (18, 72, 33), (2 ** 20, 2 ** 10, 2), (2 ** 31, 1, 1)):
        ask(n_, D_, m_, 1, [0, n_])
        ask(n_, D_, m_, 0, None)  # the shape is refused first
    for D in (1, 72, 75, 1023, 1024, 1025):
        for ld in sorted({D, D + 3, max(D, 75), 2 * D + 1}):
            for t in sorted({0, 1, D - 1 if D <= T else 5, min(D, T - 1), 517, T - 1}):
                queries.append("walk %d %d %d %d" % (D, ld, t, 45))
                want.append(walk_py(D, ld, t, 45))
    queries.append("walk 75 %d 1023 3" % (2 ** 31 // 300))  # offsets past int32 after the problem's end
    want.append(walk_py(75, 2 ** 31 // 300, 1023, 3))
    q, a = tmp_path / "queries.txt", tmp_path / "answers.txt"
    q.write_text("\n".join(queries) + "\n")
    r = subprocess.run([dump_exe, str(q), str(a)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and not r.stdout, r.stdout  # a sanitizer report is a failure
    got = a.read_text().split("\n")[:-1]
    assert len(got) == len(want)
    assert {w.split(" ")[0] for w in want if ":" not in w} >= {"ok", "n", "D", "m", "P", "row_start", "row_start[0]", "row_start[P]"}
    assert any(w.startswith("ok") and w.split()[3] == "1" for w in want) and any(w.startswith("ok") and w.split()[3] == "0" for w in want)
    for query, g, w in zip(queries, got, want):
        assert g == w, (query, g, w)


# ---------------------------------------------------------------------------------------------------- 3. the restatement
def _solve(func, T, D, dtype, m=10, budget=500, **options):
    opt = GO.GroupedLBFGS([T], D, m, dtype, **options)
    x = np.zeros((T, D), dtype)
    GO.run(opt, [func], x, budget)
    s = opt.state()
    return int(s["status"][0]), int(s["evaluations"][0]), x.reshape(-1), opt


@pytest.mark.parametrize("T,D,cond,lam", [(15, 72, 100, 1), (40, 75, 100, 1), (3, 1, 10, 1)])
def test_float32_restatement_behaves_as_lbfgs(T, D, cond, lam):
    """Chain from x = 0, m = 10, tol_grad = 1e-3.  Measured, evaluations in float32 / float64: (15, 72, 100, 1) 62 / 57, (40, 75, 100, 1)
    73 / 55, (3, 1, 10, 1) 8 / 8."""
    func = GO.Chain(T, D, cond, lam, 7)
    st32, ev32, x32, _ = _solve(func, T, D, np.float32, tol_grad=1e-3)
    st64, ev64, x64, _ = _solve(func, T, D, np.float64, tol_grad=1e-3)
    print("chain (%d, %d, %d, %g): %d evaluations in float32, %d in float64" % (T, D, cond, lam, ev32, ev64))
    assert st32 == 1 and st64 == 1
    assert ev32 <= 1.5 * ev64 + 5
    assert np.abs(func(x32)[1]).max() <= 1e-3 and np.abs(func(x64)[1]).max() <= 1e-3
    assert np.abs(x32 - x64).max() < 1e-2  # the minimum is unique (every curvature is at least 1)


def test_chain_gradient_is_the_gradient():
    func, rng = GO.Chain(4, 3, 10, 0.7, 5), np.random.default_rng(0)
    x = rng.normal(size=12)
    f, g = func(x)
    for j in range(12):
        e = np.zeros(12)
        e[j] = 1e-6
        assert abs((func(x + e)[0] - func(x - e)[0]) / 2e-6 - g[j]) < 1e-6 * max(1.0, abs(g[j]))
    alone = sum(q(x.reshape(4, 3)[t])[0] for t, q in enumerate(func.q))
    assert abs(f - alone - 0.7 * (np.diff(x.reshape(4, 3), axis=0) ** 2).sum()) < 1e-12


# ---------------------------------------------------------------------------------------------------- 4. independence
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_problems_of_a_ragged_batch_are_independent(dtype):
    funcs, groups, x = GO.ragged_batch(dtype)
    P, D, m, budget = len(funcs), x.shape[1], 5, 300
    batch = GO.GroupedLBFGS(groups, D, m, dtype, tol_grad=1e-3)
    trail = [[] for _ in range(P)]
    xb = x.copy()
    GO.run(batch, funcs, xb, budget, after=lambda call: [trail[p].append(xb[batch.rows(p)].copy()) for p in range(P)])
    assert batch.state()["status"].tolist() == [1, 1, 4, 1] and batch.state()["running"][0] == 0
    assert _same_bits(xb[batch.rows(2)], x[batch.rows(2)])  # the NaN problem's x is untouched
    logs = batch.log
    assert "half" in logs[3] or any(w.startswith("interpolated") for w in logs[3])  # the ball problem was thrown back inside
    for p in range(P):
        alone = GO.GroupedLBFGS(groups[p:p + 1], D, m, dtype, tol_grad=1e-3)
        xa = x[batch.rows(p)].copy()
        own = []
        GO.run(alone, funcs[p:p + 1], xa, budget, after=lambda call: own.append(xa.copy()))
        assert alone.log[0] == logs[p]
        assert all(_same_bits(a, b) for a, b in zip(own, trail[p])) and _same_bits(xa, xb[batch.rows(p)])
        sa, sb = alone.state(), batch.state()
        assert all(_same_bits(np.ascontiguousarray(sa[k][:1]), np.ascontiguousarray(sb[k][p:p + 1])) for k in sa if k != "running")


def test_a_one_row_problem_follows_the_1024_rule_not_the_64_rule():
    """A grouped handle always sums by the 1024-partial rule: a problem of one row is the per-frame rule with another sum, and from
    D = 65 on the two sums round differently somewhere along a run."""
    D, func = 300, LO.Quadratic(300, 1000.0, 3)
    x0 = np.random.default_rng(1).normal(0, 0.5, D).astype(np.float32)
    wide, frame = GO.GroupedLBFGS([1], D, 5, np.float32, tol_grad=0.0), LO.LBFGS(1, D, 5, np.float32, tol_grad=0.0)
    xw, xf = x0[None].copy(), x0[None].copy()
    GO.run(wide, [func], xw, 12)
    LO.run(frame, [func], xf, 12)
    assert wide.log[0] == frame.log[0] and np.allclose(xw, xf, rtol=1e-3, atol=1e-4) and not _same_bits(xw, xf)
