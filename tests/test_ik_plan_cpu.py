"""The host plans of the IK loop (smplpp_amd/csrc/ik_plan.h) without a GPU.  tests/cpp/ik_plan_dump.cpp, built here with the address
and undefined-behaviour sanitizers, sweeps every plan function and prints one row per input; a sanitizer report ends it with a
non-zero status.  The solve plan is held, field by field, to its independent restatement tests/solve_ref.py::solve_plan — the one
tests/test_solve_ref_cpu.py uses to prove that the GPU solve tests reach every dispatch path.  The scan, side-stream, per-iteration
and roles plans have no other restatement: their rows are held to tests/golden/ik_plan.json, row counts and SHA-256 digests of the
same rows printed by the expressions of ik_iterate_enqueue / smplpp_ik_create as they stood before the plans were split out (those
lines of ik.hip pasted unchanged into a throwaway main).  The digests are data: they are never regenerated from ik_plan.h.  The
roles tables are also checked against what defines them."""
import hashlib
import json
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from smplpp_amd import model_io

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solve_ref as S  # noqa: E402

NJ, TREE_DMAX, EVAL_NT = 24, 12, 768  # layout.h; ik_types.h (SMPLPP_EVAL_NT)
TOO_WIDE = "refusal: smplpp_ik_create: kinematic tree too wide for the evaluation kernel\n"


def _parents(parent_of):
    return np.array([-1] + [parent_of(i) for i in range(1, NJ)], np.int32)


# name -> (parent[24], threads).  chain24 / star are the _tree variants of tests/test_model_tables_cpu.py (a tree deeper than 12
# levels is refused by smplpp_ik_create before the table is built: its joints beyond level 11 get no entry).
ROLES = {
    "smpl": (_parents(lambda i: int(model_io.KINEMATIC_TREE[0, i])), EVAL_NT),
    "chain12": (_parents(lambda i: i - 1 if i < 12 else (i - 12 if i < 23 else 0)), EVAL_NT),
    "star": (_parents(lambda i: 0), EVAL_NT),
    "chain24": (_parents(lambda i: i - 1), EVAL_NT),
    "smpl_64_threads": (_parents(lambda i: int(model_io.KINEMATIC_TREE[0, i])), 64),  # 12 x 64 slots for 1.2 k entries: too wide
    "star_64_threads": (_parents(lambda i: 0), 64),  # 9 + 23 x 18 = 423 entries: fits
}


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ik_plan") / "ik_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "ik_plan_dump.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "ik_plan.json")) as f:
        return json.load(f)


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr  # a sanitizer report is a failure
    return r.stdout


def digest(text):
    return {"rows": text.count("\n"), "sha256": hashlib.sha256(text.encode()).hexdigest()}


def roles_text(exe, tmp_path, name):
    parent, nt = ROLES[name]
    path = str(tmp_path / (name + ".bin"))
    parent.astype("<i4").tofile(path)
    return run(exe, "roles", path, nt)


def test_header_is_plain_cpp():
    src = open(os.path.join(ROOT, "smplpp_amd", "csrc", "ik_plan.h")).read()
    assert "hip_runtime" not in src and "__device__" not in src and "__global__" not in src
    assert [ln for ln in src.splitlines() if ln.startswith('#include "')] == ['#include "layout.h"']
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True,
                   input='#include "%s"\n' % os.path.join(ROOT, "smplpp_amd", "csrc", "ik_plan.h"))


def test_solve_plan_equals_its_restatement(dump_exe):
    rows = [[int(x) for x in ln.split()] for ln in run(dump_exe, "solve").splitlines()]
    assert len(rows) == 64 * 2 * 2 * 16 and len({tuple(r[:7]) for r in rows}) == len(rows)
    kernels, least, refused = Counter(), None, 0
    for K, td, bd, locked, live, qp, primal, D, nrows, m_dim, qp_k, ntr, dual_only, chunk_rows, shmem, refusal in rows:
        try:
            p = S.solve_plan(K, td, bd, bool(locked), enable_qp=bool(qp), phi_live=bool(live), primal_only=bool(primal))
        except AssertionError:
            p = None
        assert (refusal != 0) == (p is None), (K, td, bd, locked, live, qp, primal, refusal)
        if K <= 48:
            assert refusal == 0  # (both refusals stay in the library; no supported task count reaches them)
        if p is None:
            refused += 1
            continue
        got = dict(D=D, rows=nrows, m_dim=m_dim, qp=bool(qp_k), ntr=ntr, chunk_rows=chunk_rows, kernel="dual" if dual_only else "ntr%d" % ntr)
        assert got == {k: p[k] for k in got}, (K, td, bd, locked, live, qp, primal)
        fixed = 8 * ((m_dim + 1) * (m_dim + 2) // 2 + 7 * D + 2 * nrows + 128 * ntr + 4) + 4 * 2 * D
        assert shmem == fixed + 8 * chunk_rows * D and shmem <= S.SOLVE_LDS_MAX
        if K <= 48:
            kernels[got["kernel"]] += 1
            least = chunk_rows if least is None else min(least, chunk_rows)
    assert sum(kernels.values()) == 3072
    assert kernels == {"ntr5": 1080, "ntr6": 588, "ntr3": 518, "ntr11": 486, "dual": 400}
    assert least == 4  # the sweep sits on the refusal threshold: an off-by-one there shows
    assert refused > 0  # K = 49..64 reaches the refusals


@pytest.mark.parametrize("mode,rows", [("scan", 14 * 48 * 11 * 3 * 4), ("side", 64), ("iter", 6 * 31)])
def test_plans_equal_the_one_function_loop(dump_exe, golden, mode, rows):
    out = run(dump_exe, mode)
    assert out.count("\n") == rows
    assert digest(out) == golden[mode]


def test_scan_plan_reaches_every_instantiation(dump_exe):
    rows = np.array([[int(x) for x in ln.split()] for ln in run(dump_exe, "scan").splitlines()])
    assert {tuple(r) for r in rows[:, 6:8]} == {(0, 3), (0, 6), (2, 6), (4, 6)}
    assert rows[:, 5].min() == 1 and rows[:, 5].max() == 32 and rows[:, 8].min() == 1 and rows[:, 8].max() == 48


@pytest.mark.parametrize("name", list(ROLES))
def test_roles_equal_the_one_function_creation(dump_exe, golden, tmp_path, name):
    assert digest(roles_text(dump_exe, tmp_path, name)) == golden["roles"][name]


@pytest.mark.parametrize("name", list(ROLES))
def test_roles_definition(dump_exe, tmp_path, name):
    parent, nt = ROLES[name]
    text = roles_text(dump_exe, tmp_path, name)
    depth = np.zeros(NJ, int)
    for i in range(1, NJ):
        depth[i] = depth[parent[i]] + 1
    want = sorted((i, da, axis, row) for i in range(NJ) if depth[i] < TREE_DMAX for da in range(depth[i] + 1) for axis in range(3) for row in range(3))
    if len(want) > TREE_DMAX * nt:
        assert text == TOO_WIDE and name == "smpl_64_threads"
        return
    w = np.array([int(x) for x in text.split()], np.int64)
    assert len(w) == TREE_DMAX * nt
    # entry e goes to thread e % nt as its e / nt-th: slot [e / nt][e % nt] of the table, i.e. its e-th word; the rest are -1
    E = len(want)
    assert (w[:E] >= 0).all() and (w[E:] == -1).all()
    i, par, cs, row, last = w[:E] & 31, (w[:E] >> 5) & 31, (w[:E] >> 10) & 63, (w[:E] >> 16) & 3, (w[:E] >> 18) & 1
    assert (w[:E] >> 19 == 0).all()
    assert sorted(zip(i.tolist(), (cs // 3).tolist(), (cs % 3).tolist(), row.tolist())) == want  # every entry exactly once
    assert np.array_equal(par, parent[i] & 31) and np.array_equal(last, (cs // 3 == depth[i]).astype(int))
    assert np.array_equal(depth[i], np.sort(depth[i]))  # level by level
    src = open(os.path.join(ROOT, "smplpp_amd", "csrc", "ik_plan.h")).read()
    assert src.count('"%s"' % TOO_WIDE[len("refusal: "):-1]) == 1  # the text is the library's
