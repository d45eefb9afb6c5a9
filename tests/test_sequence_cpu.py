"""The sequence terms without a GPU: the numpy restatement of smplpp_sequence_smoothness and its backward (tests/sequence_oracle.py)
against float64 autograd of the definition (its 1024-partial sum is sum_rules.sum1024, pinned in test_sum_rules_cpu.py); the split / merge / sum restatements against
autograd; and the host table builder (smplpp_amd/csrc/sequence_tables.h) as a stand-alone program, tests/cpp/sequence_tables_dump.cpp, built
with the address and undefined-behaviour sanitizers: its tables equal the Python builder's, and each refusal returns its reason without a
sanitizer report."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sequence_oracle as SO  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["smplpp_sequence_create", "smplpp_sequence_destroy", "smplpp_sequence_info", "smplpp_sequence_merge", "smplpp_sequence_smoothness",
         "smplpp_sequence_smoothness_vjp", "smplpp_sequence_split", "smplpp_sequence_sum"]
U = 2.0 ** -24  # the unit roundoff of float32


def test_header_declares_the_calls():
    from smplpp_amd import _lib

    assert set(NAMES) <= set(_lib.declared_symbols())


# ---------------------------------------------------------------------------------------------------- 1. the restatement against float64
GROUPS = [([1, 2, 3, 5], 0), ([2, 3, 4, 7], 1)]  # problems of 1, 2 and 3 frames (and a longer one), without and with a shared row


def _points(F, K, C, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.normal(0, 0.05, (F, K, C)), 0) + rng.normal(0, 1.0, (1, K, C))


@pytest.mark.parametrize("groups,shared", GROUPS)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("rho", [0.0, 0.05])
def test_restatement_against_float64(groups, shared, order, rho):
    L = SO.layout(groups, shared)
    F, K, C = L["frames"], 7, 3
    x = _points(F, K, C, seed=order + len(groups))
    rng = np.random.default_rng(3)
    w = rng.uniform(0.5, 2.0, K)
    w[2] = 0.0
    gfe, gpe = rng.normal(size=F), rng.normal(size=(F, K))
    X = torch.tensor(x, requires_grad=True)
    e = SO.energy_t(L, X, order, w, rho)
    ((e.sum(1) * torch.tensor(gfe)).sum() + (e * torch.tensor(gpe)).sum()).backward()
    # float64: the restatement is the definition and its derivative
    fe, pe = SO.smoothness(L, x.reshape(F, K * C), K, C, order, w, rho)
    got = SO.smoothness_vjp(L, x.reshape(F, K * C), K, C, order, w, rho, gfe, gpe, np.zeros((F, K * C)), 0)
    print("float64 restatement: energy rel %.3g, backward rel %.3g" % (_rel(pe, e.detach().numpy()), _rel(got, X.grad.numpy().reshape(F, -1))))
    assert np.abs(X.grad.numpy()).max() > 0
    assert _rel(pe, e.detach().numpy()) <= 1e-9 and _rel(fe, e.detach().numpy().sum(1)) <= 1e-9
    assert _rel(got, X.grad.numpy().reshape(F, -1)) <= 1e-9
    # float32 forward: within rounding of float64 on the same (float32) inputs.  With u = 2^-24, a difference d = a - b of exact inputs
    # has error u |d|, a second difference (a - b) - (b' - c) has u (|a - b| + |b' - c| + |d|); q = sum_c d_c^2 then has
    # dq <= sum_c (2 |d_c| dd_c + dd_c^2) + (C + 2) u q; e = w q (or w p2 q / (p2 + q), whose slope in q is at most w) adds a few
    # roundings of its own, 8 u e covers them; the 1024-partial sum of K terms adds at most (ceil(K / 1024) + 10) u sum_k e.
    x32 = x.astype(np.float32).reshape(F, K * C)
    x64 = x32.astype(np.float64)
    fe32, pe32 = SO.smoothness(L, x32, K, C, order, w.astype(np.float32), rho)
    w64 = w.astype(np.float32).astype(np.float64)
    fe64, pe64 = SO.smoothness(L, x64, K, C, order, w64, float(np.float32(rho)))
    Xp = x64.reshape(F, K, C)
    st, d, q = SO._differences(L, x64, K, C, order)
    mag = np.zeros_like(d)
    at = np.nonzero(st)[0]
    mag[at] = np.abs(d[at]) if order == 1 else np.abs(Xp[at + 1] - Xp[at]) + np.abs(Xp[at] - Xp[at - 1]) + np.abs(d[at])
    dd = U * mag
    dq = (2 * np.abs(d) * dd + dd * dd).sum(-1) + (C + 2) * U * q
    bound = w64[None] * dq + 8 * U * np.abs(pe64)
    assert pe32.dtype == np.float32 and (np.abs(pe32 - pe64) <= bound).all(), np.abs(pe32 - pe64).max()
    assert (np.abs(fe32 - fe64) <= bound.sum(1) + 11 * U * pe64.sum(1)).all()
    # where a frame has no stencil or a weight is zero, the energies and the backward are exactly +0
    dead = ~st[:, None] | (w == 0)[None]
    assert (pe32[dead] == 0).all() and not np.signbit(pe32[dead]).any()


def test_nan_stays_in_its_stencils():
    L = SO.layout([1, 2, 5, 3], 0)
    F, K, C = L["frames"], 4, 3
    x = _points(F, K, C, 5).astype(np.float32).reshape(F, K * C)
    x[5] = np.nan  # the third frame of the problem of 5 frames (frames 3 .. 7)
    for order in (1, 2):
        fe, pe = SO.smoothness(L, x, K, C, order, None, 0.0)
        gx = SO.smoothness_vjp(L, x, K, C, order, None, 0.0, np.ones(F, np.float32), None, np.zeros_like(x), 0)
        bad = np.isnan(fe)
        assert bad.tolist() == [f in ((4, 5) if order == 1 else (4, 5, 6)) for f in range(F)]
        assert not np.isnan(gx[:3]).any() and not np.isnan(gx[8:]).any()
        # a zero cotangent keeps the NaN out entirely
        g0 = SO.smoothness_vjp(L, x, K, C, order, None, 0.0, np.zeros(F, np.float32), None, np.zeros_like(x), 0)
        assert (g0 == 0).all()


# ---------------------------------------------------------------------------------------------------- 2. split, merge and sum
def test_split_merge_sum_against_autograd():
    groups = [3, 2, 6]
    L = SO.layout(groups, 1)
    n, F, D = L["rows"], L["frames"], 12
    rng = np.random.default_rng(1)
    rows = rng.normal(size=(n, D)).astype(np.float32)
    frames, shared = SO.split(L, rows, 2, 7, 4)
    assert frames.shape == (F, 7) and shared.shape == (F, 4)
    gf, gs = rng.normal(size=(F, 7)).astype(np.float32), rng.normal(size=(F, 4)).astype(np.float32)
    R = torch.tensor(rows.astype(np.float64), requires_grad=True)
    theta = torch.cat([R[0:2], R[3:4], R[5:10]])[:, 2:9]
    beta = torch.cat([R[2, :4].expand(2, 4), R[4, :4].expand(1, 4), R[10, :4].expand(5, 4)])
    assert np.array_equal(theta.detach().numpy().astype(np.float32), frames) and np.array_equal(beta.detach().numpy().astype(np.float32), shared)
    ((theta * torch.tensor(gf.astype(np.float64))).sum() + (beta * torch.tensor(gs.astype(np.float64))).sum()).backward()
    got = SO.merge(L, gf, 2, 7, gs, 4, np.full((n, D), 7.0, np.float32), D, 0)
    assert _rel(got, R.grad.numpy()) <= 8 * U
    twice = SO.merge(L, gf, 2, 7, gs, 4, got.copy(), D, 1)
    assert _same_bits(twice, got + got)
    fv = rng.normal(size=F).astype(np.float32)
    pv = SO.seq_sum(L, fv, 0.5, np.zeros(3, np.float32), 0)
    want = [0.5 * fv[:2].astype(np.float64).sum(), 0.5 * fv[2:3].astype(np.float64).sum(), 0.5 * fv[3:].astype(np.float64).sum()]
    assert np.allclose(pv, want, rtol=8 * U, atol=8 * U)


# ---------------------------------------------------------------------------------------------------- 3. the host table builder
GOOD = {"one": ([0, 1], 0), "two": ([0, 2], 0), "three_shared": ([0, 3], 1), "ragged": ([0, 1, 3, 8, 11], 0), "ragged_shared": ([0, 2, 5, 11, 15], 1),
        "long_shared": ([0, 1031], 1)}
# name -> (P, row_start or None, shared_rows, the reason)
REFUSALS = {
    "no_problem": (0, [0], 0, "P must be positive"),
    "negative_P": (-3, None, 0, "P must be positive"),
    "no_row_start": (2, None, 0, "row_start is NULL"),
    "first_not_zero": (2, [1, 2, 3], 0, "row_start[0] must be 0"),
    "empty_problem": (3, [0, 2, 2, 5], 0, "row_start must strictly increase"),
    "decreasing": (2, [0, 4, 3], 1, "row_start must strictly increase"),
    "two_shared_rows": (1, [0, 5], 2, "shared_rows must be 0 or 1"),
    "negative_shared_rows": (1, [0, 5], -1, "shared_rows must be 0 or 1"),
    "too_many_rows": (2, [0, 5, 2 ** 31], 0, "rows beyond int32 indexing"),
    "no_frame": (3, [0, 3, 4, 9], 1, "a problem has no frame beside its shared row"),
}


def write_groups(path, P, row_start, shared_rows):
    """The dump program's input (tests/cpp/sequence_tables_dump.cpp)."""
    has = row_start is not None
    with open(path, "wb") as f:
        f.write(np.array([P, shared_rows, int(has), len(row_start) if has else 0], np.int64).tobytes())
        if has:
            f.write(np.array(row_start, np.int64).tobytes())


def read_tables(path):
    raw, out, q = open(path, "rb").read(), {}, 0
    while q < len(raw):
        name = raw[q:q + 16].rstrip(b"\0").decode()
        es, n = np.frombuffer(raw, np.int64, 2, q + 16)
        out[name] = raw[q + 32:q + 32 + es * n]
        q += 32 + es * n
    return out


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sequence_tables") / "sequence_tables_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "sequence_tables_dump.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dumped(dump_exe, tmp_path_factory):
    """name -> the program's records; the program runs once per case."""
    cases = {name: (len(rs) - 1, rs, sh) for name, (rs, sh) in GOOD.items()}
    cases.update({name: c[:3] for name, c in REFUSALS.items()})
    out = {}
    for name, (P, rs, sh) in cases.items():
        d = tmp_path_factory.mktemp(name)
        write_groups(str(d / "groups.bin"), P, rs, sh)
        r = subprocess.run([dump_exe, str(d / "groups.bin"), str(d / "tables.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=120)
        assert r.returncode == 0 and not r.stdout, (name, r.stdout)  # a sanitizer report is a failure
        out[name] = read_tables(str(d / "tables.bin"))
    return out


def test_header_is_plain_cpp():
    path = os.path.join(ROOT, "smplpp_amd", "csrc", "sequence_tables.h")
    src = open(path).read()
    assert "hip_runtime" not in src and "__device__" not in src and "__global__" not in src
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True,
                   input='#include "%s"\n' % path)


@pytest.mark.parametrize("name", list(GOOD))
def test_tables_equal_python(dumped, name):
    rs, sh = GOOD[name]
    t, want = dumped[name], SO.tables(len(rs) - 1, rs, sh)
    assert "refusal" not in t and "refusal" not in want
    assert np.frombuffer(t["dims"], np.int64).tolist() == [want[k] for k in ("P", "rows", "frames", "shared_rows")]
    for k in ("row_start", "frame_start", "problem_of", "row_of", "frame_of"):
        assert t[k] == want[k].tobytes(), k
    # what the layout promises: compact frames in row order, every row accounted for
    F = want["frames"]
    assert F == want["rows"] - want["P"] * sh and (np.diff(want["frame_start"]) == np.diff(want["row_start"]) - sh).all()
    assert (want["frame_of"][want["row_of"]] == np.arange(F)).all() and (np.diff(want["row_of"]) > 0).all()
    assert sorted(want["frame_of"][want["frame_of"] < 0].tolist()) == ([-1 - p for p in range(want["P"])][::-1] if sh else [])


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(dumped, name):
    P, rs, sh, why = REFUSALS[name]
    assert dumped[name] == {"refusal": why.encode()}
    assert SO.tables(P, rs, sh) == {"refusal": why}
