"""The keypoint term without a GPU.  (1) The float32 restatements of the two backward passes (tests/keypoints_oracle.py), the ones the
GPU tests hold the library to bit for bit, against float64 autograd of the definitions, within the project's bar: max(4 x the error
of fp32 autograd of the same graph, 1e-5 relative).  (2) The host table builder of smplpp_landmarks_create
(smplpp_amd/csrc/landmark_tables.h) as a stand-alone program, tests/cpp/landmark_tables_dump.cpp, built with the address and
undefined-behaviour sanitizers: its tables equal a numpy construction of the transposed lists, and each refusal returns its reason
without a sanitizer report."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoints_oracle as KP  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bar(got, want64, fp32, what):
    err, ref = _rel(got, want64), _rel(fp32, want64)
    print("%s: restatement rel %.3g, fp32 autograd rel %.3g" % (what, err, ref))
    assert np.abs(want64).max() > 0 and err <= max(4 * ref, 1e-5), (what, err, ref)


# ---------------------------------------------------------------------------------------------------- 1. the restatements
def test_landmarks_restatement_against_float64():
    V, n = 97, 3
    reg = KP.regressor_11(V)
    rng = np.random.default_rng(1)
    verts, joints = rng.normal(size=(n, V, 3)).astype(np.float32), rng.normal(size=(n, 24, 3)).astype(np.float32)
    g = rng.normal(size=(n, 11, 3)).astype(np.float32)
    A = KP.dense(reg, V + 24)

    def ref(dtype):
        v, j = (torch.tensor(x, dtype=dtype, requires_grad=True) for x in (verts, joints))
        p = KP.landmarks_t(torch.tensor(A, dtype=dtype), v, j)
        (p * torch.tensor(g, dtype=dtype)).sum().backward()
        return [x.detach().double().numpy() for x in (p, v.grad, j.grad)]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    pts = KP.landmarks(reg, verts, joints)
    assert pts.dtype == np.float32 and (pts[:, 0] == 0).all() and not np.signbit(pts[:, 0]).any()  # the empty row: +0
    assert _same_bits(pts[:, 1], verts[:, V // 2]) and _same_bits(pts[:, 2], joints[:, 5])  # the picks
    _bar(pts, r64[0], r32[0], "landmarks forward")
    gv, gj = KP.landmarks_vjp(reg, g, V)
    _bar(gv, r64[1], r32[1], "landmarks grad_verts")
    _bar(gj, r64[2], r32[2], "landmarks grad_joints")
    base = rng.normal(size=(n, V, 3)).astype(np.float32)
    assert _same_bits(KP.landmarks_vjp(reg, g, V, base_verts=base)[0], base + gv)


@pytest.mark.parametrize("rho", [0.0, 100.0])
@pytest.mark.parametrize("K", [1, 65, 200])
def test_projection_restatement_against_float64(K, rho):
    n = 3
    s = KP.scene(n, K, seed=K, bad=1)
    P, cam, T, guv, ge = (s[k] for k in ("points", "camera", "target", "grad_uv", "grad_energy"))

    def ref(dtype):
        p, c = (torch.tensor(x, dtype=dtype, requires_grad=True) for x in (P, cam))
        uv, valid = KP.project_t(p, c)
        e = KP.energy_t(uv, valid, torch.tensor(T, dtype=dtype), rho)
        uvm = torch.where(valid[..., None], uv, torch.zeros_like(uv))
        ((uvm * torch.tensor(guv, dtype=dtype)).sum() + (e * torch.tensor(ge, dtype=dtype)).sum()).backward()
        return [x.detach().double().numpy() for x in (uvm, e, p.grad, c.grad)] + [valid.numpy()]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    uv, e, valid = KP.project(P, cam, 0.05, T, rho)
    assert np.array_equal(valid.astype(bool), r64[4]) and (K <= 8 or not valid[:, 0].any())
    _bar(uv, r64[0], r32[0], "uv")
    _bar(e, r64[1], r32[1], "energy")
    gp, gc = KP.project_vjp(P, cam, 0.05, T, rho, guv, ge)
    _bar(gp, r64[2], r32[2], "grad_points")
    for name, sl in (("R", slice(0, 9)), ("t", slice(9, 12)), ("f", slice(12, 14)), ("c", slice(14, 16))):
        _bar(gc[:, sl], r64[3][:, sl], r32[3][:, sl], "grad_camera " + name)
    # a refused point gets +0 and gives the camera nothing; each input alone; accumulate adds the finished value
    assert K <= 8 or ((gp[:, 0] == 0).all() and not np.signbit(gp[:, 0]).any())
    a = KP.project_vjp(P, cam, 0.05, None, rho, guv, None)
    b = KP.project_vjp(P, cam, 0.05, T, rho, None, ge)
    assert _rel(a[0].astype(np.float64) + b[0], gp) < 1e-5 and _rel(a[1].astype(np.float64) + b[1], gc) < 1e-5
    base = np.ones_like(gc)
    assert _same_bits(KP.project_vjp(P, cam, 0.05, T, rho, guv, ge, base_camera=base)[1], base + gc)


# ---------------------------------------------------------------------------------------------------- 2. the table builder
REFUSALS = {
    "L_zero": (b"L must be in [1, 65535]", lambda r: dict(r, L=0)),
    "L_big": (b"L must be in [1, 65535]", lambda r: dict(r, L=65536)),
    "first_not_zero": (b"row_ptr[0] must be 0", lambda r: dict(r, row_ptr=r["row_ptr"] + 1)),
    "decreasing": (b"row_ptr must be non-decreasing", lambda r: dict(r, row_ptr=np.where(np.arange(len(r["row_ptr"])) == 4, 0, r["row_ptr"]))),
    "col_negative": (b"a column is outside [0, V + 24)", lambda r: dict(r, col=np.where(np.arange(len(r["col"])) == 5, -1, r["col"]))),
    "col_high": (b"a column is outside [0, V + 24)", lambda r: dict(r, col=np.where(np.arange(len(r["col"])) == 5, r["S"], r["col"]))),
    "val_inf": (b"a val is not finite", lambda r: dict(r, val=np.where(np.arange(len(r["val"])) == 7, np.inf, r["val"]).astype(np.float32))),
    "val_nan": (b"a val is not finite", lambda r: dict(r, val=np.where(np.arange(len(r["val"])) == 0, np.nan, r["val"]).astype(np.float32))),
    # an nnz the arrays do not hold: refused before col or val is read (the sanitizer watches)
    "nnz_beyond_int32": (b"nnz beyond int32 indexing", lambda r: dict(r, L=1, row_ptr=np.array([0, 2 ** 31], np.int64))),
}


def _regressor(reg, S):
    return dict(L=len(reg[0]) - 1, S=S, row_ptr=reg[0], col=reg[1], val=reg[2])


def _cases():
    from smplpp_amd import model_io

    synth = model_io.synthetic_model()
    out = {"eleven": _regressor(KP.regressor_11(97), 121), "fiftythree": _regressor(KP.regressor_53(synth), 6890 + 24),
           "one_empty_row": _regressor(KP.csr([[]]), 30), "L_max": _regressor(KP.csr([[(l % 40, 0.5)] for l in range(65535)]), 40)}
    for name, (_, edit) in REFUSALS.items():
        out[name] = edit(_regressor(KP.regressor_11(97), 121))
    return out


def write_regressor(path, r):
    """The dump program's input (tests/cpp/landmark_tables_dump.cpp)."""
    with open(path, "wb") as f:
        f.write(np.array([r["L"], r["S"], len(r["row_ptr"]), len(r["col"])], np.int64).tobytes())
        f.write(np.ascontiguousarray(r["row_ptr"], np.int64).tobytes())
        f.write(np.ascontiguousarray(r["col"], np.int64).tobytes())
        f.write(np.ascontiguousarray(r["val"], np.float32).tobytes())


def read_tables(path):
    raw, out, p = open(path, "rb").read(), {}, 0
    while p < len(raw):
        name = raw[p:p + 16].rstrip(b"\0").decode()
        es, n = (int(x) for x in np.frombuffer(raw, np.int64, 2, p + 16))
        out[name] = raw[p + 32:p + 32 + es * n]
        p += 32 + es * n
    assert p == len(raw)
    return out


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("landmark_tables") / "landmark_tables_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "landmark_tables_dump.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def tables(dump_exe, tmp_path_factory):
    """name -> (the regressor, the program's records); the program runs once per case."""
    out = {}
    for name, r in _cases().items():
        d = tmp_path_factory.mktemp(name)
        write_regressor(str(d / "reg.bin"), r)
        p = subprocess.run([dump_exe, str(d / "reg.bin"), str(d / "tables.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=120)
        assert p.returncode == 0 and not p.stdout, (name, p.stdout)  # a sanitizer report is a failure
        out[name] = (r, read_tables(str(d / "tables.bin")))
    return out


def test_header_is_plain_cpp():
    path = os.path.join(ROOT, "smplpp_amd", "csrc", "landmark_tables.h")
    src = open(path).read()
    assert "hip_runtime" not in src and "__device__" not in src and "__global__" not in src
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True,
                   input='#include "%s"\n' % path)


@pytest.mark.parametrize("name", ["eleven", "fiftythree", "one_empty_row", "L_max"])
def test_tables_equal_the_numpy_construction(tables, name):
    r, t = tables[name]
    assert "refusal" not in t
    L, S, nnz = r["L"], r["S"], len(r["col"])
    assert np.frombuffer(t["dims"], np.int64).tolist() == [L, nnz, S]
    assert np.array_equal(np.frombuffer(t["rowPtr"], np.int32), r["row_ptr"])
    assert np.array_equal(np.frombuffer(t["col"], np.int32), r["col"]) and t["val"] == r["val"].tobytes()
    rows = np.repeat(np.arange(L), np.diff(r["row_ptr"]))
    order = np.argsort(r["col"], kind="stable")  # per source, ascending e
    assert np.array_equal(np.frombuffer(t["srcPtr"], np.int32), np.concatenate([[0], np.cumsum(np.bincount(r["col"], minlength=S))]))
    assert np.array_equal(np.frombuffer(t["srcRow"], np.int32), rows[order]) and t["srcVal"] == r["val"][order].tobytes()


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(tables, name):
    _, t = tables[name]
    assert list(t) == ["refusal"] and t["refusal"] == REFUSALS[name][0]
