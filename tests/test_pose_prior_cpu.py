"""The pose priors without a GPU.  (1) The five entry points are declared, exported and bound, and a call without a device fails
loudly.  (2) The float32 restatement of smplpp_pose_prior and smplpp_pose_prior_vjp (tests/pose_prior_oracle.py), the one the GPU
tests hold the library to bit for bit, against the float64 definitions: the energy within 1e-6 relative, the same component on every
frame of the fixtures (so that a near-tie in a fixture is caught here and not on the GPU), the backward within the project's bar,
max(4 x the error of fp32 autograd of the same graph, 1e-5 relative).  (3) The host table builder of smplpp_pose_prior_create
(smplpp_amd/csrc/pose_prior_tables.h) as a stand-alone program, tests/cpp/pose_prior_tables_dump.cpp, built with the address and
undefined-behaviour sanitizers: its tables equal numpy's, and each refusal returns its reason without a sanitizer report."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_prior_oracle as PO  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["smplpp_pose_prior", "smplpp_pose_prior_create", "smplpp_pose_prior_destroy", "smplpp_pose_prior_info", "smplpp_pose_prior_vjp"]
FIXTURES = [(8, 69), (32, 128), (3, 9)]


# ---------------------------------------------------------------------------------------------------- 1. the ABI
def test_entry_points_are_declared_exported_and_bound():
    import __graft_entry__ as g

    g.build()
    from smplpp_amd import _lib

    L = _lib.load()
    declared = _lib.declared_symbols()
    for name, nargs in zip(NAMES, (10, 10, 1, 4, 12)):
        assert name in declared and hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == nargs, name


def test_a_call_without_a_device_fails_loudly():
    from smplpp_amd import _lib
    from smplpp_amd.priors import PosePrior

    p = PO.prior(3, 9, 1)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.SmplppError):
            PosePrior("cuda:0", p["mean"], p["mat"], p["offset"], p["lo"], p["hi"], p["weight"])
    with pytest.raises(_lib.SmplppError):  # refused on the host, with or without a device
        PosePrior("cuda:0", p["mean"], p["mat"], np.array([0, np.nan, 0], np.float32))
    with pytest.raises(_lib.SmplppError):
        PosePrior("cpu", p["mean"], p["mat"], p["offset"])


def test_python_tables_and_limits():
    from smplpp_amd import priors

    gmm = PO.synthetic_gmm(4, 11, 2)
    for a, b in zip(priors.gmm_tables(*gmm), PO.gmm_tables(*gmm)):
        assert a.dtype == np.float32 and _same_bits(a, b)
    mean, mat, offset = priors.gmm_tables(*gmm)
    assert offset.min() == 0
    x = np.random.default_rng(3).normal(0, 0.3, 11)
    for m in range(4):  # |mat d|^2 + offset is the negative log of w N(x; mean, Sigma), up to one constant for all components
        d = x - gmm[0][m]
        nll = 0.5 * d @ np.linalg.solve(gmm[1][m], d) + 0.5 * np.linalg.slogdet(gmm[1][m])[1] - np.log(gmm[2][m])
        e = ((mat[m].astype(np.float64) @ (x - mean[m])) ** 2).sum() + offset[m]
        if m == 0:
            const = nll - e
        assert abs((nll - e) - const) < 1e-4 * abs(nll)
    lo, hi, w = priors.smplify_limits(2.0)
    assert lo.shape == hi.shape == w.shape == (69,) and np.nonzero(w)[0].tolist() == [9, 12, 52, 55] and (w[w != 0] == 2).all()
    assert hi[52] == 0 and lo[52] == -np.inf and all(lo[k] == 0 and hi[k] == np.inf for k in (9, 12, 55))


# ---------------------------------------------------------------------------------------------------- 2. the restatement
def _bar(got, want64, fp32, what):
    err, ref = _rel(got, want64), _rel(fp32, want64)
    print("%s: restatement rel %.3g, fp32 autograd rel %.3g" % (what, err, ref))
    assert np.abs(want64).max() > 0 and err <= max(4 * ref, 1e-5), (what, err, ref)


@pytest.mark.parametrize("M,D", FIXTURES)
def test_restatement_against_float64(M, D):
    n = 65
    p = PO.prior(M, D, seed=M + D)
    X = PO.poses(n, D, seed=D)
    rng = np.random.default_rng(M)
    ge, gr, gl = rng.normal(size=n).astype(np.float32), rng.normal(size=(n, D)).astype(np.float32), rng.normal(size=n).astype(np.float32)

    def ref(dtype):
        t = PO.tensors(p, dtype)
        x = torch.tensor(X, dtype=dtype, requires_grad=True)
        e_all, _ = PO.mixture_t(t, x)
        e, y, comp = PO.energy_t(t, x)
        lim = PO.limit_t(t, x)
        ((e * torch.tensor(ge, dtype=dtype)).sum() + (y * torch.tensor(gr, dtype=dtype)).sum() + (lim * torch.tensor(gl, dtype=dtype)).sum()).backward()
        return dict(e_all=e_all.detach().double().numpy(), energy=e.detach().double().numpy(), residual=y.detach().double().numpy(),
                    component=comp.numpy(), limit=lim.detach().double().numpy(), grad=x.grad.double().numpy())

    r64, r32 = ref(torch.float64), ref(torch.float32)
    got = PO.forward(p, X)
    assert got["energy"].dtype == got["residual"].dtype == got["limit_energy"].dtype == np.float32 and got["component"].dtype == np.int64
    rel = np.abs(got["energy"] - r64["energy"]) / np.abs(r64["energy"])
    two = np.sort(r64["e_all"], 1)[:, :2]
    print("(M, D) = (%d, %d): energy rel max %.3g; smallest relative gap between the best two components %.3g; components used %s" %
          (M, D, rel.max(), ((two[:, 1] - two[:, 0]) / two[:, 0]).min(), np.unique(got["component"]).tolist()))
    assert rel.max() <= 1e-6
    assert np.array_equal(got["component"], r64["component"])
    assert _rel(got["residual"], r64["residual"]) <= 1e-6 and _rel(got["limit_energy"], r64["limit"]) <= 1e-6
    assert (got["limit_energy"] > 0).mean() > 0.5 and len(np.unique(got["component"])) > 1
    g = PO.backward(p, X, got["component"], ge, gr, gl)
    _bar(g, r64["grad"], r32["grad"], "grad_pose")
    # the component chosen in the backward; each part alone; accumulate adds the finished element
    assert _same_bits(PO.backward(p, X, None, ge, gr, gl), g)
    parts = [PO.backward(p, X, got["component"], ge, None, None), PO.backward(p, X, got["component"], None, gr, None), PO.backward(p, X, None, None, None, gl)]
    assert _rel(sum(x.astype(np.float64) for x in parts), g) < 1e-5
    base = rng.normal(size=(n, D)).astype(np.float32)
    assert _same_bits(PO.backward(p, X, got["component"], ge, gr, gl, base=base), base + g)


def test_restatement_edge_cases():
    p = PO.prior(3, 9, 4)
    p["mean"][2], p["mat"][2], p["offset"][2] = p["mean"][1], p["mat"][1], p["offset"][1]  # two identical components
    X = PO.poses(6, 9, 5)
    X[:3] = p["mean"][1] + np.float32(0.01) * X[:3]  # close to the twin centre: the lower index wins
    X[4, 3] = np.nan
    X[5, 5], X[5, 6] = p["hi"][5], p["lo"][6]  # exactly at a limit
    r = PO.forward(p, X)
    assert (r["component"][:3] == 1).all() and r["component"][4] == 0 and np.isnan(r["energy"][4]) and r["limit_energy"][4] >= 0
    v, _ = PO._limit(p, X)
    assert v[5, 5] == 0 and v[5, 6] == 0 and v[4, 3] == 0 and (v[:, 0] == 0).all() and (v >= 0).all()
    ge, gl = np.ones(6, np.float32), np.ones(6, np.float32)
    ge[4] = gl[4] = 0
    g = PO.backward(p, X, None, ge, None, gl)
    assert (g[4] == 0).all() and not np.signbit(g[4]).any() and np.isfinite(g).all()
    assert (PO.backward(p, X, np.full(6, 3), ge, None, None) == 0).all()  # outside [0, M): nothing


# ---------------------------------------------------------------------------------------------------- 3. the table builder
def _file(p, M=None, D=None, flags=None):
    has_mix, has_lim = len(p["offset"]) > 0, p["lo"] is not None
    return dict(M=len(p["offset"]) if M is None else M, D=p["mean"].shape[1] if D is None else D,
                flags=[int(has_mix)] + [int(has_lim)] * 3 if flags is None else flags, prior=p)


def _edit(key, idx, value):
    def f(p):
        q = {k: None if v is None else v.copy() for k, v in p.items()}
        q[key].reshape(-1)[idx] = value
        return _file(q)
    return f


def _swap(p):
    q = {k: None if v is None else v.copy() for k, v in p.items()}
    q["lo"][3], q["hi"][3] = 0.5, 0.25
    return _file(q)


REFUSALS = {
    "M_negative": (b"M must be in [0, 32]", lambda p: _file(p, M=-1)),
    "M_big": (b"M must be in [0, 32]", lambda p: _file(p, M=33)),
    "D_zero": (b"D must be in [1, 128]", lambda p: _file(p, D=0)),
    "D_big": (b"D must be in [1, 128]", lambda p: _file(p, D=129)),
    "some_limits": (b"lo, hi and limit_weight must all be given or all be NULL", lambda p: _file(p, flags=[1, 1, 0, 1])),
    "nothing": (b"a prior without components needs limits", lambda p: _file(PO.prior(0, 9, 1, limits=False))),
    "no_mean": (b"mean, mat or offset is NULL", lambda p: _file(p, flags=[0, 1, 1, 1])),
    "mean_nan": (b"a mean is not finite", _edit("mean", 4, np.nan)),
    "mat_inf": (b"a mat is not finite", _edit("mat", 80, np.inf)),
    "offset_inf": (b"an offset is not finite", _edit("offset", 2, -np.inf)),
    "lo_nan": (b"a limit is NaN", _edit("lo", 1, np.nan)),
    "hi_nan": (b"a limit is NaN", _edit("hi", 8, np.nan)),
    "lo_above_hi": (b"lo must not exceed hi", _swap),
    "weight_negative": (b"a limit_weight is negative or not finite", _edit("weight", 0, -1.0)),
    "weight_inf": (b"a limit_weight is negative or not finite", _edit("weight", 5, np.inf)),
}
GOOD = {"m3_d9": lambda: _file(PO.prior(3, 9, 1)), "m8_d69_no_limits": lambda: _file(PO.prior(8, 69, 2, limits=False)),
        "limits_only": lambda: _file(PO.prior(0, 7, 3)), "m32_d128": lambda: _file(PO.prior(32, 128, 4)), "m1_d1": lambda: _file(PO.prior(1, 1, 5))}


def write_prior(path, c):
    """The dump program's input (tests/cpp/pose_prior_tables_dump.cpp)."""
    p, fl = c["prior"], c["flags"]
    sane = 0 <= c["M"] <= 32 and 1 <= c["D"] <= 128
    with open(path, "wb") as f:
        f.write(np.array([c["M"], c["D"]] + fl, np.int64).tobytes())
        if sane and fl[0]:
            for k in ("mean", "mat", "offset"):
                f.write(np.ascontiguousarray(p[k], np.float32).tobytes())
        for k, on in zip(("lo", "hi", "weight"), fl[1:]):
            if sane and on:
                f.write(np.ascontiguousarray(p[k], np.float32).tobytes())


def read_tables(path):
    raw, out, q = open(path, "rb").read(), {}, 0
    while q < len(raw):
        name = raw[q:q + 16].rstrip(b"\0").decode()
        es, n = (int(x) for x in np.frombuffer(raw, np.int64, 2, q + 16))
        out[name] = raw[q + 32:q + 32 + es * n]
        q += 32 + es * n
    assert q == len(raw)
    return out


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pose_prior_tables") / "pose_prior_tables_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "pose_prior_tables_dump.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def tables(dump_exe, tmp_path_factory):
    """name -> (the case, the program's records); the program runs once per case."""
    cases = {name: make() for name, make in GOOD.items()}
    cases.update({name: edit(PO.prior(3, 9, 1)) for name, (_, edit) in REFUSALS.items()})
    out = {}
    for name, c in cases.items():
        d = tmp_path_factory.mktemp(name)
        write_prior(str(d / "prior.bin"), c)
        r = subprocess.run([dump_exe, str(d / "prior.bin"), str(d / "tables.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=120)
        assert r.returncode == 0 and not r.stdout, (name, r.stdout)  # a sanitizer report is a failure
        out[name] = (c, read_tables(str(d / "tables.bin")))
    return out


def test_header_is_plain_cpp():
    path = os.path.join(ROOT, "smplpp_amd", "csrc", "pose_prior_tables.h")
    src = open(path).read()
    assert "hip_runtime" not in src and "__device__" not in src and "__global__" not in src
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True,
                   input='#include "%s"\n' % path)


@pytest.mark.parametrize("name", list(GOOD))
def test_tables_equal_numpy(tables, name):
    c, t = tables[name]
    assert "refusal" not in t
    p, M, D = c["prior"], c["M"], c["D"]
    lim = p["lo"] is not None
    assert np.frombuffer(t["dims"], np.int64).tolist() == [M, D, int(lim)]
    for k in ("mean", "mat", "offset"):
        assert t[k] == p[k].tobytes(), k
    assert t["matT"] == np.ascontiguousarray(p["mat"].transpose(0, 2, 1)).tobytes()
    for k in ("lo", "hi", "weight"):
        assert t[k] == (p[k].tobytes() if lim else b""), k


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(tables, name):
    _, t = tables[name]
    assert list(t) == ["refusal"] and t["refusal"] == REFUSALS[name][0]
