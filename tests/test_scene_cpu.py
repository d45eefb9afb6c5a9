"""The scene term without a GPU: the numpy restatement of smplpp_volume_sample / smplpp_scene_term and its backward
(tests/scene_oracle.py) against float64 autograd of the definition; its float32 forward within a bound derived from the unit roundoff; an
affine field reproduced by the interpolation; the seed of the GPU file's gradient chain; and the host plan
(smplpp_amd/csrc/volume_plan.h) as a stand-alone program, tests/cpp/volume_plan_dump.cpp, built with the address and undefined-behaviour
sanitizers: its index functions equal the Python statement of the two layouts, and each refusal returns its reason without a sanitizer
report."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_oracle as SC  # noqa: E402
from distance_cases import _rel  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["smplpp_volume_create", "smplpp_volume_set", "smplpp_volume_info", "smplpp_volume_destroy", "smplpp_volume_sample", "smplpp_scene_term",
         "smplpp_scene_term_vjp"]
U = 2.0 ** -24  # the unit roundoff of float32
ROT = np.array([[0.36, 0.48, -0.8, 0.3], [-0.8, 0.6, 0.0, -0.2], [0.48, 0.64, 0.6, 0.1]])  # a rotation and a translation
AFFINE = np.array([[1.1, 0.2, -0.1, 0.3], [0.05, 0.9, 0.3, -0.2], [-0.2, 0.1, 1.3, 0.1]])  # not orthonormal
XFS = {"none": None, "rotation": ROT, "affine": AFFINE}
G, ORIGIN, H = (5, 4, 3), (-0.3, 0.2, 0.1), (0.11, 0.07, 0.13)


def test_header_declares_the_calls():
    from smplpp_amd import _lib

    assert set(NAMES) <= set(_lib.declared_symbols())
    import smplpp_amd.scene  # noqa: F401


def draw_points(V, n, K, seed, s_min=SC.S_MIN):
    """[n,K,3] float64 world points with every fractional grid coordinate in [0.05, 0.95] and |s| > s_min (points that miss are drawn
    again), so that float32 and float64 agree on the cell and on the sign."""
    rng = np.random.default_rng(seed)
    Gz, Gy, Gx = V["v"].shape
    V64 = SC.as_dtype(V, np.float64)
    out = np.zeros((n * K, 3))
    todo = np.arange(n * K)
    while len(todo):
        cell = np.stack([rng.integers(0, g - 1, len(todo)) for g in (Gx, Gy, Gz)], -1)
        p = V64["o"] + (cell + rng.uniform(0.05, 0.95, (len(todo), 3))) * V64["h"]
        if V64["xf"] is not None:
            p = np.linalg.solve(V64["xf"][:, :3], (p - V64["xf"][:, 3]).T).T
        out[todo] = p
        p32 = out[todo].astype(np.float32).astype(np.float64)  # the test's inputs are float32 values
        s = SC.sample(V64, p32)[0]
        todo = todo[(np.abs(s) <= s_min) | (SC.cell_margin(V, p32) < 0.04)]
    return out.astype(np.float32).astype(np.float64).reshape(n, K, 3)


# ---------------------------------------------------------------------------------------------------- 1. the restatement against float64
@pytest.mark.parametrize("xf", list(XFS))
@pytest.mark.parametrize("rho", [0.0, 0.05])
def test_restatement_against_float64(xf, rho):
    n, K = 3, 40
    V = SC.volume(SC.random_field(G, seed=4), ORIGIN, H, XFS[xf], np.float64)
    P = draw_points(V, n, K, seed=len(xf))
    rng = np.random.default_rng(5)
    wp, wc = rng.uniform(0.5, 2.0, K), rng.uniform(0.5, 2.0, K)
    wp[3], wc[5], wp[7], wc[7] = 0, 0, 0, 0
    ge, gpe, gv = rng.normal(size=n), rng.normal(size=(n, K)), rng.normal(size=(n, K))
    X = torch.tensor(P, requires_grad=True)
    e = SC.energy_t(V, X, wp, wc, rho)
    s = SC.sample_t(V, X)
    ((e.sum(1) * torch.tensor(ge)).sum() + (e * torch.tensor(gpe)).sum() + (s * torch.tensor(gv)).sum()).backward()
    energy, pe, value, valid = SC.term(V, P, wp, wc, rho)
    got = SC.term_vjp(V, P, wp, wc, rho, ge, gpe, gv, np.zeros((n, K, 3)), 0)
    print("float64 restatement: value rel %.3g, energy rel %.3g, backward rel %.3g" %
          (_rel(value, s.detach().numpy()), _rel(pe, e.detach().numpy()), _rel(got, X.grad.numpy())))
    assert valid.all() and (value < 0).any() and (value > 0).any() and np.abs(X.grad.numpy()).max() > 0
    assert _rel(value, s.detach().numpy()) <= 1e-9 and _rel(pe, e.detach().numpy()) <= 1e-9 and _rel(energy, e.detach().numpy().sum(1)) <= 1e-9
    assert _rel(got, X.grad.numpy()) <= 1e-9
    # the sampled gradient alone is the derivative of the value
    X2 = torch.tensor(P, requires_grad=True)
    SC.sample_t(V, X2).sum().backward()
    assert _rel(SC.sample(V, P)[1], X2.grad.numpy()) <= 1e-9
    # a point with both weights 0 has energy +0, and without a cotangent of the value its gradient is +0
    assert (pe[:, 7] == 0).all() and not np.signbit(pe[:, 7]).any()
    assert (SC.term_vjp(V, P, wp, wc, rho, ge, gpe, None, np.zeros((n, K, 3)), 0)[:, 7] == 0).all()


def _grid_coordinate_error(V64, P):
    """dg [..., 3]: a bound on the float32 error of the grid coordinates of the float32 points P.  The transform's three products and
    three sums are within 4 u M_a, M_a = |R_a0 x| + |R_a1 y| + |R_a2 z| + |t_a| (none without a transform); the difference from the
    origin adds u |p' - o|, the division u |g|: dg_a = dp'_a / h_a + 2 u |g_a|.  f_a = g_a - i_a is exact."""
    if V64["xf"] is not None:
        R, t = V64["xf"][:, :3], V64["xf"][:, 3]
        q = P @ R.T + t
        dq = 4 * U * (np.abs(P) @ np.abs(R).T + np.abs(t))
    else:
        q, dq = P, np.zeros_like(P)
    g = (q - V64["o"]) / V64["h"]
    return dq / V64["h"] + 2 * U * np.abs(g)


def _field_size(V64):
    """(A, D [3]): the largest |node| and the largest |difference of two neighbouring nodes| along x, y, z."""
    v = V64["v"]
    return np.abs(v).max(), np.array([np.abs(np.diff(v, axis=2)).max(), np.abs(np.diff(v, axis=1)).max(), np.abs(np.diff(v, axis=0)).max()])


@pytest.mark.parametrize("xf", list(XFS))
@pytest.mark.parametrize("rho", [0.0, 0.05])
def test_float32_forward_within_roundoff(xf, rho):
    """float32 against float64 on the same float32 inputs.  With u = 2^-24: the value is a convex combination of the cell's nodes whose
    slope along axis a is at most D_a, so the error dg of the grid coordinates moves it by at most sum_a dg_a D_a; each of the three
    levels of lerps a + f (b - a) rounds three times on magnitudes of at most 2 A, 2 A and A (A the largest |node|): 5 u A a level, 16 u A
    covers the three.  q = s s then has dq <= 2 |s| ds + ds^2 + u q; e_pen = wp q and e_con = wc q (or wc p2 q / (p2 + q), whose slope
    in q is at most wc) add a few roundings of their own, 8 u e covers them; the 1024-partial sum of K <= 1024 terms adds at most 11 u
    sum_k e."""
    n, K = 3, 40
    V32 = SC.volume(SC.random_field(G, seed=6), ORIGIN, H, XFS[xf])
    V64 = SC.as_dtype(V32, np.float64)
    P = draw_points(V32, n, K, seed=10 + len(xf))
    rng = np.random.default_rng(7)
    wp, wc = rng.uniform(0.5, 2.0, K).astype(np.float32), rng.uniform(0.5, 2.0, K).astype(np.float32)
    e32, pe32, s32, ok32 = SC.term(V32, P.astype(np.float32), wp, wc, rho)
    e64, pe64, s64, ok64 = SC.term(V64, P, wp.astype(np.float64), wc.astype(np.float64), float(np.float32(rho)))
    A, D = _field_size(V64)
    ds = _grid_coordinate_error(V64, P) @ D + 16 * U * A
    assert s32.dtype == np.float32 and ok32.all() and ok64.all()
    assert (np.abs(s32 - s64) <= ds).all(), (np.abs(s32 - s64) / ds).max()
    assert (np.sign(s32) == np.sign(s64)).all()
    dq = 2 * np.abs(s64) * ds + ds * ds + U * s64 * s64
    bound = (np.where(s64 < 0, wp[None], 0) + wc[None]) * dq + 8 * U * np.abs(pe64)
    assert (np.abs(pe32 - pe64) <= bound).all(), (np.abs(pe32 - pe64) / bound).max()
    assert (np.abs(e32 - e64) <= bound.sum(1) + 11 * U * pe64.sum(1)).all()
    print("float32 forward: value error / bound %.3g, energy error / bound %.3g" % ((np.abs(s32 - s64) / ds).max(), (np.abs(pe32 - pe64) / bound).max()))


@pytest.mark.parametrize("xf", list(XFS))
def test_plane_is_reproduced(xf):
    """Trilinear interpolation reproduces an affine field exactly in real arithmetic: the float32 sample of the plane n . p' - c is the
    plane, and its gradient is n pulled to world coordinates.  The bound on the value is the one above plus u A for the rounding of the
    nodes to float32.  The gradient's components in volume coordinates are differences of such values over one cell, divided by h_a: the
    x difference of two nodes is within 2 u A of n_x h_x before and u |n_x h_x| after the subtraction, and its two lerps add 5 u of it
    each; the y and z components subtract lerped values that are within 6 u A and 11 u A of the plane, so 24 u A covers every numerator,
    12 u |n_a h_a| its own roundings, and the error of the grid coordinates enters through the slopes only: 2 sum_b dg_b D_b.  The
    division adds u |n_a|.  The pull to world coordinates is three products and two sums on |R_ba g_b|: 3 u of their sum."""
    n, K = 2, 60
    Gp, o, h = (7, 6, 5), (-0.4, -0.3, -0.2), (0.13, 0.11, 0.17)
    values, nrm = SC.plane(Gp, o, h, (0.3, -0.5, 0.8), 0.07)
    V32 = SC.volume(values, o, h, XFS[xf])
    V64 = SC.as_dtype(V32, np.float64)
    P = draw_points(V32, n, K, seed=3, s_min=0.0)
    s32, g32, ok = SC.sample(V32, P.astype(np.float32))
    q = P if V64["xf"] is None else P @ V64["xf"][:, :3].T + V64["xf"][:, 3]
    want = q @ nrm - 0.07
    A, D = _field_size(V64)
    dg = _grid_coordinate_error(V64, P)
    ds = dg @ D + 17 * U * A
    assert ok.all() and (np.abs(s32 - want) <= ds).all(), (np.abs(s32 - want) / ds).max()
    hh = V64["h"]
    dvol = (24 * U * A + 12 * U * np.abs(nrm * hh) + 2 * (dg @ D)[..., None]) / hh + U * np.abs(nrm)  # [n,K,3]
    if V64["xf"] is None:
        gwant, dworld = nrm, dvol
    else:
        R = V64["xf"][:, :3]
        gwant = R.T @ nrm
        dworld = dvol @ np.abs(R) + 3 * U * (np.abs(nrm) @ np.abs(R))
    assert (np.abs(g32 - gwant) <= dworld).all(), (np.abs(g32 - gwant) / dworld).max()
    print("plane: value error / bound %.3g, gradient error / bound %.3g" % ((np.abs(s32 - want) / ds).max(), (np.abs(g32 - gwant) / dworld).max()))


def test_rule_at_the_edges():
    """Nodes, far faces, one ulp outside, points that are not finite, a NaN node, in the restatement itself."""
    V = SC.volume(SC.random_field(G, seed=8), (0.0, 0.0, 0.0), (0.125, 0.25, 0.5))  # (the grid coordinates of the points below are exact)
    o, h = V["o"].astype(np.float64), V["h"].astype(np.float64)
    nodes = (SC.node_positions(G, o, h)).astype(np.float32)
    s, _, ok = SC.sample(V, nodes)
    # f = 0 returns the node itself; on a far face f = 1, and a + 1 (b - a) is b within two roundings
    assert ok.all() and np.array_equal(s[:-1, :-1, :-1], V["v"][:-1, :-1, :-1]) and np.allclose(s, V["v"], rtol=0, atol=4 * U * np.abs(V["v"]).max())
    far = nodes[-1, -1, -1]
    for a in range(3):
        out = far.copy()
        out[a] = np.nextafter(out[a], np.float32(np.inf))
        assert SC.sample(V, out)[2] == 0 and SC.sample(V, far)[2] == 1
        out = nodes[0, 0, 0].copy()
        out[a] = np.nextafter(out[a], np.float32(-np.inf))
        assert SC.sample(V, out)[2] == 0
    for bad in (np.nan, np.inf, -np.inf):
        p = nodes[1, 1, 1].copy()
        p[1] = bad
        s, g, ok = SC.sample(V, p)
        assert ok == 0 and s == 0 and (g == 0).all()
    V["v"][1, 2, 3] = np.nan
    centres = (SC.node_positions(G, o, h)[:-1, :-1, :-1] + 0.5 * h).astype(np.float32)
    ok = SC.sample(V, centres)[2]
    touched = np.zeros_like(ok, bool)
    touched[0:2, 1:3, 2:4] = True
    assert np.array_equal(ok == 0, touched)


# ---------------------------------------------------------------------------------------------------- 2. the GPU file's chains
def test_gradient_case_keeps_enough(synth_model):
    """The seed of test_scene_gpu's gradient chain: the float64 run alone leaves out fewer than 20 % of the vertices."""
    case = SC.gradient_case(synth_model)
    skipped = 1.0 - case["keep"].all(0).mean()  # (a weight is per vertex: a vertex stays when it is clear in both frames)
    s = SC.sample(SC.as_dtype(case["V"], np.float64), case["verts64"])[0]
    print("gradient chain: %.1f %% of the vertices left out; %.1f %% inside the sphere" % (100 * skipped, 100 * (s < 0).mean()))
    assert skipped < 0.2
    assert 0.2 < (s[case["keep"]] < 0).mean() < 0.8  # both branches of the penetration term


def test_fit_case_in_float64(synth_model):
    case = SC.fit_case(synth_model)
    depth = SC.fit_float64(synth_model, case)
    print("float64 fit: largest penetration depth %.1f -> %.1f mm" % (1e3 * depth[0], 1e3 * depth[-1]))
    assert abs(depth[0] - SC.FIT_DEPTH) < 1e-6 and depth[-1] < 0.7 * depth[0]


# ---------------------------------------------------------------------------------------------------- 3. the host plan
ENV = {None: 0, "linear": 1, "cells": 2, "bricks": 3, "": 4}
GOOD = {"smallest": ((2, 2, 2), None), "unequal": ((5, 4, 3), None), "unequal_linear": ((5, 4, 3), "linear"), "unequal_cells": ((5, 4, 3), "cells"),
        "empty_env": ((33, 9, 6), ""), "body": ((128, 128, 128), None), "large": ((256, 256, 256), "cells"), "past_the_bound": ((512, 512, 512), "cells"),
        "widest": ((1024, 1024, 128), None)}
OK = dict(origin=(0.0, 1.0, -2.0), spacing=(0.1, 0.2, 0.3), xf=None, space=0, has_out=1)
# name -> (changes to OK and G, the reason)
REFUSALS = {
    "no_out": (dict(has_out=0), "no out"),
    "G_one": (dict(G=(1, 4, 4)), "Gx, Gy and Gz must be in [2, 1024]"),
    "G_zero": (dict(G=(4, 0, 4)), "Gx, Gy and Gz must be in [2, 1024]"),
    "G_negative": (dict(G=(4, 4, -3)), "Gx, Gy and Gz must be in [2, 1024]"),
    "G_wide": (dict(G=(4, 1025, 4)), "Gx, Gy and Gz must be in [2, 1024]"),
    "too_many_nodes": (dict(G=(1024, 1024, 129)), "Gx Gy Gz must not exceed 2^27"),
    "no_origin": (dict(origin=None), "origin or spacing is NULL"),
    "zero_spacing": (dict(spacing=(0.1, 0.0, 0.3)), "a spacing is not finite and positive"),
    "negative_spacing": (dict(spacing=(-0.1, 0.2, 0.3)), "a spacing is not finite and positive"),
    "nan_spacing": (dict(spacing=(0.1, 0.2, np.nan)), "a spacing is not finite and positive"),
    "inf_spacing": (dict(spacing=(np.inf, 0.2, 0.3)), "a spacing is not finite and positive"),
    "nan_origin": (dict(origin=(0.0, np.nan, 0.0)), "an origin entry is not finite"),
    "inf_origin": (dict(origin=(0.0, 0.0, -np.inf)), "an origin entry is not finite"),
    "nan_transform": (dict(xf=[1, 0, 0, 0, 0, 1, 0, np.nan, 0, 0, 1, 0]), "a world_to_volume entry is not finite"),
    "inf_transform": (dict(xf=[np.inf, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), "a world_to_volume entry is not finite"),
    "bad_space": (dict(space=2), "bad memory space"),
    "negative_space": (dict(space=-1), "bad memory space"),
    "unknown_layout": (dict(env="bricks"), "SMPLPP_VOLUME_LAYOUT must be linear or cells"),
}


def write_description(path, G_, env=None, origin=OK["origin"], spacing=OK["spacing"], xf=None, space=0, has_out=1):
    """The dump program's input (tests/cpp/volume_plan_dump.cpp)."""
    fl = np.zeros(18, np.float32)
    if origin is not None:
        fl[:3], fl[3:6] = origin, spacing
    if xf is not None:
        fl[6:] = xf
    with open(path, "wb") as f:
        f.write(np.array([G_[0], G_[1], G_[2], space, has_out, int(origin is not None), int(xf is not None), ENV[env]], np.int64).tobytes())
        f.write(fl.tobytes())


def read_records(path):
    raw, out, q = open(path, "rb").read(), {}, 0
    while q < len(raw):
        name = raw[q:q + 16].rstrip(b"\0").decode()
        es, n = np.frombuffer(raw, np.int64, 2, q + 16)
        out[name] = raw[q + 32:q + 32 + es * n]
        q += 32 + es * n
    return out


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("volume_plan") / "volume_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "volume_plan_dump.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def dumped(dump_exe, tmp_path_factory):
    """name -> the program's records; the program runs once per case."""
    cases = {name: dict(G_=g, env=env) for name, (g, env) in GOOD.items()}
    for name, (change, _) in REFUSALS.items():
        change = dict(change)
        cases[name] = dict(G_=change.pop("G", (5, 4, 3)), **change)
    out = {}
    for name, kw in cases.items():
        d = tmp_path_factory.mktemp(name)
        write_description(str(d / "in.bin"), **kw)
        r = subprocess.run([dump_exe, str(d / "in.bin"), str(d / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0 and not r.stdout, (name, r.stdout)  # a sanitizer report is a failure
        out[name] = read_records(str(d / "out.bin"))
    return out


def test_header_is_plain_cpp():
    path = os.path.join(ROOT, "smplpp_amd", "csrc", "volume_plan.h")
    src = open(path).read()
    assert "hip_runtime" not in src and "__device__" not in src and "__global__" not in src
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-"], check=True, text=True, input='#include "%s"\n' % path)


@pytest.mark.parametrize("name", list(GOOD))
def test_plan(dumped, name):
    (Gx, Gy, Gz), env = GOOD[name]
    t = dumped[name]
    assert "refusal" not in t
    layout, lin, cel, avail = np.frombuffer(t["dims"], np.int64).tolist()
    cells = (Gx - 1) * (Gy - 1) * (Gz - 1)
    assert lin == Gx * Gy * Gz and cel == 8 * cells and avail == int(32 * cells <= 2 ** 30)
    default = np.frombuffer(dumped["unequal"]["dims"], np.int64)[0]  # what a small grid gets when nothing is asked for
    want = {"linear": 0, "cells": 1}.get(env, default)
    assert layout == (want if avail else 0)
    if name == "past_the_bound":
        assert not avail and layout == 0
    if name == "large":
        assert avail and layout == 1  # 256^3: the larger of the bench's grids still has the choice
    if lin <= 4096:
        k, j, i = np.meshgrid(np.arange(Gz), np.arange(Gy), np.arange(Gx), indexing="ij")
        li = np.frombuffer(t["linear_index"], np.int64).reshape(Gz, Gy, Gx)
        assert np.array_equal(li, (k * Gy + j) * Gx + i) and np.array_equal(np.sort(li.ravel()), np.arange(lin))
        ci = np.frombuffer(t["cells_index"], np.int64).reshape(Gz - 1, Gy - 1, Gx - 1, 8)
        assert np.array_equal(np.sort(ci.ravel()), np.arange(cel))  # every float of the records is some corner of some cell, once
        assert (ci[..., 0] % 8 == 0).all() and np.array_equal(ci, ci[..., :1] + np.arange(8))  # a record is eight consecutive floats, 32-byte aligned
        # filled through the two index functions, a cell's record holds its eight nodes in the order dx + 2 dy + 4 dz
        values = np.random.default_rng(0).normal(size=lin)
        records = np.zeros(cel)
        for c in range(8):
            dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
            records[ci[..., c]] = values[li[dz:Gz - 1 + dz, dy:Gy - 1 + dy, dx:Gx - 1 + dx]]
        field = values.reshape(Gz, Gy, Gx)
        assert np.array_equal(records.reshape(Gz - 1, Gy - 1, Gx - 1, 8)[..., 5], field[1:, :-1, 1:])  # corner 5 = (1, 0, 1)


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals(dumped, name):
    assert dumped[name] == {"refusal": REFUSALS[name][1].encode()}
