"""The scene term on the MI355X (smplpp_volume_create / _set / _info / _sample, smplpp_scene_term, smplpp_scene_term_vjp): every bit
against the numpy restatement of tests/scene_oracle.py, in both storage layouts; points on nodes, on far faces, one ulp outside every
face, not finite, and in cells with a NaN node; independence of the batch, the slot, the memory space and the outputs asked for; set();
the refusals; the C++ shim; the gradient through FK against float64 autograd; and a fit that lifts a body out of a plane."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import scene_oracle as SC  # noqa: E402
from test_scene_cpu import AFFINE, ROT  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 7.0
f32 = np.float32
XFS = {"none": None, "rotation": ROT, "affine": AFFINE}
# (Gx, Gy, Gz) -> origin, spacing: unequal axes catch a swapped stride
GRIDS = {(2, 2, 2): ((0.2, -0.1, 0.3), (0.3, 0.2, 0.25)), (5, 4, 3): ((-0.3, 0.2, 0.1), (0.11, 0.07, 0.13)), (33, 9, 6): ((-1.0, -0.2, 0.4), (0.05, 0.09, 0.12))}
KS = (1, 63, 64, 65, 1024, 1025, 1030)  # the work split changes after 64 and after 1024
LAYOUTS = ("linear", "cells")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _same(a, b):
    """The same bits where neither is NaN, and NaN in the same places."""
    a, b = np.ascontiguousarray(_host(a)), np.ascontiguousarray(b)
    if a.dtype == np.uint8:
        return a.shape == b.shape and b.dtype == np.uint8 and np.array_equal(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.where(np.isnan(a), f32(0), a).tobytes() == np.where(np.isnan(b), f32(0), b).tobytes()


def _volume(V, layout=None, dev=False):
    """The library's handle for the restatement's volume V, in `layout` (None: the default)."""
    from smplpp_amd.scene import Volume

    old = os.environ.pop("SMPLPP_VOLUME_LAYOUT", None)
    if layout is not None:
        os.environ["SMPLPP_VOLUME_LAYOUT"] = layout
    try:
        vol = Volume("cuda:0", _dev(V["v"]) if dev else V["v"], V["o"], V["h"], V["xf"])
    finally:
        os.environ.pop("SMPLPP_VOLUME_LAYOUT", None)
        if old is not None:
            os.environ["SMPLPP_VOLUME_LAYOUT"] = old
    assert layout is None or vol.layout == layout
    return vol


def _field(G, xf, seed, nan_node=True):
    o, h = GRIDS[G]
    v = SC.random_field(G, seed)
    if nan_node and min(G) > 2:
        v[0, 0, 3] = np.nan  # node (3, 0, 0): it touches the cells (2, 0, 0) and (3, 0, 0), not the first cell's neighbourhood nor the last cell
    return SC.volume(v, o, h, XFS[xf])


def _to_world(V, q):
    """World points (float32) that the transform of V sends to about the volume points q (float64)."""
    if V["xf"] is not None:
        xf = V["xf"].astype(np.float64)
        q = np.linalg.solve(xf[:, :3], (q - xf[:, 3]).T).T
    return q.astype(f32)


def _specials(V):
    """[S,3] float32 world points: every node of the first and the last cell (far faces: f = 1), one ulp outside each of the six faces,
    points that are not finite, the centre of a cell that touches the NaN node (when there is one) and of one that does not."""
    Gz, Gy, Gx = V["v"].shape
    o, h = V["o"].astype(np.float64), V["h"].astype(np.float64)
    top = np.array([Gx - 1, Gy - 1, Gz - 1])
    corners = np.array(list(itertools.product((0, 1), repeat=3)))
    g = [corners, top - corners, (top - 1) + 0.25 + 0.5 * corners]
    pts = [_to_world(V, o + np.concatenate(g) * h)]
    mid = (o + 0.5 * top * h).astype(f32)
    lo, hi = o.astype(f32), (V["o"] + top.astype(f32) * V["h"]).astype(f32)
    if V["xf"] is None:  # (with a transform "one ulp" of the world point is not one ulp of the volume point: the random points cover it)
        for a in range(3):
            for face, way in ((lo, -np.inf), (hi, np.inf)):
                p = mid.copy()
                p[a] = face[a]
                q = p.copy()
                q[a] = np.nextafter(p[a], f32(way))
                pts.append(np.stack([p, q]))
    bad = np.repeat(mid[None], 5, 0)
    bad[0, 0], bad[1, 1], bad[2, 2], bad[3, 0], bad[4] = np.nan, np.inf, -np.inf, -np.inf, np.nan
    pts.append(bad)
    if min(V["v"].shape) > 2:
        pts.append(_to_world(V, o + np.array([[2.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0.5, 0.5, 0.5], [1.5, 0.5, 0.5]]) * h))
    return np.concatenate(pts)


def _points(V, n, K, seed):
    """[n,K,3] float32: random points over the grid and a tenth of its size beyond it, with the special points spread among them."""
    rng = np.random.default_rng(seed)
    Gz, Gy, Gx = V["v"].shape
    top = np.array([Gx - 1, Gy - 1, Gz - 1])
    g = rng.uniform(-0.1, 1.1, (n * K, 3)) * top
    P = _to_world(V, V["o"].astype(np.float64) + g * V["h"].astype(np.float64))
    S = _specials(V)
    at = (np.arange(len(S)) * 7 + seed) % (n * K)
    P[at] = S
    return P.reshape(n, K, 3)


def _weights(K, seed):
    rng = np.random.default_rng(seed)
    wp, wc = rng.uniform(0.25, 2.0, K).astype(f32), rng.uniform(0.25, 2.0, K).astype(f32)
    wp[::3], wc[1::3], wc[::6] = 0, 0, 0  # (every sixth point has both weights zero)
    return wp, wc


COTANGENTS = [c for c in itertools.product((False, True), repeat=3) if any(c)]


def _check_all(vol, V, P, wp, wc, rho, seed, case):
    """Every output of the three calls on device tensors against the restatement, every combination of cotangents, storing and adding."""
    n, K = P.shape[:2]
    dP, dwp, dwc = _dev(P), _dev(wp), _dev(wc)
    value, grad, valid = SC.sample(V, P)
    r = vol.sample(dP)
    assert _same(r["value"], value) and _same(r["gradient"], grad) and _same(r["valid"], valid), case
    energy, pe, tv, tok = SC.term(V, P, wp, wc, rho)
    r = vol.term(dP, dwp, dwc, rho)
    assert _same(r["energy"], energy) and _same(r["point_energy"], pe) and _same(r["value"], tv) and _same(r["valid"], tok), case
    assert not np.isnan(energy).any()
    rng = np.random.default_rng(seed)
    ge, gpe, gv = rng.normal(size=n).astype(f32), rng.normal(size=(n, K)).astype(f32), rng.normal(size=(n, K)).astype(f32)
    gpe[:, ::5] = 0
    for he, hp, hv in COTANGENTS:
        a, b, c = ge if he else None, gpe if hp else None, gv if hv else None
        want = SC.term_vjp(V, P, wp, wc, rho, a, b, c, np.full((n, K, 3), FILL, f32), 0)
        got = vol.termBackward(dP, dwp, dwc, rho, _dev(a), _dev(b), _dev(c))
        assert _same(got, want), (case, he, hp, hv)
        want2 = SC.term_vjp(V, P, wp, wc, rho, a, b, c, want.copy(), 1)
        assert vol.termBackward(dP, dwp, dwc, rho, _dev(a), _dev(b), _dev(c), out=got) is got and _same(got, want2), (case, he, hp, hv)
    return dict(value=value, gradient=grad, valid=valid, energy=energy, point_energy=pe)


# ---------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("xf", list(XFS))
@pytest.mark.parametrize("G", list(GRIDS), ids=lambda g: "x".join(map(str, g)))
def test_bits(G, xf, layout):
    """All three calls for every K at which the work split changes, n = 1 and 3, rho = 0 and 0.05, weights absent and given with zeros."""
    V = _field(G, xf, seed=sum(G))
    vol = _volume(V, layout)
    info = vol.info()
    assert info["G"] == G and info["layout"] == layout and _same(info["origin"], V["o"]) and _same(info["spacing"], V["h"])
    assert _same(info["world_to_volume"], np.eye(3, 4, dtype=f32) if V["xf"] is None else V["xf"])
    for i, (K, n) in enumerate(itertools.product(KS, (1, 3))):
        P = _points(V, n, K, seed=i)
        rho = (0.0, 0.05)[(i + n) % 2]
        for wp, wc in ((None, None), _weights(K, i)):
            out = _check_all(vol, V, P, wp, wc, rho, 100 + i, (G, xf, layout, K, n, rho, wp is not None))
        # the frame energy alone (the kernels with the sum) and the per-point outputs alone (a thread per point) give the same bits
        wp, wc = _weights(K, i)
        energy, pe, _, _ = SC.term(V, P, wp, wc, rho)
        assert _same(vol.term(_dev(P), _dev(wp), _dev(wc), rho, want=("energy",))["energy"], energy)
        assert _same(vol.term(_dev(P), _dev(wp), _dev(wc), rho, want=("point_energy",))["point_energy"], pe)
    assert (out["valid"] == 0).any() and (out["valid"] == 1).any()


@pytest.mark.parametrize("xf", list(XFS))
@pytest.mark.parametrize("G", list(GRIDS), ids=lambda g: "x".join(map(str, g)))
def test_special_points(G, xf):
    """The special points alone, in both layouts with identical bits: nodes give the node's value, far faces belong to the last cell, one
    ulp outside is outside, a point that is not finite is not valid, a NaN node takes out the cells that touch it and no others, and
    with both weights zero such a point has energy +0."""
    V = _field(G, xf, seed=3)
    S = _specials(V)[None]
    K = S.shape[1]
    value, grad, valid = SC.sample(V, S)
    got = {}
    for layout in LAYOUTS:
        vol = _volume(V, layout, dev=(layout == "cells"))
        r = vol.sample(_dev(S))
        assert _same(r["value"], value) and _same(r["gradient"], grad) and _same(r["valid"], valid), layout
        wp, wc = np.ones(K, f32), np.ones(K, f32)
        wp[-4:], wc[-4:] = 0, 0
        t = vol.term(_dev(S), _dev(wp), _dev(wc), 0.05)
        energy, pe, tv, tok = SC.term(V, S, wp, wc, 0.05)
        assert _same(t["energy"], energy) and _same(t["point_energy"], pe) and _same(t["value"], tv) and _same(t["valid"], tok)
        got[layout] = [_host(r[k]).tobytes() for k in ("value", "gradient", "valid")] + [_host(t[k]).tobytes() for k in ("energy", "point_energy")]
    assert got["linear"] == got["cells"]
    assert valid[0, 16:24].all()  # inside the last cell
    if xf == "none":
        assert valid[0, :8].all()  # the nodes of the first cell (where a rounded far node falls is the restatement's to say)
        Gz, Gy, Gx = V["v"].shape
        near = value[0, :8].reshape(2, 2, 2)  # (x, y, z) in {0, 1}^3: f = 0 returns the node itself
        if not np.isnan(V["v"][:2, :2, :2]).any():
            assert near[0, 0, 0] == V["v"][0, 0, 0]
        # (on each face and one ulp beyond it: which side the rounded grid coordinate falls on is the restatement's to say, and
        # test_scene_cpu.test_rule_at_the_edges pins it where the coordinates are exact)
        assert valid[0, 24:36].any() and not valid[0, 24:36].all()
    bad = valid[0, -9:-4] if min(G) > 2 else valid[0, -5:]
    assert (bad == 0).all()
    if min(G) > 2:
        assert valid[0, -4:].tolist() == [0, 0, 1, 1]  # the two cells at the NaN node (3, 0, 0), and two that are clear
        assert (pe[0, -4:] == 0).all() and not np.signbit(pe[0, -4:]).any() and (value[0, -4:-2] == 0).all()


# ---------------------------------------------------------------------------------------------------- 2. set and independence
@pytest.mark.parametrize("layout", LAYOUTS)
def test_set(layout):
    """set() in host and in device space; the next sample sees the new values; a volume created empty is zeros."""
    from smplpp_amd.scene import Volume

    G = (5, 4, 3)
    V = _field(G, "rotation", seed=1)
    P = _points(V, 2, 40, seed=2)
    vol = _volume(V, layout)
    first = SC.sample(V, P)
    assert _same(vol.sample(_dev(P))["value"], first[0])
    for dev in (False, True):
        V2 = _field(G, "rotation", seed=10 + dev, nan_node=dev)
        assert vol.set(_dev(V2["v"]) if dev else V2["v"]) is vol
        value, grad, valid = SC.sample(V2, P)
        r = vol.sample(_dev(P))
        assert _same(r["value"], value) and _same(r["gradient"], grad) and _same(r["valid"], valid) and not _same(r["value"], first[0])
        r = vol.sample(P)  # host space
        assert _same(r["value"], value) and _same(r["gradient"], grad) and _same(r["valid"], valid)
    os.environ["SMPLPP_VOLUME_LAYOUT"] = layout
    try:
        empty = Volume("cuda:0", None, V["o"], V["h"], V["xf"], shape=(3, 4, 5))
    finally:
        del os.environ["SMPLPP_VOLUME_LAYOUT"]
    r = empty.sample(P)
    assert (r["value"] == 0).all() and _same(r["valid"], SC.sample(SC.volume(np.zeros((3, 4, 5)), V["o"], V["h"], V["xf"]), P)[2])


@pytest.mark.parametrize("K", [24, 65, 1030])
def test_independence(K):
    """A frame's bits alone, among others, in another slot, in host and device space, in both layouts, and with single outputs."""
    G, rho = (33, 9, 6), 0.05
    V = _field(G, "affine", seed=5)
    own = _points(V, 1, K, seed=6)[0]
    wp, wc = _weights(K, 7)
    rng = np.random.default_rng(8)
    ge, gpe, gv = f32(0.75), rng.normal(size=K).astype(f32), rng.normal(size=K).astype(f32)
    ref = None
    for layout in LAYOUTS:
        vol = _volume(V, layout)
        for n, slot in ((1, 0), (3, 1), (4, 3)):
            P = _points(V, n, K, seed=20 + n)
            P[slot] = own
            g_e, g_pe, g_v = rng.normal(size=n).astype(f32), rng.normal(size=(n, K)).astype(f32), rng.normal(size=(n, K)).astype(f32)
            g_e[slot], g_pe[slot], g_v[slot] = ge, gpe, gv
            for dev in (True, False):
                p = (lambda a: _dev(a)) if dev else (lambda a: a)
                out = dict(vol.sample(p(P)))
                out.update({"t_" + k: v for k, v in vol.term(p(P), p(wp), p(wc), rho).items()})
                out["grad_points"] = vol.termBackward(p(P), p(wp), p(wc), rho, p(g_e), p(g_pe), p(g_v))
                mine = {k: _host(v)[slot] for k, v in out.items()}
                if ref is None:
                    ref = mine
                for k in ref:
                    assert _same(np.asarray(mine[k]), np.asarray(ref[k])), (layout, n, slot, dev, k)
            for k in ("value", "gradient", "valid"):
                assert _same(_host(vol.sample(_dev(P), want=(k,))[k])[slot], ref[k]), k
            for k in ("energy", "point_energy", "value", "valid"):
                assert _same(np.asarray(_host(vol.term(_dev(P), _dev(wp), _dev(wc), rho, want=(k,))[k])[slot]), np.asarray(ref["t_" + k])), k


# ---------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals():
    from smplpp_amd import _lib

    Lb = _lib.load()
    o3, h3 = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(0.1, 0.1, 0.1)

    def create(G=(4, 4, 4), origin=o3, spacing=h3, xf=None, space=_lib.HOST, out=True, env=None):
        h = C.c_void_p(123)
        if env is not None:
            os.environ["SMPLPP_VOLUME_LAYOUT"] = env
        try:
            rc = Lb.smplpp_volume_create(0, G[0], G[1], G[2], origin, spacing, xf, None, space, C.byref(h) if out else None)
        finally:
            os.environ.pop("SMPLPP_VOLUME_LAYOUT", None)
        assert not out or (rc == 0) == bool(h.value)
        if rc == 0:
            Lb.smplpp_volume_destroy(h)
        return rc, Lb.smplpp_last_error().decode()

    f3 = lambda *v: (C.c_float * 3)(*v)  # noqa: E731
    bad_xf = (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, float("nan"), 0, 0, 1, 0)
    assert create()[0] == 0 and create(env="linear")[0] == 0 and create(env="cells")[0] == 0 and create(env="")[0] == 0
    for kw, why in ((dict(G=(1, 4, 4)), "[2, 1024]"), (dict(G=(4, 1025, 4)), "[2, 1024]"), (dict(G=(4, 4, 0)), "[2, 1024]"),
                    (dict(G=(1024, 1024, 129)), "2^27"), (dict(spacing=f3(0.1, 0.0, 0.1)), "spacing"), (dict(spacing=f3(0.1, -1.0, 0.1)), "spacing"),
                    (dict(spacing=f3(0.1, float("inf"), 0.1)), "spacing"), (dict(spacing=f3(float("nan"), 0.1, 0.1)), "spacing"),
                    (dict(origin=f3(0.0, float("inf"), 0.0)), "origin"), (dict(origin=None), "NULL"), (dict(xf=bad_xf), "world_to_volume"),
                    (dict(space=2), "space"), (dict(out=False), "no out"), (dict(env="bricks"), "SMPLPP_VOLUME_LAYOUT")):
        rc, msg = create(**kw)
        assert rc == 1 and why in msg, (kw, msg)

    V = _field((5, 4, 3), "none", seed=1)
    vol = _volume(V)
    n, K = 2, 4
    dev = lambda *shape: torch.full(shape, FILL, device="cuda")  # noqa: E731
    pts = _dev(_points(V, n, K, seed=1))
    outs = dict(value=dev(n, K), gradient=dev(n, K, 3), energy=dev(n), pe=dev(n, K), gp=dev(n, K, 3))
    valid = torch.full((n, K), 7, dtype=torch.uint8, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    D = _lib.DEVICE

    def sample(vol_=vol, n_=n, K_=K, p=pts, value=outs["value"], grad=outs["gradient"], ok=valid, space=D):
        return Lb.smplpp_volume_sample(vol_.handle if vol_ else None, n_, K_, P(p), P(value), P(grad), P(ok), space, None)

    def term(vol_=vol, n_=n, K_=K, p=pts, rho=0.0, e=outs["energy"], pe=outs["pe"], value=outs["value"], ok=valid, space=D):
        return Lb.smplpp_scene_term(vol_.handle if vol_ else None, n_, K_, P(p), None, None, rho, P(e), P(pe), P(value), P(ok), space, None)

    def vjp(vol_=vol, n_=n, K_=K, p=pts, rho=0.0, ge=outs["energy"], gpe=None, gv=None, gp=outs["gp"], acc=0, space=D):
        return Lb.smplpp_scene_term_vjp(vol_.handle if vol_ else None, n_, K_, P(p), None, None, rho, P(ge), P(gpe), P(gv), P(gp), acc, space, None)

    refused = [
        sample(vol_=None), sample(p=None), sample(n_=0), sample(n_=-1), sample(K_=0), sample(n_=2 ** 20, K_=2 ** 10), sample(value=None, grad=None, ok=None),
        sample(space=2),
        term(vol_=None), term(p=None), term(n_=0), term(K_=-2), term(n_=2 ** 30, K_=1), term(e=None, pe=None, value=None, ok=None), term(rho=-0.5),
        term(rho=float("inf")), term(rho=float("nan")), term(space=3),
        vjp(vol_=None), vjp(p=None), vjp(n_=0), vjp(K_=0), vjp(n_=2 ** 29, K_=2), vjp(ge=None), vjp(gp=None), vjp(acc=2), vjp(acc=-1), vjp(rho=-1.0),
        vjp(rho=float("nan")), vjp(space=2),
        Lb.smplpp_volume_set(None, P(pts), D, None), Lb.smplpp_volume_set(vol.handle, None, D, None), Lb.smplpp_volume_set(vol.handle, P(pts), 5, None),
    ]
    torch.cuda.synchronize()
    assert all(rc == 1 for rc in refused), refused
    for k, t in outs.items():
        assert (t == FILL).all(), k
    assert (valid == 7).all()
    assert _same(vol.sample(pts)["value"], SC.sample(V, _host(pts))[0])  # the refused set() left the grid as it was
    # and the same calls go through once the argument is put right
    assert sample() == 0 and term() == 0 and vjp() == 0 and sample(n_=1, K_=n * K) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 4. C++ shim
def test_scene_cpp_shim(tmp_path):
    exe = str(tmp_path / "scene_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "scene_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    Gx, Gy, Gz, n, K = 5, 4, 3, 2, 6
    i = np.arange(Gx * Gy * Gz)
    values = (((i * 7) % 13 - 6).astype(f32) * f32(0.0625)).reshape(Gz, Gy, Gx)
    xf = np.array([1.0, 0.25, 0.0, 0.125, -0.25, 1.0, 0.5, 0.0, 0.0, 0.125, 0.75, -0.0625], f32)
    V = SC.volume(values, (-0.25, 0.125, -0.5), (0.25, 0.5, 0.375), xf)
    j = np.arange(n * K)
    P = np.stack([f32(-0.125) + f32(0.0625) * (j % 7).astype(f32), f32(0.25) + f32(0.09375) * (j % 5).astype(f32),
                  f32(-0.375) + f32(0.0625) * (j % 4).astype(f32)], -1).astype(f32)
    P[4, 0] = 7.0
    P = P.reshape(n, K, 3)
    gpe = (f32(0.5) - f32(0.125) * j.astype(f32)).reshape(n, K)
    gv = (f32(-0.25) + f32(0.0625) * j.astype(f32)).reshape(n, K)
    wp, wc = np.array([1.0, 0.5, 0.0, 2.0, 1.0, 0.0], f32), np.array([0.0, 0.25, 0.0, 1.0, 0.5, 0.75], f32)
    ge = np.array([1.0, -0.5], f32)
    value, grad, valid = SC.sample(V, P)
    energy, pe, tv, tok = SC.term(V, P, wp, wc, 0.25)
    g1 = SC.term_vjp(V, P, wp, wc, 0.25, ge, gpe, gv, np.zeros((n, K, 3), f32), 0)
    g2 = SC.term_vjp(V, P, wp, wc, 0.25, ge, None, None, g1.copy(), 1)
    V2 = SC.volume(-values, (-0.25, 0.125, -0.5), (0.25, 0.5, 0.375), xf)
    want = [np.array([Gx, Gy, Gz], f32), value, grad, valid.astype(f32), energy, pe, tv, tok.astype(f32), g1, g2, SC.sample(V2, P)[0]]
    assert valid.sum() not in (0, n * K) and (value != 0).any()
    raw = open(outp, "rb").read()
    assert len(raw) == 4 * sum(a.size for a in want)
    off = 0
    for k, a in enumerate(want):
        got = np.frombuffer(raw, f32, a.size, off).reshape(a.shape)
        off += 4 * a.size
        assert _same(got, np.ascontiguousarray(a)), k


# ---------------------------------------------------------------------------------------------------- 5. the gradient and the fit
def test_gradient_through_fk(synth_model):
    """theta, beta -> smplpp_fk -> term_differentiable -> sum on the synthetic model, n = 2, a sphere field on a 24^3 grid, against float64
    autograd of the same graph, within max(4 x the error of fp32 autograd, 1e-5).  A vertex within 0.05 cells of a cell face or with
    |s| < 1e-3 in the float64 run is left out of the graph on every side (its weights are zero): fewer than 20 % are (scene_oracle:
    gradient_case, checked in test_scene_cpu)."""
    import test_pose_prior_gpu as TP
    from smplpp_amd.smpl import SMPL

    case = SC.gradient_case(synth_model)
    keep = case["keep"].all(0)  # a weight is per vertex: a vertex stays when it is clear in both frames
    assert 1.0 - keep.mean() < 0.2
    print("vertices in the graph: %.1f %%" % (100 * keep.mean()))
    wp, wc = case["w_pen"] * keep, case["w_con"] * keep
    V, rho = case["V"], case["rho"]
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    vol = _volume(V)
    beta, theta = _dev(case["beta"]).requires_grad_(True), _dev(case["theta"]).requires_grad_(True)
    verts, _ = s.forward_differentiable(beta, theta)
    energy = vol.term_differentiable(verts, wp, wc, rho)
    energy.sum().backward()

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        b, t = torch.tensor(case["beta"], dtype=dtype, requires_grad=True), torch.tensor(case["theta"], dtype=dtype, requires_grad=True)
        e = SC.energy_t(SC.as_dtype(V, np.float64), FK.fk(m, b, t)["verts"], wp, wc, rho).sum(1)
        e.sum().backward()
        return e.detach().double().numpy(), b.grad.double().numpy(), t.grad.double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert np.allclose(_host(energy.detach()), r64[0], rtol=1e-4)
    TP._bar(beta.grad, r64[1], r32[1], "scene term through FK, beta")
    TP._bar(theta.grad, r64[2], r32[2], "scene term through FK, theta")
    # sample_differentiable: the value's own gradient, through the same chain
    beta.grad, theta.grad = None, None
    verts, _ = s.forward_differentiable(beta, theta)
    kk = _dev(keep.astype(f32))
    (vol.sample_differentiable(verts) * kk).sum().backward()

    def ref_value(dtype):
        m = FK.model_tensors(synth_model, dtype)
        b, t = torch.tensor(case["beta"], dtype=dtype, requires_grad=True), torch.tensor(case["theta"], dtype=dtype, requires_grad=True)
        (SC.sample_t(SC.as_dtype(V, np.float64), FK.fk(m, b, t)["verts"]) * torch.tensor(keep, dtype=dtype)).sum().backward()
        return b.grad.double().numpy(), t.grad.double().numpy()

    v64, v32 = ref_value(torch.float64), ref_value(torch.float32)
    TP._bar(theta.grad, v64[1], v32[1], "sampled value through FK, theta")


def test_fit_out_of_a_plane(synth_model):
    """Two bodies standing on a plane (a 32^3 grid around them) are moved 50 mm through it; 60 Adam steps on trans and the rotations with
    penetration plus contact (rho = 0.05) on the lowest 5 % of the vertices.  The largest penetration depth must fall, and end within 2x
    of the identical schedule in float64 on the CPU (scene_oracle.fit_float64).  Measured: float64 50.0 -> 28.3 mm; see DESIGN 3.22 for
    the MI355X's trajectory."""
    from smplpp_amd.smpl import SMPL

    case = SC.fit_case(synth_model)
    d64 = SC.fit_float64(synth_model, case)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    vol = _volume(case["V"])
    beta = _dev(case["beta"])
    trans, rot = _dev(case["theta"][:, :1]).requires_grad_(True), _dev(case["theta"][:, 1:]).requires_grad_(True)
    w = _dev(case["w"])
    opt = torch.optim.Adam([trans, rot], lr=SC.FIT_LR)
    depth = []

    def evaluate():
        verts, _ = s.forward_differentiable(beta, torch.cat([trans, rot], 1))
        r = vol.term(verts.detach(), want=("value", "valid"))
        assert bool(r["valid"].all())
        depth.append(float(-r["value"].min()))
        return vol.term_differentiable(verts, w, w, SC.FIT_RHO).sum()

    for _ in range(SC.FIT_STEPS):
        opt.zero_grad()
        evaluate().backward()
        opt.step()
    with torch.no_grad():
        evaluate()
    at = [0, 1, 5, 10, 20, 40, 60]
    print("float64: largest penetration depth (mm) at steps %s: %s" % (at, np.round(1e3 * d64[at], 2)))
    print("MI355X:  largest penetration depth (mm) at steps %s: %s" % (at, np.round(1e3 * np.array(depth)[at], 2)))
    assert abs(depth[0] - SC.FIT_DEPTH) < 1e-5
    assert depth[-1] < depth[0] and depth[-1] <= 2 * d64[-1], (depth[-1], d64[-1])
