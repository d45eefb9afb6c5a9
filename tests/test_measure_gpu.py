"""Body measurements on the MI355X (smplpp_measure, smplpp_measure_vjp): every output bit of both calls against the numpy restatement
of tests/measure_oracle.py for region lengths on both sides of every frame_sum_split threshold, with a NaN vertex, dead planes and
zero cotangents in the batch; independence of n, slot, space, outputs asked for and of what shares the handle; accumulate; the
refusals; the exact ties; accuracy against float64 with and without a centre; the chain from theta and beta; a shape fit; the C++
shim."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import measure_oracle as MO  # noqa: E402
import stage_oracle as SO  # noqa: E402
import test_measure_cpu as CPU  # noqa: E402  (sphere, the octahedra)
import vjp_blocks as VB  # noqa: E402
from distance_cases import _same_bits  # noqa: E402
from test_vertex_offsets_gpu import _dev, _smpl  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
NMAX = 33
LENGTHS = [1, 63, 64, 65, 1023, 1024, 1025, 2049]  # both sides of frame_sum_split's thresholds, and a second lap of the partials
SECTIONS = {0: [], 1: [0], 5: [0, 2, 0, 0, 2]}


def _host(a):
    return None if a is None else a.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ball():
    """A handle on a closed sphere mesh of 2052 faces and NMAX frames of its vertices, 1 m from the origin."""
    from smplpp_amd import model_io

    v, f = CPU.sphere(2052)
    rng = np.random.default_rng(2052)
    verts = np.stack([(v.astype(f64) * (0.4 + 0.005 * i) + 0.01 * rng.standard_normal(v.shape) + [0.6, -0.7, 0.4]).astype(f32)
                      for i in range(NMAX)])
    return dict(s=_smpl(model_io.tiny_model(len(v), seed=3, faces=f + 1)), f=f, v=verts, perm=rng.permutation(len(f)))


def _regions(ball, K):
    """R = 3: K faces in shuffled order, an empty region, and a shuffled region that overlaps the first."""
    perm = ball["perm"]
    other = perm[K // 3:K // 3 + max(1, K // 2) + 3].copy()
    np.random.default_rng(K).shuffle(other)
    return [perm[:K].copy(), np.zeros(0, np.int64), other]


def _case(ball, K, S, n, shared, centre, seed=0):
    """Inputs of one bit case: a NaN vertex in the last frame, a dead plane of each kind and zero cotangents in the batch."""
    rng = np.random.default_rng(1000 * K + 10 * S + n + seed)
    regions, sections = _regions(ball, K), SECTIONS[S]
    v = ball["v"][:n].copy()
    v[n - 1, ball["f"][regions[0][0]][1], 2] = np.nan
    pf = 1 if shared else n
    cen = np.nanmean(v, 1)
    nrm = rng.normal(0, 1, (pf, S, 3))
    at = cen[:pf, None] + rng.normal(0, 0.1, (pf, S, 3))
    pl = np.concatenate([nrm, (nrm * at).sum(-1, keepdims=True)], -1).astype(f32) if S else None
    if S == 5:
        pl[0, 3, 1] = np.nan
        pl[pf - 1, 4, :3] = 0.0
    w = dict(grad_area=rng.normal(0, 1, (n, 3)).astype(f32), grad_volume=rng.normal(0, 1, (n, 3)).astype(f32),
             grad_section=rng.normal(0, 1, (n, S)).astype(f32) if S else None)
    w["grad_area"][0, 0] = 0.0
    if S == 5:
        w["grad_section"][:, 2] = 0.0
    return dict(regions=regions, sections=sections, v=v, pl=pl, c=cen.astype(f32) if centre else None, w=w)


def _run(ms, c, device=True, want=("area", "volume", "section", "crossings"), want_bwd=("verts", "planes"), w=None):
    """Every output of the forward and of the backward call, as numpy."""
    conv = (lambda a: None if a is None else _dev(a)) if device else (lambda a: a)
    back = _host if device else (lambda a: a)
    w = c["w"] if w is None else w
    res = {k: back(a) for k, a in ms.evaluate(conv(c["v"]), conv(c["pl"]), conv(c["c"]), want=want).items()}
    bwd = ms.evaluateBackward(conv(c["v"]), conv(c["pl"]), conv(c["c"]), conv(w["grad_area"]), conv(w["grad_volume"]), conv(w["grad_section"]),
                              want=want_bwd)
    res.update({"g" + k: back(a) for k, a in bwd.items()})
    return res


def _expect(ball, c, w=None):
    w = c["w"] if w is None else w
    ref = MO.measure(c["v"], ball["f"], c["regions"], c["sections"], c["pl"], c["c"])
    bwd = MO.measure_vjp(c["v"], ball["f"], c["regions"], c["sections"], c["pl"], c["c"], **w)
    ref.update({"g" + k: a for k, a in bwd.items()})
    if not c["sections"]:
        for k in ("section", "crossings", "gplanes"):
            del ref[k]
    return ref


def _check(got, ref, what):
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k in got:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert _same_bits(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()), got[k].ravel()[:4], ref[k].ravel()[:4])


# ---------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("K", LENGTHS)
def test_every_output_bit(ball, K):
    from smplpp_amd.measure import Measure

    crossed = 0
    for S in (0, 1, 5):
        ms = Measure(ball["s"], _regions(ball, K), SECTIONS[S])
        assert ms.info() == dict(region_num=3, nnz=sum(len(r) for r in _regions(ball, K)), section_num=S)
        for n in (1, 3) + ((NMAX,) if K == 65 and S == 5 else ()):
            for shared in (False, True) if S else (False,):
                for centre in (True, False):
                    if n == NMAX and not (shared and centre):
                        continue
                    c = _case(ball, K, S, n, shared, centre)
                    ref = _expect(ball, c)
                    _check(_run(ms, c), ref, (K, S, n, shared, centre))
                    if S:
                        crossed += int(ref["crossings"].sum())
                        assert ref["gplanes"].shape == ((1 if shared else n), S, 4)
                    if S == 5:
                        assert (ref["section"][0, 3] == 0) and (ref["crossings"][0, 3] == 0) and (ref["gplanes"][0, 3] == 0).all()
                    assert (ref["area"][:, 1] == 0).all() and np.isfinite(ref["gverts"]).all() and np.isfinite(ref["area"]).all()
    assert crossed > (0 if K < 63 else 30)


def test_synthetic_model_bits(synth_model):
    from smplpp_amd import model_io
    from smplpp_amd.measure import Measure, regions_by_joint

    s = _smpl(synth_model)
    f = synth_model["face_indices"].astype(np.int64) - 1
    regions = regions_by_joint(synth_model, [list(range(24)), [0, 3, 6, 9, 12, 13, 14, 15], [16, 18, 20, 22], [1, 4, 7, 10]])
    sections = [0, 1, 2, 3, 0, 0]
    beta, theta = model_io.synthetic_inputs(2, seed=5)
    out = s.launch(beta, theta)
    v = out["verts"]
    posed = s.skeleton(beta, theta)["posed"]
    at, to = posed[:, [3, 6, 18, 4, 18, 4]], posed[:, [6, 9, 20, 7, 20, 7]]
    nrm = to - at
    pl = np.concatenate([nrm, (nrm * at).sum(-1, keepdims=True)], -1).astype(f32)
    rng = np.random.default_rng(9)
    w = dict(grad_area=rng.normal(0, 1, (2, 4)).astype(f32), grad_volume=rng.normal(0, 1, (2, 4)).astype(f32),
             grad_section=rng.normal(0, 1, (2, 6)).astype(f32))
    ms = Measure(s, regions, sections)
    for shared in (False, True):
        c = dict(regions=regions, sections=sections, v=v, pl=pl[:1] if shared else pl, c=posed[:, 0].copy(), w=w)
        ref = _expect(dict(f=f), c)
        assert (ref["crossings"][0] >= 32).all() and (ref["volume"][:, 0] > 0.1).all()
        _check(_run(ms, c), ref, ("synthetic", shared))


# ---------------------------------------------------------------------------------------------------- 2. independence
def test_bits_do_not_depend_on_n_slot_space_outputs_or_company(ball):
    from smplpp_amd.measure import Measure

    K, S, n = 1025, 5, 3
    ms = Measure(ball["s"], _regions(ball, K), SECTIONS[S])
    for shared in (False, True):
        c = _case(ball, K, S, n, shared, True)
        full = _run(ms, c)
        _check(_run(ms, c, device=False), full, ("host space", shared))
        for i in range(n):  # each frame alone
            ci = dict(c, v=c["v"][i:i + 1], c=c["c"][i:i + 1], pl=c["pl"] if shared else c["pl"][i:i + 1])
            one = _run(ms, ci, w={k: a[i:i + 1] for k, a in c["w"].items()})
            for k in ("area", "volume", "section", "crossings", "gverts") + (() if shared else ("gplanes",)):
                assert _same_bits(one[k][0], full[k][i]), (shared, i, k)
        for want, want_bwd in ((("volume",), ("planes",)), (("section",), ("verts",)), (("area", "crossings"), ("verts", "planes"))):
            part = _run(ms, c, want=want, want_bwd=want_bwd)
            assert set(part) == set(want) | {"g" + k for k in want_bwd}
            for k in part:
                assert _same_bits(part[k], full[k]), (shared, k)
        # a NULL cotangent is a zero one
        for drop in ("grad_area", "grad_volume", "grad_section"):
            zeroed, nulled = dict(c["w"]), dict(c["w"])
            zeroed[drop], nulled[drop] = np.zeros_like(c["w"][drop]), None
            a, b = _run(ms, c, w=zeroed), _run(ms, c, w=nulled)
            assert _same_bits(a["gverts"], b["gverts"]) and _same_bits(a["gplanes"], b["gplanes"]), drop
        # the first region alone on a handle of its own, with its three sections
        solo = Measure(ball["s"], c["regions"][:1], [0, 0, 0])
        mine = [0, 2, 3]
        wz = {k: a.copy() for k, a in c["w"].items()}
        wz["grad_area"][:, 1:], wz["grad_volume"][:, 1:] = 0.0, 0.0
        wz["grad_section"][:, [1, 4]] = 0.0
        shared_handle = _run(ms, c, w=wz)
        cs = dict(c, regions=c["regions"][:1], sections=[0, 0, 0], pl=np.ascontiguousarray(c["pl"][:, mine]))
        alone = _run(solo, cs, w=dict(grad_area=wz["grad_area"][:, :1].copy(), grad_volume=wz["grad_volume"][:, :1].copy(),
                                      grad_section=np.ascontiguousarray(wz["grad_section"][:, mine])))
        for k in ("area", "volume"):
            assert _same_bits(alone[k][:, 0], shared_handle[k][:, 0]), k
        for k in ("section", "crossings"):
            assert _same_bits(alone[k], shared_handle[k][:, mine]), k
        assert _same_bits(alone["gverts"], shared_handle["gverts"]) and _same_bits(alone["gplanes"], shared_handle["gplanes"][:, mine])


def test_accumulate_adds_exactly_once(ball):
    from smplpp_amd.measure import Measure

    K, S = 65, 5
    ms = Measure(ball["s"], _regions(ball, K), SECTIONS[S])
    for n, shared in ((3, True), (3, False), (NMAX, True)):
        c = _case(ball, K, S, n, shared, True)
        plain = ms.evaluateBackward(c["v"], c["pl"], c["c"], **c["w"])
        for device in (False, True):
            conv = (lambda a: None if a is None else _dev(a)) if device else (lambda a: a)
            acc = {k: conv(np.full(a.shape, 1.5, f32)) for k, a in plain.items()}
            res = ms.evaluateBackward(conv(c["v"]), conv(c["pl"]), conv(c["c"]), *(conv(c["w"][k]) for k in ("grad_area", "grad_volume", "grad_section")),
                                      out=acc)
            assert set(res) == set(plain)
            for k, a in plain.items():
                got = _host(acc[k]) if device else acc[k]
                assert _same_bits(got, f32(1.5) + a), (n, shared, k, device)


# ---------------------------------------------------------------------------------------------------- 3. the call rules
def test_refusals_leave_the_outputs_untouched(ball):
    from smplpp_amd import _lib
    from smplpp_amd.measure import Measure

    L = _lib.load()
    K, S, n = 64, 5, 2
    ms = Measure(ball["s"], _regions(ball, K), SECTIONS[S])
    c = _case(ball, K, S, n, False, True)
    V = c["v"].shape[1]
    out = {k: np.full(sh, 7.0, f32) for k, sh in dict(area=(n, 3), volume=(n, 3), section=(n, S), gv=(n, V, 3), gp=(n, S, 4)).items()}
    cr = np.full((n, S), 7, np.int32)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    base = dict(h=ms.handle, n=n, v=c["v"], c=c["c"], pl=c["pl"], pf=n, space=0, acc=0)

    def fwd(outs=("area", "volume", "section", "crossings"), **kw):
        k = dict(base, **kw)
        o = lambda key: p(out[key]) if key in outs else None  # noqa: E731
        return L.smplpp_measure(k["h"], k["n"], p(k["v"]), p(k["c"]), p(k["pl"]), k["pf"], o("area"), o("volume"), o("section"),
                                p(cr) if "crossings" in outs else None, k["space"], None)

    def vjp(outs=("gv", "gp"), **kw):
        k = dict(base, **kw)
        o = lambda key: p(out[key]) if key in outs else None  # noqa: E731
        return L.smplpp_measure_vjp(k["h"], k["n"], p(k["v"]), p(k["c"]), p(k["pl"]), k["pf"], p(c["w"]["grad_area"]), p(c["w"]["grad_volume"]),
                                    p(c["w"]["grad_section"]), o("gv"), o("gp"), k["acc"], k["space"], None)

    common = [dict(h=None), dict(n=0), dict(n=-1), dict(v=None), dict(pl=None), dict(pf=0), dict(pf=3), dict(pf=-1), dict(space=2),
              dict(n=2 ** 30, pf=1), dict(outs=())]
    for kw in common:
        assert fwd(**kw) == 1 and L.smplpp_last_error(), list(kw)
    for kw in common + [dict(acc=2), dict(acc=-1)]:
        assert vjp(**kw) == 1 and L.smplpp_last_error(), list(kw)
    assert all((a == 7).all() for a in out.values()) and (cr == 7).all()
    assert fwd() == 0 and vjp() == 0 and fwd(c=None) == 0 and fwd(pf=1) == 0  # the base calls are good ones
    # creation: every refusal leaves *out NULL
    ptr, face, sec = np.array([0, 2, 2], np.int64), np.array([5, 9], np.int64), np.array([1, 0], np.int64)

    def create(R=2, ptr=ptr, face=face, S=2, sec=sec, model=ball["s"].handle):
        h = C.c_void_p(12345)
        rc = L.smplpp_measure_create(model, R, p(ptr), p(face), S, p(sec), C.byref(h))
        if rc == 0:
            _lib.check(L.smplpp_measure_destroy(h))
        else:
            assert h.value is None
        return rc

    assert create() == 0 and create(S=0, sec=None) == 0
    F = len(ball["f"])
    for kw in (dict(model=None), dict(R=0), dict(R=257), dict(S=-1), dict(S=257), dict(ptr=None), dict(face=None), dict(sec=None),
               dict(face=np.array([5, F], np.int64)), dict(face=np.array([-1, 9], np.int64)), dict(face=np.array([9, 9], np.int64)),
               dict(ptr=np.array([0, 2, 1], np.int64)), dict(ptr=np.array([1, 2, 2], np.int64)), dict(sec=np.array([2, 0], np.int64)),
               dict(sec=np.array([0, -1], np.int64))):
        assert create(**kw) == 1 and L.smplpp_last_error(), list(kw)
    # the binding words its own refusals
    for bad in (dict(verts=c["v"][:, :5]), dict(planes=c["pl"][:, :3]), dict(planes=None), dict(center=c["c"][:1]), dict(want=())):
        kw = dict(verts=c["v"], planes=c["pl"], center=c["c"])
        kw.update(bad)
        with pytest.raises(_lib.SmplppError):
            ms.evaluate(**kw)
    with pytest.raises(_lib.SmplppError):
        ms.evaluateBackward(c["v"], c["pl"], c["c"], want=())


# ---------------------------------------------------------------------------------------------------- 4. ties
def test_exact_ties_on_the_device():
    from smplpp_amd import model_io
    from smplpp_amd.measure import Measure

    planes = np.array([[[0, 0, 1, 0], [0, 0, 1, 1], [0, 0, 1, -1], [1, 0, 1, 1], [0, 0, 1, 5], [0, 0, -1, 0]]], f32)
    S = planes.shape[1]
    w = dict(grad_area=np.ones((1, 1), f32), grad_volume=np.ones((1, 1), f32), grad_section=np.ones((1, S), f32))
    for trial, v, f in CPU.relabelled_octahedra():
        s = _smpl(model_io.tiny_model(6, seed=3, faces=f + 1))
        ms = Measure(s, [np.arange(8)], [0] * S)
        c = dict(regions=[np.arange(8)], sections=[0] * S, v=v[None].copy(), pl=planes, c=None, w=w)
        got = _run(ms, c)
        _check(got, _expect(dict(f=f), c), ("octahedron", trial))
        assert got["section"][0].tolist() == [f32(4) * np.sqrt(f32(2)), 0, 0, f32(2) * np.sqrt(f32(2)), 0, f32(4) * np.sqrt(f32(2))], trial
        assert got["crossings"][0].tolist() == [4, 4, 0, 6, 0, 4] and got["volume"][0, 0] == f32(8) / f32(6)
    # a face lying in the plane: its border is counted once, by the faces below
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, -1]], f32)
    f = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int64)
    s = _smpl(model_io.tiny_model(4, seed=3, faces=f + 1))
    ms = Measure(s, [np.arange(4)], [0])
    c = dict(regions=[np.arange(4)], sections=[0], v=v[None], pl=CPU.Z0.astype(f32), c=None,
             w=dict(grad_area=None, grad_volume=None, grad_section=np.ones((1, 1), f32)))
    got = _run(ms, c)
    _check(got, _expect(dict(f=f), c), "face in the plane")
    assert got["crossings"][0, 0] == 3 and got["section"][0, 0] == (f32(1) + f32(1)) + np.sqrt(f32(2))


# ---------------------------------------------------------------------------------------------------- 5. accuracy
GROUPS = [list(range(24)), [0, 3, 6, 9, 12, 13, 14, 15], [16, 18, 20, 22], [1, 4, 7, 10]]  # all, trunk, left arm, left leg
GIRTHS = [(0, 3, 6), (1, 6, 9), (2, 18, 20), (3, 4, 7), (0, 18, 20), (0, 4, 7)]  # (region, joint the plane passes through, joint it faces)


def _body(synth_model):
    from smplpp_amd.measure import Measure, regions_by_joint

    s = _smpl(synth_model)
    regions = regions_by_joint(synth_model, GROUPS)
    sections = [g[0] for g in GIRTHS]
    return s, regions, sections, Measure(s, regions, sections), synth_model["face_indices"].astype(np.int64) - 1


def _planes_of(posed):
    at, to = posed[:, [g[1] for g in GIRTHS]], posed[:, [g[2] for g in GIRTHS]]
    from smplpp_amd.measure import plane_through

    return plane_through(at, to - at)


def test_forward_accuracy_far_from_the_origin(synth_model):
    """The synthetic body posed with theta ~ N(0, 0.3^2), 2.5 m from the origin: area, volume and section against the float64 rule on
    the same float32 inputs, under 4x the error of the float32 torch evaluation of the same definition; the volume both about the
    root joint and about the origin, each against its own float32 evaluation."""
    s, regions, sections, ms, f = _body(synth_model)
    n = 4
    rng = np.random.default_rng(31)
    beta = rng.standard_normal((n, 10)).astype(f32)
    theta = (0.3 * rng.standard_normal((n, 25, 3))).astype(f32)
    u = rng.standard_normal((n, 3))
    theta[:, 0] = (2.5 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(f32)
    v = s.launch(beta, theta)["verts"]
    posed = s.skeleton(beta, theta)["posed"]
    pl = _planes_of(torch.from_numpy(posed)).numpy()
    for name, cen in (("root joint", posed[:, 0].copy()), ("NULL", None)):
        got = ms.evaluate(v, pl, cen)
        ref = MO.measure(v, f, regions, sections, pl, cen, dtype=f64)
        assert (ref["crossings"] == got["crossings"]).all() and (ref["crossings"] >= 32).all()
        low = MO.measure_torch(torch.from_numpy(v), f, regions, sections, torch.from_numpy(pl), None if cen is None else torch.from_numpy(cen))
        for k, lo in zip(("area", "volume", "section"), low):
            e, e32 = SO.scaled_error(got[k], ref[k]), SO.scaled_error(lo.numpy(), ref[k])
            print("forward accuracy, center = %s: %s E = %.3g (fp32 torch %.3g)" % (name, k, e, e32))
            assert e <= SO.bar(e32), (name, k, e, e32)


def test_chain_from_theta_and_beta(synth_model):
    """theta, beta -> verts and posed joints -> planes through the joints -> the weighted measurements, against float64 autograd.
    A girth is continuous in its inputs but its gradient is not: it jumps where a vertex passes through the plane, because the contour
    then runs over other faces.  The device sees float32 vertices, about 1e-7 m from the float64 ones, so a case with a vertex that
    close to a plane has two crossing patterns and no reference (seed 41 has one 1.0e-7 m from a plane; one-ulp changes of the
    inputs then move the beta gradient, of this rule and of fp32 autograd alike, between 1.2e-4 and 4e-3).  The case is therefore
    checked, in float64, to keep every vertex of a cut region 1e-5 m from its plane: a hundred times that distance."""
    s, regions, sections, ms, f = _body(synth_model)
    n = 2
    rng = np.random.default_rng(42)
    beta = rng.standard_normal((n, 10)).astype(f32)
    theta = (0.3 * rng.standard_normal((n, 25, 3))).astype(f32)
    theta[:, 0] = rng.uniform(-1, 1, (n, 3))
    wa, wv, ws = (rng.uniform(0.5, 1.5, sh) for sh in ((n, 4), (n, 4), (n, 6)))
    dev = torch.device("cuda")
    b, t = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (beta, theta))
    verts, _ = s.forward_differentiable(b, t)
    _, posed, _ = s.skeleton_differentiable(b, t)
    area, vol, sec = ms.forward_differentiable(verts, _planes_of(posed), posed[:, 0])
    assert area.requires_grad and vol.requires_grad and sec.requires_grad
    tw = lambda a, like: torch.as_tensor(a, dtype=like.dtype, device=like.device)  # noqa: E731
    ((area * tw(wa, area)).sum() + 10 * (vol * tw(wv, vol)).sum() + (sec * tw(ws, sec)).sum()).backward()

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        bb, tt = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (beta, theta))
        o = FK.fk(m, bb, tt)
        X, J = o["xforms"], o["joints"]
        posed = (X[:, :, :3, :3] @ J[..., None])[..., 0] + X[:, :, :3, 3] + tt[:, 0:1]
        pl = _planes_of(posed)
        a, vv, ss = MO.measure_torch(o["verts"], f, regions, sections, pl, posed[:, 0])
        ((a * tw(wa, a)).sum() + 10 * (vv * tw(wv, vv)).sum() + (ss * tw(ws, ss)).sum()).backward()
        return bb.grad.double().numpy(), tt.grad.double().numpy(), o["verts"].detach().double().numpy(), pl.detach().double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    v64, p64 = r64[2], r64[3]
    clear = min((np.abs((v64[:, np.unique(f[regions[r]])] * p64[:, None, k, :3]).sum(-1) - p64[:, None, k, 3])
                 / np.linalg.norm(p64[:, None, k, :3], axis=-1)).min() for k, r in enumerate(sections))
    print("chain: the nearest vertex of a cut region is %.3g m from its plane" % clear)
    assert clear >= 1e-5
    # Every measurement is unchanged by a rotation about the root joint, which is also the centre of the cones: the gradient to the
    # root's rotation, theta row 1, is zero, and float64 leaves 1.7e-10 of the largest block there.  A block has no scale of its own
    # then, so that row is held against the scale of the whole array.  (Row 0, the translation, is a block like any other: the open
    # regions' cones reach to a centre that does not move with it.)
    scale = np.abs(r64[1]).max()
    still = np.abs(r64[1]).max(axis=2) <= 1e-8 * scale
    assert still[:, 1].all() and still.sum() == n
    e, e32 = (float(np.abs(a[still]).max() / scale) for a in (_host(t.grad), r32[1]))
    print("chain theta, the root's rotation: %.3g of the largest block (fp32 autograd %.3g)" % (e, e32))
    assert e <= max(4 * e32, 1e-5), (e, e32)
    for got, want, low, name, axes in ((b.grad, r64[0], r32[0], "beta", (1,)), (t.grad, r64[1], r32[1], "theta", VB.THETA)):
        keep = ~still if name == "theta" else np.ones(n, bool)
        e, e32 = (float(VB.block_errors(a, want, axes)[keep].max()) for a in (_host(got), low))
        print("chain %s: %.3g per block (fp32 autograd %.3g)" % (name, e, e32))
        assert e <= max(4 * e32, 1e-5), (name, e, e32)


# ---------------------------------------------------------------------------------------------------- 6. a shape fit
def test_shape_fit_from_measurements(synth_model):
    """Whole-body volume and area, two part volumes and three girths of a beta* ~ N(0, 1) at a fixed pose; Adam on beta from 0, 60
    steps, on the device in fp32 and the same loop in float64 on the CPU oracle.  Seven measurements do not determine ten
    coefficients, so the bar is on the loss: the device ends no further from the float64 end than the float64 loop's own loss moved
    over its last ten steps."""
    s, regions, sections, ms, f = _body(synth_model)
    rng = np.random.default_rng(51)
    star = rng.standard_normal((1, 10)).astype(f32)
    theta = (0.2 * rng.standard_normal((1, 25, 3))).astype(f32)
    theta[0, 0] = (0.3, -0.2, 0.5)
    steps, lr = 60, 0.05
    pick_v, pick_s = [1, 3], [0, 2, 3]  # the trunk's and the leg's volume; waist, arm and thigh girth

    def seven(area, vol, sec):
        return torch.cat([vol[:, :1], area[:, :1], vol[:, pick_v], sec[:, pick_s]], 1)

    m64 = FK.model_tensors(synth_model, torch.float64)
    t64 = torch.tensor(theta, dtype=torch.float64)

    def cpu_measure(beta):
        o = FK.fk(m64, beta, t64)
        X, J = o["xforms"], o["joints"]
        posed = (X[:, :, :3, :3] @ J[..., None])[..., 0] + X[:, :, :3, 3] + t64[:, 0:1]
        pl = _planes_of(posed)
        return seven(*MO.measure_torch(o["verts"], f, regions, sections, pl, posed[:, 0])), o["verts"], pl, posed

    with torch.no_grad():
        target, v_star, pl_star, posed_star = cpu_measure(torch.tensor(star, dtype=torch.float64))
    cr = MO.measure(v_star.numpy(), f, regions, sections, pl_star.numpy(), posed_star[:, 0].numpy(), dtype=f64)["crossings"]
    assert (cr[0, pick_s] >= 32).all(), cr
    scale = 1.0 / target

    def fit(beta, measure_of, tgt, sc):
        opt = torch.optim.Adam([beta], lr=lr)
        hist = []
        for _ in range(steps):
            opt.zero_grad()
            loss = (((measure_of(beta) - tgt) * sc) ** 2).sum()
            loss.backward()
            opt.step()
            hist.append(float(loss.detach()))
        return hist

    dev = torch.device("cuda")
    td = torch.from_numpy(theta).to(dev)

    def dev_measure(beta):
        verts, _ = s.forward_differentiable(beta, td)
        _, posed, _ = s.skeleton_differentiable(beta, td)
        return seven(*ms.forward_differentiable(verts, _planes_of(posed), posed[:, 0]))

    bd = torch.zeros(1, 10, device=dev, requires_grad=True)
    hist = fit(bd, dev_measure, target.to(dev).float(), scale.to(dev).float())
    b64 = torch.zeros(1, 10, dtype=torch.float64, requires_grad=True)
    hist64 = fit(b64, lambda beta: cpu_measure(beta)[0], target, scale)
    spread = max(hist64[-10:]) - min(hist64[-10:])
    print("shape fit: loss %.6g -> %.6g on the device, %.6g -> %.6g in float64; the float64 loss over its last 10 steps spans %.6g; "
          "the two ends are %.6g apart" % (hist[0], hist[-1], hist64[0], hist64[-1], spread, abs(hist[-1] - hist64[-1])))
    assert hist64[-1] < 0.1 * hist64[0] and hist[-1] < 0.1 * hist[0]
    assert abs(hist[-1] - hist64[-1]) <= spread


# ---------------------------------------------------------------------------------------------------- 7. C++ shim
def test_measure_cpp_shim(tmp_path):
    from smplpp_amd import model_io
    from smplpp_amd.measure import Measure

    exe = str(tmp_path / "measure_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "measure_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    v, f = CPU.sphere(128)
    model = model_io.tiny_model(len(v), seed=9, faces=f + 1)
    model["vertices_template"] = (0.5 * v).astype(model["vertices_template"].dtype)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    # the shim's inputs, restated
    n, F = 3, len(f)
    beta = (np.arange(n * 10, dtype=f32).reshape(n, 10) % 7 - 3) * f32(0.1)
    theta = ((np.arange(n * 75, dtype=f32).reshape(n, 25, 3) % 11) - 5) * f32(0.05)
    regions = [np.arange(F), np.arange(0, F, 3), np.zeros(0, np.int64), np.arange(F - 1, F // 2, -1)]
    sections = [0, 1, 0, 3]
    s = _smpl(model)
    verts = s.launch(beta, theta)["verts"]
    ms = Measure(s, regions, sections)
    i = np.arange(n * 4 * 4, dtype=f32).reshape(n, 4, 4)
    pl = ((i % 5) - 2) * f32(0.25) + f32(0.125)
    cen = ((np.arange(n * 3, dtype=f32).reshape(n, 3) % 4) - 1) * f32(0.125)
    ga, gvol = ((np.arange(n * 4, dtype=f32).reshape(n, 4) % 5) - 2) * f32(0.5), ((np.arange(n * 4, dtype=f32).reshape(n, 4) % 3) - 1) * f32(0.75)
    gs = ((np.arange(n * 4, dtype=f32).reshape(n, 4) % 4) - 1) * f32(0.5)
    parts, crossed = [], 0
    for pf in (n, 1):
        fw = ms.evaluate(verts, pl[:pf], cen)
        bw = ms.evaluateBackward(verts, pl[:pf], cen, ga, gvol, gs)
        crossed += int(fw["crossings"].sum())
        parts += [fw["area"], fw["volume"], fw["section"], fw["crossings"].astype(np.int64), bw["verts"], bw["planes"]]
    assert crossed > 50
    want = b"".join(np.ascontiguousarray(a).tobytes() for a in parts)
    assert len(raw) == len(want) and raw == want
