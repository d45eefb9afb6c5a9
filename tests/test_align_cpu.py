"""Rigid and similarity alignment without a GPU: the numpy restatement of smplpp_align / smplpp_align_vjp (tests/align_oracle.py) in
float64 against the SVD definition (weighted Kabsch / Umeyama with the determinant correction) and float64 autograd of it; the special
cases of the rule; its float32 form within the project's bar; the sweep count; the seeds of the GPU file's chain and fit; and the entry
points: declared, exported, bound, and refusing before they touch a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_oracle as AL  # noqa: E402
from distance_cases import _rel  # noqa: E402

import smplpp_amd.align  # noqa: E402,F401  (every test here belongs to the feature: without the module the file does not load)

NAMES = ["smplpp_align", "smplpp_align_vjp"]
f32 = np.float32


@pytest.fixture(autouse=True)
def _the_entry_points_exist():
    """The restatement is the rule of the two entry points: no test of it passes on a tree that does not declare them."""
    from smplpp_amd import _lib

    assert set(NAMES) <= set(_lib.declared_symbols())


def _definition(x, y, w, with_scale, dtype, cot=None):
    """The definition's (transform [n,13], aligned, energy) and, with cotangents (gtr, gal, ge), its autograd gradients to x and y."""
    X, Y = torch.tensor(x, dtype=dtype, requires_grad=True), torch.tensor(y, dtype=dtype, requires_grad=True)
    R, t, s, al, e = AL.definition_t(X, Y, None if w is None else torch.tensor(w, dtype=dtype), with_scale)
    n = len(x)
    tr = torch.cat([R.reshape(n, 9), t, s[:, None]], 1)
    grads = None
    if cot is not None:
        gtr, gal, ge = (torch.tensor(c, dtype=dtype) for c in cot)
        ((tr * gtr).sum() + (al * gal).sum() + (e * ge).sum()).backward()
        gy = Y.grad if Y.grad is not None else torch.zeros_like(Y)
        grads = (X.grad.double().numpy(), gy.double().numpy())
    return [v.detach().double().numpy() for v in (tr, al, e)], grads


def _cots(n, K, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 13)), rng.normal(size=(n, K, 3)), rng.normal(size=n)


# ---------------------------------------------------------------------------------------------------- 1. the entry points
def test_entry_points_are_declared_exported_and_bound():
    from smplpp_amd import _lib
    import smplpp_amd.align as align

    assert set(NAMES) <= set(_lib.declared_symbols())
    L = _lib.load()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert len(L.smplpp_align.argtypes) == 18 and len(L.smplpp_align_vjp.argtypes) == 18
    for name in ("align", "alignBackward", "align_differentiable", "apply", "mpjpe", "pa_mpjpe"):
        assert callable(getattr(align, name))


def test_refusals_come_before_the_device():
    """Every refusal of the list returns SMPLPP_ERR_INVALID with a reason, on a machine without a GPU, and leaves host outputs as they
    were."""
    from smplpp_amd import _lib

    L = _lib.load()
    n, K = 2, 3
    x, y = AL.random_case(n, K, 1)
    wgt = np.ones((n, K), f32)
    out = {k: np.full(s, 7.0, f32) for k, s in dict(tr=(n, 13), al=(n, K, 3), e=(n,), pe=(n, K), gap=(n,), gs=(n, K, 3), gt=(n, K, 3)).items()}
    st = np.full(n, 7, np.int32)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def fwd(n_=n, K_=K, x_=x, y_=y, Tn=n, w=None, Wn=1, ws=0, mg=1e-3, tr=out["tr"], al=out["al"], e=out["e"], pe=out["pe"], gap=out["gap"], status=st,
            space=0):
        return L.smplpp_align(0, n_, K_, p(x_), p(y_), Tn, p(w), Wn, ws, mg, p(tr), p(al), p(e), p(pe), p(gap), p(status), space, None)

    def vjp(n_=n, K_=K, x_=x, y_=y, Tn=n, w=None, Wn=1, ws=0, mg=1e-3, gtr=out["tr"], gal=None, ge=None, gs=out["gs"], gt=out["gt"], acc=0, space=0):
        return L.smplpp_align_vjp(0, n_, K_, p(x_), p(y_), Tn, p(w), Wn, ws, mg, p(gtr), p(gal), p(ge), p(gs), p(gt), acc, space, None)

    common = [dict(n_=0), dict(n_=-1), dict(K_=0), dict(K_=-2), dict(Tn=3), dict(Tn=0), dict(w=wgt, Wn=3), dict(w=wgt, Wn=0), dict(Wn=5), dict(ws=2),
              dict(ws=-1), dict(mg=-0.5), dict(mg=float("inf")), dict(mg=float("nan")), dict(x_=None), dict(y_=None),
              dict(n_=2 ** 20, K_=2 ** 10, Tn=1), dict(n_=2 ** 31, Tn=1), dict(n_=1, Tn=1, K_=2 ** 30), dict(space=2), dict(space=-1)]
    calls = [(fwd, kw) for kw in common + [dict(tr=None, al=None, e=None, pe=None, gap=None, status=None)]]
    calls += [(vjp, kw) for kw in common + [dict(gtr=None), dict(gs=None, gt=None), dict(acc=2), dict(acc=-1)]]
    for fn, kw in calls:
        assert fn(**kw) == 1 and L.smplpp_last_error(), (fn.__name__, kw)
    assert "int32" in (fwd(n_=2 ** 20, K_=2 ** 10, Tn=1), L.smplpp_last_error().decode())[1]
    assert all((a == 7).all() for a in out.values()) and (st == 7).all()


# ---------------------------------------------------------------------------------------------------- 2. the restatement against the definition
@pytest.mark.parametrize("kind", ["plain", "mirrored", "coplanar", "coplanar mirrored"])
@pytest.mark.parametrize("lead", [(0, 0), (1, 1), (0, 1), (1, 0)], ids=lambda l: "T%dW%d" % l)
@pytest.mark.parametrize("with_scale", [False, True])
def test_restatement_against_the_definition(with_scale, lead, kind):
    """In float64 the restatement's transform, aligned and energy equal the SVD definition, and its backward equals autograd of the
    definition, to 1e-9; every frame's float64 gap is at least 0.05 (asserted, so that no frame is left out).  Rigid and similarity, Tn
    and Wn in {1, n}, weights of zero (whose points are still moved, and whose cotangents reach the transform), mirrored and coplanar
    sets."""
    n, K = 4, 30
    x, y = AL.random_case(n, K, 11 + 3 * lead[0] + lead[1], mirrored="mirrored" in kind, coplanar="coplanar" in kind, scale=1.3 if with_scale else 1.0,
                          dtype=np.float64, shared=not lead[0])
    Tn, Wn = (n if v else 1 for v in lead)
    y = y[:Tn]
    w = np.random.default_rng(5).uniform(0.5, 2.0, (Wn, K))
    w[:, ::5] = 0
    assert (AL.float64_gap(x, y, w) >= 0.05).all(), AL.float64_gap(x, y, w)
    cot = _cots(n, K, 3)
    (tr, al, e), (gx, gy) = _definition(x, np.broadcast_to(y, x.shape).copy(), np.broadcast_to(w, (n, K)).copy(), with_scale, torch.float64, cot)
    got = AL.align(x, y, w, with_scale, dtype=np.float64)
    gs, gt = AL.align_vjp(x, y, w, with_scale, AL.MIN_GAP, *cot, np.zeros_like(x), np.zeros_like(x), 0, dtype=np.float64)
    errs = (_rel(got[0], tr), _rel(got[1], al), _rel(got[2], e), _rel(gs, gx), _rel(gt, gy))
    print("float64 restatement: transform %.3g, aligned %.3g, energy %.3g, grad_source %.3g, grad_target %.3g" % errs)
    assert (got[5] == 0).all() and np.abs(gx).max() > 0 and np.abs(gy).max() > 0
    assert max(errs) <= 1e-9, errs
    R = got[0][:, :9].reshape(n, 3, 3)
    assert np.allclose(np.linalg.det(R), 1.0, atol=1e-12) and np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-12)
    # point_error and energy agree with each other; a point of weight 0 has error +0 and gradient +0 to the target
    zero = np.broadcast_to(w, (n, K)) == 0
    assert (got[3][zero] == 0).all() and not np.signbit(got[3][zero]).any() and (gt[zero] == 0).all() and (gs[zero] != 0).any()
    assert np.allclose((np.broadcast_to(w, (n, K)) * got[3]).sum(1), got[2], rtol=1e-12)
    # each cotangent alone, and storing against adding
    for i in range(3):
        one = [c if j == i else None for j, c in enumerate(cot)]
        zeros = [c if j == i else np.zeros_like(c) for j, c in enumerate(cot)]
        _, (hx, hy) = _definition(x, np.broadcast_to(y, x.shape).copy(), np.broadcast_to(w, (n, K)).copy(), with_scale, torch.float64, zeros)
        a, b = AL.align_vjp(x, y, w, with_scale, AL.MIN_GAP, *one, np.zeros_like(x), np.zeros_like(x), 0, dtype=np.float64)
        assert _rel(a, hx) <= 1e-9 and (_rel(b, hy) <= 1e-9 or np.abs(hy).max() == 0), i
    a, b = AL.align_vjp(x, y, w, with_scale, AL.MIN_GAP, *cot, gs.copy(), gt.copy(), 1, dtype=np.float64)
    assert np.array_equal(a, gs + gs) and np.array_equal(b, gt + gt)
    assert AL.align_vjp(x, y, w, with_scale, AL.MIN_GAP, *cot, None, gt, 0, dtype=np.float64)[0] is None


# ---------------------------------------------------------------------------------------------------- 3. special cases
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_cases(dtype):
    """K = 1 and 2; all weights 0 (bit 0); coincident source points (bit 1); collinear points (bit 2 at min_gap = 1e-3); points that are
    not live through NaN and infinite coordinates and weights; and an N whose off-diagonals are tiny against its diagonal (theta^2
    overflows): no NaN."""
    T = np.dtype(dtype).type
    # K = 1: the translation alone; K = 2: the segment is matched, the rotation about it is free (bit 2)
    x, y = AL.random_case(3, 1, 2, dtype=dtype)
    tr, al, e, pe, gap, st = AL.align(x, y, None, True, dtype=dtype)
    assert (st == 6).all() and np.array_equal(tr[:, :9], np.tile(np.eye(3, dtype=dtype).reshape(9), (3, 1))) and (tr[:, 12] == 1).all()
    assert np.allclose(al, y, rtol=0, atol=4e-7) and (e <= 1e-12).all() and (gap == 0).all()  # t = y - x rounds, then x + t
    x, y = AL.random_case(3, 2, 3, noise=0.0, dtype=dtype)
    tr, al, e, pe, gap, st = AL.align(x, y, None, False, dtype=dtype)
    assert (st == 4).all() and np.isfinite(tr).all() and np.allclose(al, y, atol=1e-5) and (gap <= 1e-3).all()
    # all weights 0 in frame 1 of 3
    x, y = AL.random_case(3, 9, 4, dtype=dtype)
    w = np.ones((3, 9), dtype)
    w[1] = 0
    tr, al, e, pe, gap, st = AL.align(x, y, w, True, dtype=dtype)
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], dtype)
    assert st.tolist() == [0, 1, 0] and np.array_equal(tr[1], ident) and e[1] == 0 and gap[1] == 0 and np.array_equal(al[1], x[1]) and (pe[1] == 0).all()
    gs, gt = AL.align_vjp(x, y, w, True, AL.MIN_GAP, *_cots(3, 9, 1), np.zeros_like(x), np.zeros_like(x), 0, dtype=dtype)
    assert np.isfinite(gs).all() and (gt[1] == 0).all() and np.array_equal(gs[1], _cots(3, 9, 1)[1][1].astype(dtype))
    # coincident source points, at coordinates whose sums are exact
    x[0] = np.array([0.25, -0.5, 0.75], dtype)
    tr, al, e, pe, gap, st = AL.align(x, y, None, True, dtype=dtype)
    assert st[0] & 2 and np.array_equal(tr[0, :9], ident[:9]) and tr[0, 12] == 1 and st[2] == 0
    assert np.allclose(tr[0, 9:12], y[0].mean(0) - x[0, 0], atol=1e-6)
    # collinear points
    line = np.linspace(-1, 1, 9, dtype=dtype)[:, None]
    x[2] = line * np.array([0.5, 0.25, -0.125], dtype) + T(0.25)
    y[2] = line * np.array([0.25, -0.5, 0.125], dtype) - T(0.5)
    tr, al, e, pe, gap, st = AL.align(x, y, None, False, 1e-3, dtype=dtype)
    assert st[2] == 4 and np.isfinite(tr).all() and np.allclose(al[2], y[2], atol=1e-5)
    gs, gt = AL.align_vjp(x, y, None, False, 1e-3, *_cots(3, 9, 2), np.zeros_like(x), np.zeros_like(x), 0, dtype=dtype)
    assert np.isfinite(gs).all() and np.isfinite(gt).all()
    # points that are not live leave every result as it is without them
    x, y = AL.random_case(2, 40, 6, dtype=dtype)
    w = np.random.default_rng(1).uniform(0.5, 2, (2, 40)).astype(dtype)
    x2, y2, w2 = x.copy(), y.copy(), w.copy()
    AL.special_points(x2, y2, w2, seed=3)
    dead = ~(np.isfinite(x2).all(-1) & np.isfinite(y2).all(-1) & np.isfinite(w2) & (w2 > 0))
    assert 8 <= dead.sum() < 30
    w0 = np.where(dead, 0, w).astype(dtype)
    a, b = AL.align(x2, y2, w2, True, dtype=dtype), AL.align(x, y, w0, True, dtype=dtype)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and (a[5] == 0).all()
    assert np.isfinite(a[0]).all() and np.array_equal(a[1][~dead], b[1][~dead])
    cot = _cots(2, 40, 4)
    gs, gt = AL.align_vjp(x2, y2, w2, True, AL.MIN_GAP, *cot, np.zeros_like(x), np.zeros_like(x), 0, dtype=dtype)
    assert np.isfinite(gs).all() and np.isfinite(gt).all() and (gt[dead] == 0).all()
    # theta^2 overflows: a diagonal of order 1e25 beside off-diagonals of order 1e-15
    A = np.diag(np.array([3e25, -1e25, 2e25, -4e25], dtype))[None].repeat(2, 0)
    A[0, 0, 1] = A[0, 1, 0] = T(1e-15)
    A[1, 2, 3] = A[1, 3, 2] = T(-3e-16)
    with np.errstate(over="ignore"):
        big = ((A[0, 1, 1] - A[0, 0, 0]) / (T(2) * A[0, 0, 1])) ** 2
    lam, V = AL.jacobi(A.astype(dtype))
    assert (dtype is np.float64 or np.isinf(big)) and np.isfinite(lam).all() and np.isfinite(V).all()
    assert np.allclose(np.abs(V), np.eye(4), rtol=0, atol=1e-30) and (dtype is np.float64 or np.array_equal(np.abs(V), np.broadcast_to(np.eye(4, dtype=dtype), V.shape)))


# ---------------------------------------------------------------------------------------------------- 4. float32 and the sweeps
def test_float32_within_the_bar():
    """The float32 restatement against float64 on the same float32 inputs, within max(4 x the error of the fp32 SVD definition in torch
    on the CPU, 1e-5 relative): transform, aligned, energy and both gradients, over rigid and similarity, mirrored and coplanar sets."""
    worst = {}
    for i, (with_scale, kind) in enumerate([(a, b) for a in (False, True) for b in ("plain", "mirrored", "coplanar")]):
        n, K = 6, 53
        x, y = AL.random_case(n, K, 40 + i, mirrored=kind == "mirrored", coplanar=kind == "coplanar", scale=1.3 if with_scale else 1.0)
        w = np.random.default_rng(i).uniform(0.5, 2.0, (n, K)).astype(f32)
        w[:, ::6] = 0
        cot = tuple(c.astype(f32) for c in _cots(n, K, i))
        x64, y64, w64, cot64 = x.astype(np.float64), y.astype(np.float64), w.astype(np.float64), tuple(c.astype(np.float64) for c in cot)
        assert (AL.float64_gap(x64, y64, w64) >= 0.05).all()
        ref = AL.align(x64, y64, w64, with_scale, dtype=np.float64)[:3] + AL.align_vjp(x64, y64, w64, with_scale, AL.MIN_GAP, *cot64, np.zeros_like(x64),
                                                                                      np.zeros_like(x64), 0, dtype=np.float64)
        got = AL.align(x, y, w, with_scale)[:3] + AL.align_vjp(x, y, w, with_scale, AL.MIN_GAP, *cot, np.zeros_like(x), np.zeros_like(x), 0)
        (tr, al, e), (gx, gy) = _definition(x, y, w, with_scale, torch.float32, cot)
        for name, g, r, d in zip(("transform", "aligned", "energy", "grad_source", "grad_target"), got, ref, (tr, al, e, gx, gy)):
            assert g.dtype == f32
            err, bar = _rel(g, r), max(4 * _rel(d, r), 1e-5)
            worst[name] = max(worst.get(name, (0, 0)), (err / bar, err))
            assert err <= bar, (name, with_scale, kind, err, bar)
    print("float32 restatement, worst error / bar (error): " + ", ".join("%s %.3g (%.3g)" % (k, v[0], v[1]) for k, v in worst.items()))


def test_sweep_count_on_the_test_inputs():
    """The constant of the rule is the smallest count after which one more sweep changes no float32 bit of the transform, plus two: on
    the inputs of this file and of the GPU file, the counts SWEEPS - 2 to SWEEPS + 1 all give the bits of SWEEPS."""
    import itertools

    cases = [AL.random_case(6, 53, 40 + i, mirrored=i % 3 == 1, coplanar=i % 3 == 2) for i in range(6)]
    cases += [AL.random_case(n, K, 300 + i) for i, (K, n) in enumerate(itertools.product((3, 4, 63, 64, 65, 1024, 1025, 1030), (1, 3)))]
    for x, y in cases:
        base = AL.align(x, y, None, True)[0]
        for s in (AL.SWEEPS - 2, AL.SWEEPS - 1, AL.SWEEPS + 1):
            assert np.array_equal(AL.align(x, y, None, True, sweeps=s)[0], base), s


# ---------------------------------------------------------------------------------------------------- 5. the GPU file's chain and fit
def test_chain_case_is_well_posed(synth_model):
    import image_oracle as IM

    case = AL.chain_case(synth_model)
    with torch.no_grad():
        lm = IM.landmarks64(synth_model, case["dense"], case["beta"], case["theta"]).numpy()
    gap = AL.float64_gap(lm, case["target"].astype(np.float64), case["weight"].astype(np.float64))
    print("chain: float64 gaps %s" % gap)
    assert (gap >= 0.05).all()


def test_icp_in_float64(synth_model):
    """The ICP schedule of test_align_gpu in float64: the RMS falls at every step, by more than half in ten steps."""
    import fk_vjp_oracle as FK
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(2, seed=5)
    m = FK.model_tensors(synth_model, torch.float64)
    with torch.no_grad():
        v64 = FK.fk(m, torch.tensor(beta, dtype=torch.float64), torch.tensor(theta, dtype=torch.float64))["verts"].numpy()
    rms = AL.icp_float64(v64, AL.icp_case(v64))
    for f in range(2):
        print("float64 frame %d: RMS (mm) %s" % (f, np.round(1e3 * rms[f], 3)))
    assert (np.diff(rms, axis=1) < 0).all() and (rms[:, -1] < 0.5 * rms[:, 0]).all()
