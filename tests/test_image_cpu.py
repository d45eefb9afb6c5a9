"""The image term without a GPU: the numpy restatement of smplpp_image_sample / smplpp_image_term and its backward (tests/image_oracle.py)
against float64 autograd of the definition, to uv and to the image; its float32 forward within a bound derived from the unit roundoff;
an affine image reproduced by the interpolation; the rule at pixel centres, far edges, one ulp outside, points that are not finite and
a NaN pixel; the seeds of the GPU file's gradient chain and fit; and the entry points: declared, exported, bound, and refusing before
they touch a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_oracle as IM  # noqa: E402
from distance_cases import _rel  # noqa: E402

NAMES = ["smplpp_image_sample", "smplpp_image_term", "smplpp_image_term_vjp"]
U = 2.0 ** -24  # the unit roundoff of float32
H, W = 7, 9


def draw_uv(n, K, seed, Hh=H, Ww=W):
    """[n,K,2] float64 holding float32 values: every point inside, with both fractional parts in [0.05, 0.95], so that float32 and float64
    agree on the cell."""
    rng = np.random.default_rng(seed)
    cell = np.stack([rng.integers(0, Ww - 1, (n, K)), rng.integers(0, Hh - 1, (n, K))], -1)
    uv = (0.5 + cell + rng.uniform(0.05, 0.95, (n, K, 2))).astype(np.float32).astype(np.float64)
    assert (IM.cell_margin(uv) >= 0.04).all()
    return uv


def _case(n, K, C, channel, lead, seed, dtype=np.float64):
    """image [B,H,W,C], uv, channel, target [Tn,K,Cs], weight [Wn,K] (two zeros) and the three cotangents, in `dtype`."""
    B, Tn, Wn = (n if x else 1 for x in lead)
    rng = np.random.default_rng(seed)
    Cs = 1 if channel else C
    ch = rng.integers(0, C, K) if channel else None
    image = IM.random_image(B, H, W, C, seed + 1).astype(np.float32).astype(dtype)
    target = rng.normal(0, 0.5, (Tn, K, Cs)).astype(np.float32).astype(dtype)
    weight = rng.uniform(0.5, 2.0, (Wn, K)).astype(np.float32).astype(dtype)
    weight[0, 3], weight[-1, 7] = 0, 0
    cot = [rng.normal(size=s).astype(np.float32).astype(dtype) for s in ((n,), (n, K), (n, K, Cs))]
    return image, draw_uv(n, K, seed + 2).astype(dtype), ch, target, weight, cot


# ---------------------------------------------------------------------------------------------------- 1. the entry points
def test_entry_points_are_declared_exported_and_bound():
    from smplpp_amd import _lib
    import smplpp_amd.image as image

    assert set(NAMES) <= set(_lib.declared_symbols())
    L = _lib.load()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert len(L.smplpp_image_sample.argtypes) == 15 and len(L.smplpp_image_term.argtypes) == 21 and len(L.smplpp_image_term_vjp.argtypes) == 23
    for name in ("sample", "term", "termBackward", "sample_differentiable", "term_differentiable"):
        assert callable(getattr(image, name))
    assert "permute(0, 2, 3, 1).contiguous()" in image.__doc__


def test_refusals_come_before_the_device():
    """Every refusal of the list returns SMPLPP_ERR_INVALID with a reason, on a machine without a GPU, and leaves host outputs as they
    were."""
    from smplpp_amd import _lib

    L = _lib.load()
    n, K, Hh, Ww, Cc = 2, 3, 4, 5, 2
    uv = np.full((n, K, 2), 1.5, np.float32)
    img = np.zeros((n, Hh, Ww, Cc), np.float32)
    ch = np.array([0, 1, 1], np.int64)
    out = {k: np.full(s, 7.0, np.float32) for k, s in dict(value=(n, K, Cc), grad=(n, K, Cc, 2), energy=(n,), pe=(n, K), guv=(n, K, 2), gimg=img.shape).items()}
    ok = np.full((n, K), 7, np.uint8)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def sample(n_=n, K_=K, uv_=uv, img_=img, B=n, H_=Hh, W_=Ww, C_=Cc, ch_=None, value=out["value"], grad=out["grad"], valid=ok, space=0):
        return L.smplpp_image_sample(0, n_, K_, p(uv_), p(img_), B, H_, W_, C_, p(ch_), p(value), p(grad), p(valid), space, None)

    def term(n_=n, K_=K, uv_=uv, img_=img, B=n, H_=Hh, W_=Ww, C_=Cc, ch_=None, t=None, Tn=1, w=None, Wn=1, rho=0.0, e=out["energy"], pe=out["pe"],
             value=out["value"], valid=ok, space=0):
        return L.smplpp_image_term(0, n_, K_, p(uv_), p(img_), B, H_, W_, C_, p(ch_), p(t), Tn, p(w), Wn, rho, p(e), p(pe), p(value), p(valid), space, None)

    def vjp(n_=n, K_=K, uv_=uv, img_=img, B=n, H_=Hh, W_=Ww, C_=Cc, ch_=None, t=None, Tn=1, w=None, Wn=1, rho=0.0, ge=out["energy"], gpe=None, gv=None,
            guv=out["guv"], gimg=out["gimg"], acc=0, space=0):
        return L.smplpp_image_term_vjp(0, n_, K_, p(uv_), p(img_), B, H_, W_, C_, p(ch_), p(t), Tn, p(w), Wn, rho, p(ge), p(gpe), p(gv), p(guv), p(gimg),
                                       acc, space, None)

    tgt, wgt = np.zeros((n, K, Cc), np.float32), np.ones((n, K), np.float32)
    common = [dict(n_=0), dict(n_=-1), dict(K_=0), dict(H_=1), dict(H_=8193), dict(W_=1), dict(W_=8193), dict(C_=0), dict(C_=33), dict(B=3), dict(B=0),
              dict(n_=2 ** 20, B=1, K_=2 ** 10), dict(n_=2 ** 31, B=1), dict(B=1, n_=1, H_=8192, W_=8192, C_=32), dict(uv_=None), dict(img_=None),
              dict(space=2), dict(space=-1), dict(ch_=np.array([0, 2, 1], np.int64)), dict(ch_=np.array([-1, 0, 1], np.int64))]
    calls = [(sample, kw) for kw in common + [dict(value=None, grad=None, valid=None)]]
    both = common + [dict(rho=-0.5), dict(rho=float("inf")), dict(rho=float("nan")), dict(t=tgt, Tn=3), dict(t=tgt, Tn=0), dict(w=wgt, Wn=3)]
    calls += [(term, kw) for kw in both + [dict(e=None, pe=None, value=None, valid=None)]]
    calls += [(vjp, kw) for kw in both + [dict(ge=None), dict(guv=None, gimg=None), dict(acc=2), dict(acc=-1)]]
    for fn, kw in calls:
        assert fn(**kw) == 1 and L.smplpp_last_error(), (fn.__name__, kw)
    # n K Cs 2 counts the sampled channels: the same n K passes the check with `channel` only (it is then refused for its space)
    assert "int32" in (term(n_=2 ** 14, B=1, K_=2 ** 13, C_=32, space=5), L.smplpp_last_error().decode())[1]
    assert "space" in (term(n_=2 ** 14, B=1, K_=2 ** 13, C_=32, ch_=ch, space=5), L.smplpp_last_error().decode())[1]
    assert all((a == 7).all() for a in out.values()) and (ok == 7).all()


# ---------------------------------------------------------------------------------------------------- 2. the restatement against float64
@pytest.mark.parametrize("rho", [0.0, 0.05])
@pytest.mark.parametrize("lead", [(0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1)], ids=lambda l: "B%dT%dW%d" % l)
@pytest.mark.parametrize("channel", [False, True])
@pytest.mark.parametrize("C", [1, 3, 32])
def test_restatement_against_float64(C, channel, lead, rho):
    """value, energy, grad_uv and grad_image of the restatement in float64 against autograd of the definition, to 1e-9: B, Tn and Wn
    each 1 or n, with and without `channel`, two weights of zero."""
    n, K = 3, 20
    image, uv, ch, target, weight, (ge, gpe, gv) = _case(n, K, C, channel, lead, seed=C + 7 * channel)
    X, I = torch.tensor(uv, requires_grad=True), torch.tensor(image, requires_grad=True)
    e = IM.energy_t(I, X, ch, target, weight, rho)
    s = IM.sample_t(I, X, ch)
    ((e.sum(1) * torch.tensor(ge)).sum() + (e * torch.tensor(gpe)).sum() + (s * torch.tensor(gv)).sum()).backward()
    energy, pe, value, valid = IM.term(image, uv, ch, target, weight, rho)
    guv, gimg = IM.term_vjp(image, uv, ch, target, weight, rho, ge, gpe, gv, np.zeros((n, K, 2)), np.zeros(image.shape), 0)
    errs = (_rel(value, s.detach().numpy()), _rel(pe, e.detach().numpy()), _rel(energy, e.detach().numpy().sum(1)), _rel(guv, X.grad.numpy()),
            _rel(gimg, I.grad.numpy()))
    print("float64 restatement: value %.3g, point energy %.3g, energy %.3g, grad_uv %.3g, grad_image %.3g" % errs)
    assert valid.all() and np.abs(X.grad.numpy()).max() > 0 and np.abs(I.grad.numpy()).max() > 0
    assert max(errs) <= 1e-9, errs
    # the sampled gradient alone is the derivative of the value, channel by channel
    Cs = value.shape[-1]
    grad = IM.sample(image, uv, ch)[1]
    for c in range(Cs):
        X2 = torch.tensor(uv, requires_grad=True)
        IM.sample_t(torch.tensor(image), X2, ch)[..., c].sum().backward()
        assert _rel(grad[..., c, :], X2.grad.numpy()) <= 1e-9
    # a point with weight 0 has energy +0, and without a cotangent of the value it contributes +0 to both gradients
    zero = np.broadcast_to(weight, (n, K)) == 0
    assert zero.sum() >= 2 and (pe[zero] == 0).all() and not np.signbit(pe[zero]).any()
    g0, _ = IM.term_vjp(image, uv, ch, target, weight, rho, ge, gpe, None, np.zeros((n, K, 2)), None, 0)
    assert (g0[zero] == 0).all()
    # storing and adding
    a, b = IM.term_vjp(image, uv, ch, target, weight, rho, ge, gpe, gv, guv.copy(), gimg.copy(), 1)
    assert np.array_equal(a, guv + guv) and np.array_equal(b, gimg + gimg)


# ---------------------------------------------------------------------------------------------------- 3. float32 within roundoff
@pytest.mark.parametrize("rho", [0.0, 0.05])
@pytest.mark.parametrize("C,channel", [(1, False), (3, False), (32, False), (32, True)])
def test_float32_forward_within_roundoff(C, channel, rho):
    """float32 against float64 on the same float32 inputs.  With u = 2^-24 and A the largest |pixel|: gx = u - 0.5 is exact for u >= 0.5
    (0.5 is a multiple of the ulp of u, and the difference is no larger than u), and so is f = g - i; so both runs interpolate with the
    same fractions.  A lerp a + f (b - a) rounds three times, on magnitudes of at most 2 A, 2 A and A: 5 u A; the second level carries
    the first level's 5 u A through a convex combination and adds its own: ds = 11 u A covers the two.  r = s - t: dr = ds + u |r|.
    q = sum_c r_c r_c over Cs terms, each product rounded once and each partial sum once: dq <= sum_c (2 |r_c| dr_c + dr_c^2) +
    (Cs + 2) u q.  point_energy = w q, or w p2 q / (p2 + q) whose slope in q is at most w, adds a few roundings of its own: 8 u e
    covers them.  The 1024-partial sum of K <= 1024 terms adds at most 11 u sum_k e."""
    n, K = 3, 40
    image, uv, ch, target, weight, _ = _case(n, K, C, channel, (1, 1, 1), seed=40 + C)
    i32, t32, w32 = image.astype(np.float32), target.astype(np.float32), weight.astype(np.float32)
    e32, pe32, s32, ok32 = IM.term(i32, uv.astype(np.float32), ch, t32, w32, rho)
    e64, pe64, s64, ok64 = IM.term(image, uv, ch, target, weight, float(np.float32(rho)))
    A = np.abs(image).max()
    ds = 11 * U * A
    assert s32.dtype == np.float32 and pe32.dtype == np.float32 and e32.dtype == np.float32 and ok32.all() and ok64.all()
    assert (np.abs(s32 - s64) <= ds).all(), np.abs(s32 - s64).max() / ds
    r = s64 - target
    dr = ds + U * np.abs(r)
    q = (r * r).sum(-1)
    dq = (2 * np.abs(r) * dr + dr * dr).sum(-1) + (r.shape[-1] + 2) * U * q
    bound = weight * dq + 8 * U * np.abs(pe64)
    assert (np.abs(pe32 - pe64) <= bound).all(), (np.abs(pe32 - pe64) / np.maximum(bound, 1e-300)).max()
    assert (np.abs(e32 - e64) <= bound.sum(1) + 11 * U * pe64.sum(1)).all()
    print("float32 forward: value error / bound %.3g, energy error / bound %.3g" %
          (np.abs(s32 - s64).max() / ds, (np.abs(pe32 - pe64) / np.maximum(bound, 1e-300)).max()))


def test_affine_image_is_reproduced():
    """Bilinear interpolation reproduces an affine image exactly in real arithmetic: the float32 sample of a u + b v + c, given at the pixel
    centres, is the plane at (u, v), and its gradient is (a, b).  The pixels are within u A of the plane (their rounding to float32),
    the fractions are exact, so the value is within 11 u A + u A.  ds/du = d_0 + fy (d_1 - d_0): a difference of two neighbouring pixels
    is within 2 u A of a before and u |a| after the subtraction; d_1 - d_0 is then within 4 u A + 2 u |a| of zero and is scaled by fy <=
    1; the product and the sum round on magnitudes of that size and of |a|: 8 u A + 4 u |a| covers it.  ds/dv = c_1 - c_0, each lerp
    within 6 u A of the plane: 12 u A + u |b|.  Both components are held to 14 u A + 4 u max(|a|, |b|)."""
    n, K, Hh, Ww = 2, 60, 11, 13
    a, b, c = 0.3, -0.5, 0.07
    v, u = np.meshgrid(np.arange(Hh) + 0.5, np.arange(Ww) + 0.5, indexing="ij")
    plane = np.stack([a * u + b * v + c, -b * u + 2 * a * v - c], -1)[None]  # [1,H,W,2]: a second channel with the slopes (-b, 2 a)
    uv = draw_uv(n, K, seed=3, Hh=Hh, Ww=Ww)
    s32, g32, ok = IM.sample(plane.astype(np.float32), uv.astype(np.float32))
    A = np.abs(plane).max()
    want = np.stack([a * uv[..., 0] + b * uv[..., 1] + c, -b * uv[..., 0] + 2 * a * uv[..., 1] - c], -1)
    slopes = np.array([[a, b], [-b, 2 * a]])
    ds, dgrad = 12 * U * A, 14 * U * A + 4 * U * np.abs(slopes).max()
    assert ok.all() and s32.dtype == np.float32
    assert (np.abs(s32 - want) <= ds).all(), np.abs(s32 - want).max() / ds
    assert (np.abs(g32 - slopes) <= dgrad).all(), np.abs(g32 - slopes).max() / dgrad
    print("affine image: value error / bound %.3g, gradient error / bound %.3g" % (np.abs(s32 - want).max() / ds, np.abs(g32 - slopes).max() / dgrad))


# ---------------------------------------------------------------------------------------------------- 4. special points
def test_rule_at_the_edges():
    """Pixel centres, far edges, one ulp outside each edge, points that are not finite, a NaN pixel and a channel out of range, in the
    restatement itself (W = 5, H = 4: the coordinates of the points below are exact in float32)."""
    Hh, Ww, Cc = 4, 5, 2
    img = IM.random_image(1, Hh, Ww, Cc, seed=8).astype(np.float32)
    j, i = np.meshgrid(np.arange(Hh), np.arange(Ww), indexing="ij")
    centres = np.stack([i + 0.5, j + 0.5], -1).astype(np.float32).reshape(1, -1, 2)
    s, g, ok = IM.sample(img, centres)
    s = s.reshape(Hh, Ww, Cc)
    # f = 0 returns the pixel itself; on a far edge f = 1, and a + 1 (b - a) is b within two roundings, twice
    assert ok.all() and np.array_equal(s[:-1, :-1], img[0, :-1, :-1]) and np.allclose(s, img[0], rtol=0, atol=8 * U * np.abs(img).max())
    assert np.array_equal(IM.sample(img, centres, np.ones(Hh * Ww, np.int64))[0][0, :, 0].reshape(Hh, Ww)[:-1, :-1], img[0, :-1, :-1, 1])
    mid = np.array([2.25, 1.75], np.float32)
    for a, top in ((0, Ww), (1, Hh)):
        for edge, way in ((np.float32(0.5), -np.inf), (np.float32(top - 0.5), np.inf)):
            on, off = mid.copy(), mid.copy()
            on[a], off[a] = edge, np.nextafter(edge, np.float32(way))
            assert IM.sample(img, on[None, None])[2] == 1 and IM.sample(img, off[None, None])[2] == 0
    for bad in (np.nan, np.inf, -np.inf):
        for a in (0, 1):
            p = mid.copy()
            p[a] = bad
            s, g, ok = IM.sample(img, p[None, None])
            assert ok == 0 and (s == 0).all() and (g == 0).all() and not np.signbit(s).any()
            e, pe, _, _ = IM.term(img, p[None, None], None, None, None, 0.05)
            assert e == 0 and pe == 0 and not np.signbit(pe).any()
    img[0, 1, 2, 0] = np.nan  # pixel (row 1, column 2), channel 0: it touches the cells i in {1, 2}, j in {0, 1}
    cells = (centres.reshape(Hh, Ww, 2)[:-1, :-1] + np.float32(0.5)).reshape(1, -1, 2)
    ok = IM.sample(img, cells)[2].reshape(Hh - 1, Ww - 1)
    touched = np.zeros_like(ok, bool)
    touched[0:2, 1:3] = True
    assert np.array_equal(ok == 0, touched)
    Kc = cells.shape[1]
    assert IM.sample(img, cells, np.ones(Kc, np.int64))[2].all()  # channel 1 holds no NaN
    assert np.array_equal(IM.sample(img, cells, np.zeros(Kc, np.int64))[2].reshape(Hh - 1, Ww - 1) == 0, touched)
    # a point that is not valid contributes to neither gradient, and leaves no NaN there
    gv = np.ones((1, Kc, Cc), np.float32)
    guv, gimg = IM.term_vjp(img, cells, None, None, None, 0.0, None, None, gv, np.zeros((1, Kc, 2), np.float32), np.zeros_like(img), 0)
    assert np.isfinite(guv).all() and np.isfinite(gimg).all() and (guv.reshape(Hh - 1, Ww - 1, 2)[touched] == 0).all()
    assert gimg[0, :, :, 1].sum() == pytest.approx(float((~touched).sum()), rel=1e-6)  # each valid point's four tap weights sum to 1
    # a channel outside [0, C) in device space: the point is not valid
    chan = np.ones(Kc, np.int64)
    chan[0], chan[1] = Cc, -1
    ok = IM.sample(img, cells, chan)[2][0]
    assert ok[:2].tolist() == [0, 0] and ok[2:].all()


# ---------------------------------------------------------------------------------------------------- 5. the GPU file's chains
def test_gradient_case_keeps_enough(synth_model):
    """The seed of test_image_gpu's gradient chain: the float64 run alone leaves out fewer than 20 % of the points."""
    case = IM.gradient_case(synth_model)
    near_edge = 1.0 - case["keep"].sum() / case["inside"].sum()
    skipped = 1.0 - case["keep"].mean()
    print("gradient chain: %.1f %% of the points left out (%.1f %% of the inside points are within %.2f px of a cell edge)" %
          (100 * skipped, 100 * near_edge, IM.MARGIN))
    assert skipped < 0.2


def test_fit_case_in_float64(synth_model):
    case = IM.fit_case(synth_model)
    err = IM.fit_float64(case)
    at = [0, 1, 5, 10, 20, 40, 80]
    print("float64 fit: mean reprojection error (px) at steps %s: %s" % (at, np.round(err[at], 3)))
    start = np.linalg.norm(case["uv_start"] - case["uv_true"], axis=-1)
    print("start: the joints are %.2f px from their peaks on average, %.2f px at most (sigma = %g)" % (start.mean(), start.max(), IM.FIT_SIGMA))
    assert start.max() <= 1.6 * IM.FIT_SIGMA and start.mean() > 0.25 * IM.FIT_SIGMA
    assert err[-1] < 0.5 * err[0]
