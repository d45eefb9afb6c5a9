"""The image term on the MI355X (smplpp_image_sample, smplpp_image_term, smplpp_image_term_vjp): every bit against the numpy restatement
of tests/image_oracle.py; points on pixel centres, on far edges, one ulp outside every edge, not finite, and in cells with a NaN pixel;
grad_image under collision; independence of the batch, the slot, the memory space and the outputs asked for; the refusals; the C++ shim;
the gradient through FK, the landmarks and the projection against float64 autograd; and a fit to joint heatmaps."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import image_oracle as IM  # noqa: E402
import keypoints_oracle as KP  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 7.0
f32 = np.float32
SIZES = ((2, 2), (5, 4), (33, 9))        # (W, H): unequal sides catch a swapped stride
CS = (1, 3, 4, 5, 32)                    # 4 and 32: the 16-byte reads; 5: a last channel group of one
KS = (1, 63, 64, 65, 1024, 1025, 1030)   # the work split changes after 64 and after 1024
COTANGENTS = [c for c in itertools.product((False, True), repeat=3) if any(c)]


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


def _image(B, W, H, C, seed, nan_pixel=True):
    """[B,H,W,C] float32; with room for it, pixel (row 0, column 3) of image 0 is NaN in channel 0: it touches the cells (2, 0) and
    (3, 0), not the first cell nor the last."""
    img = IM.random_image(B, H, W, C, seed).astype(f32)
    if nan_pixel and W > 4:
        img[0, 0, 3, 0] = np.nan
    return img


def _specials(W, H):
    """[S,2] float32: the pixel centres at the corners of the first and of the last cell (far edges: f = 1), a point inside the last cell,
    on each of the four edges and one ulp outside it, points that are not finite, and (W > 4) the centres of the two cells that touch
    the NaN pixel and of two that do not."""
    corners = np.array(list(itertools.product((0, 1), repeat=2)), np.float64)
    top = np.array([W - 1, H - 1], np.float64)
    pts = [(0.5 + np.concatenate([corners, top - corners, (top - 1)[None] + 0.25])).astype(f32)]
    mid = (0.5 + np.array([0.25, 0.6]) * top).astype(f32)  # (its cell, and those of the edge points below, are clear of the NaN pixel)
    for a in range(2):
        for edge, way in ((f32(0.5), -np.inf), (f32(top[a] + 0.5), np.inf)):
            p = mid.copy()
            p[a] = edge
            q = p.copy()
            q[a] = np.nextafter(edge, f32(way))
            pts.append(np.stack([p, q]))
    bad = np.repeat(mid[None], 5, 0)
    bad[0, 0], bad[1, 1], bad[2, 0], bad[3, 1], bad[4] = np.nan, np.inf, -np.inf, -np.inf, np.nan
    pts.append(bad)
    if W > 4:
        pts.append(np.array([[3.0, 1.0], [4.0, 1.0], [1.0, 1.0], [2.0, 1.0]], f32))  # the cells (2, 0), (3, 0), (0, 0), (1, 0)
    return np.concatenate(pts)


def _points(n, K, W, H, seed, span=(-0.1, 1.1)):
    """[n,K,2] float32: random points over the image and a tenth of its size beyond it, with the special points spread among them."""
    rng = np.random.default_rng(seed)
    uv = (0.5 + rng.uniform(span[0], span[1], (n * K, 2)) * np.array([W - 1, H - 1])).astype(f32)
    S = _specials(W, H)
    at = (np.arange(len(S)) * 7 + seed) % (n * K)
    uv[at] = S
    return uv.reshape(n, K, 2)


def _terms(n, K, Cs, mode, seed):
    """target and weight: absent (mode 0), shared (1) or per frame (2), every third weight 0."""
    if mode == 0:
        return None, None
    rng = np.random.default_rng(seed)
    lead = 1 if mode == 1 else n
    w = rng.uniform(0.25, 2.0, (lead, K)).astype(f32)
    w[:, ::3] = 0
    return rng.normal(0, 0.5, (lead, K, Cs)).astype(f32), w


def _check_all(img, uv, ch, target, weight, rho, seed, cots, case):
    """Every output of the three calls on device tensors against the restatement; the cotangent combinations `cots`, storing and adding,
    both gradients together and each alone."""
    from smplpp_amd import image as I

    n, K = uv.shape[:2]
    d_img, d_uv, d_ch, d_t, d_w = _dev(img), _dev(uv), _dev(ch), _dev(target), _dev(weight)
    value, grad, valid = IM.sample(img, uv, ch)
    r = I.sample(d_uv, d_img, d_ch)
    assert _same(r["value"], value) and _same(r["gradient"], grad) and _same(r["valid"], valid), case
    energy, pe, tv, tok = IM.term(img, uv, ch, target, weight, rho)
    r = I.term(d_uv, d_img, d_t, d_w, rho, d_ch)
    assert _same(r["energy"], energy) and _same(r["point_energy"], pe) and _same(r["value"], tv) and _same(r["valid"], tok), case
    assert not np.isnan(energy).any()
    # the frame energy alone (the kernels with the sum) and the per-point outputs alone (a thread per point) give the same bits
    assert _same(I.term(d_uv, d_img, d_t, d_w, rho, d_ch, want=("energy",))["energy"], energy), case
    assert _same(I.term(d_uv, d_img, d_t, d_w, rho, d_ch, want=("point_energy",))["point_energy"], pe), case
    rng = np.random.default_rng(seed)
    Cs = value.shape[-1]
    ge, gpe, gv = rng.normal(size=n).astype(f32), rng.normal(size=(n, K)).astype(f32), rng.normal(size=(n, K, Cs)).astype(f32)
    gpe[:, ::5] = 0
    for he, hp, hv in cots:
        a, b, c = ge if he else None, gpe if hp else None, gv if hv else None
        wu, wi = IM.term_vjp(img, uv, ch, target, weight, rho, a, b, c, np.full((n, K, 2), FILL, f32), np.full(img.shape, FILL, f32), 0)
        kw = dict(grad_energy=_dev(a), grad_point_energy=_dev(b), grad_value=_dev(c))
        got = I.termBackward(d_uv, d_img, d_t, d_w, rho, d_ch, **kw)
        assert _same(got["uv"], wu) and _same(got["image"], wi), (case, he, hp, hv)
        wu2, wi2 = IM.term_vjp(img, uv, ch, target, weight, rho, a, b, c, wu.copy(), wi.copy(), 1)
        again = I.termBackward(d_uv, d_img, d_t, d_w, rho, d_ch, out=got, **kw)
        assert again is got and _same(got["uv"], wu2) and _same(got["image"], wi2), (case, he, hp, hv)
        assert _same(I.termBackward(d_uv, d_img, d_t, d_w, rho, d_ch, want=("uv",), **kw)["uv"], wu), (case, he, hp, hv)
        assert _same(I.termBackward(d_uv, d_img, d_t, d_w, rho, d_ch, want=("image",), **kw)["image"], wi), (case, he, hp, hv)
    return dict(valid=valid, energy=energy)


# ---------------------------------------------------------------------------------------------------- 1. bits
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_bits(size, C):
    """All three calls for every K at which the work split changes and n = 1 and 3.  Along the fourteen (K, n) the other choices take
    turns, so that each C and size meets every one of them several times: with and without `channel`, B = 1 and n, rho = 0 and 0.05,
    targets and weights absent, shared and per frame.  All seven cotangent combinations up to K = 65, two of them above."""
    W, H = size
    seen = set()
    for i, (K, n) in enumerate(itertools.product(KS, (1, 3))):
        ki, ni = i // 2, i % 2
        channel, per_frame, rho, mode = (ki + ni + C + W) % 2 == 1, (ki // 2 + ni) % 2 == 1, (0.0, 0.05)[(ki + C) % 2], (ki + ni + C) % 3
        seen.add((channel, per_frame, rho, mode))
        img = _image(n if per_frame else 1, W, H, C, seed=i + C)
        uv = _points(n, K, W, H, seed=i)
        ch = np.random.default_rng(i).integers(0, C, K) if channel else None
        target, weight = _terms(n, K, 1 if channel else C, mode, seed=50 + i)
        cots = COTANGENTS if K <= 65 else [(True, True, True), COTANGENTS[i % 7]]
        out = _check_all(img, uv, ch, target, weight, rho, 100 + i, cots, (size, C, K, n, channel, per_frame, rho, mode))
        if K >= 63:
            assert (out["valid"] == 0).any() and (out["valid"] == 1).any()
    assert len({s[0] for s in seen}) == 2 and len({s[1] for s in seen}) == 2 and len({s[2] for s in seen}) == 2 and len({s[3] for s in seen}) == 3


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_special_points(size):
    """The special points alone: far edges belong to the last cell, one ulp outside is outside, a point that is not finite is not valid,
    a NaN pixel takes out the cells that touch it and no others (and none when another channel is read), a device-space channel outside
    [0, C) makes its point not valid, and with weight zero such a point has energy +0."""
    from smplpp_amd import image as I

    W, H = size
    C = 3
    img = _image(1, W, H, C, seed=3)
    S = _specials(W, H)[None]
    K = S.shape[1]
    value, grad, valid = IM.sample(img, S)
    r = I.sample(_dev(S), _dev(img))
    assert _same(r["value"], value) and _same(r["gradient"], grad) and _same(r["valid"], valid)
    assert valid[0, :9].all()                                     # the corners of the first and last cell, and inside the last cell
    assert valid[0, 9:17].tolist() == [1, 0, 1, 0, 1, 0, 1, 0]    # on each edge, and one ulp outside it
    assert (valid[0, 17:22] == 0).all()                           # not finite
    w = np.ones((1, K), f32)
    w[0, -4:] = 0
    energy, pe, tv, tok = IM.term(img, S, None, None, w, 0.05)
    t = I.term(_dev(S), _dev(img), None, _dev(w), 0.05)
    assert _same(t["energy"], energy) and _same(t["point_energy"], pe) and _same(t["value"], tv) and _same(t["valid"], tok)
    if W > 4:
        assert valid[0, -4:].tolist() == [0, 0, 1, 1]  # the two cells at the NaN pixel, and two that are clear
        assert (pe[0, -4:] == 0).all() and not np.signbit(pe[0, -4:]).any() and (value[0, -4:-2] == 0).all()
        ones = np.ones(K, np.int64)
        r = I.sample(_dev(S), _dev(img), _dev(ones))
        want = IM.sample(img, S, ones)
        assert _same(r["value"], want[0]) and _same(r["valid"], want[2]) and want[2][0, -4:].all()  # channel 1 holds no NaN
    # channels out of range, on the device only (host space refuses them)
    ch = np.arange(K, dtype=np.int64) % C
    ch[0], ch[1], ch[4] = C, -1, 2 ** 40
    want = IM.sample(img, S, ch)
    r = I.sample(_dev(S), _dev(img), _dev(ch))
    assert _same(r["value"], want[0]) and _same(r["gradient"], want[1]) and _same(r["valid"], want[2]) and want[2][0, [0, 1, 4]].tolist() == [0, 0, 0]
    gv = np.ones((1, K, 1), f32)
    wu, wi = IM.term_vjp(img, S, ch, None, None, 0.0, None, None, gv, np.zeros((1, K, 2), f32), np.zeros_like(img), 0)
    got = I.termBackward(_dev(S), _dev(img), None, None, 0.0, _dev(ch), grad_value=_dev(gv))
    assert _same(got["uv"], wu) and _same(got["image"], wi) and np.isfinite(wi).all()


# ---------------------------------------------------------------------------------------------------- 2. grad_image under collision
@pytest.mark.parametrize("channel", [False, True])
def test_grad_image_under_collision(channel):
    """Every point of three frames of 1030 in the one cell of a shared 2 x 2 image: each pixel element is one sum of up to 3090 shares in
    ascending point index.  Then each frame into its own image."""
    from smplpp_amd import image as I

    n, K, C = 3, 1030, 3
    rng = np.random.default_rng(5)
    uv = (0.5 + rng.uniform(0, 1, (n, K, 2))).astype(f32)
    ch = rng.integers(0, C, K) if channel else None
    Cs = 1 if channel else C
    target, weight = _terms(n, K, Cs, 2, seed=6)
    ge, gv = rng.normal(size=n).astype(f32), rng.normal(size=(n, K, Cs)).astype(f32)
    for B in (1, n):
        img = _image(B, 2, 2, C, seed=7 + B)
        _, want = IM.term_vjp(img, uv, ch, target, weight, 0.05, ge, None, gv, None, np.zeros_like(img), 0)
        got = I.termBackward(_dev(uv), _dev(img), _dev(target), _dev(weight), 0.05, _dev(ch), grad_energy=_dev(ge), grad_value=_dev(gv), want=("image",))
        assert _same(got["image"], want) and (want != 0).all(), B
        # a second run gives the same bits: the order is fixed
        again = I.termBackward(_dev(uv), _dev(img), _dev(target), _dev(weight), 0.05, _dev(ch), grad_energy=_dev(ge), grad_value=_dev(gv), want=("image",))
        assert _same(again["image"], want)


def test_grad_image_sparse():
    """Five points on a 70 x 40 image (five tiles by three) with five channels: the pixels no point touches are +0 when storing, and keep
    their value when adding."""
    from smplpp_amd import image as I

    W, H, C, n, K = 70, 40, 5, 1, 5
    img = _image(1, W, H, C, seed=9, nan_pixel=False)
    uv = np.array([[[0.5, 0.5], [15.9, 15.9], [16.5, 16.2], [69.5, 39.5], [40.25, 20.75]]], f32)  # corners, a tile border, the far corner
    gv = np.random.default_rng(10).normal(size=(n, K, C)).astype(f32)
    _, want = IM.term_vjp(img, uv, None, None, None, 0.0, None, None, gv, None, np.full(img.shape, FILL, f32), 0)
    got = I.termBackward(_dev(uv), _dev(img), grad_value=_dev(gv), want=("image",))["image"]
    assert _same(got, want)
    assert 0 < (want != 0).sum() <= 4 * K * C and not np.signbit(want[want == 0]).any() and not np.signbit(_host(got)[want == 0]).any()
    base = np.full(img.shape, FILL, f32)
    _, want2 = IM.term_vjp(img, uv, None, None, None, 0.0, None, None, gv, None, base.copy(), 1)
    out = {"image": _dev(base)}
    I.termBackward(_dev(uv), _dev(img), grad_value=_dev(gv), out=out)
    assert _same(out["image"], want2) and (want2 == FILL).sum() >= img.size - 4 * K * C


# ---------------------------------------------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("K", [24, 65, 1030])
def test_independence(K):
    """A frame's bits alone, among others, in another slot, in host and device space, and with single outputs (B = n: the frame has its
    own image, and its slice of grad_image is its own)."""
    from smplpp_amd import image as I

    W, H, C, rho = 33, 9, 4, 0.05
    own_uv = _points(1, K, W, H, seed=6)[0]
    own_img = _image(1, W, H, C, seed=5)[0]
    rng = np.random.default_rng(8)
    own_t, own_w = rng.normal(0, 0.5, (K, C)).astype(f32), rng.uniform(0.25, 2.0, K).astype(f32)
    own_w[::4] = 0
    ge, gpe, gv = f32(0.75), rng.normal(size=K).astype(f32), rng.normal(size=(K, C)).astype(f32)
    ref = None
    for n, slot in ((1, 0), (3, 1), (4, 3)):
        uv, img = _points(n, K, W, H, seed=20 + n), _image(n, W, H, C, seed=30 + n)
        t, w = rng.normal(0, 0.5, (n, K, C)).astype(f32), rng.uniform(0.25, 2.0, (n, K)).astype(f32)
        g_e, g_pe, g_v = rng.normal(size=n).astype(f32), rng.normal(size=(n, K)).astype(f32), rng.normal(size=(n, K, C)).astype(f32)
        uv[slot], img[slot], t[slot], w[slot], g_e[slot], g_pe[slot], g_v[slot] = own_uv, own_img, own_t, own_w, ge, gpe, gv
        for dev in (True, False):
            p = (lambda a: _dev(a)) if dev else (lambda a: a)
            out = dict(I.sample(p(uv), p(img)))
            out.update({"t_" + k: v for k, v in I.term(p(uv), p(img), p(t), p(w), rho).items()})
            out.update({"g_" + k: v for k, v in I.termBackward(p(uv), p(img), p(t), p(w), rho, None, p(g_e), p(g_pe), p(g_v)).items()})
            mine = {k: _host(v)[slot] for k, v in out.items()}
            if ref is None:
                ref = mine
            for k in ref:
                assert _same(np.asarray(mine[k]), np.asarray(ref[k])), (n, slot, dev, k)
        for k in ("value", "gradient", "valid"):
            assert _same(_host(I.sample(_dev(uv), _dev(img), want=(k,))[k])[slot], ref[k]), k
        for k in ("energy", "point_energy", "value", "valid"):
            assert _same(np.asarray(_host(I.term(_dev(uv), _dev(img), _dev(t), _dev(w), rho, want=(k,))[k])[slot]), np.asarray(ref["t_" + k])), k
        for k in ("uv", "image"):
            got = I.termBackward(_dev(uv), _dev(img), _dev(t), _dev(w), rho, None, _dev(g_e), _dev(g_pe), _dev(g_v), want=(k,))[k]
            assert _same(_host(got)[slot], ref["g_" + k]), k
    # and the restatement agrees with what all of them gave
    one = lambda a: a[None]  # noqa: E731
    wu, wi = IM.term_vjp(one(own_img), one(own_uv), None, one(own_t), one(own_w), rho, np.array([ge]), one(gpe), one(gv), np.zeros((1, K, 2), f32),
                         np.zeros((1, H, W, C), f32), 0)
    assert _same(ref["g_uv"], wu[0]) and _same(ref["g_image"], wi[0])


# ---------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals():
    """Every refusal of the list on device tensors: SMPLPP_ERR_INVALID, and the outputs keep their values."""
    from smplpp_amd import _lib

    Lb = _lib.load()
    n, K, H, W, C = 2, 4, 4, 5, 2
    dev = lambda *shape: torch.full(shape, FILL, device="cuda")  # noqa: E731
    uv = _dev(_points(n, K, W, H, seed=1))
    img = _dev(_image(n, W, H, C, seed=2))
    outs = dict(value=dev(n, K, C), gradient=dev(n, K, C, 2), energy=dev(n), pe=dev(n, K), guv=dev(n, K, 2), gimg=dev(n, H, W, C))
    valid = torch.full((n, K), 7, dtype=torch.uint8, device="cuda")
    tgt, wgt = dev(n, K, C), dev(n, K)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    D = _lib.DEVICE

    def sample(n_=n, K_=K, uv_=uv, img_=img, B=n, H_=H, W_=W, C_=C, ch=None, value=outs["value"], grad=outs["gradient"], ok=valid, space=D):
        return Lb.smplpp_image_sample(0, n_, K_, P(uv_), P(img_), B, H_, W_, C_, ch, P(value), P(grad), P(ok), space, None)

    def term(n_=n, K_=K, uv_=uv, img_=img, B=n, H_=H, W_=W, C_=C, ch=None, t=None, Tn=1, w=None, Wn=1, rho=0.0, e=outs["energy"], pe=outs["pe"],
             value=outs["value"], ok=valid, space=D):
        return Lb.smplpp_image_term(0, n_, K_, P(uv_), P(img_), B, H_, W_, C_, ch, P(t), Tn, P(w), Wn, rho, P(e), P(pe), P(value), P(ok), space, None)

    def vjp(n_=n, K_=K, uv_=uv, img_=img, B=n, H_=H, W_=W, C_=C, ch=None, t=None, Tn=1, w=None, Wn=1, rho=0.0, ge=outs["energy"], gpe=None, gv=None,
            guv=outs["guv"], gimg=outs["gimg"], acc=0, space=D):
        return Lb.smplpp_image_term_vjp(0, n_, K_, P(uv_), P(img_), B, H_, W_, C_, ch, P(t), Tn, P(w), Wn, rho, P(ge), P(gpe), P(gv), P(guv), P(gimg),
                                        acc, space, None)

    common = [dict(n_=0), dict(n_=-1), dict(K_=0), dict(H_=1), dict(H_=8193), dict(W_=1), dict(W_=8193), dict(C_=0), dict(C_=33), dict(B=3), dict(B=0),
              dict(n_=2 ** 20, B=1, K_=2 ** 10), dict(B=1, n_=1, H_=8192, W_=8192, C_=32), dict(uv_=None), dict(img_=None), dict(space=2)]
    both = common + [dict(rho=-0.5), dict(rho=float("inf")), dict(rho=float("nan")), dict(t=tgt, Tn=3), dict(w=wgt, Wn=0)]
    refused = [sample(**kw) for kw in common + [dict(value=None, grad=None, ok=None)]]
    refused += [term(**kw) for kw in both + [dict(e=None, pe=None, value=None, ok=None)]]
    refused += [vjp(**kw) for kw in both + [dict(ge=None), dict(guv=None, gimg=None), dict(acc=2), dict(acc=-1)]]
    # a host-space channel entry outside [0, C)
    bad = np.array([0, 1, C, 0], np.int64)
    h_uv, h_img = _host(uv), _host(img)
    h_out = np.full((n, K, 1), FILL, f32)
    refused.append(Lb.smplpp_image_sample(0, n, K, h_uv.ctypes.data, h_img.ctypes.data, n, H, W, C, bad.ctypes.data, h_out.ctypes.data, None, None, _lib.HOST, None))
    torch.cuda.synchronize()
    assert all(rc == 1 for rc in refused), refused
    for k, t in outs.items():
        assert (t == FILL).all(), k
    assert (valid == 7).all() and (h_out == FILL).all()
    # and the same calls go through once the argument is put right
    assert sample() == 0 and term() == 0 and vjp() == 0 and term(t=tgt, Tn=n, w=wgt, Wn=n) == 0 and sample(n_=1, B=1, K_=n * K) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 5. C++ shim
def test_image_cpp_shim(tmp_path):
    exe = str(tmp_path / "image_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "image_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    H, W, C, n, K = 4, 5, 3, 2, 6
    i = np.arange(H * W * C)
    img = (((i * 7) % 13 - 6).astype(f32) * f32(0.0625)).reshape(1, H, W, C)
    j = np.arange(n * K)
    uv = np.stack([f32(0.75) + f32(0.3125) * (j % 11).astype(f32), f32(0.625) + f32(0.4375) * (j % 7).astype(f32)], -1).astype(f32)
    uv[4, 0] = 7.0
    uv = uv.reshape(n, K, 2)
    gpe = (f32(0.5) - f32(0.125) * j.astype(f32)).reshape(n, K)
    m = np.arange(n * K * C)
    target = (f32(0.125) * (m % 5).astype(f32) - f32(0.25)).reshape(n, K, C)
    gv = (f32(-0.25) + f32(0.0625) * (m % 9).astype(f32)).reshape(n, K, C)
    weight = np.array([[1.0, 0.5, 0.0, 2.0, 1.0, 0.75]], f32)
    ge = np.array([1.0, -0.5], f32)
    ch = np.array([2, 0, 1, 1, 2, 0], np.int64)
    value, grad, valid = IM.sample(img, uv)
    energy, pe, tv, tok = IM.term(img, uv, None, target, weight, 0.25)
    u1, i1 = IM.term_vjp(img, uv, None, target, weight, 0.25, ge, gpe, gv, np.zeros((n, K, 2), f32), np.zeros_like(img), 0)
    u2, i2 = IM.term_vjp(img, uv, None, target, weight, 0.25, ge, None, None, u1.copy(), i1.copy(), 1)
    _, i3 = IM.term_vjp(img, uv, ch, None, weight, 0.0, ge, None, None, None, np.zeros_like(img), 0)
    want = [value, grad, valid.astype(f32), energy, pe, tv, tok.astype(f32), u1, i1, u2, i2, IM.sample(img, uv, ch)[0], IM.term(img, uv, ch, None, weight, 0.0)[0], i3]
    assert valid.sum() not in (0, n * K) and (value != 0).any() and (i3 != 0).any()
    raw = open(outp, "rb").read()
    assert len(raw) == 4 * sum(a.size for a in want)
    off = 0
    for k, a in enumerate(want):
        got = np.frombuffer(raw, f32, a.size, off).reshape(a.shape)
        off += 4 * a.size
        assert _same(got, np.ascontiguousarray(a)), k


# ---------------------------------------------------------------------------------------------------- 6. the gradient and the fit
def _smpl(model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    return s


def test_gradient_through_the_chain(synth_model):
    """theta, beta, camera -> smplpp_fk -> Landmarks -> project_points_differentiable -> term_differentiable -> sum on the synthetic
    model, n = 2, a smooth 96 x 96 image of Gaussian blobs with C = 3, against float64 autograd of the same graph, within max(4 x the
    error of fp32 autograd, 1e-5): theta, beta, the 16 camera entries and the image.  A point whose float64 gx or gy lies within 0.02 px
    of a cell edge has weight 0 on every side (the interpolant's derivative jumps there, and the two precisions may choose different
    cells): fewer than 20 % are left out (image_oracle.gradient_case, checked in test_image_cpu)."""
    import test_pose_prior_gpu as TP
    from smplpp_amd import image as I
    from smplpp_amd import smpl as S
    from smplpp_amd.landmarks import Landmarks

    case = IM.gradient_case(synth_model)
    keep = case["keep"]
    assert 1.0 - keep.mean() < 0.2
    print("points in the graph: %.1f %%" % (100 * keep.mean()))
    weight = (case["weight"] * keep).astype(f32)
    rho = case["rho"]
    s = _smpl(synth_model)
    lm = Landmarks(s, *case["reg"])
    beta, theta, cam, img = (_dev(case[k]).requires_grad_(True) for k in ("beta", "theta", "camera", "image"))
    verts, joints = s.forward_differentiable(beta, theta)
    K = keep.shape[1]
    uv, _, valid = S.project_points_differentiable(lm.forward_differentiable(verts, joints), cam, torch.zeros(2, K, 3, device="cuda"), 0.0, IM.NEAR)
    energy = I.term_differentiable(uv, img, _dev(case["target"]), _dev(weight), rho)
    energy.sum().backward()

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        b, t, c, im = (torch.tensor(case[k], dtype=dtype, requires_grad=True) for k in ("beta", "theta", "camera", "image"))
        out = FK.fk(m, b, t)
        uvr, _ = KP.project_t(KP.landmarks_t(torch.tensor(case["dense"], dtype=dtype), out["verts"], out["joints"]), c, IM.NEAR)
        kept = torch.tensor(keep[..., None])
        safe = torch.where(kept, uvr, torch.full_like(uvr, 1.0))  # (a point that is left out, or outside, has weight 0)
        e = IM.energy_t(im, safe, None, case["target"], weight, rho).sum(1)
        e.sum().backward()
        return [x.detach().double().numpy() for x in (e, b.grad, t.grad, c.grad, im.grad)]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert np.allclose(_host(energy.detach()), r64[0], rtol=1e-4)
    TP._bar(beta.grad, r64[1], r32[1], "image term through the chain, beta")
    TP._bar(theta.grad, r64[2], r32[2], "image term through the chain, theta")
    for name, sl in (("R", slice(0, 9)), ("t", slice(9, 12)), ("f", slice(12, 14)), ("c", slice(14, 16))):
        TP._bar(cam.grad[:, sl], r64[3][:, sl], r32[3][:, sl], "image term through the chain, camera " + name)
    TP._bar(img.grad, r64[4], r32[4], "image term through the chain, image")
    # sample_differentiable: the value's own gradient to uv and to the image
    uv0 = uv.detach().clone().requires_grad_(True)
    img0 = img.detach().clone().requires_grad_(True)
    kk = _dev(keep.astype(f32))[..., None]
    (I.sample_differentiable(uv0, img0) * kk).sum().backward()

    def ref_value(dtype):
        u, im = torch.tensor(_host(uv.detach()), dtype=dtype, requires_grad=True), torch.tensor(case["image"], dtype=dtype, requires_grad=True)
        safe = torch.where(torch.tensor(keep[..., None]), u, torch.full_like(u, 1.0))
        (IM.sample_t(im, safe) * torch.tensor(keep[..., None], dtype=dtype)).sum().backward()
        return u.grad.double().numpy(), im.grad.double().numpy()

    v64, v32 = ref_value(torch.float64), ref_value(torch.float32)
    TP._bar(uv0.grad, v64[0], v32[0], "sampled value, uv")
    TP._bar(img0.grad, v64[1], v32[1], "sampled value, image")


def test_fit_to_heatmaps(synth_model):
    """Two bodies, 24 joint heatmaps each (Gaussians of sigma = 4 px at the true projections, 96 x 96) read through `channel`, target 1,
    weight from valid; from a start with every joint within about 1.5 sigma, 80 Adam steps on trans and the rotations.  The mean
    reprojection error must fall, and end within 2x of the identical schedule in float64 on the CPU (image_oracle.fit_float64).  See
    DESIGN 3.24 for both trajectories."""
    from smplpp_amd import image as I
    from smplpp_amd import smpl as S
    from smplpp_amd.landmarks import Landmarks

    case = IM.fit_case(synth_model)
    e64 = IM.fit_float64(case)
    s = _smpl(synth_model)
    lm = Landmarks(s, *case["reg"])
    beta, cam, heat = _dev(case["beta"]), _dev(case["camera"]), _dev(case["heat"])
    trans, rot = _dev(case["theta"][:, :1]).requires_grad_(True), _dev(case["theta"][:, 1:]).requires_grad_(True)
    channel = _dev(case["channel"].astype(np.int64))
    target, no_target = torch.ones(1, 24, 1, device="cuda"), torch.zeros(2, 24, 3, device="cuda")
    uv_true = _dev(case["uv_true"].astype(f32))
    opt = torch.optim.Adam([trans, rot], lr=IM.FIT_LR)
    errors = []

    def evaluate():
        verts, joints = s.forward_differentiable(beta, torch.cat([trans, rot], 1))
        uv, _, _ = S.project_points_differentiable(lm.forward_differentiable(verts, joints), cam, no_target, 0.0, IM.NEAR)
        errors.append(float((uv.detach() - uv_true).norm(dim=-1).mean()))
        valid = I.sample(uv.detach(), heat, channel, want=("valid",))["valid"]
        return I.term_differentiable(uv, heat, target, valid.float(), 0.0, channel).sum()

    for _ in range(IM.FIT_STEPS):
        opt.zero_grad()
        evaluate().backward()
        opt.step()
    with torch.no_grad():
        evaluate()
    at = [0, 1, 5, 10, 20, 40, 80]
    print("float64: mean reprojection error (px) at steps %s: %s" % (at, np.round(e64[at], 3)))
    print("MI355X:  mean reprojection error (px) at steps %s: %s" % (at, np.round(np.array(errors)[at], 3)))
    assert abs(errors[0] - e64[0]) < 1e-3
    assert errors[-1] < errors[0] and errors[-1] <= 2 * e64[-1], (errors[-1], e64[-1])
