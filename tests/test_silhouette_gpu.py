"""The silhouette term on the MI355X (smplpp_mask_distance_transform, smplpp_silhouette, smplpp_silhouette_vjp): every output bit of
the transform and of the two residual sets against the numpy restatement; independence of batch, slot, space and the rasteriser's
work split; the backward pass against float64 autograd of the restated loss and its call rules; refusals; the chain to theta and
beta against float64 finite differences; a fit that the depth term cannot make; and the C++ shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_raster_oracle as DR  # noqa: E402
import silhouette_oracle as SO  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402
from test_silhouette_cpu import MASKS  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("vert_target", "vert_sq", "pix_source", "pix_sq")


def _synth(synth_model, env=None):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        s.init(synth_model)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    return s


@pytest.fixture(scope="module")
def smpl(synth_model):
    return _synth(synth_model)


@pytest.fixture(scope="module")
def faces(synth_model):
    return synth_model["face_indices"].astype(np.int64) - 1


def _pose(smpl, n, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    theta = np.zeros((n, 25, 3), np.float32)
    theta[:, 1:] = rng.normal(0, scale, (n, 24, 3))
    return theta


def _cams(verts, H, W, views):
    return np.stack([DR.look_at_camera((v.min(0) + v.max(0)) / 2, d, yaw, H, W) for v, (d, yaw) in zip(verts, views)])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


# ---------------------------------------------------------------------------------------------------- the transform
def _check_transform(got, want, what):
    for name, g, w in zip(("nearest", "sqdist"), got, want):
        g = _host(g)
        assert g.dtype == w.dtype and _same_bits(g, w), (what, name, int((g != w).sum()))


def test_transform_bits_on_the_hand_masks(smpl):
    alone = {}
    for name, m in MASKS.items():
        alone[name] = smpl.maskDistanceTransform(m[None])
        _check_transform(alone[name], SO.transform_batch(m[None]), name)
    # a frame's bits inside a batch, at several slots; host and device space; each output alone
    same = [k for k, m in MASKS.items() if m.shape == (9, 11)]
    assert len(same) >= 6
    batch = np.stack([MASKS[k] for k in same] + [MASKS[same[0]]] * 3 + [MASKS[same[2]]])
    order = same + [same[0]] * 3 + [same[2]]
    host = smpl.maskDistanceTransform(batch)
    dev = smpl.maskDistanceTransform(_dev(batch))
    for slot, k in enumerate(order):
        for o in range(2):
            assert _same_bits(host[o][slot], alone[k][o][0]) and _same_bits(_host(dev[o])[slot], alone[k][o][0]), (slot, k, o)
    n_only, none = smpl.maskDistanceTransform(batch, want=("nearest",))
    none2, d_only = smpl.maskDistanceTransform(_dev(batch), want=("sqdist",))
    assert none is None and none2 is None and _same_bits(n_only, host[0]) and _same_bits(_host(d_only), host[1])
    # a boolean mask is a mask
    assert _same_bits(smpl.maskDistanceTransform(batch.astype(bool))[0], host[0])


@pytest.mark.parametrize("H,W", [(128, 128), (256, 256), (384, 512)])
def test_transform_bits_on_rendered_coverage(smpl, faces, H, W):
    """Brute force over all set pixels up to 256 x 256; at 384 x 512 the separable restatement, which test_silhouette_cpu.py pins to
    the brute force."""
    v = smpl.launch(np.zeros((3, 10), np.float32), _pose(smpl, 3, 17), want=("verts",))["verts"]
    cams = _cams(v, H, W, ((2.5, 0.0), (2.5, 0.7), (6.0, -0.4)))
    cov = (smpl.depthRaster(v, cams, H, W, want=())["face"] >= 0).astype(np.uint8)
    assert cov.any(axis=(1, 2)).all() and not cov.all()
    restate = SO.feature_transform if H * W <= 256 * 256 else SO.feature_transform_separable
    want = [restate(c) for c in cov]
    want = (np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))
    got = smpl.maskDistanceTransform(cov)
    _check_transform(got, want, (H, W))
    _check_transform(smpl.maskDistanceTransform(_dev(cov)), want, (H, W, "device"))
    one = smpl.maskDistanceTransform(cov[2:3])
    assert _same_bits(one[0][0], got[0][2]) and _same_bits(one[1][0], got[1][2])


# ---------------------------------------------------------------------------------------------------- the residuals
@pytest.fixture(scope="module")
def scene(smpl, faces):
    """Eight frames at 96 x 128: two usual views against a mask rendered from a displaced pose (root moved sideways, pose perturbed), a
    close camera (vertices that project outside the image), an empty mask, a body behind the camera (every face culled: no
    coverage), a few NaN vertices, a frame of NaN vertices, a full mask."""
    H, W = 96, 128
    n = 8
    theta = _pose(smpl, n, 29)
    verts = smpl.launch(np.zeros((n, 10), np.float32), theta, want=("verts",))["verts"]
    moved = theta.copy()
    moved[:, 0] = (0.08, 0.03, 0.0)
    moved[:, 1:] += np.random.default_rng(4).normal(0, 0.08, (n, 24, 3)).astype(np.float32)
    target = smpl.launch(np.zeros((n, 10), np.float32), moved, want=("verts",))["verts"]
    cams = _cams(verts, H, W, ((2.5, 0.0), (2.5, 0.8), (1.0, 0.3), (2.5, 0.0), (-2.5, 0.0), (2.5, 0.2), (2.5, 0.0), (2.5, 0.0)))
    mask = (smpl.depthRaster(target, cams, H, W, want=())["face"] >= 0).astype(np.uint8)
    mask[3] = 0
    mask[4] = mask[0]
    mask[7] = 1
    verts = verts.copy()
    verts[5, 100:140] = np.nan
    verts[6] = np.nan
    face = smpl.depthRaster(verts, cams, H, W, want=())["face"]
    assert (face[4] == -1).all() and (face[6] == -1).all() and (face[5] >= 0).any() and mask[4].any()
    return dict(H=H, W=W, verts=verts, cams=cams, mask=mask, face=face)


def test_forward_bits(smpl, scene):
    H, W, v, cams, mask, face = (scene[k] for k in ("H", "W", "verts", "cams", "mask", "face"))
    want = SO.silhouette_batch(v, cams, H, W, face, mask)
    got = smpl.silhouette(v, cams, H, W, mask, face=face)
    for k in OUT:
        assert got[k].dtype == want[k].dtype and _same_bits(got[k], want[k]), (k, int((got[k] != want[k]).sum()))
    # what the frames were built to show
    vt, ps = want["vert_target"], want["pix_source"]
    assert (vt[0] >= 0).mean() > 0.02 and (ps[0] >= 0).sum() > 20 and (vt[1] >= 0).any() and (ps[1] >= 0).any()
    u, w_, ok = SO.project(v[2], cams[2], 0.05)
    outside = ok & ((u < 0) | (u >= W) | (w_ < 0) | (w_ >= H))
    assert outside.sum() > 100
    assert (vt[3] == -1).all() and (ps[3] == -1).all()                      # an empty mask
    assert (vt[4] == -1).all() and (ps[4] == -1).all()                      # behind the camera: refused vertices, no coverage
    assert (vt[5, 100:140] == -1).all() and (vt[5] >= 0).any()              # NaN vertices are refused vertices
    assert (vt[6] == -1).all() and (ps[6] == -1).all() and (want["vert_sq"][6] == 0).all()
    assert (vt[7] == -1).all() and (ps[7] >= 0).sum() == (face[7] < 0).sum()  # a full mask: every vertex is inside it
    # rasterising itself gives the same; so does device space; so does each frame alone
    own = smpl.silhouette(v, cams, H, W, mask)
    assert _same_bits(own["face"], face)
    dv = smpl.silhouette(_dev(v), _dev(cams), H, W, _dev(mask), face=_dev(face))
    for k in OUT:
        assert _same_bits(own[k], got[k]) and _same_bits(_host(dv[k]), got[k]), k
    for slot in (0, 2, 5):
        one = smpl.silhouette(v[slot:slot + 1], cams[slot:slot + 1], H, W, mask[slot:slot + 1], face=face[slot:slot + 1])
        for k in OUT:
            assert _same_bits(one[k][0], got[k][slot]), (slot, k)
    # nullable outputs
    half = smpl.silhouette(v, cams, H, W, mask, face=face, want=("vert_sq",))
    assert set(half) == {"vert_sq", "face"} and _same_bits(half["vert_sq"], got["vert_sq"])
    half = smpl.silhouette(_dev(v), _dev(cams), H, W, _dev(mask), face=_dev(face), want=("pix_source", "pix_sq"))
    assert _same_bits(_host(half["pix_source"]), got["pix_source"]) and _same_bits(_host(half["pix_sq"]), got["pix_sq"])


def test_forward_independent_of_the_rasterisers_work_split(synth_model, scene, smpl):
    H, W, v, cams, mask = (scene[k] for k in ("H", "W", "verts", "cams", "mask"))
    ref = smpl.silhouette(v, cams, H, W, mask)
    for px in ("0", "4096"):
        s2 = _synth(synth_model, {"SMPLPP_DEPTH_RASTER_INLINE": px})
        r = s2.silhouette(v, cams, H, W, mask)
        for k in OUT + ("face",):
            assert _same_bits(r[k], ref[k]), (px, k)


# ---------------------------------------------------------------------------------------------------- backward
def _cotangents(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.normal(size=shape).astype(np.float32)
    g[rng.random(shape) < 1 / 3] = 0.0
    return g


def test_vjp_vs_float64_and_semantics(smpl, faces, scene):
    H, W = scene["H"], scene["W"]
    sl = slice(0, 3)
    v, cams, mask, face = (scene[k][sl] for k in ("verts", "cams", "mask", "face"))
    fwd = smpl.silhouette(v, cams, H, W, mask, face=face)
    vt, ps = fwd["vert_target"], fwd["pix_source"]
    gs, gp = _cotangents(vt.shape, 8), _cotangents(ps.shape, 9)
    both = smpl.silhouetteBackward(v, cams, H, W, face, vt, ps, gs, gp)
    only_v = smpl.silhouetteBackward(v, cams, H, W, face, vert_target=vt, grad_vert_sq=gs)
    only_p = smpl.silhouetteBackward(v, cams, H, W, face, pix_source=ps, grad_pix_sq=gp)
    for name, got, a, b in (("both", both, gs, gp), ("vertex term", only_v, gs, None), ("pixel term", only_p, None, gp)):
        for i in range(3):
            args = (faces, cams[i], H, W, face[i], vt[i], ps[i], None if a is None else a[i], None if b is None else b[i])
            r64 = SO.vjp_autograd(v[i], *args, dtype=torch.float64)
            r32 = SO.vjp_autograd(v[i], *args, dtype=torch.float32)
            err, bar = _rel(got[i], r64), max(4 * _rel(r32, r64), 1e-5)
            print("%s, frame %d: rel %.3g, fp32 autograd %.3g, bar %.3g" % (name, i, err, _rel(r32, r64), bar))
            assert np.abs(r64).max() > 0 and err <= bar, (name, i, err, bar)
    # a vertex without a term and outside every source face gets exactly 0
    touched = np.zeros(v.shape[:2], bool)
    for i in range(3):
        src = ps[i][(ps[i] >= 0) & (gp[i] != 0)]
        touched[i, faces[face[i].ravel()[src]].ravel()] = True
        touched[i] |= (vt[i] >= 0) & (gs[i] != 0)
    assert (both[~touched] == 0).all() and (np.abs(both[touched]).sum(1) > 0).mean() > 0.9
    # two launches, device space: the same bits
    assert _same_bits(smpl.silhouetteBackward(v, cams, H, W, face, vt, ps, gs, gp), both)
    gd = smpl.silhouetteBackward(_dev(v), _dev(cams), H, W, _dev(face), _dev(vt), _dev(ps), _dev(gs), _dev(gp))
    assert _same_bits(_host(gd), both)
    # accumulate
    base = np.random.default_rng(9).normal(size=both.shape).astype(np.float32)
    out = base.copy()
    r = smpl.silhouetteBackward(v, cams, H, W, face, vt, ps, gs, gp, out=out)
    assert r is out and _same_bits(out, base + both)
    # NaN under zero cotangents and -1 ids: a vertex with a term, and the corners of a source face
    k = int(np.nonzero((vt[0] >= 0) & (gs[0] != 0))[0][7])
    q = np.argwhere((ps[0] >= 0) & (gp[0] != 0))[11]
    corners = faces[face[0].ravel()[ps[0][tuple(q)]]]
    hit = (ps[0] >= 0) & np.isin(faces[face[0].ravel()[np.maximum(ps[0], 0)]], np.append(corners, k)).any(-1)
    gs2, gp2, v2 = gs.copy(), gp.copy(), v.copy()
    gs2[0, np.append(corners, k)] = 0.0
    gp2[0][hit] = 0.0
    v2[0, np.append(corners, k)] = np.nan
    gn = smpl.silhouetteBackward(v2, cams, H, W, face, vt, ps, gs2, gp2)
    assert np.isfinite(gn).all() and _same_bits(gn, smpl.silhouetteBackward(v, cams, H, W, face, vt, ps, gs2, gp2))
    vt3, ps3 = vt.copy(), ps.copy()
    vt3[0, k] = -1
    ps3[0][tuple(q)] = -1
    gs3, gp3 = gs.copy(), gp.copy()
    gs3[0, k] = 0.0
    gp3[0][tuple(q)] = 0.0
    assert _same_bits(smpl.silhouetteBackward(v, cams, H, W, face, vt3, ps3, gs, gp), smpl.silhouetteBackward(v, cams, H, W, face, vt, ps, gs3, gp3))
    # device space: a source whose face is -1 or out of range, a source or target outside the image, contribute nothing
    f4, ps4, vt4 = face.copy(), ps.copy(), vt.copy()
    q2 = np.argwhere((ps[1] >= 0) & (gp[1] != 0))
    f4[1].ravel()[ps[1][tuple(q2[3])]] = 10 ** 7
    f4[1].ravel()[ps[1][tuple(q2[-1])]] = -1
    ps4[1][tuple(q2[40])] = H * W + 5
    vt4[0, k] = 1 << 40
    gp4 = gp.copy()
    gp4[1][(ps[1] == ps[1][tuple(q2[3])]) | (ps[1] == ps[1][tuple(q2[-1])])] = 0.0
    gp4[1][tuple(q2[40])] = 0.0
    assert _same_bits(_host(smpl.silhouetteBackward(_dev(v), _dev(cams), H, W, _dev(f4), _dev(vt4), _dev(ps4), _dev(gs), _dev(gp))),
                      smpl.silhouetteBackward(v, cams, H, W, face, vt, ps, gs3, gp4))
    # frame bits independent of n and slot
    one = smpl.silhouetteBackward(v[1:2], cams[1:2], H, W, face[1:2], vt[1:2], ps[1:2], gs[1:2], gp[1:2])
    assert _same_bits(one[0], both[1])
    arrs = dict(v=v, c=cams, f=face, vt=vt, ps=ps, gs=gs, gp=gp)
    big = {k_: np.repeat(a[:1], 5, 0) for k_, a in arrs.items()}
    for k_, a in arrs.items():
        big[k_][3] = a[1]
    assert _same_bits(smpl.silhouetteBackward(big["v"], big["c"], H, W, big["f"], big["vt"], big["ps"], big["gs"], big["gp"])[3], both[1])
    # through torch.autograd
    dvt = _dev(v).requires_grad_(True)
    vsq, psq = smpl.silhouette_differentiable(dvt, cams, H, W, _dev(mask))
    assert vsq.requires_grad and psq.requires_grad
    assert _same_bits(_host(vsq.detach()), fwd["vert_sq"]) and _same_bits(_host(psq.detach()), fwd["pix_sq"])
    ((vsq * _dev(gs)).sum() + (psq * _dev(gp)).sum()).backward()
    assert _same_bits(_host(dvt.grad), both)
    dvt = _dev(v).requires_grad_(True)
    vsq, _ = smpl.silhouette_differentiable(dvt, cams, H, W, _dev(mask))
    (vsq * _dev(gs)).sum().backward()
    assert _same_bits(_host(dvt.grad), only_v)


def test_refusals_leave_the_outputs_alone(smpl, synth_model, scene):
    import ctypes as C

    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import _ptr

    L = _lib.load()
    H, W = scene["H"], scene["W"]
    v, cam, mask, face = (np.ascontiguousarray(scene[k][:1]) for k in ("verts", "cams", "mask", "face"))
    V = smpl.vertex_num
    nearest, sqd = np.full((1, H, W), 7, np.int64), np.full((1, H, W), 7, np.int32)
    vt, vs = np.full((1, V), 7, np.int64), np.full((1, V), 7.0, np.float32)
    ps, pq = np.full((1, H, W), 7, np.int64), np.full((1, H, W), 7.0, np.float32)
    gv = np.full((1, V, 3), 7.0, np.float32)

    def dt(handle=None, n=1, mp=mask, h=H, w=W, np_=nearest, sp=sqd, space=_lib.HOST):
        return L.smplpp_mask_distance_transform(smpl.handle if handle is None else handle, n, _ptr(mp), h, w, _ptr(np_), _ptr(sp), space, None)

    for kw in (dict(h=0), dict(w=0), dict(h=8193), dict(w=1 << 20), dict(n=0), dict(n=-1), dict(n=1 << 22), dict(mp=None),
               dict(np_=None, sp=None), dict(space=5)):
        with pytest.raises(_lib.SmplppError):
            _lib.check(dt(**kw))
    assert (nearest == 7).all() and (sqd == 7).all()

    def fwd(handle=None, n=1, vp=v, cp=cam, h=H, w=W, near=0.05, fp=face, mp=mask, outs=(vt, vs, ps, pq), space=_lib.HOST):
        return L.smplpp_silhouette(smpl.handle if handle is None else handle, n, _ptr(vp), _ptr(cp), h, w, near, _ptr(fp), _ptr(mp),
                                   *[_ptr(o) for o in outs], space, None)

    wrong = [face.copy() for _ in range(3)]
    for w_, idx in zip(wrong, (smpl.face_num, -2, 1 << 40)):
        w_[0, 3, 4] = idx
    bad = [dict(h=0), dict(w=0), dict(h=-3), dict(h=8193), dict(w=1 << 20), dict(near=0.0), dict(near=-1.0), dict(near=float("nan")),
           dict(near=float("inf")), dict(n=0), dict(n=-1), dict(n=1 << 22), dict(vp=None), dict(cp=None), dict(fp=None), dict(mp=None),
           dict(outs=(None, None, None, None)), dict(space=5)] + [dict(fp=w_) for w_ in wrong]
    for kw in bad:
        with pytest.raises(_lib.SmplppError):
            _lib.check(fwd(**kw))
    assert (vt == 7).all() and (vs == 7).all() and (ps == 7).all() and (pq == 7).all()
    _lib.check(fwd())
    g_s, g_p = np.ones((1, V), np.float32), np.ones((1, H, W), np.float32)

    def bwd(n=1, h=H, w=W, near=0.05, fp=face, tp=vt, sp=ps, gs=g_s, gp=g_p, out=gv, acc=0, space=_lib.HOST):
        return L.smplpp_silhouette_vjp(smpl.handle, n, _ptr(v), _ptr(cam), h, w, near, _ptr(fp), _ptr(tp), _ptr(sp), _ptr(gs), _ptr(gp),
                                       _ptr(out), acc, space, None)

    vt_bad, ps_bad, ps_low = vt.copy(), ps.copy(), ps.copy()
    vt_bad[0, 5], ps_bad[0, 2, 2], ps_low[0, 1, 1] = H * W, 1 << 40, -2
    bad = [dict(h=0), dict(w=8193), dict(acc=2), dict(acc=-1), dict(n=0), dict(n=1 << 22), dict(fp=None), dict(out=None), dict(space=3),
           dict(near=0.0), dict(near=float("nan")), dict(gs=None, gp=None), dict(tp=None), dict(sp=None), dict(tp=vt_bad), dict(sp=ps_bad),
           dict(sp=ps_low)] + [dict(fp=w_) for w_ in wrong]
    for kw in bad:
        with pytest.raises(_lib.SmplppError):
            _lib.check(bwd(**kw))
    assert (gv == 7.0).all()
    _lib.check(bwd(tp=None, gs=None))  # a cotangent left out needs no correspondences
    _lib.check(bwd(sp=None, gp=None))
    # a model without faces: the transform runs, the residuals are refused
    m = model_io._normalise(synth_model)
    h = C.c_void_p()
    _lib.check(L.smplpp_model_create(m["vertices_template"].shape[0], 0, _ptr(m["vertices_template"]), _ptr(m["shape_blend_shapes"]),
                                     _ptr(m["pose_blend_shapes"]), _ptr(m["joint_regressor"]), _ptr(m["weights"]), _ptr(m["kinematic_tree"]),
                                     None, 0, C.byref(h)))
    try:
        _lib.check(dt(handle=h))
        with pytest.raises(_lib.SmplppError):
            _lib.check(fwd(handle=h))
    finally:
        L.smplpp_model_destroy(h)
    want = SO.transform_batch(mask)
    assert _same_bits(nearest, want[0]) and _same_bits(sqd, want[1])


# ---------------------------------------------------------------------------------------------------- the chain and the fit
def test_chain_to_theta_and_beta(smpl, synth_model, faces):
    """torch.autograd through silhouette_differentiable and forward_differentiable against central differences of the restated
    fixed-correspondence loss through a float64 FK, along random directions of (beta, theta); the bar of the depth rasteriser's chain
    test: 4 x the error of the same graph in fp32 autograd, or 1e-5 relative."""
    import fk_vjp_oracle as FK
    from smplpp_amd import model_io

    H, W = 96, 96
    n = 2
    beta, theta = model_io.synthetic_inputs(n, seed=21)
    theta[:, 0] = 0.0
    theta[:, 1:] *= 0.5
    _, tt = model_io.synthetic_inputs(n, seed=22)
    tt[:, 0] = (0.05, 0.02, 0.0)
    tt[:, 1:] = theta[:, 1:] + 0.05 * tt[:, 1:]
    rest = smpl.launch(beta, theta, want=("verts",))["verts"]
    cams = _cams(rest, H, W, ((2.5, 0.2), (2.3, -0.5)))
    mask = (smpl.depthRaster(smpl.launch(beta, tt, want=("verts",))["verts"], cams, H, W, want=())["face"] >= 0).astype(np.uint8)
    b = _dev(beta).requires_grad_(True)
    t = _dev(theta).requires_grad_(True)
    verts, _ = smpl.forward_differentiable(b, t)
    vsq, psq = smpl.silhouette_differentiable(verts, cams, H, W, _dev(mask))
    live = psq > 0
    assert int(live.sum()) > 20 and int((vsq > 0).sum()) > 100
    (vsq.mean() + psq.sum() / live.sum()).backward()
    gb, gt = _host(b.grad).astype(np.float64), _host(t.grad).astype(np.float64)
    fwd = smpl.silhouette(_host(verts.detach()), cams, H, W, mask)
    gs = np.full(vsq.shape, 1.0 / vsq.numel(), np.float64)
    gp = np.where(_host(live), 1.0 / float(live.sum()), 0.0)
    v0 = _host(verts.detach()).astype(np.float64)

    def value(m, bb, th):
        vv = FK.fk(m, bb, th)["verts"]
        return sum(SO.loss(vv[i], faces, cams[i], H, W, fwd["face"][i], fwd["vert_target"][i], fwd["pix_source"][i], gs[i], gp[i], at=v0[i])
                   for i in range(n))

    m64, m32 = FK.model_tensors(synth_model, torch.float64), FK.model_tensors(synth_model, torch.float32)
    b32 = torch.tensor(beta, requires_grad=True)
    t32 = torch.tensor(theta, requires_grad=True)
    value(m32, b32, t32).backward()
    rng = np.random.default_rng(6)
    for _ in range(4):
        db, dth = rng.normal(size=beta.shape), rng.normal(size=theta.shape)
        h = 1e-6
        with torch.no_grad():
            fd = float(value(m64, torch.tensor(beta + h * db), torch.tensor(theta + h * dth)) -
                       value(m64, torch.tensor(beta - h * db), torch.tensor(theta - h * dth))) / (2 * h)
        got = (gb * db).sum() + (gt * dth).sum()
        f32 = float((b32.grad.double().numpy() * db).sum() + (t32.grad.double().numpy() * dth).sum())
        bar = max(4 * abs(f32 - fd), 1e-5 * abs(fd))
        print("direction: fd %.6e, library %.6e, fp32 autograd %.6e" % (fd, got, f32))
        assert fd != 0 and abs(got - fd) <= bar, (got, fd, f32)


def test_silhouette_fit_where_the_depth_term_is_blind(smpl, synth_model):
    """The target mask is the coverage of (beta*, theta*) at 128 x 128 from 2.5 m; the start is theta* with the root moved 6 cm
    parallel to the image plane.  (i) The depth term at fixed faces puts a cotangent on no pixel where coverage and mask disagree.
    (ii) STEPS plain gradient steps of rate RATE on mean(vert_sq) + mean over the live pixels of pix_sq.  Measured on the MI355X
    (DESIGN §3.13): loss 5.34 -> 0.0897 px^2, disagreeing pixels 703 -> 147, lateral root error 60.0 mm -> 9.9 mm.  Asserted: all
    three fell."""
    STEPS, RATE = 60, 3e-5
    H = W = 128
    rng = np.random.default_rng(31)
    beta = rng.normal(0, 0.5, (1, 10)).astype(np.float32)
    star = np.zeros((1, 25, 3), np.float32)
    star[0, 1:] = rng.normal(0, 0.2, (24, 3))
    v_star = smpl.launch(beta, star, want=("verts",))["verts"]
    cam = _cams(v_star, H, W, ((2.5, 0.0),))
    target = smpl.depthRaster(v_star, cam, H, W)
    mask = _dev((target["face"] >= 0).astype(np.uint8))
    side = cam[0, 0:3].astype(np.float64)  # the image's x axis in world coordinates: the first row of R
    start = star.copy()
    start[0, 0] += (0.06 * side).astype(np.float32)
    b = _dev(beta)
    t = _dev(start).requires_grad_(True)
    # (i) the depth term
    verts, _ = smpl.forward_differentiable(b, t)
    depth, fimg, _ = smpl.depth_raster_differentiable(verts, cam, H, W)
    tg = _dev(target["depth"])
    valid = (fimg >= 0) & (tg > 0)
    disagree = (fimg >= 0) != (tg > 0)
    d = depth.detach().requires_grad_(True)
    cot, = torch.autograd.grad((((d - tg) ** 2) * valid).sum() / valid.sum(), d)
    assert int(disagree.sum()) > 100 and (cot[disagree] == 0).all() and (cot[valid] != 0).any()
    blind = smpl.depthRasterBackward(verts.detach(), cam, H, W, torch.where(disagree, torch.full_like(fimg, -1), fimg), cot)
    assert _same_bits(_host(blind), _host(smpl.depthRasterBackward(verts.detach(), cam, H, W, fimg, cot)))
    # (ii) the silhouette term
    trace = []
    for step in range(STEPS + 1):
        verts, _ = smpl.forward_differentiable(b, t)
        vsq, psq = smpl.silhouette_differentiable(verts, cam, H, W, mask)
        live = psq > 0
        loss = vsq.mean() + psq.sum() / live.sum().clamp(min=1)
        cover = smpl.depthRaster(verts.detach(), cam, H, W, want=())["face"] >= 0
        err = abs(float(((t.detach().cpu().numpy()[0, 0] - star[0, 0]).astype(np.float64) * side).sum()))
        trace.append((float(loss.detach()), int((cover != (mask != 0)).sum()), err))
        if step == STEPS:
            break
        g, = torch.autograd.grad(loss, t)
        t = (t - RATE * g).detach().requires_grad_(True)
    (l0, p0, e0), (l1, p1, e1) = trace[0], trace[-1]
    print("silhouette fit: loss %.3e -> %.3e px^2, disagreeing pixels %d -> %d, lateral root error %.1f mm -> %.1f mm" %
          (l0, l1, p0, p1, 1e3 * e0, 1e3 * e1))
    assert l1 < l0 and p1 < p0 and e1 < e0


def test_silhouette_cpp_shim(tmp_path):
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    exe = str(tmp_path / "silhouette_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "silhouette_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    n, H, W = 1, 48, 64
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    v = s.launch(beta, theta, want=("verts",))["verts"]
    cam = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.05, -0.1, 2.0, 70.0, -70.0, 32.0, 24.0], np.float32)
    face = s.depthRaster(v, cam, H, W, near=0.1, want=())["face"]
    mask = np.zeros((n, H, W), np.uint8)
    mask[:, 1:, 3:] = face[:, :-1, :-3] >= 0
    assert mask.any() and ((mask != 0) & (face < 0)).any()
    nearest, sqd = s.maskDistanceTransform(mask)
    out = s.silhouette(v, cam, H, W, mask, near=0.1, face=face)
    want = SO.silhouette_batch(v, cam[None], H, W, face, mask, near=0.1)
    for k in OUT:
        assert _same_bits(out[k], want[k]), k
    gs = ((np.arange(n * 40, dtype=np.float32).reshape(n, 40) % 5) - 2) * np.float32(0.25)
    gp = ((np.arange(n * H * W, dtype=np.float32).reshape(n, H, W) % 7) - 3) * np.float32(0.5)
    gv = s.silhouetteBackward(v, cam, H, W, face, out["vert_target"], out["pix_source"], gs, gp, near=0.1)
    assert np.abs(gv).max() > 0
    want = b"".join(np.ascontiguousarray(x).tobytes() for x in (nearest, sqd.astype(np.int64), out["vert_target"], out["vert_sq"],
                                                                 out["pix_source"], out["pix_sq"], gv))
    assert len(raw) == len(want) and raw == want
