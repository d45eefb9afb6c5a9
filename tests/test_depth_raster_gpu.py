"""The depth rasteriser on the MI355X (smplpp_depth_raster, smplpp_depth_raster_vjp): every output bit against the numpy oracle on
the hand cases, two spheres and the synthetic body from a usual, a close and a far camera; independence of batch, slot, space,
stream, optional outputs and the work split; refusals; the backward pass against float64 autograd and its call rules; the chain to
theta and beta; a depth fit with the visibility mask; and the C++ shim."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_raster_oracle as DR  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("face", "depth", "bary", "visible", "culled")
UNIT = DR.pinhole(np.eye(3), np.zeros(3), 1.0, 1.0, 0.0, 0.0)


def _model_for(nverts, faces, env=None):
    """An SMPL handle whose faces are `faces` over nverts vertices (the calls here take vertices directly)."""
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    m = model_io.tiny_model(nverts, seed=3, faces=np.asarray(faces) + 1)
    s = SMPL()
    s.setDevice("cuda:0")
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        s.init(m)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    return s


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


@pytest.fixture(scope="module")
def posed(smpl):
    rng = np.random.default_rng(17)
    theta = np.zeros((3, 25, 3), np.float32)
    theta[1:, 1:] = rng.normal(0, 0.3, (2, 24, 3))
    return smpl.launch(np.zeros((3, 10), np.float32), theta, want=("verts",))["verts"]


def _cams(verts, H, W, views):
    return np.stack([DR.look_at_camera((v.min(0) + v.max(0)) / 2, d, yaw, H, W) for v, (d, yaw) in zip(verts, views)])


def _check_bits(got, verts, faces, cams, H, W, near=0.05, keys=KEYS):
    want = DR.raster_batch(verts, faces, cams, H, W, near)
    for k in keys:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        assert g.dtype == want[k].dtype and _same_bits(g, want[k]), (k, int((g != want[k]).sum()))
    return want


def _plane(xy, z=1.0):
    return np.array([[x * z, y * z, z] for x, y in xy], np.float32)


# ---------------------------------------------------------------------------------------------------- bits
def test_bits_hand_cases():
    pad = _plane([(100.0, 100.0)] * 8)  # vertices no face uses
    sq = np.concatenate([_plane([(0.5, 0.5), (4.5, 0.5), (4.5, 4.5), (0.5, 4.5)]), pad])[None]
    cam = UNIT[None]
    for tris in ([[0, 1, 2], [0, 2, 3]], [[2, 1, 0], [0, 2, 3]], [[0, 1, 3], [1, 2, 3]], [[3, 1, 0], [3, 2, 1]], [[0, 1, 2]], [[0, 2, 3]]):
        s = _model_for(12, tris)
        w = _check_bits(s.depthRaster(sq, cam, 6, 6), sq, tris, cam, 6, 6)
        if len(tris) == 2:
            assert (w["face"] >= 0).sum() == 16
    # six faces on their own vertices, two frames: the skipped faces; the depth tie, the nearer face, zero areas, the image's border
    good = _plane([(0.2, 0.3), (5.1, 0.4), (2.2, 5.3)])
    behind = _plane([(0.2, 0.3), (5.1, 0.4), (2.2, 5.3)], 0.01)
    straddle, band, nan, inf = good.copy(), good.copy(), good.copy(), good.copy()
    straddle[1] = (0.0, 0.0, 0.05)
    band[2, 0] = 40000.0
    nan[0, 1] = np.nan
    inf[2, 2] = np.inf
    t = _plane([(0.2, 0.3), (5.1, 0.4), (2.2, 5.3)], 1.5)
    f1 = np.concatenate([t, t, _plane([(0.6, 0.7), (3.1, 0.9), (1.2, 3.3)], 1.2), _plane([(0.5, 0.5), (2.5, 2.5), (4.5, 4.5)]),
                         _plane([(1.5, 1.5), (1.501, 1.5), (1.5, 1.501)]), _plane([(-3.2, -2.1), (7.3, 1.2), (1.1, 9.7)], 2.0)])
    v = np.stack([np.concatenate([behind, straddle, good, band, nan, inf]), f1]).astype(np.float32)
    tris = np.arange(18).reshape(6, 3)
    s = _model_for(18, tris)
    cams = np.stack([UNIT, UNIT])
    w = _check_bits(s.depthRaster(v, cams, 6, 6), v, tris, cams, 6, 6)
    assert w["culled"].tolist() == [5, 0] and set(np.unique(w["face"][1]).tolist()) == {-1, 0, 2, 5}


def test_bits_two_spheres():
    H = W = 160
    cam = DR.pinhole(np.eye(3), np.zeros(3), 150.0, 150.0, W / 2, H / 2)
    va, f = DR.two_spheres(2, (0.0, 0.0, 3.0), (0.0, 0.0, 5.0))
    vb, _ = DR.two_spheres(2, (0.0, 0.0, 3.0), (1.15, 0.1, 3.2))
    v = np.stack([va, vb]).astype(np.float32)
    s = _model_for(len(va), f)
    cams = np.stack([cam, cam])
    w = _check_bits(s.depthRaster(v, cams, H, W), v, f, cams, H, W)
    half = len(va) // 2
    assert not w["visible"][0, half:].any() and w["visible"][1, half:].any() and w["visible"][:, :half].any(1).all()


@pytest.mark.parametrize("H,W", [(128, 128), (240, 320), (512, 512)])
def test_bits_synthetic(smpl, faces, posed, H, W):
    # a usual view, a camera inside arm's reach (faces of thousands of pixels, vertices behind it), one 40 m away
    cams = _cams(posed, H, W, ((2.5, 0.0), (0.3, 0.5), (40.0, 0.7)))
    w = _check_bits(smpl.depthRaster(posed, cams, H, W), posed, faces, cams, H, W)
    per_face = [np.bincount(w["face"][i][w["face"][i] >= 0], minlength=len(faces)) for i in range(3)]
    assert (w["face"][0] >= 0).mean() > 0.1 and w["culled"][0] == 0
    assert w["culled"][1] > 0 and (w["face"][1] >= 0).all()
    if (H, W) == (512, 512):
        assert per_face[1].max() > 64 * 64
    assert (per_face[2] > 0).mean() < 0.05 and (w["face"][2] >= 0).any()
    # an oblique view of every frame from the usual distance
    cams = _cams(posed, H, W, ((2.5, 0.7), (2.5, -0.9), (2.5, 2.4)))
    _check_bits(smpl.depthRaster(posed, cams, H, W), posed, faces, cams, H, W)


def test_independence(smpl, synth_model, faces, posed):
    H, W = 96, 128
    v = posed[1:2]
    cam = _cams(v, H, W, ((2.0, 0.4),))
    alone = smpl.depthRaster(v, cam, H, W)
    _check_bits(alone, v, faces, cam, H, W)
    # frame 0, 7 and 15 of 16, other frames (and cameras) around it
    rng = np.random.default_rng(5)
    batch = np.repeat(posed[:1], 16, 0) + rng.normal(0, 0.01, (16, 1, 3)).astype(np.float32)
    cams = _cams(batch, H, W, [(2.5 + 0.1 * i, 0.2 * i) for i in range(16)])
    for slot in (0, 7, 15):
        batch[slot], cams[slot] = v[0], cam[0]
    r = smpl.depthRaster(batch, cams, H, W)
    for slot in (0, 7, 15):
        for k in KEYS:
            assert _same_bits(r[k][slot], alone[k][0]), (slot, k)
    # device space, and a non-default stream
    dv, dc = torch.from_numpy(v).cuda(), torch.from_numpy(cam).cuda()
    d = smpl.depthRaster(dv, dc, H, W)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        d2 = smpl.depthRaster(dv, dc, H, W)
    st.synchronize()
    for k in KEYS:
        assert _same_bits(d[k].cpu().numpy(), alone[k]) and _same_bits(d2[k].cpu().numpy(), alone[k]), k
    # without the optional outputs
    bare = smpl.depthRaster(v, cam, H, W, want=())
    assert set(bare) == {"face", "depth"} and _same_bits(bare["face"], alone["face"]) and _same_bits(bare["depth"], alone["depth"])
    dbare = smpl.depthRaster(dv, dc, H, W, want=("visible",))
    assert _same_bits(dbare["visible"].cpu().numpy(), alone["visible"]) and _same_bits(dbare["depth"].cpu().numpy(), alone["depth"])
    # every split of the work: all faces through the wavefront queue, and the largest boxes a single thread may walk
    close = _cams(v, H, W, ((0.4, 0.3),))
    ref_close = smpl.depthRaster(v, close, H, W)
    _check_bits(ref_close, v, faces, close, H, W)
    for px in ("0", "1", "4096"):
        s2 = _synth(synth_model, {"SMPLPP_DEPTH_RASTER_INLINE": px})
        for c, ref in ((cam, alone), (close, ref_close)):
            r2 = s2.depthRaster(v, c, H, W)
            for k in KEYS:
                assert _same_bits(r2[k], ref[k]), (px, k)


def test_refusals_and_nan_frame(smpl, synth_model, faces, posed):
    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import _ptr

    L = _lib.load()
    H = W = 32
    v = posed[:1]
    cam = _cams(v, H, W, ((2.5, 0.0),))
    face, depth = np.zeros((1, H, W), np.int64), np.zeros((1, H, W), np.float32)
    gv = np.full((1, smpl.vertex_num, 3), 7.0, np.float32)

    def fwd(handle=None, n=1, vp=v, cp=cam, h=H, w=W, near=0.05, fp=face, dp=depth, space=_lib.HOST):
        return L.smplpp_depth_raster(smpl.handle if handle is None else handle, n, _ptr(vp), _ptr(cp), h, w, near, _ptr(fp), _ptr(dp), None,
                                     None, None, space, None)

    _lib.check(fwd())
    bad = (dict(h=0), dict(w=0), dict(h=-3), dict(h=8193), dict(w=1 << 20), dict(near=0.0), dict(near=-1.0), dict(near=float("nan")),
           dict(near=float("inf")), dict(n=0), dict(n=-1), dict(n=1 << 22), dict(n=1 << 19, h=64, w=64), dict(vp=None), dict(cp=None),
           dict(fp=None), dict(dp=None), dict(space=5))
    for kw in bad:
        with pytest.raises(_lib.SmplppError):
            _lib.check(fwd(**kw))

    def bwd(n=1, h=H, w=W, fp=face, acc=0, space=_lib.HOST):
        return L.smplpp_depth_raster_vjp(smpl.handle, n, _ptr(v), _ptr(cam), h, w, _ptr(fp), _ptr(depth), _ptr(gv), acc, space, None)

    _lib.check(fwd())
    for kw in (dict(h=0), dict(w=8193), dict(acc=2), dict(acc=-1), dict(n=0), dict(n=1 << 22), dict(fp=None), dict(space=3)):
        with pytest.raises(_lib.SmplppError):
            _lib.check(bwd(**kw))
    for idx in (smpl.face_num, -2, 1 << 40):
        wrong = face.copy()
        wrong[0, 3, 4] = idx
        with pytest.raises(_lib.SmplppError):
            _lib.check(bwd(fp=wrong))
    assert (gv == 7.0).all()  # refused calls leave the output alone
    # a model without faces
    m = model_io._normalise(synth_model)
    V = m["vertices_template"].shape[0]
    h = C.c_void_p()
    _lib.check(L.smplpp_model_create(V, 0, _ptr(m["vertices_template"]), _ptr(m["shape_blend_shapes"]), _ptr(m["pose_blend_shapes"]),
                                     _ptr(m["joint_regressor"]), _ptr(m["weights"]), _ptr(m["kinematic_tree"]), None, 0, C.byref(h)))
    try:
        with pytest.raises(_lib.SmplppError):
            _lib.check(fwd(handle=h))
    finally:
        L.smplpp_model_destroy(h)
    # a NaN frame among good ones: nothing drawn, every face skipped, the others' bits as before
    three = posed.copy()
    three[1] = np.nan
    cams = _cams(posed, H, W, ((2.5, 0.0), (2.5, 0.0), (2.5, 0.3)))
    r = smpl.depthRaster(three, cams, H, W)
    _check_bits(r, three, faces, cams, H, W)
    good = smpl.depthRaster(posed, cams, H, W)
    for i in (0, 2):
        for k in KEYS:
            assert _same_bits(r[k][i], good[k][i]), (i, k)
    assert (r["face"][1] == -1).all() and r["culled"][1] == smpl.face_num and not r["visible"][1].any()


# ---------------------------------------------------------------------------------------------------- backward
def _cotangents(shape, seed):
    rng = np.random.default_rng(seed)
    g = rng.normal(size=shape).astype(np.float32)
    g[rng.random(shape) < 1 / 3] = 0.0
    return g


def test_vjp_vs_float64_and_semantics(smpl, faces, posed):
    H, W = 96, 128
    v = posed[1:3].copy()
    cams = _cams(v, H, W, ((2.2, 0.3), (2.5, -0.6)))
    fwd = smpl.depthRaster(v, cams, H, W)
    face = fwd["face"]
    g = _cotangents(face.shape, 8)
    gv = smpl.depthRasterBackward(v, cams, H, W, face, g)
    for i in range(2):
        r64 = DR.vjp_autograd(v[i], faces, cams[i], face[i], g[i], torch.float64)
        r32 = DR.vjp_autograd(v[i], faces, cams[i], face[i], g[i], torch.float32)
        err, bar = _rel(gv[i], r64), max(4 * _rel(r32, r64), 1e-5)
        print("frame %d: rel %.3g, fp32 autograd %.3g" % (i, err, _rel(r32, r64)))
        assert np.abs(r64).max() > 0 and err <= bar, (i, err, bar)
        seen = fwd["visible"][i].astype(bool)
        assert (gv[i][~seen] == 0).all()
    # NaN under zero cotangents: a visible vertex of frame 0 and every pixel of a face that touches it
    vtx = int(np.nonzero(fwd["visible"][0])[0][100])
    touch = (faces == vtx).any(1)
    hit = (face[0] >= 0) & touch[np.maximum(face[0], 0)]
    assert hit.any()
    g2, v2 = g.copy(), v.copy()
    g2[0][hit] = 0.0
    v2[0, vtx] = np.nan
    gn = smpl.depthRasterBackward(v2, cams, H, W, face, g2)
    assert np.isfinite(gn).all() and _same_bits(gn, smpl.depthRasterBackward(v, cams, H, W, face, g2))
    # two launches, device space: the same bits
    assert _same_bits(smpl.depthRasterBackward(v, cams, H, W, face, g), gv)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    gd = smpl.depthRasterBackward(dev(v), dev(cams), H, W, dev(face), dev(g))
    assert _same_bits(gd.cpu().numpy(), gv)
    # accumulate
    base = np.random.default_rng(9).normal(size=gv.shape).astype(np.float32)
    out = base.copy()
    r = smpl.depthRasterBackward(v, cams, H, W, face, g, out=out)
    assert r is out and _same_bits(out, base + gv)
    # a device-space face id out of range contributes nothing
    f3, g3 = face.copy(), g.copy()
    pick = tuple(np.argwhere((face[1] >= 0) & (g[1] != 0))[5])
    f3[1][pick] = 10 ** 7
    g3[1][pick] = 0.0
    assert _same_bits(smpl.depthRasterBackward(dev(v), dev(cams), H, W, dev(f3), dev(g)).cpu().numpy(),
                      smpl.depthRasterBackward(v, cams, H, W, face, g3))
    # frame bits independent of n and slot
    one = smpl.depthRasterBackward(v[1:2], cams[1:2], H, W, face[1:2], g[1:2])
    assert _same_bits(one[0], gv[1])
    big = {k: np.repeat(a[:1], 5, 0) for k, a in (("v", v), ("c", cams), ("f", face), ("g", g))}
    for k, a in (("v", v), ("c", cams), ("f", face), ("g", g)):
        big[k][3] = a[1]
    assert _same_bits(smpl.depthRasterBackward(big["v"], big["c"], H, W, big["f"], big["g"])[3], gv[1])
    # through torch.autograd
    dv = dev(v).requires_grad_(True)
    depth, fimg, vis = smpl.depth_raster_differentiable(dv, cams, H, W)
    assert depth.requires_grad and not fimg.requires_grad and not vis.requires_grad
    assert _same_bits(depth.detach().cpu().numpy(), fwd["depth"]) and _same_bits(fimg.cpu().numpy(), face)
    assert _same_bits(vis.cpu().numpy(), fwd["visible"])
    (depth * dev(g)).sum().backward()
    assert _same_bits(dv.grad.cpu().numpy(), gv)


def test_chain_to_theta_and_beta(smpl, synth_model, faces):
    import fk_vjp_oracle as FK
    from smplpp_amd import model_io

    H, W = 96, 96
    dev = torch.device("cuda")
    beta, theta = model_io.synthetic_inputs(2, seed=21)
    theta[:, 0] = 0.0
    theta[:, 1:] *= 0.5
    tb, tt = model_io.synthetic_inputs(2, seed=22)
    tt[:, 0] = (0.0, 0.0, 0.03)
    tt[:, 1:] = theta[:, 1:] + 0.05 * tt[:, 1:]
    rest = smpl.launch(beta, theta, want=("verts",))["verts"]
    cams = _cams(rest, H, W, ((2.5, 0.2), (2.3, -0.5)))
    target = smpl.depthRaster(smpl.launch(beta, tt, want=("verts",))["verts"], cams, H, W)["depth"]
    b = torch.from_numpy(beta).to(dev).requires_grad_(True)
    t = torch.from_numpy(theta).to(dev).requires_grad_(True)
    verts, _ = smpl.forward_differentiable(b, t)
    depth, fimg, _ = smpl.depth_raster_differentiable(verts, cams, H, W)
    tg = torch.from_numpy(target).to(dev)
    valid = (fimg >= 0) & (tg > 0)
    assert valid.float().mean() > 0.1
    (((depth - tg) ** 2) * valid).sum().backward()
    fimg, valid = fimg.cpu().numpy(), valid.cpu().numpy()

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        bb = torch.tensor(beta, dtype=dtype, requires_grad=True)
        th = torch.tensor(theta, dtype=dtype, requires_grad=True)
        vv = FK.fk(m, bb, th)["verts"]
        loss = 0
        for i in range(2):
            pix, d, _ = DR.ray_plane(vv[i], faces, cams[i], np.where(valid[i], fimg[i], -1))
            loss = loss + ((d - torch.tensor(target[i].reshape(-1), dtype=dtype)[pix]) ** 2).sum()
        loss.backward()
        return bb.grad.double().numpy(), th.grad.double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    for got, want, f32, name in ((b.grad, r64[0], r32[0], "beta"), (t.grad, r64[1], r32[1], "theta")):
        got = got.cpu().numpy()
        bar = max(4 * _rel(f32, want), 1e-5)
        print("%s: rel %.3g, fp32 autograd %.3g" % (name, _rel(got, want), _rel(f32, want)))
        assert np.abs(want).max() > 0 and _rel(got, want) <= bar, (name, _rel(got, want), bar)


def test_depth_fit_and_visibility_mask(smpl, synth_model):
    """A target depth image rendered from (beta*, theta*) at 128 x 128 from 2.5 m; the start is theta* with the root moved 4 cm along
    the optical axis and N(0, 0.03^2) added to the pose; 40 plain gradient steps (rate 0.3) on the mean squared depth difference over
    the pixels valid in both images.  Measured on the MI355X: loss 2.97e-03 -> 2.03e-04 m^2, root translation error 40.0 mm ->
    3.8 mm.  Asserted: the loss fell and the root came closer.  Then the mesh-to-scan half of a two-sided fit against the cloud
    back-projected from the target, masked by `visible`: the gradient is exactly zero on every vertex the camera does not see."""
    H = W = 128
    dev = torch.device("cuda")
    rng = np.random.default_rng(31)
    beta = rng.normal(0, 0.5, (1, 10)).astype(np.float32)
    star = np.zeros((1, 25, 3), np.float32)
    star[0, 1:] = rng.normal(0, 0.2, (24, 3))
    v_star = smpl.launch(beta, star, want=("verts",))["verts"]
    cam = _cams(v_star, H, W, ((2.5, 0.0),))
    target = smpl.depthRaster(v_star, cam, H, W)["depth"]
    axis = cam[0, 6:9].astype(np.float64)  # the optical axis in world coordinates: the third row of R
    start = star.copy()
    start[0, 0] += (0.04 * axis).astype(np.float32)
    start[0, 1:] += rng.normal(0, 0.03, (24, 3)).astype(np.float32)
    b = torch.from_numpy(beta).to(dev)
    t = torch.from_numpy(start).to(dev).requires_grad_(True)
    tg = torch.from_numpy(target).to(dev)
    losses = []
    for _ in range(40):
        verts, _ = smpl.forward_differentiable(b, t)
        depth, fimg, vis = smpl.depth_raster_differentiable(verts, cam, H, W)
        valid = (fimg >= 0) & (tg > 0)
        loss = (((depth - tg) ** 2) * valid).sum() / valid.sum()
        g, = torch.autograd.grad(loss, t)
        losses.append(float(loss.detach()))
        t = (t - 0.3 * g).detach().requires_grad_(True)
    e0 = float(np.abs(start[0, 0] - star[0, 0]).max())
    e1 = float(np.abs(t.detach().cpu().numpy()[0, 0] - star[0, 0]).max())
    print("depth fit: loss %.3e -> %.3e, root translation error %.1f mm -> %.1f mm" % (losses[0], losses[-1], 1e3 * e0, 1e3 * e1))
    assert losses[-1] < losses[0] and e1 < e0
    # the single-view cloud: target pixels back-projected to world space, x = R^T (depth d - t)
    jj, ii = np.nonzero(target[0] > 0)
    d = np.stack([(ii + 0.5 - cam[0, 14]) / cam[0, 12], (jj + 0.5 - cam[0, 15]) / cam[0, 13], np.ones(len(ii))], 1)
    R = cam[0, :9].reshape(3, 3).astype(np.float64)
    cloud = ((target[0][jj, ii][:, None] * d - cam[0, 9:12]) @ R).astype(np.float32)[None]
    verts = smpl.forward_differentiable(b, t.detach())[0].detach().requires_grad_(True)
    _, _, vis = smpl.depth_raster_differentiable(verts, cam, H, W)
    _, sq = smpl.mesh_point_distance_differentiable(verts, torch.from_numpy(cloud).to(dev))
    (sq * vis.to(sq.dtype)).sum().backward()
    gm = verts.grad.cpu().numpy()[0]
    seen = vis.cpu().numpy()[0].astype(bool)
    assert 0.2 < seen.mean() < 0.7
    assert (gm[~seen] == 0).all() and (np.abs(gm[seen]).sum(1) > 0).mean() > 0.9


def test_depth_raster_cpp_shim(tmp_path):
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    exe = str(tmp_path / "depth_raster_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "depth_raster_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    n, H, W = 2, 48, 64
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    v = s.launch(beta, theta, want=("verts",))["verts"]
    cam = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.05, -0.1, 2.0, 70.0, -70.0, 32.0, 24.0], np.float32)
    out = s.depthRaster(v, cam, H, W, near=0.1)
    assert (out["face"] >= 0).mean() > 0.05
    _check_bits(out, v, model["face_indices"].astype(np.int64) - 1, np.stack([cam, cam]), H, W, near=0.1)
    g = ((np.arange(n * H * W, dtype=np.float32).reshape(n, H, W) % 5) - 2) * np.float32(0.25)
    gv = s.depthRasterBackward(v, cam, H, W, out["face"], g)
    want = b"".join(np.ascontiguousarray(x).tobytes() for x in (out["face"], out["depth"], out["bary"], out["visible"].astype(np.int64),
                                                                 out["culled"], gv))
    assert len(raw) == len(want) and raw == want
