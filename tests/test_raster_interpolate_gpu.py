"""The raster attribute interpolation on the MI355X (smplpp_raster_interpolate, smplpp_raster_interpolate_vjp): every forward bit
against the numpy oracle on the rasteriser's hand cases, two spheres and the synthetic body from a usual, a close and a far camera at
C = 1, 3, 4, 32; independence of batch, slot, space, stream and SMPLPP_DEPTH_RASTER_INLINE; the backward pass against float64
autograd and its call rules; the chain to theta and beta of the interpolated image and of the normal map; a normal-map fit; and the
C++ shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_raster_oracle as DR  # noqa: E402
import raster_interpolate_oracle as RI  # noqa: E402
from distance_cases import _rel, _same_bits  # noqa: E402
from test_depth_raster_gpu import UNIT, _cams, _model_for, _plane, _synth  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = (1, 3, 4, 32)


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


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _attr(visible, C, seed):
    """[n,V,C] normal attributes, NaN at every vertex no visible face uses."""
    a = np.random.default_rng(seed).normal(size=visible.shape + (C,)).astype(np.float32)
    a[~visible.astype(bool)] = np.nan
    return a


def _check_forward(s, v, tris, cams, H, W, near=0.05):
    r = s.depthRaster(v, cams, H, W, near)
    for C in CHANNELS:
        attr = _attr(r["visible"], C, 40 + C)
        got = s.rasterInterpolate(attr, r["face"], r["bary"])
        want = RI.interpolate_batch(attr, tris, r["face"], r["bary"])
        assert got.dtype == np.float32 and got.shape == want.shape and _same_bits(got, want), (C, int((got != want).sum()))
        assert np.isfinite(got).all() and (got[r["face"] < 0].view(np.uint32) == 0).all()
    return r


# ---------------------------------------------------------------------------------------------------- forward bits
def test_forward_bits_hand_cases():
    pad = _plane([(100.0, 100.0)] * 8)  # vertices no face uses
    sq = np.concatenate([_plane([(0.5, 0.5), (4.5, 0.5), (4.5, 4.5), (0.5, 4.5)]), pad])[None]
    cam = UNIT[None]
    for tris in ([[0, 1, 2], [0, 2, 3]], [[2, 1, 0], [0, 2, 3]], [[0, 1, 3], [1, 2, 3]], [[3, 1, 0], [3, 2, 1]], [[0, 1, 2]], [[0, 2, 3]]):
        r = _check_forward(_model_for(12, tris), sq, np.array(tris), cam, 6, 6)
        if len(tris) == 2:
            assert (r["face"] >= 0).sum() == 16
    # six faces on their own vertices, two frames: frame 0 is all background (every face skipped), frame 1 has the depth tie, the
    # nearer face, zero areas and the image's border
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
    f0 = np.concatenate([behind, straddle, behind, band, nan, inf])
    v = np.stack([f0, f1]).astype(np.float32)
    tris = np.arange(18).reshape(6, 3)
    r = _check_forward(_model_for(18, tris), v, tris, np.stack([UNIT, UNIT]), 6, 6)
    assert (r["face"][0] == -1).all() and set(np.unique(r["face"][1]).tolist()) == {-1, 0, 2, 5}


def test_forward_bits_two_spheres():
    H = W = 160
    cam = DR.pinhole(np.eye(3), np.zeros(3), 150.0, 150.0, W / 2, H / 2)
    va, f = DR.two_spheres(2, (0.0, 0.0, 3.0), (0.0, 0.0, 5.0))
    vb, _ = DR.two_spheres(2, (0.0, 0.0, 3.0), (1.15, 0.1, 3.2))
    v = np.stack([va, vb]).astype(np.float32)
    r = _check_forward(_model_for(len(va), f), v, f, np.stack([cam, cam]), H, W)
    assert not r["visible"][0, len(va) // 2:].any() and r["visible"][1, len(va) // 2:].any()


def test_forward_bits_synthetic(smpl, faces, posed):
    H = W = 128
    # a usual view, a camera inside arm's reach (vertices behind it, every pixel covered), one 40 m away
    cams = _cams(posed, H, W, ((2.5, 0.0), (0.3, 0.5), (40.0, 0.7)))
    r = _check_forward(smpl, posed, faces, cams, H, W)
    assert (r["face"][0] >= 0).mean() > 0.1 and (r["face"][1] >= 0).all() and r["culled"][1] > 0 and (r["face"][2] >= 0).any()
    # a device-space id outside [-1, F) gives +0
    attr = np.nan_to_num(_attr(r["visible"], 3, 1))
    wrong = r["face"].copy()
    pick = tuple(np.argwhere(wrong >= 0)[7])
    wrong[pick] = 10 ** 7
    wrong[tuple(np.argwhere(wrong >= 0)[9])] = -5
    got = smpl.rasterInterpolate(_dev(attr), _dev(wrong), _dev(r["bary"])).cpu().numpy()
    assert _same_bits(got, RI.interpolate_batch(attr, faces, wrong, r["bary"])) and (got[pick].view(np.uint32) == 0).all()


# ---------------------------------------------------------------------------------------------------- independence
def test_independence(smpl, synth_model, faces, posed):
    H, W, C = 96, 128, 3
    v = posed[1:2]
    cam = _cams(v, H, W, ((2.0, 0.4),))
    r = smpl.depthRaster(v, cam, H, W)
    attr = _attr(r["visible"], C, 3)
    g = np.random.default_rng(4).normal(size=(1, H, W, C)).astype(np.float32)
    fin = np.nan_to_num(attr)
    image = smpl.rasterInterpolate(attr, r["face"], r["bary"])
    grad = smpl.rasterInterpolateBackward(fin, v, cam, H, W, r["face"], r["bary"], g)
    assert np.abs(grad["attr"]).max() > 0 and np.abs(grad["verts"]).max() > 0
    # slot 2 of 3, other frames and cameras around it
    v3 = np.stack([posed[0], posed[2], v[0]])
    c3 = np.concatenate([_cams(v3[:2], H, W, ((2.5, 0.1), (2.7, -0.3))), cam])
    r3 = smpl.depthRaster(v3, c3, H, W)
    a3 = np.concatenate([_attr(r3["visible"][:2], C, 5), attr])
    g3 = np.concatenate([np.random.default_rng(6).normal(size=(2, H, W, C)).astype(np.float32), g])
    assert _same_bits(r3["face"][2], r["face"][0]) and _same_bits(r3["bary"][2], r["bary"][0])
    assert _same_bits(smpl.rasterInterpolate(a3, r3["face"], r3["bary"])[2], image[0])
    grad3 = smpl.rasterInterpolateBackward(np.nan_to_num(a3), v3, c3, H, W, r3["face"], r3["bary"], g3)
    assert _same_bits(grad3["attr"][2], grad["attr"][0]) and _same_bits(grad3["verts"][2], grad["verts"][0])
    # device space, and a non-default stream
    d = [_dev(x) for x in (attr, fin, v, cam, r["face"], r["bary"], g)]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    for stream in (torch.cuda.current_stream(), st):
        with torch.cuda.stream(stream):
            di = smpl.rasterInterpolate(d[0], d[4], d[5])
            dg = smpl.rasterInterpolateBackward(d[1], d[2], d[3], H, W, d[4], d[5], d[6])
        stream.synchronize()
        assert _same_bits(di.cpu().numpy(), image)
        assert _same_bits(dg["attr"].cpu().numpy(), grad["attr"]) and _same_bits(dg["verts"].cpu().numpy(), grad["verts"])
    # the rasteriser's work split is not read: models created under either extreme give the same backward bits
    for px in ("0", "4096"):
        s2 = _synth(synth_model, {"SMPLPP_DEPTH_RASTER_INLINE": px})
        g2 = s2.rasterInterpolateBackward(fin, v, cam, H, W, r["face"], r["bary"], g)
        assert _same_bits(g2["attr"], grad["attr"]) and _same_bits(g2["verts"], grad["verts"]), px


# ---------------------------------------------------------------------------------------------------- backward
def _scene(name, smpl, faces, posed):
    if name == "spheres":
        H = W = 160
        v, f = DR.two_spheres(2, (0.0, 0.0, 3.0), (1.15, 0.1, 3.2))
        v = v.astype(np.float32)[None]
        return _model_for(v.shape[1], f), v, f, DR.pinhole(np.eye(3), np.zeros(3), 150.0, 150.0, W / 2, H / 2)[None], H, W
    H = W = 128
    v = posed[1:2].copy()
    return smpl, v, faces, _cams(v, H, W, ((2.5, 0.0),)), H, W


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("scene", ["spheres", "body"])
def test_vjp_vs_float64_autograd(smpl, faces, posed, scene, C):
    s, v, f, cam, H, W = _scene(scene, smpl, faces, posed)
    r = s.depthRaster(v, cam, H, W)
    rng = np.random.default_rng(50 + C)
    attr = rng.normal(size=(1, v.shape[1], C)).astype(np.float32)
    random = rng.normal(size=(1, H, W, C)).astype(np.float32)
    half = random.copy()
    half[:, :, W // 2:] = 0.0
    for name, g in (("random", random), ("half zero", half)):
        both = s.rasterInterpolateBackward(attr, v, cam, H, W, r["face"], r["bary"], g)
        a64, v64 = RI.vjp_autograd(attr[0], v[0], f, cam[0], r["face"][0], g[0], torch.float64)
        a32, v32 = RI.vjp_autograd(attr[0], v[0], f, cam[0], r["face"][0], g[0], torch.float32)
        for key, got, want, w32 in (("attr", both["attr"][0], a64, a32), ("verts", both["verts"][0], v64, v32)):
            err, bar = _rel(got, want), max(4 * _rel(w32, want), 1e-5)
            print("%s C %d %s grad_%s: rel %.3g, fp32 autograd %.3g" % (scene, C, name, key, err, _rel(w32, want)))
            assert np.abs(want).max() > 0 and err <= bar, (key, err, bar)
        # one output at a time, the same bits; twice, the same bits
        only_a = s.rasterInterpolateBackward(attr, v, cam, H, W, r["face"], r["bary"], g, want=("attr",))
        only_v = s.rasterInterpolateBackward(attr, v, cam, H, W, r["face"], r["bary"], g, want=("verts",))
        assert set(only_a) == {"attr"} and set(only_v) == {"verts"}
        assert _same_bits(only_a["attr"], both["attr"]) and _same_bits(only_v["verts"], both["verts"])
        again = s.rasterInterpolateBackward(attr, v, cam, H, W, r["face"], r["bary"], g)
        assert _same_bits(again["attr"], both["attr"]) and _same_bits(again["verts"], both["verts"])
        # accumulate
        base = {k: rng.normal(size=both[k].shape).astype(np.float32) for k in both}
        out = {k: b.copy() for k, b in base.items()}
        ret = s.rasterInterpolateBackward(attr, v, cam, H, W, r["face"], r["bary"], g, out=out)
        assert all(ret[k] is out[k] and _same_bits(out[k], base[k] + both[k]) for k in both)
        # untouched vertices get exactly 0
        unseen = ~r["visible"][0].astype(bool)
        assert unseen.any() and (both["attr"][0][unseen] == 0).all() and (both["verts"][0][unseen] == 0).all()


def test_call_rules(smpl, synth_model, faces, posed):
    import ctypes as C

    from smplpp_amd import _lib, model_io
    from smplpp_amd.smpl import _ptr

    L = _lib.load()
    H = W = 32
    Cn = 3
    v = posed[:1]
    cam = _cams(v, H, W, ((2.5, 0.0),))
    r = smpl.depthRaster(v, cam, H, W)
    face, bary = r["face"], r["bary"]
    attr = np.random.default_rng(1).normal(size=(1, smpl.vertex_num, Cn)).astype(np.float32)
    g = np.random.default_rng(2).normal(size=(1, H, W, Cn)).astype(np.float32)
    image = np.full((1, H, W, Cn), 7.0, np.float32)
    ga, gv = np.full(attr.shape, 7.0, np.float32), np.full(v.shape, 7.0, np.float32)

    def fwd(handle=None, n=1, ap=attr, c=Cn, h=H, w=W, fp=face, bp=bary, ip=image, space=_lib.HOST):
        return L.smplpp_raster_interpolate(smpl.handle if handle is None else handle, n, _ptr(ap), c, h, w, _ptr(fp), _ptr(bp), _ptr(ip), space,
                                           None)

    def bwd(handle=None, n=1, ap=attr, c=Cn, vp=v, cp=cam, h=H, w=W, near=0.05, fp=face, bp=bary, gp=g, gap=ga, gvp=gv, acc=0,
            space=_lib.HOST):
        return L.smplpp_raster_interpolate_vjp(smpl.handle if handle is None else handle, n, _ptr(ap), c, _ptr(vp), _ptr(cp), h, w, near,
                                               _ptr(fp), _ptr(bp), _ptr(gp), _ptr(gap), _ptr(gvp), acc, space, None)

    shared = (dict(h=0), dict(w=0), dict(h=-3), dict(h=8193), dict(w=1 << 20), dict(c=0), dict(c=33), dict(c=-1), dict(n=0), dict(n=-1),
              dict(n=1 << 22), dict(n=1 << 19, h=64, w=64), dict(n=1 << 20, h=8, w=8, c=32), dict(n=1 << 14, h=1, w=1, c=32), dict(ap=None),
              dict(fp=None), dict(bp=None), dict(space=5))
    for kw in shared + (dict(ip=None),):
        with pytest.raises(_lib.SmplppError):
            _lib.check(fwd(**kw))
    for kw in shared + (dict(vp=None), dict(cp=None), dict(gp=None), dict(gap=None, gvp=None), dict(acc=2), dict(acc=-1), dict(near=0.0),
                        dict(near=float("nan")), dict(near=float("inf"))):
        with pytest.raises(_lib.SmplppError):
            _lib.check(bwd(**kw))
    for idx in (smpl.face_num, -2, 1 << 40):  # a host-space face id outside [-1, F)
        wrong = face.copy()
        wrong[0, 3, 4] = idx
        for call in (fwd, bwd):
            with pytest.raises(_lib.SmplppError):
                _lib.check(call(fp=wrong))
    # a model without faces
    m = model_io._normalise(synth_model)
    V = m["vertices_template"].shape[0]
    h = C.c_void_p()
    _lib.check(L.smplpp_model_create(V, 0, _ptr(m["vertices_template"]), _ptr(m["shape_blend_shapes"]), _ptr(m["pose_blend_shapes"]),
                                     _ptr(m["joint_regressor"]), _ptr(m["weights"]), _ptr(m["kinematic_tree"]), None, 0, C.byref(h)))
    try:
        for call in (fwd, bwd):
            with pytest.raises(_lib.SmplppError):
                _lib.check(call(handle=h))
    finally:
        L.smplpp_model_destroy(h)
    assert (image == 7.0).all() and (ga == 7.0).all() and (gv == 7.0).all()  # refused calls leave the outputs alone
    _lib.check(fwd())
    _lib.check(bwd())
    assert (image[face >= 0] != 7.0).all() and (image[face < 0] == 0).all()
    # NaN in grad_image and in bary at background pixels, and under zero cotangents, changes nothing
    ref = smpl.rasterInterpolateBackward(attr, v, cam, H, W, face, bary, g)
    assert _same_bits(ref["attr"], ga) and _same_bits(ref["verts"], gv)
    g2, b2 = g.copy(), bary.copy()
    g2[face < 0] = np.nan
    b2[face < 0] = np.nan
    got = smpl.rasterInterpolateBackward(attr, v, cam, H, W, face, b2, g2)
    assert np.isfinite(got["attr"]).all() and _same_bits(got["attr"], ref["attr"]) and _same_bits(got["verts"], ref["verts"])
    assert _same_bits(smpl.rasterInterpolate(attr, face, b2), image)
    vtx = int(np.nonzero(r["visible"][0])[0][50])
    touch = (faces == vtx).any(1)
    hit = (face[0] >= 0) & touch[np.maximum(face[0], 0)]
    assert hit.any()
    g3, a3, v3 = g.copy(), attr.copy(), v.copy()
    g3[0][hit] = 0.0
    a3[0, vtx], v3[0, vtx] = np.nan, np.nan
    clean = smpl.rasterInterpolateBackward(attr, v, cam, H, W, face, bary, g3)
    dirty = smpl.rasterInterpolateBackward(a3, v3, cam, H, W, face, bary, g3)
    assert np.isfinite(dirty["attr"]).all() and np.isfinite(dirty["verts"]).all()
    assert _same_bits(dirty["attr"], clean["attr"]) and _same_bits(dirty["verts"], clean["verts"])


# ---------------------------------------------------------------------------------------------------- chain
@pytest.fixture(scope="module")
def chain(smpl, synth_model):
    """n = 2 at 96 x 96: beta, theta, cameras, and the float64 / float32 reference graphs' inputs."""
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(2, seed=21)
    theta[:, 0] = 0.0
    theta[:, 1:] *= 0.5
    rest = smpl.launch(beta, theta, want=("verts",))["verts"]
    return beta, theta, _cams(rest, 96, 96, ((2.5, 0.2), (2.3, -0.5)))


def _chain_check(got, r64, r32):
    for g, want, w32, name in ((got[0], r64[0], r32[0], "beta"), (got[1], r64[1], r32[1], "theta")):
        g = g.cpu().numpy()
        bar = max(4 * _rel(w32, want), 1e-5)
        print("%s: rel %.3g, fp32 autograd %.3g" % (name, _rel(g, want), _rel(w32, want)))
        assert np.abs(want).max() > 0 and _rel(g, want) <= bar, (name, _rel(g, want), bar)


def test_chain_interpolated_image(smpl, synth_model, faces, chain):
    import fk_vjp_oracle as FK

    beta, theta, cams = chain
    H = W = 96
    dev = torch.device("cuda")
    rng = np.random.default_rng(7)
    weight = rng.normal(size=(2, H, W, 3)).astype(np.float32)
    b = torch.from_numpy(beta).to(dev).requires_grad_(True)
    t = torch.from_numpy(theta).to(dev).requires_grad_(True)
    verts, _ = smpl.forward_differentiable(b, t)
    # the attribute is the posed vertex itself: gradient arrives through attr and through the barycentrics
    image, fimg, depth = smpl.raster_interpolate_differentiable(verts, verts, cams, H, W)
    assert image.requires_grad and not fimg.requires_grad and not depth.requires_grad
    assert (fimg >= 0).float().mean() > 0.1
    (image * torch.from_numpy(weight).to(dev)).sum().backward()
    fnp = fimg.cpu().numpy()

    def ref(dtype, detach_attr=False):
        m = FK.model_tensors(synth_model, dtype)
        bb = torch.tensor(beta, dtype=dtype, requires_grad=True)
        th = torch.tensor(theta, dtype=dtype, requires_grad=True)
        vv = FK.fk(m, bb, th)["verts"]
        vv.retain_grad()
        loss = 0
        for i in range(2):
            pix, val = RI.interpolate_torch(vv[i].detach() if detach_attr else vv[i], vv[i], faces, cams[i], fnp[i])
            loss = loss + (val * torch.tensor(weight[i].reshape(-1, 3), dtype=dtype)[pix]).sum()
        loss.backward()
        return bb.grad.double().numpy(), th.grad.double().numpy(), vv.grad.double().numpy()

    _chain_check((b.grad, t.grad), ref(torch.float64), ref(torch.float32))
    # stage two: with attr detached the bary route alone is live
    v2 = verts.detach().clone().requires_grad_(True)
    image2, _, _ = smpl.raster_interpolate_differentiable(v2.detach(), v2, cams, H, W)
    (image2 * torch.from_numpy(weight).to(dev)).sum().backward()
    r64, r32 = ref(torch.float64, True)[2], ref(torch.float32, True)[2]
    got = v2.grad.cpu().numpy()
    print("bary route: rel %.3g, fp32 autograd %.3g" % (_rel(got, r64), _rel(r32, r64)))
    assert np.abs(got).max() > 0 and np.abs(r64).max() > 0 and _rel(got, r64) <= max(4 * _rel(r32, r64), 1e-5)


def test_chain_normal_map(smpl, synth_model, faces, chain):
    import fk_vjp_oracle as FK
    import normals_vjp_oracle as NV

    beta, theta, cams = chain
    H = W = 96
    dev = torch.device("cuda")
    weight = np.random.default_rng(8).normal(size=(2, H, W, 3)).astype(np.float32)
    b = torch.from_numpy(beta).to(dev).requires_grad_(True)
    t = torch.from_numpy(theta).to(dev).requires_grad_(True)
    verts, _ = smpl.forward_differentiable(b, t)
    normals, fimg = smpl.normal_map_differentiable(verts, cams, H, W)
    cov = fimg >= 0
    length = normals.detach().norm(dim=-1)
    assert cov.float().mean() > 0.1 and (length[cov] - 1).abs().max() < 1e-5 and (normals.detach()[~cov] == 0).all()
    assert (normals.detach()[..., 2][cov] < 0).float().mean() > 0.9  # the visible surface faces the camera
    (normals * torch.from_numpy(weight).to(dev)).sum().backward()
    fnp = fimg.cpu().numpy()
    mesh = NV.Mesh(faces, smpl.vertex_num)

    def ref(dtype, detach_attr=False):
        m = FK.model_tensors(synth_model, dtype)
        bb = torch.tensor(beta, dtype=dtype, requires_grad=True)
        th = torch.tensor(theta, dtype=dtype, requires_grad=True)
        vv = FK.fk(m, bb, th)["verts"]
        vv.retain_grad()
        vn = NV.vertex_normals(mesh, vv)
        loss = 0
        for i in range(2):
            R = torch.tensor(cams[i, :9].reshape(3, 3).astype(np.float64), dtype=dtype)
            nc = vn[i] @ R.T
            pix, val = RI.interpolate_torch(nc.detach() if detach_attr else nc, vv[i], faces, cams[i], fnp[i])
            val = val / val.norm(dim=-1, keepdim=True)
            loss = loss + (val * torch.tensor(weight[i].reshape(-1, 3), dtype=dtype)[pix]).sum()
        loss.backward()
        return bb.grad.double().numpy(), th.grad.double().numpy(), vv.grad.double().numpy()

    _chain_check((b.grad, t.grad), ref(torch.float64), ref(torch.float32))
    # stage two: the bary route alone (the vertex normals detached)
    v2 = verts.detach().clone().requires_grad_(True)
    R = torch.from_numpy(cams[:, :9].reshape(2, 3, 3)).to(dev)
    nc = torch.matmul(smpl.vertex_normals_differentiable(v2.detach()), R.transpose(1, 2))
    image, _, _ = smpl.raster_interpolate_differentiable(nc, v2, cams, H, W)
    c3 = cov.unsqueeze(-1)
    unit = torch.where(c3, image / torch.where(c3, image.norm(dim=-1, keepdim=True), torch.ones_like(image[..., :1])), torch.zeros_like(image))
    (unit * torch.from_numpy(weight).to(dev)).sum().backward()
    r64, r32 = ref(torch.float64, True)[2], ref(torch.float32, True)[2]
    got = v2.grad.cpu().numpy()
    print("bary route: rel %.3g, fp32 autograd %.3g" % (_rel(got, r64), _rel(r32, r64)))
    assert np.abs(got).max() > 0 and np.abs(r64).max() > 0 and _rel(got, r64) <= max(4 * _rel(r32, r64), 1e-5)


def test_normal_map_fit(smpl):
    """n = 1 at 96 x 96: the target is the normal map of a pose; the start has the left elbow moved by 0.2 rad; 20 Adam steps (rate
    0.01) on theta with the mean squared difference over the pixels covered in both images.  Asserted: the loss fell."""
    H = W = 96
    dev = torch.device("cuda")
    rng = np.random.default_rng(33)
    beta = torch.zeros(1, 10, device=dev)
    star = np.zeros((1, 25, 3), np.float32)
    star[0, 1:] = rng.normal(0, 0.15, (24, 3))
    v_star = smpl.launch(np.zeros((1, 10), np.float32), star, want=("verts",))["verts"]
    cam = _cams(v_star, H, W, ((2.5, 0.0),))
    with torch.no_grad():
        target, tface = smpl.normal_map_differentiable(_dev(v_star), cam, H, W)
    start = star.copy()
    start[0, 1 + 18, 1] += 0.2  # joint 18: the left elbow
    t = torch.from_numpy(start).to(dev).requires_grad_(True)
    opt = torch.optim.Adam([t], lr=0.01)
    losses = []
    for _ in range(21):
        opt.zero_grad()
        verts, _ = smpl.forward_differentiable(beta, t)
        normals, face = smpl.normal_map_differentiable(verts, cam, H, W)
        both = ((face >= 0) & (tface >= 0)).unsqueeze(-1)
        loss = (((normals - target) ** 2) * both).sum() / both.sum()
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    print("normal-map fit: loss %.3e -> %.3e" % (losses[0], losses[-1]))
    assert losses[0] > 0 and losses[-1] < losses[0]


# ---------------------------------------------------------------------------------------------------- C++ shim
def test_raster_interpolate_cpp_shim(tmp_path):
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    exe = str(tmp_path / "raster_interpolate_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "raster_interpolate_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=9)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, path, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    raw = open(outp, "rb").read()
    n, H, W, C = 2, 48, 64, 3
    beta = (np.arange(n * 10, dtype=np.float32).reshape(n, 10) % 7 - 3) * np.float32(0.1)
    theta = ((np.arange(n * 75, dtype=np.float32).reshape(n, 25, 3) % 11) - 5) * np.float32(0.05)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    v = s.launch(beta, theta, want=("verts",))["verts"]
    cam = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.05, -0.1, 2.0, 70.0, -70.0, 32.0, 24.0], np.float32)
    out = s.depthRaster(v, cam, H, W, near=0.1)
    assert (out["face"] >= 0).mean() > 0.05
    attr = ((np.arange(n * s.vertex_num * C, dtype=np.float32).reshape(n, s.vertex_num, C) % 13) - 6) * np.float32(0.125)
    image = s.rasterInterpolate(attr, out["face"], out["bary"])
    assert _same_bits(image, RI.interpolate_batch(attr, model["face_indices"].astype(np.int64) - 1, out["face"], out["bary"]))
    g = ((np.arange(n * H * W * C, dtype=np.float32).reshape(n, H, W, C) % 5) - 2) * np.float32(0.25)
    both = s.rasterInterpolateBackward(attr, v, cam, H, W, out["face"], out["bary"], g, near=0.1)
    acc = {"attr": np.ones_like(attr)}
    s.rasterInterpolateBackward(attr, v, cam, H, W, out["face"], out["bary"], g, near=0.1, want=("attr",), out=acc)
    want = b"".join(np.ascontiguousarray(x).tobytes() for x in (out["face"], image, both["attr"], both["verts"], acc["attr"]))
    assert np.abs(both["attr"]).max() > 0 and np.abs(both["verts"]).max() > 0
    assert len(raw) == len(want) and raw == want
