"""smplpp_orientation_term / smplpp_orientation_term_vjp and smplpp_axis_angle_to_rotmat_vjp on the MI355X:

 1. bits: every output of both term calls against the float32 restatement (tests/orientation_oracle.py), over the work splits of the
    frame sum (S = 1, 6, 64, 65, 1030) and of the sums across the frames (n = 1030), C = 1, 2, 3, row strides 3 and 4, rho 0 and 0.5, Tn
    and Wn in {1, n}, shared joints, and offset = NULL against the identity columns;
 2. independence: of n, of the memory space, of which outputs, gradients and cotangents are asked for; accumulate is one fp32 add,
    and column 3 of a row_stride 4 gradient buffer keeps what it held;
 3. dead sensors of every kind;
 4. the Rodrigues VJP against float64 autograd, and its tie to smplpp_skeleton_vjp;
 5. three chains against float64 autograd within the fp32 bar per block;
 6. the three fits of tests/test_orientation_cpu.py through the library;
 7. the C++ shim."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoints_oracle as KP  # noqa: E402
import orientation_oracle as OR  # noqa: E402
import skeleton_oracle as SO  # noqa: E402
import test_orientation_cpu as CPU  # noqa: E402  (the fits and their float64 runs)
import test_skeleton_cpu as SK  # noqa: E402
import vjp_blocks as VB  # noqa: E402

torch = SO.torch
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
OUT = ("energy", "sensor_energy", "residual")
GRAD = ("frames", "offset", "target")

_cache = {}


def _cached(key, make):
    """One model, handle or reference per key for the whole module; never modified."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _model():
    from smplpp_amd import model_io

    return _cached("model", model_io.synthetic_model)


def _handle():
    def make():
        from smplpp_amd.smpl import SMPL

        s = SMPL()
        s.setDevice("cuda:0")
        s.init(_model())
        return s

    return _cached("handle", make)


def _m64():
    return _cached("m64", lambda: SO.model_tensors(_model()))


def _dev(a):
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(v):
    return v.cpu().numpy() if torch.is_tensor(v) else v


def _same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _lib_all(case, rho, C, cot, to=lambda a: a):
    """Every output and gradient of the two calls, as numpy."""
    import smplpp_amd.orientation as ori

    frames, joint, offset, target, weight = case
    fr, tg, of, w = to(frames), to(target), to(offset), to(weight)
    out = ori.term(fr, joint, tg, of, w, rho, C)
    g = ori.termBackward(fr, joint, tg, of, w, rho, C, *(to(c) for c in cot))
    return {k: _host(v) for k, v in {**out, **g}.items()}


def _oracle_all(case, rho, C, cot):
    frames, joint, offset, target, weight = case
    n, S = frames.shape[0], len(joint)
    e, se, r = OR.term(frames, joint, target, offset, weight, rho, C)
    gf, go, gt = OR.term_vjp(frames, joint, target, offset, weight, rho, C, *cot, np.zeros(frames.shape, f32), np.zeros((S, 3, C), f32),
                             np.zeros((target.shape[0], S, 3, C), f32), 0)
    return dict(energy=e, sensor_energy=se, residual=r, frames=gf, offset=go, target=gt)


# ---------------------------------------------------------------------------------------------- 1. bits
# (n, S, C, row_stride, J, all sensors on one joint, rho, Tn = n, Wn = n, offsets)
BITS = [(n, S, 1 + (i + k) % 3, 3 + (i + k) % 2, 24, False, 0.5 * ((i + k // 2) % 2), bool((i + k) % 2), bool((i // 2 + k) % 2), (i + k) % 4 != 3)
        for i, n in enumerate((1, 3, 67)) for k, S in enumerate((1, 6, 64, 65))]
BITS += [(2, 1030, 3, 4, 24, False, 0.5, True, False, True), (2, 1030, 1, 3, 24, False, 0.0, False, True, False),
         (1030, 2, 3, 4, 24, False, 0.0, True, True, True), (1030, 2, 2, 3, 24, False, 0.5, False, False, True),
         (3, 6, 3, 4, 5, True, 0.0, True, True, True), (3, 65, 2, 3, 5, True, 0.5, False, True, True), (67, 6, 1, 4, 5, True, 0.5, True, False, False)]


def test_bit_cases_cover_the_list():
    for i, name in ((2, "C"), (3, "rs"), (6, "rho"), (7, "Tn"), (8, "Wn"), (9, "offsets")):
        assert len({c[i] for c in BITS}) == (3 if name == "C" else 2), name
    assert {(c[0], c[1]) for c in BITS} >= set(itertools.product((1, 3, 67), (1, 6, 64, 65))) | {(2, 1030), (1030, 2)}


@pytest.mark.parametrize("case", BITS, ids=lambda c: "n%d-S%d-C%d-rs%d-J%d%s-rho%g-T%dW%d-%s" % (c[0], c[1], c[2], c[3], c[4], "one" if c[5] else "",
                                                                                              c[6], c[7], c[8], "off" if c[9] else "id"))
def test_bits_against_the_restatement(case):
    n, S, C, rs, J, one, rho, tn, wn, offsets = case
    data = OR.random_case(n, S, C, J=J, rs=rs, seed=n + S, Tn=n if tn else 1, Wn=n if wn else 1, offsets=offsets, one_joint=one)
    cot = OR.cotangents(n, S, C, seed=S)
    got, want = _lib_all(data, rho, C, cot), _oracle_all(data, rho, C, cot)
    assert all(np.isfinite(v).all() for v in got.values())
    for k in OUT + GRAD:
        assert _same(got[k], want[k]), (k, float(np.abs(got[k] - want[k]).max()))
    assert all(np.abs(got[k]).max() > 0 for k in OUT + GRAD)


@pytest.mark.parametrize("C", [1, 2, 3])
def test_offset_null_is_the_identity_columns(C):
    n, S = 3, 7
    frames, joint, _, target, weight = OR.random_case(n, S, C, seed=40 + C, offsets=False)
    frames[0, joint[0], 0, 0] = -0.0
    eye = np.eye(3, dtype=f32)[None, :, :C].repeat(S, 0)
    cot = OR.cotangents(n, S, C, seed=C)
    a, b = _lib_all((frames, joint, None, target, weight), 0.5, C, cot), _lib_all((frames, joint, eye, target, weight), 0.5, C, cot)
    for k in OUT + GRAD:
        assert _same(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- 2. independence
def _subsets(keys):
    return [c for r in range(1, len(keys) + 1) for c in itertools.combinations(keys, r)]


def test_independence_of_n_space_and_what_is_asked_for():
    import smplpp_amd.orientation as ori

    n, S, C, rho = 67, 9, 3, 0.5
    frames, joint, offset, target, weight = OR.random_case(n, S, C, seed=5, Wn=1)
    cot = OR.cotangents(n, S, C, seed=6)
    full = _lib_all((frames, joint, offset, target, weight), rho, C, cot)
    # a frame alone has the bits it has inside n = 67 (per-frame outputs)
    for f in (0, 3, 4, 33, 66):
        sl = slice(f, f + 1)
        one = _lib_all((frames[sl], joint, offset, target[sl], weight), rho, C, tuple(c[sl] for c in cot))
        for k in OUT + ("frames",):
            assert _same(one[k][0], full[k][f]), (f, k)
    # (Tn = n = 1 is the shared form of grad_target: the frame's -G through the sum, which turns -0 into +0 and changes nothing else)
    # device space
    dev = _lib_all((frames, joint, offset, target, weight), rho, C, cot, to=_dev)
    for k in OUT + GRAD:
        assert _same(dev[k], full[k]), k
    # every subset of outputs, of gradients and of cotangents
    for want in _subsets(OUT):
        a = ori.term(frames, joint, target, offset, weight, rho, C, want=want)
        assert set(a) == set(want) and all(_same(a[k], full[k]) for k in want), want
    for want in _subsets(GRAD):
        a = ori.termBackward(frames, joint, target, offset, weight, rho, C, *cot, want=want)
        assert set(a) == set(want) and all(_same(a[k], full[k]) for k in want), want
    for on in itertools.product((0, 1), repeat=3):
        if not any(on):
            continue
        sub = tuple(c if o else None for c, o in zip(cot, on))
        dense = tuple(c if o else np.zeros_like(c) for c, o in zip(cot, on))
        a = ori.termBackward(frames, joint, target, offset, weight, rho, C, *sub)
        b = ori.termBackward(frames, joint, target, offset, weight, rho, C, *dense)
        assert all(_same(a[k], b[k]) for k in GRAD), on
    # twice
    again = _lib_all((frames, joint, offset, target, weight), rho, C, cot)
    assert all(_same(again[k], full[k]) for k in OUT + GRAD)


@pytest.mark.parametrize("space", ["host", "device"])
def test_accumulate_is_one_fp32_add(space):
    """Onto random buffers, the restatement's accumulate form: one add per entry, a joint without a live sensor left alone, column 3 of
    a row_stride 4 buffer untouched; also on top of a grad_world filled for smplpp_skeleton_vjp, which then takes the buffer."""
    import smplpp_amd.orientation as ori

    to = _dev if space == "device" else (lambda a: a)
    rng = np.random.default_rng(9)
    for rs, Tn in ((4, 3), (3, 1)):
        n, S, C, rho = 3, 7, 3, 0.5
        frames, joint, offset, target, weight = OR.random_case(n, S, C, rs=rs, seed=12 + rs, Tn=Tn)
        weight[1, 2] = 0
        cot = OR.cotangents(n, S, C, seed=2)
        pre = [rng.standard_normal(s).astype(f32) for s in (frames.shape, (S, 3, C), (Tn, S, 3, C))]
        want = OR.term_vjp(frames, joint, target, offset, weight, rho, C, *cot, *(p.copy() for p in pre), 1)
        out = {k: to(p.copy()) for k, p in zip(GRAD, pre)}
        res = ori.termBackward(to(frames), joint, to(target), to(offset), to(weight), rho, C, *(to(c) for c in cot), out=out)
        assert res is out
        got = {k: _host(v) for k, v in out.items()}
        for k, w, p in zip(GRAD, want, pre):
            assert _same(got[k], w) and not _same(got[k], p), (rs, k)
        if rs == 4:
            assert _same(got["frames"][..., 3], pre[0][..., 3])
        untouched = np.ones(24, bool)
        untouched[joint] = False
        assert untouched.any() and _same(got["frames"][:, untouched], pre[0][:, untouched])
        # a subset accumulates into what it is given only
        only = {"offset": to(pre[1].copy())}
        ori.termBackward(to(frames), joint, to(target), to(offset), to(weight), rho, C, *(to(c) for c in cot), out=only)
        assert _same(_host(only["offset"]), want[1])
    # the grad_world of a loss on `posed` and `world`, then the term on top of it, then smplpp_skeleton_vjp
    s = _handle()
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(3, seed=4)
    world = s.skeleton(beta, theta, want=("world",))["world"]
    joint = np.array(SK.IMU_JOINTS)
    _, _, offset, target, _ = OR.random_case(3, 6, 3, seed=8)
    gw = rng.standard_normal(world.shape).astype(f32)
    ge = np.ones(3, f32)
    want = OR.term_vjp(world, joint, target, offset, None, 0.0, 3, ge, None, None, gw.copy(), None, None, 1)[0]
    buf = to(gw.copy())
    ori.termBackward(to(world), joint, to(target), to(offset), None, 0.0, 3, grad_energy=to(ge), out={"frames": buf})
    assert _same(_host(buf), want) and _same(_host(buf)[..., 3], gw[..., 3])
    a = s.skeletonBackward(to(beta), to(theta), grad_world=buf)
    b = s.skeletonBackward(beta, theta, grad_world=want)
    assert all(_same(_host(a[k]), b[k]) for k in b)


# ---------------------------------------------------------------------------------------------- 3. dead sensors
@pytest.mark.parametrize("space", ["host", "device"])
def test_dead_sensors(space):
    """Weight 0 and NaN, a NaN in A, O or T, an index of -1 and of J: +0 in every output and gradient, the neighbours' bits unchanged."""
    to = _dev if space == "device" else (lambda a: a)
    n, S, C, J, rho = 5, 12, 3, 24, 0.5
    frames, joint, offset, target, weight = OR.random_case(n, S, C, seed=21)
    joint[:] = np.arange(S)  # a joint per sensor, so that a NaN in A kills one sensor
    cot = OR.cotangents(n, S, C, seed=22)
    clean = _lib_all((frames, joint, offset, target, weight), rho, C, cot, to)
    f2, j2, o2, t2, w2 = (a.copy() for a in (frames, joint, offset, target, weight))
    w2[0, 0], w2[1, 1] = 0, np.nan
    w2[2, 2] = np.inf
    f2[0, 3, 1, 2] = np.nan
    f2[3, 4, 0, 0] = np.inf
    o2[5, 2, 1] = np.nan  # sensor 5 in every frame
    t2[1, 6, 0, 0] = np.nan
    j2[7], j2[8] = -1, J
    f2[:, 9, :, 3] = np.nan  # column 3 is never read
    live = OR.live_mask(f2, j2, t2, o2, w2, C)
    dead = ~live
    assert dead.sum() == 6 + 3 * n and live[:, 9].all()
    got, want = _lib_all((f2, j2, o2, t2, w2), rho, C, cot, to), _oracle_all((f2, j2, o2, t2, w2), rho, C, cot)
    for k in OUT + GRAD:
        assert _same(got[k], want[k]) and np.isfinite(got[k]).all(), k
    for k in ("sensor_energy", "residual", "target"):
        z = got[k][dead]
        assert (z == 0).all() and not np.signbit(z).any(), k
        assert _same(got[k][live], clean[k][live]), k
    # a joint whose only sensor is dead gets +0 (sensors 7 and 8 left their joints); the others keep their bits
    gf, cf = got["frames"][:, :S, :, :3], clean["frames"][:, :S, :, :3]
    for s in (0, 1, 2, 3, 4, 5, 6):
        z = gf[:, s][dead[:, s]]
        assert (z == 0).all() and not np.signbit(z).any(), s
    assert (gf[:, 7:9] == 0).all() and not np.signbit(gf[:, 7:9]).any()
    keep = live.copy()
    keep[:, 7:9] = False
    assert _same(gf[keep], cf[keep])
    assert (got["offset"][[5, 7, 8]] == 0).all() and not np.signbit(got["offset"][[5, 7, 8]]).any()
    alive = [s for s in range(S) if live[:, s].all()]
    assert _same(got["offset"][alive], clean["offset"][alive])


# ---------------------------------------------------------------------------------------------- 4. the Rodrigues VJP
def _rel(a, b):
    return np.linalg.norm((np.asarray(a, np.float64) - b).ravel()) / max(np.linalg.norm(np.asarray(b).ravel()), 1e-30)


def test_rodrigues_vjp_against_float64():
    """Random rows: every [3] block within stage_oracle.bar(e32), e32 the block error of an fp32 autograd of the same graph.  Rows of
    exactly 0 and of norm pi: finite, and per row within the bar tests/test_fk_vjp_gpu.py holds those points to, relative L2 at most
    max(4 x fp32 autograd's, 1e-5).  Host and device space agree to the bit; accumulate is one add."""
    import smplpp_amd.orientation as ori

    s = _handle()
    rng = np.random.default_rng(31)
    n = 300
    aa = (0.8 * rng.standard_normal((n, 3))).astype(f32)
    g = rng.standard_normal((n, 3, 3)).astype(f32)
    got = s.axisAngleToRotmatBackward(aa, g)
    r64, r32 = OR.rodrigues_vjp(aa, g), OR.rodrigues_vjp(aa, g, torch.float32)
    e, e32 = VB.block_error(got, r64, (1,)), VB.block_error(r32, r64, (1,))
    print("Rodrigues VJP, random rows: E %.3g, fp32 autograd %.3g, bar %.3g" % (e, e32, VB.bar(e32)))
    assert got.shape == (n, 3) and np.isfinite(got).all() and e <= VB.bar(e32), (e, e32)
    ax = rng.standard_normal((8, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    sp = np.concatenate([np.zeros((4, 3)), np.pi * ax]).astype(f32)
    gs = rng.standard_normal((12, 3, 3)).astype(f32)
    got_s = s.axisAngleToRotmatBackward(sp, gs)
    s64, s32 = OR.rodrigues_vjp(sp, gs), OR.rodrigues_vjp(sp, gs, torch.float32)
    assert np.isfinite(got_s).all()
    for i in range(12):
        err, bar = _rel(got_s[i], s64[i]), max(4 * _rel(s32[i], s64[i]), 1e-5)
        print("Rodrigues VJP, %s row %d: err %.3g bar %.3g" % ("zero" if i < 4 else "pi", i, err, bar))
        assert err <= bar, (i, err, bar)
    d = ori.axis_angle_to_rotmat_backward(_dev(aa.reshape(10, 30, 3)), _dev(g.reshape(10, 30, 3, 3)))
    assert tuple(d.shape) == (10, 30, 3) and _same(_host(d).reshape(n, 3), got)
    pre = rng.standard_normal((n, 3)).astype(f32)
    for to in (lambda a: a, _dev):
        out = to(pre.copy())
        assert s.axisAngleToRotmatBackward(to(aa), to(g), out=out) is out
        assert _same(_host(out), pre + got)


def test_rodrigues_vjp_ties_the_two_skeleton_backwards():
    """Fed with the grad_rot of smplpp_skeleton_rotmat_vjp it gives smplpp_skeleton_vjp's grad_theta[:, 1:], within the block bar of
    the float64 reference; whether the bits are equal is printed, not asserted (the shared inline function is compiled into each kernel)."""
    from smplpp_amd import model_io

    s, n = _handle(), 5
    beta, theta = model_io.synthetic_inputs(n, seed=17)
    rng = np.random.default_rng(18)
    gw, gp = rng.standard_normal((n, 24, 3, 4)).astype(f32), rng.standard_normal((n, 24, 3)).astype(f32)
    rot = s.axisAngleToRotmat(theta[:, 1:])
    h = s.skeletonRotmatBackward(beta, np.ascontiguousarray(theta[:, 0]), rot, gw, gp, None)
    got = s.axisAngleToRotmatBackward(np.ascontiguousarray(theta[:, 1:]), h["rot"])
    direct = s.skeletonBackward(beta, theta, gw, gp, None)["theta"][:, 1:]
    m = _m64()
    a64, a32 = SO.vjp(m, beta, theta, gw, gp, None), SO.vjp(m, beta, theta, gw, gp, None, dtype=torch.float32)
    e, e32 = VB.block_error(got, a64[1][:, 1:], VB.THETA), VB.block_error(a32[1][:, 1:], a64[1][:, 1:], VB.THETA)
    print("tie: E %.3g, fp32 autograd %.3g, bar %.3g; bits equal to smplpp_skeleton_vjp: %s (%d of %d entries)"
          % (e, e32, VB.bar(e32), _same(got, direct), int((got.view(np.uint32) == np.ascontiguousarray(direct).view(np.uint32)).sum()), got.size))
    assert e <= VB.bar(e32), (e, e32)


# ---------------------------------------------------------------------------------------------- 5. chains
def _blocks(tag, got, r64, r32, axes):
    got = _host(got.detach()) if torch.is_tensor(got) else got
    axes = VB.axes_of(axes, r64)
    assert np.isfinite(got).all() and np.abs(r64).max() > 0, tag
    e, e32 = VB.block_error(got, r64, axes), VB.block_error(r32, r64, axes)
    print("%s: E %.3g, fp32 autograd %.3g, bar %.3g" % (tag, e, e32, VB.bar(e32)))
    assert e <= VB.bar(e32), (tag, e, e32)


@pytest.mark.parametrize("C", [3, 1])
def test_chain_skeleton_to_term(C):
    """theta, beta -> skeleton_differentiable -> term_differentiable -> sum energy (rho = 0.5, offsets, per-frame weights): the
    gradients to theta, beta, offset and target against float64 autograd of the oracle graph."""
    import smplpp_amd.orientation as ori
    from smplpp_amd import model_io

    s, n, S, rho = _handle(), 3, 8, 0.5
    beta, theta = model_io.synthetic_inputs(n, seed=60 + C)
    _, joint, offset, target, weight = OR.random_case(n, S, C, seed=61 + C)

    def ref(dtype):
        m = SO.cast(_m64(), dtype)
        bb, th, O, T = (torch.tensor(x, dtype=dtype, requires_grad=True) for x in (beta, theta, offset, target))
        e = OR.definition_t(SO.skeleton(m, bb, th)["world"], joint, T, O, torch.tensor(weight, dtype=dtype), rho, C)[0]
        e.sum().backward()
        return [x.detach().double().numpy() for x in (e, bb.grad, th.grad, O.grad, T.grad)]

    b, t, o, tg = (_dev(x).requires_grad_(True) for x in (beta, theta, offset, target))
    world, _, _ = s.skeleton_differentiable(b, t)
    energy, _, _ = ori.term_differentiable(world, joint, tg, o, _dev(weight), rho, C)
    energy.sum().backward()
    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert _rel(_host(energy.detach()), r64[0]) < 1e-5
    _blocks("chain C=%d grad_theta" % C, t.grad[:, 1:], r64[2][:, 1:], r32[2][:, 1:], VB.THETA)
    # an orientation does not depend on the shape or on the translation: both gradients are exactly zero, in the library as in float64
    assert not _host(b.grad).any() and not r64[1].any() and not _host(t.grad[:, 0]).any() and not r64[2][:, 0].any()
    _blocks("chain C=%d grad_offset" % C, o.grad, r64[3], r32[3], None)
    _blocks("chain C=%d grad_target" % C, tg.grad, r64[4], r32[4], (2, 3))


def test_chain_rotmat_to_smoothness():
    """theta -> axis_angle_to_rotmat_differentiable -> smoothness_differentiable(K=24, C=9) over two problems of 4 and 3 frames."""
    import smplpp_amd.orientation as ori
    from smplpp_amd import model_io
    from smplpp_amd.sequence import SequenceLayout

    lens = [4, 3]
    F = sum(lens)
    _, theta = model_io.synthetic_inputs(F, seed=70)
    ge = np.random.default_rng(71).uniform(0.5, 1.5, F).astype(f32)

    def ref(dtype):
        th = torch.tensor(theta, dtype=dtype, requires_grad=True)
        R = OR.rodrigues(th[:, 1:]).reshape(F, 24, 9)
        g, loss, at = torch.tensor(ge, dtype=dtype), 0, 0
        for T in lens:
            d = R[at + 1:at + T] - R[at:at + T - 1]
            loss = loss + ((d * d).sum((1, 2)) * g[at:at + T - 1]).sum()
            at += T
        loss.backward()
        return float(loss.detach()), th.grad.double().numpy()

    layout = SequenceLayout("cuda:0", lens)
    t = _dev(theta).requires_grad_(True)
    rot = ori.axis_angle_to_rotmat_differentiable(t[:, 1:])
    fe = layout.smoothness_differentiable(rot.reshape(F, 24, 9), order=1, K=24, C=9)
    (fe * _dev(ge)).sum().backward()
    (l64, g64), (_, g32) = ref(torch.float64), ref(torch.float32)
    assert abs(float((fe.detach() * _dev(ge)).sum()) / l64 - 1) < 1e-5
    assert not _host(t.grad[:, 0]).any()
    _blocks("smoothness chain grad_theta", t.grad[:, 1:], g64[:, 1:], g32[:, 1:], VB.THETA)


def test_chain_with_projection():
    """The orientation term in one graph with project_points_differentiable on `posed`: sum energy + sum keypoint energy, gradients to
    theta and beta."""
    import smplpp_amd.orientation as ori
    from smplpp_amd import model_io
    from smplpp_amd import smpl as S_

    s, n, near, rho = _handle(), 3, 0.05, 0.0
    beta, theta = model_io.synthetic_inputs(n, seed=80)
    joint = np.array(SK.IMU_JOINTS)
    _, _, offset, target, _ = OR.random_case(n, 6, 3, seed=81)
    rng = np.random.default_rng(82)
    cam = np.empty((n, 16), f32)
    for f in range(n):
        a = rng.normal(0, 0.2)
        c, sn = np.cos(a), np.sin(a)
        R = np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]]) @ np.diag([1.0, -1.0, -1.0])
        cam[f] = np.concatenate([R.reshape(9), [0.02 * f, -0.03, 4.0], [500.0, 490.0, 320.0, 240.0]])

    def ref(dtype, T2):
        m = SO.cast(_m64(), dtype)
        bb, th = (torch.tensor(x, dtype=dtype, requires_grad=True) for x in (beta, theta))
        sk = SO.skeleton(m, bb, th)
        uv, ok = KP.project_t(sk["posed"], torch.tensor(cam, dtype=dtype), near)
        if T2 is None:
            return uv.detach().numpy()
        e = OR.definition_t(sk["world"], joint, torch.tensor(target, dtype=dtype), torch.tensor(offset, dtype=dtype), None, rho, 3)[0]
        loss = e.sum() + 1e-3 * KP.energy_t(uv, ok, torch.tensor(T2, dtype=dtype), 0.0).sum()
        loss.backward()
        return float(loss.detach()), bb.grad.double().numpy(), th.grad.double().numpy()

    uv0 = ref(torch.float64, None)
    T2 = np.concatenate([uv0 + rng.normal(0, 20.0, uv0.shape), rng.uniform(0.2, 1.0, uv0.shape[:2] + (1,))], -1).astype(f32)
    b, t = (_dev(x).requires_grad_(True) for x in (beta, theta))
    world, posed, _ = s.skeleton_differentiable(b, t)
    energy, _, _ = ori.term_differentiable(world, joint, _dev(target), _dev(offset), None, rho, 3)
    _, e2, ok = S_.project_points_differentiable(posed, _dev(cam), _dev(T2), 0.0, near)
    assert bool(ok.all())
    loss = energy.sum() + 1e-3 * e2.sum()
    loss.backward()
    r64, r32 = ref(torch.float64, T2), ref(torch.float32, T2)
    assert abs(float(loss.detach()) / r64[0] - 1) < 1e-5
    _blocks("projection chain grad_beta", b.grad, r64[1], r32[1], None)
    _blocks("projection chain grad_theta", t.grad, r64[2], r32[2], VB.THETA)


# ---------------------------------------------------------------------------------------------- 6. the three fits
@pytest.mark.parametrize("kind", ["imu", "calibration", "smooth"])
def test_fit_beside_float64(kind):
    """The fits of tests/test_orientation_cpu.py through the library calls, Adam(lr 0.05), 200 steps, beside that file's float64 run on
    the CPU: the last loss is at most twice the float64 run's, or below 1e-6."""
    import smplpp_amd.orientation as ori
    from smplpp_amd import smpl as S_
    from smplpp_amd.sequence import SequenceLayout

    s = _handle()
    term_energy = lambda frames, joint, T, O, w, C: ori.term_differentiable(frames, joint, T, O, w, 0.0, C)[0]  # noqa: E731

    def forward_of(n):
        beta = torch.zeros(n, 10, device="cuda")
        return lambda theta: s.skeleton_differentiable(beta, theta)[:2]

    if kind == "imu":
        got = OR.imu_fit(forward_of(SK.FIT_N), term_energy, torch.float32, "cuda")
    elif kind == "calibration":
        world = s.skeleton(None, _dev(OR.calibration_case()[0]), want=("world",))["world"]
        got = OR.calibration_fit(world, term_energy, S_.rot6d_to_rotmat, torch.float32, "cuda")
    else:
        layout = SequenceLayout("cuda:0", [OR.SMOOTH_T])
        got = OR.smooth_fit(forward_of(OR.SMOOTH_T), term_energy, ori.axis_angle_to_rotmat_differentiable,
                            lambda rot: layout.smoothness_differentiable(rot, order=1), torch.float32, "cuda")
    f64 = CPU.run_fit(kind, torch.float64)
    print("fit %s: device %.6g -> %.6g, float64 %.6g -> %.6g" % (kind, got[0], got[1], f64[0], f64[1]))
    print("fit %s device trajectory  %s" % (kind, " ".join("%.4g" % v for v in got[2])))
    print("fit %s float64 trajectory %s" % (kind, " ".join("%.4g" % v for v in f64[2])))
    assert OR.fit_passes(got[1], f64[1]), (got[:2], f64[:2])


# ---------------------------------------------------------------------------------------------- 7. C++ shim
def test_orientation_cpp_shim(tmp_path):
    import smplpp_amd.orientation as ori

    exe = str(tmp_path / "orientation_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "orientation_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    n, J, S = 3, 5, 4
    ar = lambda count: np.arange(count)  # noqa: E731
    world = (((ar(n * J * 12) * 7) % 23 - 11).astype(f32) * f32(0.0625)).reshape(n, J, 3, 4)
    rot = (((ar(n * J * 9) * 5) % 19 - 9).astype(f32) * f32(0.125)).reshape(n, J, 3, 3)
    offset = (((ar(S * 9) * 3) % 11 - 5).astype(f32) * f32(0.25)).reshape(S, 3, 3)
    target = (((ar(n * S * 9) * 11) % 17 - 8).astype(f32) * f32(0.125)).reshape(n, S, 3, 3)
    axis = ((ar(S * 3) % 5 - 2).astype(f32) * f32(0.5)).reshape(1, S, 3, 1)
    gse = ((ar(n * S) % 7 - 3).astype(f32) * f32(0.25)).reshape(n, S)
    gr = (f32(-0.25) + f32(0.0625) * (ar(n * S * 9) % 9).astype(f32)).reshape(n, S, 3, 3)
    aa = ((ar(n * J * 3) % 11 - 5).astype(f32) * f32(0.05)).reshape(n, J, 3)
    joint = np.array([4, 1, 1, 0])
    weight = np.array([[1.0, 0.5, 2.0, 0.0]], f32)
    ge = np.array([1.0, -0.5, 0.25], f32)
    a = ori.term(world, joint, target, offset, weight)
    g = ori.termBackward(world, joint, target, offset, weight, grad_energy=ge, grad_sensor_energy=gse, grad_residual=gr)
    g2 = {k: v.copy() for k, v in g.items()}
    ori.termBackward(world, joint, target, offset, weight, grad_energy=ge, out=g2)
    b = ori.term(rot, joint, axis, None, None, 0.5, 1, want=("energy",))
    h = ori.termBackward(rot, joint, axis, None, None, 0.5, 1, grad_energy=ge)
    ga = ori.axis_angle_to_rotmat_backward(aa, rot)
    ga2 = ori.axis_angle_to_rotmat_backward(aa, rot, out=ga.copy())
    want = [a["energy"], a["sensor_energy"], a["residual"], g["frames"], g["offset"], g["target"], g2["frames"], g2["offset"], g2["target"],
            b["energy"], h["frames"], h["offset"], h["target"], ga, ga2]
    assert (g["frames"] != 0).any() and (h["target"] != 0).any() and (ga != 0).any()
    raw = open(outp, "rb").read()
    assert len(raw) == 4 * sum(v.size for v in want)
    off = 0
    for k, v in enumerate(want):
        got = np.frombuffer(raw, f32, v.size, off).reshape(v.shape)
        off += 4 * v.size
        assert _same(got, v), k
