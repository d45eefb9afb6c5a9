"""Rigid and similarity alignment on the MI355X (smplpp_align, smplpp_align_vjp): every bit against the float32 restatement of
tests/align_oracle.py at the form boundaries of frame_sum_split, with points that are not live, mirrored targets and every status bit; all
cotangent combinations, storing and adding, each gradient alone; independence of the batch, the slot, the memory space and the outputs
asked for; the refusals; the C++ shim; the gradient through FK and the landmarks against float64 autograd of the SVD definition; a shared
target under autograd; an ICP fit; and pa_mpjpe."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_oracle as AL  # noqa: E402
import fk_vjp_oracle as FK  # noqa: E402
import keypoints_oracle as KP  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 7.0
f32 = np.float32
KS = (1, 2, 3, 4, 63, 64, 65, 1024, 1025, 1030)  # the work split changes after 64 and after 1024
COTANGENTS = [c for c in itertools.product((False, True), repeat=3) if any(c)]
OUTS = ("transform", "aligned", "energy", "point_error", "gap", "status")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _same(a, b):
    """The same bits where neither is NaN, and NaN in the same places."""
    a, b = np.ascontiguousarray(_host(a)), np.ascontiguousarray(b)
    if a.dtype == np.int32:
        return a.shape == b.shape and b.dtype == np.int32 and np.array_equal(a, b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.where(np.isnan(a), f32(0), a).tobytes() == np.where(np.isnan(b), f32(0), b).tobytes()


def _case(K, n, i):
    """The case of turn i: rigid or similarity, Tn and Wn in {1, n}, mirrored targets, points that are not live (K >= 63), and for
    n = 3 with per-frame weights a middle frame without a live point."""
    ki, ni = i // 2, i % 2
    with_scale, Tn, Wn, mirrored = (ki + ni) % 2 == 1, (n, 1)[(ki // 2 + ni) % 2], (n, 1, 0)[(ki + 2 * ni) % 3], ki % 3 == 1
    x, y = AL.random_case(n, K, 300 + i, mirrored=mirrored, scale=1.3 if with_scale else 1.0, shared=Tn == 1)
    y = np.ascontiguousarray(y[:Tn])
    w = None if Wn == 0 else np.random.default_rng(400 + i).uniform(0.25, 2.0, (Wn, K)).astype(f32)
    if K >= 63:
        AL.special_points(x, y, w, seed=i)
    if w is not None and Wn == n and n == 3:
        w[1] = 0.0
    return x, y, w, with_scale


def _check_all(x, y, w, with_scale, seed, cots, case):
    """Every output of both calls on device tensors against the restatement; the cotangent combinations `cots`, storing and adding,
    both gradients together and each alone."""
    from smplpp_amd import align as A

    n, K = x.shape[:2]
    dx, dy, dw = _dev(x), _dev(y), _dev(w)
    want = dict(zip(OUTS, AL.align(x, y, w, with_scale)))
    got = A.align(dx, dy, dw, with_scale)
    for k in OUTS:
        assert _same(got[k], want[k]), (case, k)
    rng = np.random.default_rng(seed)
    gtr, gal, ge = rng.normal(size=(n, 13)).astype(f32), rng.normal(size=(n, K, 3)).astype(f32), rng.normal(size=n).astype(f32)
    fill = np.full((n, K, 3), FILL, f32)
    for ht, ha, he in cots:
        a, b, c = gtr if ht else None, gal if ha else None, ge if he else None
        ws, wt = AL.align_vjp(x, y, w, with_scale, AL.MIN_GAP, a, b, c, fill, fill, 0)
        kw = dict(grad_transform=_dev(a), grad_aligned=_dev(b), grad_energy=_dev(c))
        g = A.alignBackward(dx, dy, dw, with_scale, **kw)
        assert _same(g["source"], ws) and _same(g["target"], wt), (case, ht, ha, he)
        ws2, wt2 = AL.align_vjp(x, y, w, with_scale, AL.MIN_GAP, a, b, c, ws.copy(), wt.copy(), 1)
        again = A.alignBackward(dx, dy, dw, with_scale, out=g, **kw)
        assert again is g and _same(g["source"], ws2) and _same(g["target"], wt2), (case, ht, ha, he)
        assert _same(A.alignBackward(dx, dy, dw, with_scale, want=("source",), **kw)["source"], ws), (case, ht, ha, he)
        assert _same(A.alignBackward(dx, dy, dw, with_scale, want=("target",), **kw)["target"], wt), (case, ht, ha, he)
    return want


# ---------------------------------------------------------------------------------------------------- 1. bits
def test_bits():
    """Both calls for every K at which the work split changes and n = 1 and 3.  Along the twenty (K, n) the other choices take turns: rigid
    or similarity, Tn and Wn, mirrored targets, points that are not live, a frame without a live point.  All seven cotangent combinations up
    to K = 65, two of them above.  Every status bit appears, and most frames have none."""
    seen, status = set(), []
    for i, (K, n) in enumerate(itertools.product(KS, (1, 3))):
        x, y, w, with_scale = _case(K, n, i)
        seen.add((with_scale, y.shape[0] == n, None if w is None else w.shape[0] == n))
        cots = COTANGENTS if K <= 65 else [(True, True, True), COTANGENTS[i % 7]]
        out = _check_all(x, y, w, with_scale, 100 + i, cots, (K, n, i))
        status += out["status"].tolist()
        if K >= 63:
            assert np.isnan(out["aligned"]).any() and np.isfinite(out["transform"]).all() and np.isfinite(out["energy"]).all()
    assert len({s[0] for s in seen}) == 2 and len({s[1] for s in seen}) >= 2 and len({s[2] for s in seen}) == 3
    assert any(s & 1 for s in status) and any(s & 2 for s in status) and any(s & 4 for s in status) and status.count(0) >= len(status) // 2


def test_degenerate_frames():
    """Coincident source points (bit 1), collinear points (bit 2 at min_gap = 1e-3), all weights zero (bit 0) and a sound frame, in one
    batch at K = 5, 70 and 1100: the bits of both calls, and the gradient of a frame with a status bit is the direct part alone."""
    from smplpp_amd import align as A

    for K in (5, 70, 1100):
        x, y = AL.random_case(4, K, 500 + K)
        x[0] = np.array([0.25, -0.5, 0.75], f32)  # coincident, at coordinates whose weighted sums are exact
        line = np.linspace(-1, 1, K, dtype=f32)[:, None]
        x[1] = line * np.array([0.5, 0.25, -0.125], f32) + f32(0.25)
        y[1] = line * np.array([0.25, -0.5, 0.125], f32) - f32(0.5)
        w = np.ones((4, K), f32)
        w[2] = 0
        want = dict(zip(OUTS, AL.align(x, y, w, True)))
        got = A.align(_dev(x), _dev(y), _dev(w), True)
        for k in OUTS:
            assert _same(got[k], want[k]), (K, k)
        st = want["status"]
        assert st[0] & 2 and st[1] == 4 and st[2] == 1 and st[3] == 0, st
        rng = np.random.default_rng(K)
        gtr, gal, ge = rng.normal(size=(4, 13)).astype(f32), rng.normal(size=(4, K, 3)).astype(f32), rng.normal(size=4).astype(f32)
        ws, wt = AL.align_vjp(x, y, w, True, AL.MIN_GAP, gtr, gal, ge, np.zeros_like(x), np.zeros_like(x), 0)
        g = A.alignBackward(_dev(x), _dev(y), _dev(w), True, grad_transform=_dev(gtr), grad_aligned=_dev(gal), grad_energy=_dev(ge))
        assert _same(g["source"], ws) and _same(g["target"], wt) and np.isfinite(ws).all() and np.isfinite(wt).all(), K
        assert (wt[2] == 0).all()


# ---------------------------------------------------------------------------------------------------- 2. independence
@pytest.mark.parametrize("K", [24, 65, 1030])
def test_independence(K):
    """A frame's bits alone, among others, in another slot, in host and device space, and with single outputs."""
    from smplpp_amd import align as A

    own_x, own_y = (a[0] for a in AL.random_case(1, K, 600 + K, scale=1.2))
    rng = np.random.default_rng(8)
    own_w = rng.uniform(0.25, 2.0, K).astype(f32)
    own_w[::4] = 0
    own_gtr, own_gal, own_ge = rng.normal(size=13).astype(f32), rng.normal(size=(K, 3)).astype(f32), f32(0.75)
    ref = None
    for n, slot in ((1, 0), (3, 1), (4, 3)):
        x, y = AL.random_case(n, K, 700 + n)
        w = rng.uniform(0.25, 2.0, (n, K)).astype(f32)
        gtr, gal, ge = rng.normal(size=(n, 13)).astype(f32), rng.normal(size=(n, K, 3)).astype(f32), rng.normal(size=n).astype(f32)
        x[slot], y[slot], w[slot], gtr[slot], gal[slot], ge[slot] = own_x, own_y, own_w, own_gtr, own_gal, own_ge
        for dev in (True, False):
            p = (lambda a: _dev(a)) if dev else (lambda a: a)
            out = dict(A.align(p(x), p(y), p(w), True))
            out.update({"g_" + k: v for k, v in A.alignBackward(p(x), p(y), p(w), True, grad_transform=p(gtr), grad_aligned=p(gal), grad_energy=p(ge)).items()})
            mine = {k: np.asarray(_host(v)[slot]) for k, v in out.items()}
            if ref is None:
                ref = mine
            for k in ref:
                assert _same(mine[k], ref[k]), (n, slot, dev, k)
        for k in OUTS:
            assert _same(np.asarray(_host(A.align(_dev(x), _dev(y), _dev(w), True, want=(k,))[k])[slot]), ref[k]), k
        for k in ("source", "target"):
            got = A.alignBackward(_dev(x), _dev(y), _dev(w), True, grad_transform=_dev(gtr), grad_aligned=_dev(gal), grad_energy=_dev(ge), want=(k,))[k]
            assert _same(_host(got)[slot], ref["g_" + k]), k
    one = lambda a: a[None]  # noqa: E731
    want = AL.align(one(own_x), one(own_y), one(own_w), True)
    for k, v in zip(OUTS, want):
        assert _same(ref[k], v[0]), k
    ws, wt = AL.align_vjp(one(own_x), one(own_y), one(own_w), True, AL.MIN_GAP, one(own_gtr), one(own_gal), np.array([own_ge]),
                          np.zeros((1, K, 3), f32), np.zeros((1, K, 3), f32), 0)
    assert _same(ref["g_source"], ws[0]) and _same(ref["g_target"], wt[0]) and ref["status"] == 0


# ---------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals():
    """Every refusal of the list on device tensors: SMPLPP_ERR_INVALID, and the outputs keep their values."""
    from smplpp_amd import _lib

    Lb = _lib.load()
    n, K = 2, 4
    dev = lambda *shape: torch.full(shape, FILL, device="cuda")  # noqa: E731
    x, y = (_dev(a) for a in AL.random_case(n, K, 1))
    wgt = torch.ones(n, K, device="cuda")
    outs = dict(tr=dev(n, 13), al=dev(n, K, 3), e=dev(n), pe=dev(n, K), gap=dev(n), gs=dev(n, K, 3), gt=dev(n, K, 3))
    status = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    D = _lib.DEVICE

    def fwd(n_=n, K_=K, x_=x, y_=y, Tn=n, w=None, Wn=1, ws=0, mg=1e-3, tr=outs["tr"], al=outs["al"], e=outs["e"], pe=outs["pe"], gap=outs["gap"],
            st=status, space=D):
        return Lb.smplpp_align(0, n_, K_, P(x_), P(y_), Tn, P(w), Wn, ws, mg, P(tr), P(al), P(e), P(pe), P(gap), P(st), space, None)

    def vjp(n_=n, K_=K, x_=x, y_=y, Tn=n, w=None, Wn=1, ws=0, mg=1e-3, gtr=outs["tr"], gal=None, ge=None, gs=outs["gs"], gt=outs["gt"], acc=0, space=D):
        return Lb.smplpp_align_vjp(0, n_, K_, P(x_), P(y_), Tn, P(w), Wn, ws, mg, P(gtr), P(gal), P(ge), P(gs), P(gt), acc, space, None)

    common = [dict(n_=0), dict(n_=-1), dict(K_=0), dict(K_=-3), dict(Tn=3), dict(Tn=0), dict(w=wgt, Wn=3), dict(Wn=0), dict(ws=2), dict(ws=-1),
              dict(mg=-0.5), dict(mg=float("inf")), dict(mg=float("nan")), dict(x_=None), dict(y_=None), dict(n_=2 ** 20, K_=2 ** 10, Tn=1),
              dict(space=2)]
    refused = [fwd(**kw) for kw in common + [dict(tr=None, al=None, e=None, pe=None, gap=None, st=None)]]
    refused += [vjp(**kw) for kw in common + [dict(gtr=None), dict(gs=None, gt=None), dict(acc=2), dict(acc=-1)]]
    torch.cuda.synchronize()
    assert all(rc == 1 for rc in refused), refused
    for k, t in outs.items():
        assert (t == FILL).all(), k
    assert (status == 7).all()
    # and the same calls go through once the argument is put right
    assert fwd() == 0 and vjp() == 0 and fwd(w=wgt, Wn=n, ws=1) == 0 and fwd(tr=None, al=None, e=None, pe=None, gap=None) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 4. C++ shim
def test_align_cpp_shim(tmp_path):
    exe = str(tmp_path / "align_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "align_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    n, K = 2, 7
    j = np.arange(n * K * 3)
    x = (((j * 7) % 23 - 11).astype(f32) * f32(0.0625)).reshape(n, K, 3)
    y = (((j * 5) % 19 - 9).astype(f32) * f32(0.125)).reshape(n, K, 3)
    w = np.array([[1.0, 0.5, 0.0, 2.0, 1.0, 0.75, 1.5]], f32)
    m = np.arange(n * 13)
    gtr = (f32(0.25) - f32(0.0625) * (m % 7).astype(f32)).reshape(n, 13)
    gal = (f32(-0.25) + f32(0.0625) * (j % 9).astype(f32)).reshape(n, K, 3)
    ge = np.array([1.0, -0.5], f32)
    a = AL.align(x, y, w, True)
    b = AL.align(x, y[:1], None, False)
    s1, t1 = AL.align_vjp(x, y, w, True, AL.MIN_GAP, gtr, gal, ge, np.zeros_like(x), np.zeros_like(x), 0)
    s2, t2 = AL.align_vjp(x, y, w, True, AL.MIN_GAP, None, None, ge, s1.copy(), t1.copy(), 1)
    want = [a[0], a[1], a[2], a[3], a[4], a[5].astype(f32), b[0], b[2], s1, t1, s2, t2]
    assert (a[5] == 0).all() and (s1 != 0).any() and (t1 != 0).any()
    raw = open(outp, "rb").read()
    assert len(raw) == 4 * sum(v.size for v in want)
    off = 0
    for k, v in enumerate(want):
        got = np.frombuffer(raw, f32, v.size, off).reshape(v.shape)
        off += 4 * v.size
        assert _same(got, np.ascontiguousarray(v)), k


# ---------------------------------------------------------------------------------------------------- 5. the gradient and the fit
def _smpl(model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    return s


def test_gradient_through_the_chain(synth_model):
    """theta, beta -> smplpp_fk -> Landmarks (53 rows) -> align_differentiable (similarity) against fixed noisy targets -> energy, n = 2,
    against float64 autograd of the same graph with the SVD definition, within max(4 x the error of fp32 autograd, 1e-5)."""
    import test_pose_prior_gpu as TP
    from smplpp_amd import align as A
    from smplpp_amd.landmarks import Landmarks

    case = AL.chain_case(synth_model)
    s = _smpl(synth_model)
    lm = Landmarks(s, *case["reg"])
    beta, theta = (_dev(case[k]).requires_grad_(True) for k in ("beta", "theta"))
    verts, joints = s.forward_differentiable(beta, theta)
    _, _, energy = A.align_differentiable(lm.forward_differentiable(verts, joints), _dev(case["target"]), _dev(case["weight"]), True)
    energy.sum().backward()

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        b, t = (torch.tensor(case[k], dtype=dtype, requires_grad=True) for k in ("beta", "theta"))
        out = FK.fk(m, b, t)
        pts = KP.landmarks_t(torch.tensor(case["dense"], dtype=dtype), out["verts"], out["joints"])
        e = AL.definition_t(pts, torch.tensor(case["target"], dtype=dtype), torch.tensor(case["weight"], dtype=dtype), True)[4]
        e.sum().backward()
        return [v.detach().double().numpy() for v in (e, b.grad, t.grad)]

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert np.allclose(_host(energy.detach()), r64[0], rtol=1e-3)
    TP._bar(beta.grad, r64[1], r32[1], "alignment energy through the chain, beta")
    TP._bar(theta.grad, r64[2], r32[2], "alignment energy through the chain, theta")


def test_differentiable_with_a_shared_target():
    """align_differentiable with one target for three frames: the gradient to the source is alignBackward's, the gradient to the target
    is its per-frame gradient summed over the frames, and a target of shape (K, 3) gets its own shape back."""
    from smplpp_amd import align as A

    x, y = AL.random_case(3, 40, 900, scale=1.2, shared=True)
    w = np.random.default_rng(2).uniform(0.5, 2.0, (3, 40)).astype(f32)
    for shape in ((1, 40, 3), (40, 3)):
        src, tgt = _dev(x).requires_grad_(True), _dev(y[0].reshape(shape)).requires_grad_(True)
        tr, al, e = A.align_differentiable(src, tgt, _dev(w), True)
        (e.sum() + (al * al).sum() + tr.sum()).backward()
        g = A.alignBackward(_dev(x), _dev(y[:1]), _dev(w), True, grad_transform=torch.ones_like(tr), grad_aligned=2 * al.detach(),
                            grad_energy=torch.ones_like(e))
        assert _same(src.grad, _host(g["source"])) and tgt.grad.shape == shape
        assert _same(tgt.grad.reshape(40, 3), _host(g["target"].sum(0)))


def test_icp_fit(synth_model):
    """Two bodies, each with a cloud of 2000 of its posed vertices under 2 mm noise, turned by 25 degrees and moved 0.2 m; ten steps of
    meshPointDistance -> gather -> align (rigid; source: the matched cloud points, target: the vertices) -> apply.  The RMS falls at
    every step and ends within 2x of the float64 schedule on the CPU (align_oracle.icp_float64; DESIGN 3.25 has both trajectories)."""
    from smplpp_amd import align as A
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(2, seed=5)
    m = FK.model_tensors(synth_model, torch.float64)
    with torch.no_grad():
        v64 = FK.fk(m, torch.tensor(beta, dtype=torch.float64), torch.tensor(theta, dtype=torch.float64))["verts"].numpy()
    cloud0 = AL.icp_case(v64)
    r64 = AL.icp_float64(v64, cloud0)
    s = _smpl(synth_model)
    verts = _dev(s.launch(beta, theta, want=("verts",))["verts"])
    cloud = _dev(cloud0)
    rms = []
    rows = torch.arange(2, device="cuda")[:, None]
    for _ in range(AL.ICP_STEPS):
        index, sq = s.meshPointDistance(verts, cloud)
        rms.append(_host(sq.double().mean(1).sqrt()))
        tr = A.align(cloud[rows, index].contiguous(), verts, want=("transform",))["transform"]
        cloud = A.apply(tr, cloud).contiguous()
    rms.append(_host(s.meshPointDistance(verts, cloud)[1].double().mean(1).sqrt()))
    rms = np.stack(rms, 1)
    for f in range(2):
        print("float64 frame %d: RMS (mm) %s" % (f, np.round(1e3 * r64[f], 3)))
        print("MI355X  frame %d: RMS (mm) %s" % (f, np.round(1e3 * rms[f], 3)))
    assert (np.diff(rms, axis=1) < 0).all(), rms
    assert (rms[:, -1] <= 2 * r64[:, -1]).all(), (rms[:, -1], r64[:, -1])


def test_pa_mpjpe(synth_model):
    """pa_mpjpe of a body's joints against their own similarity transform is below the float32 bar (1e-5 of the body's size), and plain
    mpjpe equals the numpy mean."""
    from smplpp_amd import align as A
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(3, seed=9)
    s = _smpl(synth_model)
    joints = s.launch(beta, theta, want=("joints",))["joints"]
    n, K = joints.shape[:2]
    rng = np.random.default_rng(3)
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    Q = Q * np.sign(np.linalg.det(Q))[:, None, None]
    gt = (1.7 * np.einsum("nab,nkb->nka", Q, joints.astype(np.float64)) + rng.normal(0, 1, (n, 1, 3))).astype(f32)
    size = np.linalg.norm(gt - gt.mean(1, keepdims=True), axis=-1).max()
    for p in (lambda a: a, _dev):
        pa = _host(A.pa_mpjpe(p(joints), p(gt)))
        print("pa_mpjpe of a similarity-transformed body: %s m (size %.3g m)" % (pa, size))
        assert pa.shape == (n,) and (pa <= 1e-5 * size).all(), pa
        plain = _host(A.mpjpe(p(joints), p(gt)))
        want = np.linalg.norm(joints - gt, axis=-1).mean(-1)
        assert np.allclose(plain, want, rtol=1e-6) and (plain > 100 * pa).all()
