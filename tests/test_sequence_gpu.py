"""The sequence terms on the MI355X (smplpp_sequence_split, _merge, _sum, _smoothness, _smoothness_vjp): every bit against the numpy
restatement of tests/sequence_oracle.py; independence of the other problems, of the slot, of the memory space and of the outputs asked
for; NaN containment; the gradient through the autograd wrappers against float64 autograd, alone, in one graph with FK and through the
shared row; the refusals; the C++ shim; and the two-sequence fit of test_lbfgs_groups_gpu with its torch glue replaced by these calls."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import sequence_oracle as SO  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
FILL = 7.0
f32 = np.float32


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _same(a, b):
    """The same bits where neither is NaN, and NaN in the same places (a NaN's sign and payload are not part of the rule)."""
    a, b = np.ascontiguousarray(_host(a)), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.where(np.isnan(a), f32(0), a).tobytes() == np.where(np.isnan(b), f32(0), b).tobytes()


def _layout(groups, shared=0):
    from smplpp_amd.sequence import SequenceLayout

    return SequenceLayout("cuda:0", groups, shared)


def _put(a, dev):
    return _dev(a) if dev and a is not None else a


def _points(F, K, C, ld, seed, pad=np.nan):
    """[F, ld] float32: a random walk in time of K C coordinates per frame, `pad` in the floats past them."""
    rng = np.random.default_rng(seed)
    x = np.full((F, ld), pad, f32)
    x[:, :K * C] = (np.cumsum(rng.normal(0, 0.05, (F, K * C)), 0) + rng.normal(0, 1.0, (1, K * C))).astype(f32)
    return x


def _weights(K, seed):
    w = np.random.default_rng(seed).uniform(0.25, 2.0, K).astype(f32)
    w[::3] = 0.0
    return w


# ---------------------------------------------------------------------------------------------------- 1. bits
GROUPS = [[1], [2], [3], [1, 2, 5, 3]]
KS, CS = (1, 24, 65, 1030), (1, 3, 9)


@pytest.mark.parametrize("shared", [0, 1])
@pytest.mark.parametrize("frames", GROUPS, ids=lambda g: "-".join(map(str, g)))
def test_smoothness_bits(frames, shared):
    """Both calls of the temporal term for every K, C, order, rho and weight, in rows longer than K C with NaN in the padding, storing and
    adding.  `frames` are the frames per problem; with a shared row the optimiser's groups are one longer."""
    from smplpp_amd import _lib

    seq = _layout([t + shared for t in frames], shared)
    L = SO.layout([t + shared for t in frames], shared)
    F = L["frames"]
    assert seq.frames == F == sum(frames) and seq.frame_start.tolist() == L["frame_start"].tolist()
    for i, (K, C, order, rho, weighted) in enumerate(itertools.product(KS, CS, (1, 2), (0.0, 0.05), (False, True))):
        ld = K * C + 1 + i % 3
        x = _points(F, K, C, ld, seed=i)
        w = _weights(K, i) if weighted else None
        rng = np.random.default_rng(1000 + i)
        gfe, gpe = rng.normal(size=F).astype(f32), rng.normal(size=(F, K)).astype(f32)
        gfe[F // 2] = 0.0
        case = (K, C, order, rho, weighted)
        fe, pe = SO.smoothness(L, x, K, C, order, w, rho)
        r = seq.smoothness(_dev(x), order, _dev(w), rho, K=K, C=C)
        assert _same(r["frame_energy"], fe) and _same(r["point_energy"], pe), case
        dx, dw = _dev(x), _dev(w)
        for gf, gp in ((gfe, gpe), (gfe, None), (None, gpe)):
            dgf, dgp = _dev(gf), _dev(gp)
            want = SO.smoothness_vjp(L, x, K, C, order, w, rho, gf, gp, np.full((F, ld), FILL, f32), 0)
            got = torch.full((F, ld), FILL, device="cuda")  # stored through the ABI into a buffer of our own: the padding stays
            _lib.check(_lib.load().smplpp_sequence_smoothness_vjp(seq.handle, dx.data_ptr(), ld, K, C, order, None if w is None else dw.data_ptr(), rho,
                                                                  None if gf is None else dgf.data_ptr(), None if gp is None else dgp.data_ptr(),
                                                                  got.data_ptr(), 0, _lib.DEVICE, torch.cuda.current_stream().cuda_stream))
            assert _same(got, want), case
            want2 = SO.smoothness_vjp(L, x, K, C, order, w, rho, gf, gp, want.copy(), 1)
            got2 = seq.smoothnessBackward(dx, dgf, dgp, order, dw, rho, K=K, C=C, out=got)
            assert got2 is got and _same(got, want2), case
        fresh = seq.smoothnessBackward(dx, dgf, dgp, order, dw, rho, K=K, C=C)  # without out: zeros in the padding
        assert _same(fresh, SO.smoothness_vjp(L, x, K, C, order, w, rho, gf, gp, np.zeros((F, ld), f32), 0)), case


@pytest.mark.parametrize("K", [64, 1024, 1025])
def test_smoothness_bits_at_the_kernel_thresholds(K):
    """The forward changes its work split after K = 64 and after K = 1024: the last K of one split and the first of the next (65 is above)."""
    groups = [1, 2, 5, 3]
    seq, L = _layout(groups), SO.layout(groups)
    F, C = L["frames"], 3
    x, w = _points(F, K, C, K * C + 1, seed=K), _weights(K, K)
    for order, rho in ((1, 0.05), (2, 0.0)):
        fe, pe = SO.smoothness(L, x, K, C, order, w, rho)
        r = seq.smoothness(_dev(x), order, _dev(w), rho, K=K, C=C)
        assert _same(r["frame_energy"], fe) and _same(r["point_energy"], pe), (K, order)
        assert _same(seq.smoothness(_dev(x), order, _dev(w), rho, K=K, C=C, want=("frame_energy",))["frame_energy"], fe)


def test_theta_view():
    """The rotations of a theta buffer read in place: (theta + 3, ld 75, K 24, C 3), NaN in the translations."""
    groups = [4, 6]
    seq, L = _layout(groups), SO.layout(groups)
    F = L["frames"]
    theta = np.random.default_rng(2).normal(0, 0.3, (F, 25, 3)).astype(f32)
    theta[:, 0] = np.nan
    x = np.ascontiguousarray(theta.reshape(F, 75)[:, 3:])
    w = _weights(24, 3)
    for order, rho in ((1, 0.0), (2, 0.05)):
        fe, pe = SO.smoothness(L, x, 24, 3, order, w, rho)
        r = seq.smoothness(_dev(theta), order, _dev(w), rho, K=24, C=3, offset=3)
        assert _same(r["frame_energy"], fe) and _same(r["point_energy"], pe)
        g = np.random.default_rng(4).normal(size=F).astype(f32)
        want = np.full((F, 75), FILL, f32)
        want[:, 3:] = SO.smoothness_vjp(L, x, 24, 3, order, w, rho, g, None, np.full((F, 72), FILL, f32), 1)
        got = seq.smoothnessBackward(_dev(theta), _dev(g), None, order, _dev(w), rho, K=24, C=3, offset=3, out=torch.full((F, 25, 3), FILL, device="cuda"))
        assert _same(got.reshape(F, 75), want)
        fresh = seq.smoothnessBackward(_dev(theta), _dev(g), None, order, _dev(w), rho, K=24, C=3, offset=3)
        assert (_host(fresh)[:, 0] == 0).all() and _same(_host(fresh).reshape(F, 75)[:, 3:], SO.smoothness_vjp(L, x, 24, 3, order, w, rho, g, None, np.zeros((F, 72), f32), 0))


def _buffer_case(L, ld, off_f, C_f, C_s, seed):
    """rows [n, ld] with NaN outside the slices that split reads, and the cotangents."""
    rng = np.random.default_rng(seed)
    n, F = L["rows"], L["frames"]
    rows = np.full((n, ld), np.nan, f32)
    fr = L["frame_of"] >= 0
    rows[fr, off_f:off_f + C_f] = rng.normal(size=(int(fr.sum()), C_f)).astype(f32)
    if C_s:
        rows[~fr, :C_s] = rng.normal(size=(int((~fr).sum()), C_s)).astype(f32)
    return rows, rng.normal(size=(F, C_f)).astype(f32), rng.normal(size=(F, max(C_s, 1))).astype(f32), rng.normal(size=F).astype(f32)


@pytest.mark.parametrize("shared", [0, 1])
@pytest.mark.parametrize("frames", GROUPS + [[1030]], ids=lambda g: "-".join(map(str, g)))
def test_split_merge_sum_bits(frames, shared):
    """split, merge and sum, with (off_f, C_f, C_s) = (3, 72, 10) in rows of 80 floats holding D = 76 coordinates; [1030] is a problem whose
    shared sum and frame sum run past partial 1023."""
    groups = [t + shared for t in frames]
    seq, L = _layout(groups, shared), SO.layout(groups, shared)
    n, F, P, ld, D, off_f, C_f, C_s = L["rows"], L["frames"], L["P"], 80, 76, 3, 72, 10 if shared else 0
    rows, gf, gs, fv = _buffer_case(L, ld, off_f, C_f, C_s, seed=len(frames) + shared)
    want_f, want_s = SO.split(L, rows, off_f, C_f, C_s if shared else None)
    got_f, got_s = seq.split(_dev(rows), off_f, C_f, C_s if shared else None)
    assert _same(got_f, want_f) and not np.isnan(want_f).any() and (got_s is None if not shared else _same(got_s, want_s) and not np.isnan(want_s).any())
    if shared:  # each output alone
        assert _same(seq.split(_dev(rows), off_f, C_f)[0], want_f) and _same(seq.split(_dev(rows), C_s=C_s)[1], want_s)
    for a, b in ((gf, gs if shared else None), (gf, None), (None, gs)) if shared else ((gf, None),):
        want = SO.merge(L, a, off_f, C_f, b, C_s, np.full((n, ld), FILL, f32), D, 0)
        out = torch.full((n, ld), FILL, device="cuda")
        assert seq.merge(_dev(a), off_f, _dev(b), out=out[:, :D]) is not None and _same(out, want)
        assert (want[:, D:] == FILL).all() and (want[L["frame_of"] >= 0][:, :off_f] == 0).all()
        want2 = SO.merge(L, a, off_f, C_f, b, C_s, want.copy(), D, 1)
        seq.merge(_dev(a), off_f, _dev(b), out=out[:, :D], accumulate=True)
        assert _same(out, want2)
        fresh = seq.merge(_dev(a), off_f, _dev(b), D=D)
        assert _same(fresh, want[:, :D])
    want_p = SO.seq_sum(L, fv, 0.75, np.zeros(P, f32), 0)
    got_p = seq.sum(_dev(fv), 0.75)
    assert _same(got_p, want_p)
    seq.sum(_dev(fv), -2.0, out=got_p, accumulate=True)
    assert _same(got_p, SO.seq_sum(L, fv, -2.0, want_p.copy(), 1))


# ---------------------------------------------------------------------------------------------------- 2. independence
def _all_five(seq, L, rows, x, K, C, order, w, rho, gfe, gpe, gf, gs, fv, dev, off_f=3, C_f=72, C_s=10, D=76):
    """Every output of the five calls in one memory space, as numpy arrays."""
    sh = L["shared_rows"] == 1
    p = lambda a: _put(a, dev)  # noqa: E731
    out = {}
    out["frames"], out["shared"] = seq.split(p(rows), off_f, C_f, C_s if sh else None)
    base = np.full((L["rows"], D), FILL, f32)
    out["merged"] = seq.merge(p(gf), off_f, p(gs) if sh else None, out=p(base), accumulate=True)
    out["problems"] = seq.sum(p(fv), 1.5)
    out.update(seq.smoothness(p(x), order, p(w), rho, K=K, C=C))
    out["grad_x"] = seq.smoothnessBackward(p(x), p(gfe), p(gpe), order, p(w), rho, K=K, C=C)
    return {k: _host(v) for k, v in out.items() if v is not None}


@pytest.mark.parametrize("K,order,rho", [(24, 1, 0.0), (65, 2, 0.05), (1030, 2, 0.0)])
def test_independence(K, order, rho):
    """A problem of 5 frames (+ its shared row) among others, in another slot, alone, in host space, and with single outputs asked for."""
    C, shared = 3, 1
    batch = {"among": ([2, 4, 6, 3], 2), "first": ([6, 3], 0), "last": ([3, 2, 6], 2), "alone": ([6], 0)}
    ref = None
    for name, (groups, slot) in batch.items():
        seq, L = _layout(groups, shared), SO.layout(groups, shared)
        F, n, ld = L["frames"], L["rows"], K * C + 2
        f0, f1, r0, r1 = L["frame_start"][slot], L["frame_start"][slot + 1], L["row_start"][slot], L["row_start"][slot + 1]
        # the problem's own data from fixed seeds, everybody else's from the batch's
        rows, gf, gs, fv = _buffer_case(L, 80, 3, 72, 10, seed=sum(map(ord, name)))
        x = _points(F, K, C, ld, seed=len(name))
        rng = np.random.default_rng(len(name))
        gfe, gpe = rng.normal(size=F).astype(f32), rng.normal(size=(F, K)).astype(f32)
        own = SO.layout([6], shared)
        rows[r0:r1], gf[f0:f1], gs[f0:f1], fv[f0:f1] = _buffer_case(own, 80, 3, 72, 10, seed=77)
        x[f0:f1] = _points(5, K, C, ld, seed=78)
        orng = np.random.default_rng(79)
        gfe[f0:f1], gpe[f0:f1] = orng.normal(size=5).astype(f32), orng.normal(size=(5, K)).astype(f32)
        w = _weights(K, 5)
        for dev in (True, False):
            got = _all_five(seq, L, rows, x, K, C, order, w, rho, gfe, gpe, gf, gs, fv, dev)
            mine = {k: v[slot:slot + 1] if k == "problems" else (v[r0:r1] if k == "merged" else v[f0:f1]) for k, v in got.items()}
            if ref is None:
                ref = mine
            for k in ref:
                assert _same(mine[k], ref[k]), (name, dev, k)
        # single outputs
        assert _same(seq.smoothness(_dev(x), order, _dev(w), rho, K=K, C=C, want=("frame_energy",))["frame_energy"][f0:f1], ref["frame_energy"])
        assert _same(seq.smoothness(_dev(x), order, _dev(w), rho, K=K, C=C, want=("point_energy",))["point_energy"][f0:f1], ref["point_energy"])


# ---------------------------------------------------------------------------------------------------- 3. NaN containment
@pytest.mark.parametrize("order", [1, 2])
def test_nan_containment(order):
    groups = [1, 2, 5, 3]
    seq, L = _layout(groups), SO.layout(groups)
    F, K, C = L["frames"], 24, 3
    x = _points(F, K, C, K * C, seed=8, pad=0.0)
    clean = seq.smoothness(_dev(x), order, None, 0.05, K=K, C=C)
    g = np.ones(F, f32)
    clean_g = _host(seq.smoothnessBackward(_dev(x), _dev(g), None, order, None, 0.05, K=K, C=C))
    bad = x.copy()
    bad[5] = np.nan  # the third frame of the problem of 5 (frames 3 .. 7)
    r = seq.smoothness(_dev(bad), order, None, 0.05, K=K, C=C)
    touched = [4, 5] if order == 1 else [4, 5, 6]
    fe = _host(r["frame_energy"])
    assert np.isnan(fe[touched]).all() and _same(np.delete(fe, touched), np.delete(_host(clean["frame_energy"]), touched))
    gx = _host(seq.smoothnessBackward(_dev(bad), _dev(g), None, order, None, 0.05, K=K, C=C))
    assert _same(gx[:3], clean_g[:3]) and _same(gx[8:], clean_g[8:]) and np.isnan(gx[3:8]).any()
    pv = _host(seq.sum(r["frame_energy"]))
    assert np.isnan(pv[2]) and not np.isnan(np.delete(pv, 2)).any()
    # a zero weight keeps the NaN of a point out; an exactly-zero cotangent keeps a NaN stencil out
    w = np.ones(K, f32)
    w[7] = 0.0
    part = x.copy()
    part[5, 7 * C:8 * C] = np.nan
    r = seq.smoothness(_dev(part), order, _dev(w), 0.0, K=K, C=C)
    assert not np.isnan(_host(r["frame_energy"])).any() and (_host(r["point_energy"])[:, 7] == 0).all()
    assert not np.isnan(_host(seq.smoothnessBackward(_dev(part), _dev(g), None, order, _dev(w), 0.0, K=K, C=C))).any()
    g0 = g.copy()
    g0[touched] = 0.0
    gx = _host(seq.smoothnessBackward(_dev(bad), _dev(g0), None, order, None, 0.0, K=K, C=C))
    want = SO.smoothness_vjp(L, bad, K, C, order, None, 0.0, g0, None, np.zeros_like(bad), 0)
    assert _same(gx, want) and not np.isnan(gx).any()  # (frame 5 itself included: every stencil on it is off)
    # problems too short for the order: +0 energies and gradients, even on NaN data
    short = [1, 2] if order == 2 else [1, 1]
    seq2 = _layout(short)
    nanx = np.full((sum(short), K * C), np.nan, f32)
    if order == 1:
        r = seq2.smoothness(_dev(nanx), 1, None, 0.0, K=K, C=C)
        gx = _host(seq2.smoothnessBackward(_dev(nanx), _dev(np.ones(2, f32)), None, 1, None, 0.0, K=K, C=C))
    else:
        r = seq2.smoothness(_dev(nanx), 2, None, 0.0, K=K, C=C)
        gx = _host(seq2.smoothnessBackward(_dev(nanx), _dev(np.ones(3, f32)), None, 2, None, 0.0, K=K, C=C))
    for a in (_host(r["frame_energy"]), _host(r["point_energy"]), gx):
        assert (a == 0).all() and not np.signbit(a).any()


# ---------------------------------------------------------------------------------------------------- 4. gradients
def _bar(got, want64, fp32, what):
    import test_pose_prior_gpu as TP

    TP._bar(got, want64, fp32, what)


@pytest.mark.parametrize("order,rho", [(1, 0.0), (2, 0.0), (1, 0.3), (2, 0.3)])
def test_gradient_alone(order, rho):
    """x -> smoothness_differentiable -> sum_differentiable -> a weighted sum of the problems' values, against float64 autograd."""
    groups = [1, 2, 3, 7]
    seq, L = _layout(groups), SO.layout(groups)
    F, K, C = L["frames"], 24, 3
    x = _points(F, K, C, K * C, seed=order, pad=0.0).reshape(F, K, C)
    w, c = _weights(K, 9), np.array([0.5, -1.0, 2.0, 1.5], f32)
    X = _dev(x).requires_grad_(True)
    val = seq.sum_differentiable(seq.smoothness_differentiable(X, order, w, rho), 10.0)
    (val * _dev(c)).sum().backward()

    def ref(dtype):
        Xr = torch.tensor(x, dtype=dtype, requires_grad=True)
        fe = SO.energy_t(L, Xr, order, w, rho).sum(1)
        pv = torch.stack([10.0 * fe[int(a):int(b)].sum() for a, b in zip(L["frame_start"][:-1], L["frame_start"][1:])])
        (pv * torch.tensor(c, dtype=dtype)).sum().backward()
        return pv.detach().double().numpy(), Xr.grad.double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert np.allclose(_host(val.detach()), r64[0], rtol=1e-4, atol=1e-7)
    _bar(X.grad, r64[1], r32[1], "smoothness alone, order %d, rho %g" % (order, rho))


def test_gradient_with_fk_and_shared_beta(synth_model):
    """buf [12,75] -> split_differentiable -> FK on the synthetic model (10 frames) -> velocity of the joints + acceleration of the
    rotations in theta + |beta|^2 -> sum_differentiable, in one graph, against float64 autograd of the restated graph.  The gradient of
    the shared rows is the sum over each problem's frames."""
    from smplpp_amd.smpl import SMPL

    groups, shared = [7, 5], 1
    seq, L = _layout(groups, shared), SO.layout(groups, shared)
    F = L["frames"]
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    rng = np.random.default_rng(12)
    buf = np.zeros((12, 75), f32)
    buf[:, 3:] = rng.normal(0, 0.2, (12, 72))
    buf[6, :10], buf[11, :10] = rng.normal(0, 1.0, 10), rng.normal(0, 1.0, 10)
    buf[6, 10:], buf[11, 10:] = 0, 0
    c = np.array([1.0, 0.5], f32)
    B = _dev(buf).requires_grad_(True)
    theta, beta = seq.split_differentiable(B, 0, 75, 10)
    verts, joints = s.forward_differentiable(beta, theta.reshape(F, 25, 3))
    frames = 10.0 * seq.smoothness_differentiable(joints, 1) + 0.1 * seq.smoothness_differentiable(theta, 2, K=24, C=3, offset=3) + \
        0.01 * beta.pow(2).sum(1)
    val = seq.sum_differentiable(frames)
    (val * _dev(c)).sum().backward()

    def ref(dtype):
        m = FK.model_tensors(synth_model, dtype)
        Br = torch.tensor(buf, dtype=dtype, requires_grad=True)
        th = torch.cat([Br[0:6], Br[7:11]]).reshape(F, 25, 3)
        be = torch.cat([Br[6, :10].expand(6, 10), Br[11, :10].expand(4, 10)])
        j = FK.fk(m, be, th)["joints"]
        fr = 10.0 * SO.energy_t(L, j, 1, None, 0.0).sum(1) + 0.1 * SO.energy_t(L, th[:, 1:], 2, None, 0.0).sum(1) + 0.01 * be.pow(2).sum(1)
        pv = torch.stack([fr[:6].sum(), fr[6:].sum()])
        (pv * torch.tensor(c, dtype=dtype)).sum().backward()
        return pv.detach().double().numpy(), Br.grad.double().numpy()

    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert np.allclose(_host(val.detach()), r64[0], rtol=1e-4)
    g = _host(B.grad)
    assert (g[6, 10:] == 0).all() and (g[11, 10:] == 0).all() and np.abs(g[6, :10]).min() > 0
    _bar(g, r64[1], r32[1], "FK graph, the whole buffer")
    _bar(g[[6, 11], :10], r64[1][[6, 11], :10], r32[1][[6, 11], :10], "FK graph, the shared rows")
    _bar(g[:6], r64[1][:6], r32[1][:6], "FK graph, theta of the first sequence")


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals():
    from smplpp_amd import _lib
    from smplpp_amd.sequence import SequenceLayout

    Lb = _lib.load()
    import ctypes as C

    def create(P, start, shared):
        h = C.c_void_p(123)
        arr = None if start is None else (C.c_int64 * len(start))(*start)
        rc = Lb.smplpp_sequence_create(0, P, arr, shared, C.byref(h))
        assert (rc == 0) == bool(h.value)
        if rc == 0:
            Lb.smplpp_sequence_destroy(h)
        return rc, Lb.smplpp_last_error().decode()

    assert create(2, [0, 3, 5], 1)[0] == 0
    for args, why in (((0, [0], 0), "P must be positive"), ((-1, [0], 0), "P must be positive"), ((2, None, 0), "row_start is NULL"),
                      ((2, [1, 2, 3], 0), "row_start[0] must be 0"), ((2, [0, 2, 2], 0), "strictly increase"), ((1, [0, 4], 2), "shared_rows"),
                      ((1, [0, 4], -1), "shared_rows"), ((2, [0, 1, 3], 1), "no frame"), ((1, [0, 2 ** 31], 0), "int32")):
        rc, msg = create(*args)
        assert rc == 1 and why in msg, (args, msg)
    with pytest.raises(_lib.SmplppError):
        SequenceLayout("cuda:0", [2.5, 1])

    seq, plain = _layout([4, 3], 1), _layout([4, 3], 0)
    F, n, K, C_ = seq.frames, seq.rows, 4, 3
    dev = lambda *shape: torch.full(shape, FILL, device="cuda")  # noqa: E731
    x, rows = dev(F, K * C_), dev(n, 16)
    outs = dict(fe=dev(F), pe=dev(F, K), gx=dev(F, K * C_), frames=dev(F, 6), shared=dev(F, 4), gr=dev(n, 16), pv=dev(2))
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    w_bad = np.array([1.0, -1.0, 1.0, 1.0], f32)
    w_inf = np.array([1.0, np.inf, 1.0, 1.0], f32)
    xh = np.zeros((F, K * C_), f32)
    feh = np.full(F, FILL, f32)
    D, H = _lib.DEVICE, _lib.HOST

    def smooth(seq_=seq, x_=x, ld=K * C_, K_=K, C__=C_, order=1, w=None, rho=0.0, fe=outs["fe"], pe=outs["pe"], space=D):
        return Lb.smplpp_sequence_smoothness(seq_.handle if seq_ else None, P(x_), ld, K_, C__, order, P(w), rho, P(fe), P(pe), space, None)

    def vjp(x_=x, ld=K * C_, K_=K, C__=C_, order=1, rho=0.0, gfe=outs["fe"], gpe=None, gx=outs["gx"], acc=0, space=D):
        return Lb.smplpp_sequence_smoothness_vjp(seq.handle, P(x_), ld, K_, C__, order, None, rho, P(gfe), P(gpe), P(gx), acc, space, None)

    def split(seq_=seq, rows_=rows, ld=16, off=2, Cf=6, frames=outs["frames"], Cs=4, shared=outs["shared"], space=D):
        return Lb.smplpp_sequence_split(seq_.handle, P(rows_), ld, off, Cf, P(frames), Cs, P(shared), space, None)

    def merge(seq_=seq, gf=outs["frames"], off=2, Cf=6, gs=outs["shared"], Cs=4, gr=outs["gr"], ld=16, D_=12, acc=0, space=D):
        return Lb.smplpp_sequence_merge(seq_.handle, P(gf), off, Cf, P(gs), Cs, P(gr), ld, D_, acc, space, None)

    def total(seq_=seq, fv=outs["fe"], pv=outs["pv"], acc=0, space=D):
        return Lb.smplpp_sequence_sum(seq_.handle if seq_ else None, P(fv), 1.0, P(pv), acc, space, None)

    refused = [
        smooth(seq_=None), smooth(x_=None), smooth(K_=0), smooth(K_=-1), smooth(C__=0), smooth(C__=17, ld=17 * K), smooth(ld=K * C_ - 1), smooth(order=0),
        smooth(order=3), smooth(rho=-0.5), smooth(rho=float("inf")), smooth(rho=float("nan")), smooth(fe=None, pe=None), smooth(space=2),
        smooth(ld=2 ** 31),
        Lb.smplpp_sequence_smoothness(seq.handle, xh.ctypes.data, K * C_, K, C_, 1, w_bad.ctypes.data, 0.0, feh.ctypes.data, None, H, None),
        Lb.smplpp_sequence_smoothness(seq.handle, xh.ctypes.data, K * C_, K, C_, 1, w_inf.ctypes.data, 0.0, feh.ctypes.data, None, H, None),
        vjp(x_=None), vjp(K_=0), vjp(C__=17, ld=17 * K), vjp(ld=K * C_ - 1), vjp(order=3), vjp(rho=-1.0), vjp(gfe=None, gpe=None), vjp(gx=None), vjp(acc=2),
        vjp(acc=-1), vjp(space=7),
        split(rows_=None), split(frames=None, shared=None), split(ld=0), split(off=-1), split(Cf=0), split(off=11, Cf=6), split(Cs=0), split(Cs=17),
        split(seq_=plain), split(space=2), split(ld=2 ** 31),
        merge(gf=None, gs=None), merge(gr=None), merge(D_=0), merge(D_=17), merge(off=-1), merge(Cf=0), merge(off=7, Cf=6), merge(Cs=13), merge(Cs=0),
        merge(seq_=plain), merge(acc=2), merge(space=2), merge(D_=7), merge(D_=3, gf=None),
        total(seq_=None), total(fv=None), total(pv=None), total(acc=2), total(acc=-1), total(space=2),
    ]
    torch.cuda.synchronize()
    assert all(rc == 1 for rc in refused), refused
    assert "smplpp_sequence_sum" in Lb.smplpp_last_error().decode()
    for k, t in outs.items():
        assert (t == FILL).all(), k
    assert (feh == FILL).all()
    # and the same calls go through once the argument is put right
    assert smooth() == 0 and vjp() == 0 and split() == 0 and merge() == 0 and total() == 0
    wide = dev(plain.frames, 6)  # (a layout without shared rows has 7 frames here)
    assert split(seq_=plain, frames=wide, shared=None) == 0 and merge(seq_=plain, gf=wide, gs=None) == 0  # ... and serves the frame side
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 6. C++ shim
def test_sequence_cpp_shim(tmp_path):
    exe = str(tmp_path / "sequence_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sequence_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    groups, n, D, K, C = [4, 3], 7, 8, 2, 3
    L = SO.layout(groups, 1)
    F, P = L["frames"], L["P"]
    i = np.arange(n * D)
    rows = (((i * 7) % 11 - 5).astype(f32) * f32(0.125) + (i // D).astype(f32) * f32(0.0625)).astype(f32).reshape(n, D)
    frames, shared = SO.split(L, rows, 2, K * C, 3)
    w = np.array([0.5, 2.0], f32)
    f, k = np.arange(F, dtype=f32), np.arange(K, dtype=f32)
    gfe = (f32(1) + f32(0.25) * f).astype(f32)
    gpe = (f32(0.5) - f32(0.125) * (f[:, None] + k[None])).astype(f32)
    want = [L["frame_start"].astype(f32), frames, shared]
    for order in (1, 2):
        rho = 0.0 if order == 1 else 0.75
        want += list(SO.smoothness(L, frames, K, C, order, w, rho))
        grad = SO.smoothness_vjp(L, frames, K, C, order, w, rho, gfe, gpe, np.zeros((F, K * C), f32), 0)
        want.append(grad)
    merged = SO.merge(L, grad, 2, K * C, shared, 3, np.zeros((n, D), f32), D, 0)
    want += [merged, SO.merge(L, grad, 2, K * C, shared, 3, merged.copy(), D, 1)]
    pv = SO.seq_sum(L, gfe, 0.5, np.zeros(P, f32), 0)
    want += [pv, SO.seq_sum(L, gfe, 3.0, pv.copy(), 1)]
    raw = open(outp, "rb").read()
    assert len(raw) == 4 * sum(a.size for a in want)
    off = 0
    for j, a in enumerate(want):
        got = np.frombuffer(raw, f32, a.size, off).reshape(a.shape)
        off += 4 * a.size
        assert _same(got, np.ascontiguousarray(a)), j


# ---------------------------------------------------------------------------------------------------- 7. the sequence fit
def test_sequence_fit_with_native_glue(synth_model):
    """The two-sequence fit of test_lbfgs_groups_gpu (T = 6 and 4, shared beta, velocity weight 10 on the joints, 123 evaluations) with
    seq_layout's cat / expand, the velocity term and the per-problem sums replaced by split_differentiable, smoothness_differentiable
    (order 1, K = 24, C = 3) and sum_differentiable, under that test's criterion: against the float64 run of the same budget, energies
    within 2x + 1e-6, landmark error and |beta - beta_true| within 2x.  At the starting point and at a random point its energies agree
    with the torch-glue evaluation to fp32 rounding: both evaluations sum the same non-negative terms in different orders, the 72 squares of
    a velocity pair and at most 8 further terms per problem; any order of summing m non-negative fp32 terms is within (m - 1) u of the exact
    sum, so each side is within 80 u and the two within 160 u of each other: the bar is 256 u."""
    import test_lbfgs_groups_gpu as TG
    import test_pose_prior_gpu as TP
    from smplpp_amd import smpl as S
    from smplpp_amd.landmarks import Landmarks
    from smplpp_amd.optim import BatchedLBFGS
    from smplpp_amd.priors import PosePrior
    from smplpp_amd.sequence import SequenceLayout
    from smplpp_amd.smpl import SMPL

    fs = TG.seq_setup(synth_model)
    n, B = fs["n"], TG.SEQ_BUDGET
    x64, f64 = TG.seq_float64(fs["energies64"], B)
    with torch.no_grad():
        _, pts64, shared64 = fs["energies64"](torch.tensor(x64))
    err64, beta64 = TG.seq_errors(pts64, shared64, fs)

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    lm = Landmarks(s, *fs["reg"])
    p = fs["prior"]
    prior = PosePrior("cuda:0", p["mean"], p["mat"], p["offset"])
    dev = torch.device("cuda:0")
    cam32, target32 = torch.from_numpy(fs["cam"]).to(dev), fs["target64"].float().to(dev)
    buf = torch.zeros(sum(TG.SEQ_GROUPS), 75, device=dev, requires_grad=True)
    opt = BatchedLBFGS(buf, history=10, groups=TG.SEQ_GROUPS)
    seq = SequenceLayout.from_optimizer(opt, shared_rows=1)
    assert seq.frames == n and seq.frame_start.tolist() == [0, TG.SEQ_T[0], n]
    keep = [None, None]

    def frame_terms(theta, beta):
        verts, joints = s.forward_differentiable(beta, theta)
        pts = lm.forward_differentiable(verts, joints)
        _, e, _ = S.project_points_differentiable(pts, cam32, target32, TP.FIT_RHO, TP.NEAR)
        return e.mean(1) + TP.FIT_PRIOR * prior.forward_differentiable(theta)[0], joints, pts

    def closure():
        theta, beta = seq.split_differentiable(buf, 0, 75, 10)
        theta = theta.reshape(n, 25, 3)
        frames, joints, pts = frame_terms(theta, beta)
        shared = torch.stack([beta[0], beta[n - 1]])  # (the ridge on the shared rows stays in torch: it is no sequence term)
        keep[:] = pts, shared
        return seq.sum_differentiable(frames + TG.SEQ_VELOCITY * seq.smoothness_differentiable(joints, 1)) + TG.SEQ_BETA * shared.pow(2).sum(1)

    def glue():
        theta, beta, shared = TG.seq_layout(buf)
        frames, joints, _ = frame_terms(theta, beta)
        return TG.seq_energy(frames, joints, shared)

    def agree():
        with torch.no_grad():
            a, b = closure().cpu().numpy(), glue().cpu().numpy()
        print("native glue %s, torch glue %s" % (a, b))
        assert (a > 0).all() and np.allclose(a, b, rtol=256 * U, atol=0)

    agree()
    with torch.no_grad():
        buf.copy_(torch.from_numpy(np.random.default_rng(5).normal(0, 0.1, (12, 75)).astype(f32)))
    agree()
    with torch.no_grad():
        buf.zero_()
    trail = []
    for _ in range(B):
        opt.step(closure)
        trail.append(buf.detach().clone())
    st = {k: _host(v) for k, v in opt.run(closure, 0).items()}
    with torch.no_grad():
        e32 = closure().cpu().numpy()
    err32, beta32 = TG.seq_errors(keep[0].detach(), keep[1].detach(), fs)
    trail = torch.stack(trail).cpu().numpy()
    print("float64: %s, landmark error %s mm, |beta - beta_true| %s" % (f64, err64, beta64))
    print("MI355X, native glue: %s, landmark error %s mm, |beta - beta_true| %s, status %s, iterations %s" % (e32, err32, beta32, st["status"], st["iterations"]))
    assert (st["evaluations"] == B).all() and np.allclose(e32, st["f_best"], rtol=1e-5)
    assert (trail[:, 6, 10:] == 0).all() and (trail[:, 11, 10:] == 0).all()  # merge hands the unused coordinates of the beta rows +0
    assert (e32 <= 2 * f64 + 1e-6).all(), (e32, f64)
    assert (err32 <= 2 * err64).all(), (err32, err64)
    assert (beta32 <= 2 * beta64).all(), (beta32, beta64)
