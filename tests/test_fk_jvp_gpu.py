"""smplpp_fk_jvp / smplpp_fk_rotmat_jvp on the MI355X: every (frame, tangent) block against float64 forward-mode autograd of the torch
restatements (tests/fk_jvp_oracle.py), adjointness against the shipped backward passes, the bits of a column alone and inside a
batch, the two entries against each other, call semantics, SMPL+D, torch.autograd.forward_ad, a Levenberg-Marquardt fit on dense
Jacobians and the C++ shim."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_jvp_oracle as JO  # noqa: E402
import vjp_blocks as VB  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("verts", "joints", "world")
# (n, T, shared): n T columns on both sides of the 32-column tile of jvp_skin_kernel, and the full one-hot basis
CASES = [(1, 1, False), (3, 5, False), (3, 33, False), (33, 1, False), (2, 85, True)]
_smpls = {}


def smpl_of(which):
    from smplpp_amd.smpl import SMPL

    if which not in _smpls:
        s = SMPL()
        s.setDevice("cuda:0")
        s.init(VB.model(which))
        _smpls[which] = (s, JO.model_tensors(VB.model(which)))
    return _smpls[which]


def _tangents(n, T, shared, seed):
    """(dbeta, dtheta, dtrans, drot) fp32: N(0,1), or (T = 85, shared) the one-hot basis, beta first, then theta row-major."""
    lead = (T,) if shared else (n, T)
    rng = np.random.default_rng(seed)
    f32 = lambda *s: rng.standard_normal(lead + s).astype(np.float32)
    db, dth, dtr, dr = f32(10), f32(25, 3), f32(3), f32(24, 3, 3)
    if shared and T == 85:
        eye = np.eye(85, dtype=np.float32)
        db, dth = np.ascontiguousarray(eye[:, :10]), np.ascontiguousarray(eye[:, 10:]).reshape(85, 25, 3)
    return db, dth, dtr, dr


def _general_rot(theta, seed):
    R = JO.RO.rodrigues_np(theta[:, 1:])
    return (R + 0.05 * np.random.default_rng(seed).standard_normal(R.shape)).astype(np.float32)


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-30)


def check_blocks(got, ref64, ref32, what):
    """Every (frame, tangent) block of every output: finite, and within max(4 x the float32 forward mode's error, 1e-5) of float64 in
    relative L2."""
    worst = 0.0
    for k in got:
        n, T = got[k].shape[:2]
        assert got[k].shape == ref64[k].shape, (what, k, got[k].shape, ref64[k].shape)
        for f in range(n):
            for t in range(T):
                g = got[k][f, t]
                assert np.isfinite(g).all(), (what, k, f, t)
                bar = max(4 * _rel(ref32[k][f, t], ref64[k][f, t]), 1e-5)
                err = _rel(g.astype(np.float64), ref64[k][f, t])
                worst = max(worst, err / bar)
                assert err <= bar, (what, k, f, t, err, bar)
    print(what, "worst error / bar: %.3g" % worst)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-T%d%s" % (c[0], c[1], "-shared" if c[2] else ""))
@pytest.mark.parametrize("entry", ["axis_angle", "rotmat"])
@pytest.mark.parametrize("which", VB.MODELS)
def test_jvp_parity_per_block(which, entry, case):
    s, m64 = smpl_of(which)
    n, T, shared = case
    beta, theta = VB.dense_inputs(n, seed=10 * n + T)
    db, dth, dtr, dr = _tangents(n, T, shared, seed=n + T)
    if entry == "axis_angle":
        got = s.launchTangent(beta, theta, db, dth, shared=shared)
        ref = [JO.tangent(m64, beta, theta, db, dth, shared=shared, dtype=dt) for dt in (JO.torch.float64, JO.torch.float32)]
    else:
        rot, trans = _general_rot(theta, seed=n + 7), np.ascontiguousarray(theta[:, 0])
        if shared and T == 85:  # the one-hot basis of (beta, trans, the first 72 entries of rot)
            eye = np.eye(85, dtype=np.float32)
            dtr, dr = np.ascontiguousarray(eye[:, 10:13]), np.zeros((85, 216), np.float32)
            dr[:, :72] = eye[:, 13:]
            dr = dr.reshape(85, 24, 3, 3)
        got = s.launchRotmatTangent(beta, trans, rot, db, dtr, dr, shared=shared)
        ref = [JO.tangent_rotmat(m64, beta, trans, rot, db, dtr, dr, shared=shared, dtype=dt) for dt in (JO.torch.float64, JO.torch.float32)]
    assert set(got) == set(KEYS)
    check_blocks(got, ref[0], ref[1], "%s %s %s" % (which, entry, case))


def _dot(a, b):
    return float((np.asarray(a, np.float64) * np.asarray(b, np.float64)).sum())


def _norm(*xs):
    return float(np.sqrt(sum((np.asarray(x, np.float64) ** 2).sum() for x in xs)))


@pytest.mark.parametrize("which", VB.MODELS)
def test_jvp_is_the_adjoint_of_the_shipped_vjps(which):
    s, _ = smpl_of(which)
    n, T, V = 3, 2, s.vertex_num
    beta, theta = VB.dense_inputs(n, seed=41)
    db, dth, dtr, dr = _tangents(n, T, False, seed=42)
    rng = np.random.default_rng(43)
    gv, gj = rng.standard_normal((n, V, 3)).astype(np.float32), rng.standard_normal((n, 24, 3)).astype(np.float32)
    gw = rng.standard_normal((n, 24, 3, 4)).astype(np.float32)
    rot, trans = _general_rot(theta, seed=44), np.ascontiguousarray(theta[:, 0])
    Jv = s.launchTangent(beta, theta, db, dth)
    Jg = s.launchBackward(beta, theta, grad_verts=gv, grad_joints=gj)
    Sg = s.skeletonBackward(beta, theta, grad_world=gw, grad_joints=gj)
    Rv = s.launchRotmatTangent(beta, trans, rot, db, dtr, dr)
    Rg = s.launchRotmatBackward(beta, trans, rot, grad_verts=gv, grad_joints=gj)
    for f in range(n):
        for t in range(T):
            pairs = (
                ("fk", [(gv[f], Jv["verts"][f, t]), (gj[f], Jv["joints"][f, t])], [(Jg["beta"][f], db[f, t]), (Jg["theta"][f], dth[f, t])]),
                ("skeleton", [(gw[f], Jv["world"][f, t]), (gj[f], Jv["joints"][f, t])], [(Sg["beta"][f], db[f, t]), (Sg["theta"][f], dth[f, t])]),
                ("rotmat", [(gv[f], Rv["verts"][f, t]), (gj[f], Rv["joints"][f, t])],
                 [(Rg["beta"][f], db[f, t]), (Rg["trans"][f], dtr[f, t]), (Rg["rot"][f], dr[f, t])]),
            )
            for name, out_side, in_side in pairs:
                lhs, rhs = sum(_dot(g, x) for g, x in out_side), sum(_dot(g, x) for g, x in in_side)
                bound = 1e-5 * (_norm(*[g for g, _ in out_side]) * _norm(*[x for _, x in out_side]) +
                                _norm(*[g for g, _ in in_side]) * _norm(*[x for _, x in in_side]))
                assert abs(lhs - rhs) <= bound, (which, name, f, t, lhs, rhs, bound)


@pytest.mark.parametrize("which", ["synth", "tiny"])
def test_jvp_bits_of_a_column_alone_and_in_a_batch(which):
    import torch

    s, _ = smpl_of(which)
    n, T = 7, 5
    beta, theta = VB.dense_inputs(n, seed=51)
    db, dth, _, _ = _tangents(n, T, False, seed=52)
    full = s.launchTangent(beta, theta, db, dth)
    again = s.launchTangent(beta, theta, db, dth)
    for k in KEYS:
        assert np.array_equal(full[k], again[k]), k  # deterministic
    slots = [(f, t) for f in range(n) for t in range(T)] if which == "tiny" else [(0, 0), (2, 3), (4, 1), (6, 4)]
    for f, t in slots:
        one = s.launchTangent(beta[f:f + 1], theta[f:f + 1], db[f:f + 1, t:t + 1], dth[f:f + 1, t:t + 1])
        for k in KEYS:
            assert np.array_equal(one[k][0, 0], full[k][f, t]), (k, f, t)
    # shared tangents against the same tangents repeated per frame
    sh = s.launchTangent(beta, theta, db[3], dth[3], shared=True)
    pf = s.launchTangent(beta, theta, np.repeat(db[3:4], n, 0), np.repeat(dth[3:4], n, 0))
    for k in KEYS:
        assert np.array_equal(sh[k], pf[k]), k
        assert np.array_equal(sh[k][3], full[k][3]), k
    # device space against host space
    dev = lambda a: torch.from_numpy(a).cuda()
    d = s.launchTangent(dev(beta), dev(theta), dev(db), dev(dth))
    torch.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(d[k].cpu().numpy(), full[k]), k
    # subsets of the outputs; without the vertices the call is the chain kernel alone
    for want in (("verts",), ("joints", "world"), ("world",), ("verts", "joints")):
        sub = s.launchTangent(beta, theta, db, dth, want=want)
        assert set(sub) == set(want)
        for k in want:
            assert np.array_equal(sub[k], full[k]), (want, k)
    # rest passed against rest recomputed (the default form)
    rest = s.launch(beta, theta, want=("rest",))["rest"]
    assert np.array_equal(s.launchTangent(beta, theta, db, dth, rest=rest, want=("verts",))["verts"], full["verts"])
    # only one of the two tangents: the other reads as zero
    only = s.launchTangent(beta, theta, dtheta=dth, want=("verts", "joints"))
    zero = s.launchTangent(beta, theta, np.zeros_like(db), dth, want=("verts", "joints"))
    assert np.array_equal(only["verts"], zero["verts"]) and not only["joints"].any()


@pytest.mark.parametrize("which", VB.MODELS)
def test_jvp_rotmat_entry_is_consistent_with_the_axis_angle_entry(which):
    s, m64 = smpl_of(which)
    n, T = 3, 4
    beta, theta = VB.dense_inputs(n, seed=61)
    db, dth, _, _ = _tangents(n, T, False, seed=62)
    rot, trans = s.axisAngleToRotmat(theta[:, 1:]), np.ascontiguousarray(theta[:, 0])
    drot = JO.rodrigues_tangent(np.repeat(theta[:, None, 1:], T, 1), dth[:, :, 1:]).astype(np.float32)
    got = s.launchRotmatTangent(beta, trans, rot, db, np.ascontiguousarray(dth[:, :, 0]), drot)
    ref = [JO.tangent(m64, beta, theta, db, dth, dtype=dt) for dt in (JO.torch.float64, JO.torch.float32)]
    check_blocks(got, ref[0], ref[1], "%s rotmat entry on the axis-angle tangent" % which)
    # a shape tangent alone: nothing differs between the entries, to the bit
    a = s.launchTangent(beta, theta, dbeta=db)
    for dr in (None, np.zeros((n, T, 24, 3, 3), np.float32)):
        b = s.launchRotmatTangent(beta, trans, rot, dbeta=db, drot=dr)
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), k


def test_jvp_call_semantics():
    from smplpp_amd import _lib

    s, _ = smpl_of("tiny")
    L, V = _lib.load(), s.vertex_num
    n, T = 3, 2
    beta, theta = VB.dense_inputs(n, seed=71)
    db, dth, dtr, dr = _tangents(n, T, False, seed=72)
    rot = _general_rot(theta, seed=73)
    outs = [np.full((n, T, V, 3), 7.0, np.float32), np.full((n, T, 24, 3), 7.0, np.float32), np.full((n, T, 24, 3, 4), 7.0, np.float32)]
    P = lambda a: None if a is None else a.ctypes.data
    o = [P(a) for a in outs]

    def fk(n_=n, T_=T, b=beta, th=theta, d0=db, d1=dth, sh=0, out=o):
        return L.smplpp_fk_jvp(s.handle, n_, T_, P(b), P(th), None, P(d0), P(d1), sh, out[0], out[1], out[2], _lib.HOST, None)

    def rm(r=rot, d0=db, d1=dtr, d2=dr, sh=0, out=o, n_=n, T_=T):
        return L.smplpp_fk_rotmat_jvp(s.handle, n_, T_, P(beta), None, P(r), None, P(d0), P(d1), P(d2), sh, out[0], out[1], out[2], _lib.HOST, None)

    bad = [fk(n_=0), fk(n_=-1), fk(T_=0), fk(b=None), fk(th=None), fk(d0=None, d1=None), fk(out=[None] * 3), fk(sh=2), fk(sh=-1),
           rm(r=None), rm(d0=None, d1=None, d2=None), rm(out=[None] * 3), rm(sh=2), rm(n_=0), rm(T_=0)]
    assert all(rc == 1 for rc in bad), bad  # SMPLPP_ERR_INVALID
    assert all((a == 7.0).all() for a in outs)
    assert fk() == _lib.OK and all(np.isfinite(a).all() for a in outs)
    clean = s.launchTangent(beta, theta, db, dth)
    for a, k in zip(outs, KEYS):
        assert np.array_equal(a, clean[k]), k
    # a frame of NaNs, then a tangent of NaNs: the other columns keep their bits
    th2 = theta.copy()
    th2[1] = np.nan
    nanf = s.launchTangent(beta, th2, db, dth)
    d2 = dth.copy()
    d2[0, 1] = np.nan
    nant = s.launchTangent(beta, theta, db, d2)
    for k in KEYS:
        assert np.array_equal(nanf[k][[0, 2]], clean[k][[0, 2]]), k
        assert np.array_equal(nant[k][1:], clean[k][1:]) and np.array_equal(nant[k][0, 0], clean[k][0, 0]), k
    assert np.isnan(nant["verts"][0, 1]).all() and np.isnan(nanf["verts"][1]).all() and np.isnan(nanf["world"][1]).any()
    # the forward after a tangent call (rest recomputed inside it) returns the same bits
    ref_fk = {k: v.copy() for k, v in s.launch(beta, theta).items()}
    s.launchTangent(beta, theta, db, dth)
    again = s.launch(beta, theta)
    for k in ref_fk:
        assert np.array_equal(again[k], ref_fk[k]), k
    # the Python layer refuses what the ABI refuses
    from smplpp_amd._lib import SmplppError

    with pytest.raises(SmplppError):
        s.launchTangent(beta, theta)
    with pytest.raises(SmplppError):
        s.launchTangent(beta, theta, db, dth, want=())
    J = s.jacobian(beta, theta, want=KEYS)
    assert J["verts"].shape == (n, 85, V, 3) and J["world"].shape == (n, 85, 24, 3, 4)
    assert s.jacobian(beta, theta, wrt=("theta",))["verts"].shape == (n, 75, V, 3)
    eye = np.eye(85, dtype=np.float32)
    basis = s.launchTangent(beta, theta, np.ascontiguousarray(eye[:, :10]), np.ascontiguousarray(eye[:, 10:]).reshape(85, 25, 3), shared=True)
    for k in KEYS:
        assert np.array_equal(J[k], basis[k]), k


@pytest.mark.parametrize("which", ["synth", "tiny"])
def test_jvp_of_a_displaced_body(which):
    s, m64 = smpl_of(which)
    n, T = 3, 2
    beta, theta = VB.dense_inputs(n, seed=81)
    db, dth, _, _ = _tangents(n, T, False, seed=82)
    D = (0.01 * np.random.default_rng(83).standard_normal((n, s.vertex_num, 3))).astype(np.float32)
    rd = s.launch(beta, theta, want=("rest",))["rest"] + D
    got = s.launchTangent(beta, theta, db, dth, rest=rd, want=("verts",))
    ref = [JO.tangent(m64, beta, theta, db, dth, dtype=dt, rest=rd) for dt in (JO.torch.float64, JO.torch.float32)]
    check_blocks(got, {"verts": ref[0]["verts"]}, {"verts": ref[1]["verts"]}, "%s SMPL+D" % which)
    plain = s.launchTangent(beta, theta, db, dth, want=("verts",))["verts"]
    assert not np.array_equal(plain, got["verts"])  # the displacement is read


def test_jvp_offsets_past_two_to_the_31():
    """n T V 3 = 1223 x 85 x 6890 x 3 = 2 148 749 850 elements of dverts (8.6 GB): the last columns have the bits of the column alone."""
    import torch

    s, _ = smpl_of("synth")
    n, T, V = 1223, 85, s.vertex_num
    assert n * T * V * 3 > 2 ** 31
    beta, theta = VB.dense_inputs(n, seed=95)
    db, dth, _, _ = _tangents(n, T, True, seed=96)
    dev = lambda a: torch.from_numpy(a).cuda()
    b, t, ddb, ddth = dev(beta), dev(theta), dev(db), dev(dth)
    out = s.launchTangent(b, t, ddb, ddth, shared=True, want=("verts",))["verts"]
    for f, k in ((n - 1, 84), (n - 1, 0), (n - 2, 41), (0, 0), (611, 84)):
        one = s.launchTangent(b[f:f + 1], t[f:f + 1], ddb[k:k + 1], ddth[k:k + 1], shared=True, want=("verts",))["verts"]
        assert torch.equal(out[f, k], one[0, 0]), (f, k)
    assert bool(torch.isfinite(out[-1]).all())
    del out
    torch.cuda.empty_cache()


def test_jvp_forward_ad():
    import torch
    import torch.autograd.forward_ad as fwAD

    s, _ = smpl_of("synth")
    n = 5
    beta, theta = VB.dense_inputs(n, seed=91)
    db, dth, dtr, dr = (torch.from_numpy(a[:, 0].copy()).cuda() for a in _tangents(n, 1, False, seed=92))
    b, t = torch.from_numpy(beta).cuda(), torch.from_numpy(theta).cuda()
    fwd = s.launch(b, t)
    plain = [a.clone() for a in s.forward_differentiable(b, t)]
    ref = s.launchTangent(b, t, db[:, None].contiguous(), dth[:, None].contiguous(), rest=fwd["rest"], want=("verts", "joints"))
    with fwAD.dual_level():
        verts, joints = s.forward_differentiable(fwAD.make_dual(b, db), fwAD.make_dual(t, dth))
        (pv, tv), (pj, tj) = fwAD.unpack_dual(verts), fwAD.unpack_dual(joints)
        assert torch.equal(tv, ref["verts"][:, 0]) and torch.equal(tj, ref["joints"][:, 0])
        assert torch.equal(pv, plain[0]) and torch.equal(pj, plain[1])
        verts, joints = s.forward_differentiable(b, fwAD.make_dual(t, dth))  # a tangent of None counts as zero
        only = s.launchTangent(b, t, dtheta=dth[:, None].contiguous(), rest=fwd["rest"], want=("verts", "joints"))
        assert torch.equal(fwAD.unpack_dual(verts).tangent, only["verts"][:, 0])
        assert fwAD.unpack_dual(joints).tangent is None or not fwAD.unpack_dual(joints).tangent.any()
    rot = s.axisAngleToRotmat(t[:, 1:].contiguous())
    tr = t[:, 0].contiguous()
    fr = s.launchRotmat(b, tr, rot)
    ref = s.launchRotmatTangent(b, tr, rot, db[:, None].contiguous(), dtr[:, None].contiguous(), dr[:, None].contiguous(), rest=fr["rest"],
                                want=("verts", "joints"))
    with fwAD.dual_level():
        verts, joints, xforms = s.forward_rotmat_differentiable(fwAD.make_dual(b, db), fwAD.make_dual(tr, dtr), fwAD.make_dual(rot, dr))
        assert torch.equal(fwAD.unpack_dual(verts).tangent, ref["verts"][:, 0])
        assert torch.equal(fwAD.unpack_dual(joints).tangent, ref["joints"][:, 0])
        assert fwAD.unpack_dual(xforms).tangent is None
    # reverse mode is what it was: the bits of launchBackward, as without the forward-mode methods
    gv, gj = torch.randn(n, s.vertex_num, 3, device="cuda"), torch.randn(n, 24, 3, device="cuda")
    bq, tq = b.clone().requires_grad_(True), t.clone().requires_grad_(True)
    verts, joints = s.forward_differentiable(bq, tq)
    assert torch.equal(verts, plain[0]) and torch.equal(joints, plain[1])
    gb, gt = torch.autograd.grad((verts * gv).sum() + (joints * gj).sum(), (bq, tq))
    want = s.launchBackward(b, t, grad_verts=gv, grad_joints=gj, rest=fwd["rest"])
    assert torch.equal(gb, want["beta"]) and torch.equal(gt, want["theta"])


def test_jvp_levenberg_marquardt_on_dense_jacobians():
    from test_fk_jvp_cpu import LM_LAST64

    s, _ = smpl_of("synth")
    beta = np.zeros((JO.LM_N, 10), np.float32)
    forward = lambda theta: s.launch(beta, theta, want=("verts",))["verts"]
    jacobian = lambda theta: s.jacobian(beta, theta, wrt=("theta",))["verts"]
    first, last = JO.lm_fit(forward, jacobian, dtype=np.float32)
    print("LM on the device's Jacobians: %.4g -> %.4g (float64 oracle: -> %.4g)" % (first, last, LM_LAST64))
    assert JO.lm_passes(first, last, LM_LAST64), (first, last)


def test_jvp_cpp_shim(tmp_path):
    import __graft_entry__ as g
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    g.build()
    exe = str(tmp_path / "fk_jvp_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fk_jvp_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    model = model_io.tiny_model(40, seed=3)
    path = str(tmp_path / "tiny.json")
    model_io.save_model_json(path, model)
    out = subprocess.run([exe, path], stdout=subprocess.PIPE, text=True, timeout=300)
    assert out.returncode == 0, out.stdout
    vals = {}
    for line in out.stdout.splitlines():
        k, *v = line.split()
        vals[k] = np.array([float(x) for x in v], np.float32)
    # the program's inputs, restated
    n, T = 2, 3
    fill = lambda shape, mod, off, scale: ((np.arange(int(np.prod(shape)), dtype=np.int64) % mod - off).astype(np.float32) *
                                           np.float32(scale)).reshape(shape)
    beta, theta = fill((n, 10), 7, 3, 0.1), fill((n, 25, 3), 11, 5, 0.05)
    dbeta, dtheta = fill((n, T, 10), 5, 2, 0.25), fill((n, T, 25, 3), 13, 6, 0.125)
    sbeta, drot, dtrans = fill((T, 10), 3, 1, 0.5), fill((T, 24, 3, 3), 9, 4, 0.0625), fill((T, 3), 4, 1, 0.5)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(model)
    rest = s.launch(beta, theta, want=("rest",))["rest"]
    a = s.launchTangent(beta, theta, dbeta, dtheta, rest=rest)
    trans, rot = np.ascontiguousarray(theta[:, 0]), s.axisAngleToRotmat(theta[:, 1:])
    rest = s.launchRotmat(beta, trans, rot, want=("rest",))["rest"]
    r = s.launchRotmatTangent(beta, trans, rot, sbeta, dtrans, drot, rest=rest, shared=True)
    for key, ref in (("VERTS", a["verts"]), ("JOINTS", a["joints"]), ("WORLD", a["world"]), ("R_VERTS", r["verts"]), ("R_JOINTS", r["joints"]),
                     ("R_WORLD", r["world"])):
        assert np.array_equal(vals[key], ref.ravel()), key
