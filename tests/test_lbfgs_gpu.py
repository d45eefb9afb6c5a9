"""The batched L-BFGS on the MI355X (smplpp_lbfgs_step and its handle): after every call, x and every output of smplpp_lbfgs_state
against the float32 numpy restatement of tests/lbfgs_oracle.py, bit for bit; independence of batch, slot, space and leading dimension;
a mixed batch with NaN and +inf frames, whose stopped rows are poisoned; the rejection branches; best(), reset(), the refusals, the C++
shim; and a single-view fit against the float64 restatement on the float64 graph.  Energies and gradients of the bit tests are computed
on the host by the float32 numpy functions, so the library and the restatement see identical inputs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoints_oracle as KP  # noqa: E402
import lbfgs_oracle as LO  # noqa: E402
import pose_prior_oracle as PO  # noqa: E402
from distance_cases import _same_bits  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF, LD = 3, 75  # where the coordinates start in a row of a strided buffer, and its rows (rotation and pose in a row of theta)
FILL = 7.0
KEYS = ("status", "iterations", "evaluations", "f_best", "step", "running")


def _host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else a


def _same(a, b):
    """_same_bits where neither is NaN, and NaN in the same places (a NaN's sign and payload are not part of the rule)."""
    a, b = np.ascontiguousarray(_host(a)), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a.dtype == b.dtype and np.array_equal(a, b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and _same_bits(np.where(np.isnan(a), np.float32(0), a), np.where(np.isnan(b), np.float32(0), b))


class Driver:
    """A BatchedLBFGS on x0 [n,D] in host or device space, in rows of D floats or at offset OFF inside rows of LD floats, fed by the
    float32 numpy functions: only running frames are evaluated, the rows of the others keep what they held."""

    def __init__(self, funcs, x0, m, dev, strided=False, **options):
        from smplpp_amd.optim import BatchedLBFGS

        n, D = x0.shape
        self.funcs, self.n, self.D, self.dev = funcs, n, D, dev
        buf = np.full((n, LD), FILL, np.float32) if strided else np.empty((n, D), np.float32)
        gbuf = np.full((n, LD), FILL, np.float32) if strided else np.zeros((n, D), np.float32)
        cut = (slice(None), slice(OFF, OFF + D)) if strided else (slice(None), slice(None))
        buf[cut] = x0
        self.buf, self.gbuf = (torch.from_numpy(buf).cuda(), torch.from_numpy(gbuf).cuda()) if dev else (buf, gbuf)
        self.x, self.g = self.buf[cut], self.gbuf[cut]
        self.f = torch.zeros(n).cuda() if dev else np.zeros(n, np.float32)
        self.opt = BatchedLBFGS(self.x, history=m, **options)
        self.status = np.zeros(n, np.int32)

    def points(self):
        return np.array(_host(self.x), np.float32)

    def call(self, poison=False):
        """One evaluation and one step; returns (x [n,D], state) on the host.  poison: rows of stopped frames get NaN energies and
        gradients and the sentinel FILL in x beforehand."""
        x = self.points()
        f, g = np.array(_host(self.f)), np.array(_host(self.g))
        for i in range(self.n):
            if self.status[i] == 0:
                f[i], g[i] = self.funcs[i](x[i])
            elif poison:
                f[i], g[i], x[i] = np.nan, np.nan, FILL
        if self.dev:
            self.f.copy_(torch.from_numpy(f))
            self.g.copy_(torch.from_numpy(g))
            if poison:
                self.x.copy_(torch.from_numpy(x))
        else:
            self.f[:], self.g[:] = f, g
            if poison:
                self.x[:] = x
        self.opt.step_with(self.f, self.g)
        st = {k: np.array(_host(v)) for k, v in self.opt.state().items()}
        self.status = st["status"]
        return self.points(), st

    def margins_untouched(self):
        """The floats outside the D coordinates of a strided buffer."""
        return all((np.delete(_host(b), np.s_[OFF:OFF + self.D], axis=1) == FILL).all() for b in (self.buf, self.gbuf))


def reference(funcs, x0, m, calls, **options):
    """[(x, state)] after each call of the float32 restatement, and the restatement itself."""
    opt = LO.LBFGS(len(funcs), x0.shape[1], m, np.float32, **options)
    x, trail = x0.copy(), []
    LO.run(opt, funcs, x, calls, after=lambda call: trail.append((x.copy(), opt.state())))
    return trail, opt


def agrees(got, want, rows=None):
    """(x, state) of one call against the restatement's, for all frames or for the restatement's rows `rows`."""
    (xg, sg), (xw, sw) = got, want
    rows = slice(None) if rows is None else rows
    ok = _same(xg, xw[rows]) and all(_same(sg[k], sw[k][rows]) for k in KEYS[:-1])
    return ok and (rows != slice(None) or sg["running"][0] == sw["running"][0])


# ---------------------------------------------------------------------------------------------------- 1. bits
CASES = [(1, 1, 1), (2, 3, 3), (63, 3, 3), (64, 10, 65), (65, 1, 3), (72, 10, 65), (128, 32, 3), (129, 3, 1), (300, 10, 3), (20670, 3, 2)]


def case_functions(D, n):
    """Frame k: a quadratic of condition 1000 (even k; below D = 8, where a quadratic ends in a few exact steps, the soft absolute value
    of condition 30 from further away) or the chained Rosenbrock function from its usual start (odd k, D >= 2)."""
    rng = np.random.default_rng(1000 * D + n)
    funcs, x0 = [], np.zeros((n, D), np.float32)
    for k in range(n):
        if k % 2 and D >= 2:
            funcs.append(LO.Rosenbrock())
            x0[k] = LO.Rosenbrock.start(D, np.float32) + rng.normal(0, 0.05, D).astype(np.float32)
        else:
            funcs.append(LO.Quadratic(D, 1000.0, seed=100 * D + k) if D >= 8 else LO.SoftAbs(D, 30.0, seed=100 * D + k))
            x0[k] = rng.normal(0, 0.5 if D >= 8 else 3.0, D).astype(np.float32)
    return funcs, x0


def case_reference(D, m, n):
    """The case runs until every frame has m + 4 accepted steps (the ring has wrapped); the largest D for 6 calls.  tol_grad = 0, so
    that no frame stops on the way."""
    funcs, x0 = case_functions(D, n)
    if D > 10000:
        trail, opt = reference(funcs, x0, m, 6, tol_grad=0.0)
    else:
        opt = LO.LBFGS(n, D, m, np.float32, tol_grad=0.0)
        x, trail = x0.copy(), []
        for call in range(4 * (m + 4) + 20):
            LO.run(opt, funcs, x, 1)
            trail.append((x.copy(), opt.state()))
            if opt.state()["iterations"].min() >= m + 4:
                break
    return dict(funcs=funcs, x0=x0, trail=trail, opt=opt)


@pytest.fixture(scope="module")
def cases():
    return {c: case_reference(*c) for c in CASES}


@pytest.mark.parametrize("D,m,n", CASES)
def test_bits(cases, D, m, n):
    c = cases[D, m, n]
    funcs, x0, trail = c["funcs"], c["x0"], c["trail"]
    it = trail[-1][1]["iterations"]
    assert len(trail) == 6 if D > 10000 else it.min() >= m + 4
    if 1 < D < 10000:  # the ring has wrapped in some frame: more pairs were pushed than it holds
        assert any(a.count == m and a.head != 0 or (m == 1 and a.count == 1 and a.iterations > 1) for a in c["opt"].frames)
    assert any("accepted" in log for log in c["opt"].log)
    layouts = [(False, False), (True, False)] + ([(False, True), (True, True)] if D == 72 else [])
    for dev, strided in layouts:
        d = Driver(funcs, x0, m, dev, strided, tol_grad=0.0)
        assert d.opt.info() == dict(n=n, dim=D, history=m)
        for k, want in enumerate(trail):
            assert agrees(d.call(), want), (dev, strided, k)
        assert not strided or d.margins_untouched()
    for k in sorted({0, n // 2, n - 1}):  # a frame alone has the bits it has at its slot of the batch
        for dev in ((True, False) if k == 0 else (True,)):
            d = Driver(funcs[k:k + 1], x0[k:k + 1], m, dev, tol_grad=0.0)
            for j, want in enumerate(trail):
                assert agrees(d.call(), want, slice(k, k + 1)), (k, dev, j)


# ---------------------------------------------------------------------------------------------------- 2. a mixed batch
def test_mixed_batch_and_poisoned_rows():
    funcs, x0 = LO.mixed_batch(np.float32)
    m, calls, opts = 5, 100, dict(tol_grad=1e-3)
    trail, ref = reference(funcs, x0, m, calls, **opts)
    assert trail[-1][1]["status"].tolist() == [1, 1, 4, 1] and len(trail) < calls
    clean, _ = reference(funcs[:2], x0[:2], m, calls, **opts)  # without the NaN frame and the +inf frame beside them
    for dev in (False, True):
        d, alone = Driver(funcs, x0, m, dev, **opts), Driver(funcs[:2], x0[:2], m, dev, **opts)
        for k, want in enumerate(trail):
            x, st = d.call(poison=True)
            stopped = trail[k - 1][1]["status"] != 0 if k else np.zeros(4, bool)
            assert (x[stopped] == FILL).all()  # a stopped frame's row is never written again
            x[stopped] = want[0][stopped]
            assert agrees((x, st), want), (dev, k)
            if k < len(clean):
                xa, sa = alone.call()
                live = clean[k - 1][1]["status"] == 0 if k else np.ones(2, bool)
                assert _same(xa[live], x[:2][live]) and agrees((xa, sa), clean[k])
        assert int(_host(d.opt.state(("running",))["running"])[0]) == 0


# ---------------------------------------------------------------------------------------------------- 3. rejections
def rejection_case():
    q = LO.Quadratic(8, 4, 11, scale=1000.0)
    q.c = q.c * (0.01 / np.linalg.norm(q.c))
    return [LO.InfOutsideBall(q, 0.05), LO.Quadratic(8, 10, 1)], np.zeros((2, 8), np.float32)


def test_rejection_path():
    funcs, x0 = rejection_case()
    trail, ref = reference(funcs, x0, 5, 14, tol_grad=1e-3)
    log = ref.log
    rejected = [w == "half" or w.startswith("interpolated") for w in log[0]]
    run3 = [k for k in range(len(rejected) - 2) if all(rejected[k:k + 3])]
    assert run3 and all(w == "accepted" for w in log[1][run3[0]:run3[0] + 3])  # three rejections in a row while the other frame accepts
    assert "half" in log[0] and "interpolated" in log[0]  # the 0.5 branch (f = +inf) and the interpolation (f finite, too high)
    for dev in (False, True):
        d = Driver(funcs, x0, 5, dev, tol_grad=1e-3)
        for k, want in enumerate(trail):
            assert agrees(d.call(), want), (dev, k)


# ---------------------------------------------------------------------------------------------------- 4. best, reset
def test_best_gives_the_accepted_point_of_a_frame_caught_mid_search():
    funcs, x0 = rejection_case()
    calls = 3  # frame 0 is in its line search, frame 1 has accepted twice
    trail, ref = reference(funcs, x0, 5, calls, tol_grad=1e-3)
    assert ref.frames[0].ls == 2 and ref.frames[0].iterations == 0 and ref.frames[1].iterations == 2
    want_x = ref.best(trail[-1][0].copy())
    assert not _same(want_x[0], trail[-1][0][0]) and _same(want_x[0], x0[0])
    for dev in (False, True):
        for strided in (False, True):
            d = Driver(funcs, x0, 5, dev, strided, tol_grad=1e-3)
            for _ in range(calls):
                d.call()
            f = d.opt.best(want_f=True)
            assert _same(d.points(), want_x) and _same(f, ref.state()["f_best"]) and (not strided or d.margins_untouched())
    fresh = Driver(funcs, x0 + np.float32(1), 5, True)  # before the first evaluation there is no accepted point: x stays
    fresh.opt.best()
    assert _same(fresh.points(), x0 + np.float32(1))


def test_reset_reproduces_the_first_run():
    funcs, x0 = case_functions(72, 5)
    trail, _ = reference(funcs, x0, 3, 12, tol_grad=0.0)
    for dev in (False, True):
        d = Driver(funcs, x0, 3, dev, tol_grad=0.0)
        first = [d.call() for _ in trail]
        assert all(agrees(a, b) for a, b in zip(first, trail))
        d.opt.reset()
        st = {k: _host(v) for k, v in d.opt.state().items()}
        assert all((st[k] == 0).all() for k in KEYS[:-1]) and st["running"][0] == 5
        if dev:
            d.x.copy_(torch.from_numpy(x0))
        else:
            d.x[:] = x0
        d.status = np.zeros(5, np.int32)
        assert all(agrees(d.call(), b) for b in trail)


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals():
    from smplpp_amd import _lib

    L = _lib.load()
    n, D, m = 3, 5, 4
    good = (1e-4, 1e-5, 0.0, 20, 1e-10)

    def create(n_=n, D_=D, m_=m, o=good):
        h = C.c_void_p(7)
        rc = L.smplpp_lbfgs_create(0, n_, D_, m_, *o, C.byref(h))
        if rc == 0:
            L.smplpp_lbfgs_destroy(h)
        else:
            assert h.value is None  # *out = NULL
        return rc

    def edit(i, v):
        o = list(good)
        o[i] = v
        return tuple(o)

    assert create() == 0 and create(m_=1) == 0 and create(m_=32) == 0 and create(o=edit(2, 1e-6)) == 0 and create(o=edit(4, 0.0)) == 0
    assert create(n_=0) == 1 and create(n_=-1) == 1 and create(D_=0) == 1 and create(D_=-5) == 1 and create(m_=0) == 1 and create(m_=33) == 1
    assert create(n_=2 ** 20, D_=2 ** 10, m_=2) == 1 and create(n_=2 ** 31) == 1  # n m D beyond int32 indexing
    for i, bad in ((0, (0.0, 1.0, -0.1, np.nan, np.inf)), (1, (-1e-9, np.nan, np.inf)), (2, (-1e-9, np.nan, np.inf)), (3, (0, 65, -1)),
                   (4, (-1e-12, 1.0, np.nan, np.inf))):
        for v in bad:
            assert create(o=edit(i, v)) == 1, (i, v)
    assert L.smplpp_lbfgs_create(0, n, D, m, *good, None) == 1  # no out

    funcs, x0 = case_functions(D, n)
    for dev in (False, True):
        d = Driver(funcs, x0, m, dev)
        d.call()
        h, space = d.opt.handle, 1 if dev else 0
        put = (lambda a: torch.from_numpy(a).cuda()) if dev else (lambda a: a)
        adr = lambda a: None if a is None else (a.data_ptr() if dev else a.ctypes.data)  # noqa: E731
        x, f, g = put(np.full((n, D), FILL, np.float32)), put(np.ones(n, np.float32)), put(np.ones((n, D), np.float32))
        outs = [put(np.full(n, 7, np.int32)) for _ in range(3)] + [put(np.full(n, FILL, np.float32)) for _ in range(2)] + [put(np.full(1, 7, np.int64))]
        before = {k: _host(v) for k, v in d.opt.state().items()}

        def step(h_=h, x_=x, ldx=D, f_=f, g_=g, ldg=D, space_=space):
            return L.smplpp_lbfgs_step(h_, adr(x_), ldx, adr(f_), adr(g_), ldg, space_, None)

        def best(h_=h, x_=x, ldx=D, f_=f, space_=space):
            return L.smplpp_lbfgs_best(h_, adr(x_), ldx, adr(f_), space_, None)

        def state(h_=h, o=outs, space_=space):
            return L.smplpp_lbfgs_state(h_, *(adr(a) for a in o), space_, None)

        for call in (step, best):
            assert call(h_=None) == 1 and call(ldx=D - 1) == 1 and call(x_=None) == 1 and call(space_=2) == 1 and call(space_=-1) == 1
            assert call(ldx=2 ** 30) == 1 and call(ldx=2 ** 31) == 1  # n ld beyond int32 indexing
        assert step(f_=None) == 1 and step(g_=None) == 1 and step(ldg=D - 1) == 1 and step(ldg=2 ** 30) == 1
        assert state(h_=None) == 1 and state(o=[None] * 6) == 1 and state(space_=2) == 1
        assert L.smplpp_lbfgs_info(None, None, None, None) == 1 and L.smplpp_lbfgs_reset(None, None) == 1
        torch.cuda.synchronize()
        assert (_host(x) == FILL).all() and (_host(f) == 1).all() and all((_host(a) == 7).all() for a in outs)
        after = {k: _host(v) for k, v in d.opt.state().items()}
        assert all(_same(after[k], before[k]) for k in KEYS)  # the state is untouched
        assert state() == 0 and all(_same(_host(a), before[k]) for a, k in zip(outs, KEYS))
        assert state(o=[None] * 5 + [outs[5]]) == 0 and best(f_=None) == 0
        torch.cuda.synchronize()
        assert (_host(x) != FILL).all()


# ---------------------------------------------------------------------------------------------------- 6. C++ shim
def test_lbfgs_cpp_shim(tmp_path):
    from smplpp_amd.optim import BatchedLBFGS

    exe = str(tmp_path / "lbfgs_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "lbfgs_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    n, D, calls, f32 = 3, 5, 12, np.float32
    x = ((np.arange(n * D) % 7 - 3) * f32(0.25)).astype(f32).reshape(n, D)
    i, k = np.arange(n)[:, None], np.arange(D)[None, :]
    lam, c = (f32(1) + (k * (1 + i)).astype(f32)).astype(f32), (f32(0.125) * (k - i).astype(f32)).astype(f32)
    opt = BatchedLBFGS(x, history=3, tol_grad=1e-3)
    want = []
    for _ in range(calls):
        e = x - c
        terms = (f32(0.5) * lam) * (e * e)
        f = np.zeros(n, f32)
        for j in range(D):
            f = f + terms[:, j]
        opt.step_with(f, lam * e)
        want.append(x.copy())
    st = opt.state()
    assert st["iterations"].min() >= 3
    want += [np.stack([st[k].astype(f32) for k in KEYS[:3]]), st["f_best"], st["step"], st["running"].astype(f32)]
    opt.best()
    want.append(x.copy())
    raw = open(outp, "rb").read()
    assert len(raw) == 4 * sum(a.size for a in want)
    off = 0
    for j, a in enumerate(want):
        got = np.frombuffer(raw, f32, a.size, off).reshape(a.shape)
        off += 4 * a.size
        assert _same_bits(got, np.ascontiguousarray(a)), j


# ---------------------------------------------------------------------------------------------------- 7. a fit
FIT_BUDGET = 126


def fit_energies(fs):
    """theta [n,25,3] float64 -> (per-frame energies [n], landmarks): the keypoint energy of a frame (the mean over its landmarks) plus
    FIT_PRIOR times its prior energy, so that their mean over the frames is the loss test_pose_prior_gpu's Adam runs minimise."""
    import test_pose_prior_gpu as TP

    cam64, t64 = torch.tensor(fs["cam"], dtype=torch.float64), PO.tensors(fs["prior"], torch.float64)

    def energies(theta, target=fs["target64"]):
        pts = fs["cpu"](theta, False)[1]
        uv, valid = KP.project_t(pts, cam64, TP.NEAR)
        e = KP.energy_t(uv, valid, target, TP.FIT_RHO).mean(1)
        return e + TP.FIT_PRIOR * PO.energy_t(t64, theta.reshape(len(theta), 75)[:, 6:])[0], pts

    return energies


def fit_float64(energies, n, budget, record=None):
    """`budget` evaluations of the float64 restatement from theta = 0, then best(): (theta [n,75], f_best [n])."""
    opt = LO.LBFGS(n, 75, 10, np.float64)
    x = np.zeros((n, 75))
    for k in range(budget):
        th = torch.tensor(x.reshape(n, 25, 3), requires_grad=True)
        e, _ = energies(th)
        e.sum().backward()
        opt.step(x, e.detach().numpy(), th.grad.numpy().reshape(n, 75))
        if record is not None:
            record.append(opt.state()["f_best"])
    opt.best(x)
    return x, opt.state()["f_best"]


def landmark_error(pts, pts_true):
    """Mean 3-D error of landmarks 24..52 per frame, in mm."""
    return 1000 * (pts[:, 24:].double().cpu() - pts_true[:, 24:]).norm(dim=-1).mean(1).numpy()


def test_fit_against_float64(synth_model):
    """The n = 4 single-view fit of test_pose_prior_gpu.fit_setup (keypoints + prior, theta from 0) with BatchedLBFGS on theta.view(n, 75),
    against the same schedule of the float64 restatement on the float64 graph.  Measured on the CPU in float64: after 200 Adam steps
    (lr 0.02) the frames' energies are 1.5092, 1.3462, 2.3703, 1.7413; the L-BFGS is at or below them in every frame from 126
    evaluations on (1.4997, 1.0901, 1.8573, 0.4229; at 100 evaluations it is not: 1.7115, 1.4749, 2.1845, 0.6508), so the budget is 126."""
    import test_pose_prior_gpu as TP
    from smplpp_amd import smpl as S
    from smplpp_amd.landmarks import Landmarks
    from smplpp_amd.optim import BatchedLBFGS
    from smplpp_amd.priors import PosePrior
    from smplpp_amd.smpl import SMPL

    fs = TP.fit_setup(synth_model)
    n, B = fs["n"], FIT_BUDGET
    energies = fit_energies(fs)
    # the property of the fixture, in float64 alone
    theta = torch.zeros(n, 25, 3, dtype=torch.float64, requires_grad=True)
    adam = torch.optim.Adam([theta], lr=TP.FIT_LR)
    for _ in range(TP.FIT_STEPS):
        adam.zero_grad()
        fs["cpu"](theta, True)[0].backward()
        adam.step()
    with torch.no_grad():
        e_adam = energies(theta)[0].numpy()
    x64, f64 = fit_float64(energies, n, B)
    with torch.no_grad():
        e64, pts64 = energies(torch.tensor(x64.reshape(n, 25, 3)))
    err64 = landmark_error(pts64, fs["pts_true"])
    print("float64: Adam %s, L-BFGS after %d evaluations %s, landmark error %s mm" % (e_adam, B, f64, err64))
    assert B <= TP.FIT_STEPS and (f64 <= e_adam).all() and np.allclose(e64.numpy(), f64, rtol=1e-12)

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    lm = Landmarks(s, *fs["reg"])
    p = fs["prior"]
    prior = PosePrior("cuda:0", p["mean"], p["mat"], p["offset"])
    dev = torch.device("cuda:0")
    cam32, beta32 = torch.from_numpy(fs["cam"]).to(dev), torch.zeros(n, 10, device=dev)

    def gpu_fit(target64):
        target32 = target64.float().to(dev)
        theta = torch.zeros(n, 25, 3, device=dev, requires_grad=True)
        pts = [None]

        def closure():
            verts, joints = s.forward_differentiable(beta32, theta)
            pts[0] = lm.forward_differentiable(verts, joints)
            _, e, _ = S.project_points_differentiable(pts[0], cam32, target32, TP.FIT_RHO, TP.NEAR)
            return e.mean(1) + TP.FIT_PRIOR * prior.forward_differentiable(theta)[0]

        opt = BatchedLBFGS(theta.view(n, 75), history=10)
        trail = []
        for _ in range(B):
            opt.step(closure)
            trail.append(theta.detach().clone())
        st = opt.run(closure, 0)  # ends with best()
        with torch.no_grad():
            e = closure()
        return theta.detach(), e.cpu().numpy(), pts[0].detach(), {k: _host(v) for k, v in st.items()}, torch.stack(trail).cpu().numpy()

    theta32, e32, pts32, st, trail = gpu_fit(fs["target64"])
    err32 = landmark_error(pts32, fs["pts_true"])
    print("MI355X: L-BFGS after %d evaluations %s, landmark error %s mm, status %s, iterations %s" % (B, e32, err32, st["status"], st["iterations"]))
    assert (st["evaluations"] == B).all() and np.allclose(e32, st["f_best"], rtol=1e-5)
    assert (e32 <= 2 * f64 + 1e-6).all(), (e32, f64)
    assert (err32 <= 2 * err64).all(), (err32, err64)

    # a frame without data (confidences 0: the prior's gradient alone) and a frame with NaN detections change no other frame's bits
    target = fs["target64"].clone()
    target[1, :, 2] = 0.0
    target[2, :, :2] = float("nan")
    _, _, _, st2, trail2 = gpu_fit(target)
    assert st2["status"][2] == 4 and st2["evaluations"][2] == 1 and (trail2[:, 2] == 0).all()
    assert not _same(trail2[:, 1], trail[:, 1])
    for k in (0, 3):
        assert _same(trail2[:, k], trail[:, k]), k
