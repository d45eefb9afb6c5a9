"""L-BFGS problems that span groups of rows on the MI355X (smplpp_lbfgs_create_grouped and the entry points that take its handle): after
every call, x and every output of smplpp_lbfgs_state against the float32 numpy restatement of tests/lbfgs_groups_oracle.py, bit for
bit, on both sides of the LDS threshold; independence of P, slot, the others' lengths, space and leading dimension; a ragged batch with
NaN and +inf problems whose stopped rows are poisoned; the rejection branches; best(), reset(), the refusals, the C++ shim; and a fit of
two sequences with a shared beta and a velocity term against the float64 restatement on the float64 graph.  Energies and gradients of
the bit tests are computed on the host by the float32 numpy functions, so the library and the restatement see identical inputs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_vjp_oracle as FK  # noqa: E402
import keypoints_oracle as KP  # noqa: E402
import lbfgs_groups_oracle as GO  # noqa: E402
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
    """A BatchedLBFGS with groups on x0 [n,D] in host or device space, in rows of D floats or at offset OFF inside rows of LD floats, fed
    by the float32 numpy functions (funcs[p] on the flat vector of problem p): only running problems are evaluated, the rows of the
    others keep what they held."""

    def __init__(self, funcs, groups, x0, m, dev, strided=False, **options):
        from smplpp_amd.optim import BatchedLBFGS

        n, D = x0.shape
        self.funcs, self.groups, self.n, self.D, self.dev, self.P = funcs, list(groups), n, D, dev, len(groups)
        self.start = np.concatenate([[0], np.cumsum(groups)])
        buf = np.full((n, LD), FILL, np.float32) if strided else np.empty((n, D), np.float32)
        gbuf = np.full((n, LD), FILL, np.float32) if strided else np.zeros((n, D), np.float32)
        cut = (slice(None), slice(OFF, OFF + D)) if strided else (slice(None), slice(None))
        buf[cut] = x0
        self.buf, self.gbuf = (torch.from_numpy(buf).cuda(), torch.from_numpy(gbuf).cuda()) if dev else (buf, gbuf)
        self.x, self.g = self.buf[cut], self.gbuf[cut]
        self.f = torch.zeros(self.P).cuda() if dev else np.zeros(self.P, np.float32)
        self.opt = BatchedLBFGS(self.x, history=m, groups=groups, **options)
        self.status = np.zeros(self.P, np.int32)

    def rows(self, p):
        return slice(int(self.start[p]), int(self.start[p + 1]))

    def points(self):
        return np.array(_host(self.x), np.float32)

    def call(self, poison=False):
        """One evaluation and one step; returns (x [n,D], state) on the host.  poison: every row of a stopped problem gets NaN gradients
        and the sentinel FILL in x beforehand, and its energy NaN."""
        x = self.points()
        f, g = np.array(_host(self.f)), np.array(_host(self.g))
        for p in range(self.P):
            if self.status[p] == 0:
                f[p], gp = self.funcs[p](x[self.rows(p)].reshape(-1))
                g[self.rows(p)] = gp.reshape(-1, self.D)
            elif poison:
                f[p], g[self.rows(p)], x[self.rows(p)] = np.nan, np.nan, FILL
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


def reference(funcs, groups, x0, m, calls, **options):
    """[(x, state)] after each call of the float32 restatement, and the restatement itself."""
    opt = GO.GroupedLBFGS(groups, x0.shape[1], m, np.float32, **options)
    x, trail = x0.copy(), []
    GO.run(opt, funcs, x, calls, after=lambda call: trail.append((x.copy(), opt.state())))
    return trail, opt


def agrees(got, want, problem=None, rows=None):
    """(x, state) of one call against the restatement's: all problems, or the restatement's problem `problem` (its rows `rows`) against a
    handle that holds that problem alone."""
    (xg, sg), (xw, sw) = got, want
    if problem is None:
        return _same(xg, xw) and all(_same(sg[k], sw[k]) for k in KEYS[:-1]) and sg["running"][0] == sw["running"][0]
    return _same(xg, xw[rows]) and all(_same(sg[k], sw[k][problem:problem + 1]) for k in KEYS[:-1])


# ---------------------------------------------------------------------------------------------------- 1. bits
# (row lengths; D; m).  The working vector lives in LDS up to N = 32768 for the longest problem of a handle, with an opt-in above 64 KiB:
# every shape of the issue runs that path, 20670 and 22500 with the opt-in; [2, 1, 2] x 1025 (N = 2050) has m = 32.  The last two are on
# either side of the threshold, N = 32768 and 32769 (one row of 1 more): the second runs the path through global memory.
CASES = [((1,), 1, 1), ((1, 3, 14), 72, 3), ((15,), 72, 10), ((14, 1), 75, 10), ((1023,), 1, 3), ((1024,), 1, 3), ((1025,), 1, 3), ((2, 1, 2), 1025, 32),
         ((1,), 20670, 3), ((300, 7), 75, 10), ((3, 32768), 1, 3), ((2, 32769), 1, 3)]
LARGEST = (((1,), 20670, 3), ((300, 7), 75, 10), ((3, 32768), 1, 3), ((2, 32769), 1, 3))


def case_functions(groups, D, seed=0):
    """Problem p on its N = rows * D unknowns: a chain of quadratics of condition 1000 coupled by a velocity term (even p), or the chained
    Rosenbrock function from its usual start (odd p); below N = 8, where a quadratic ends in a few exact steps, the soft absolute value of
    condition 30 from further away."""
    rng = np.random.default_rng(1000 * D + sum(groups) + seed)
    funcs, x0 = [], np.zeros((sum(groups), D), np.float32)
    r0 = 0
    for p, rows in enumerate(groups):
        N = rows * D
        if N < 8:
            funcs.append(LO.SoftAbs(N, 30.0, seed=100 * D + p + seed))
            xp = rng.normal(0, 3.0, N)
        elif p % 2:
            funcs.append(LO.Rosenbrock())
            xp = LO.Rosenbrock.start(N, np.float32) + rng.normal(0, 0.05, N)
        else:
            funcs.append(GO.Chain(rows, D, 1000.0, 1.0, seed=100 * D + 7 * p + seed))
            xp = rng.normal(0, 0.5, N)
        x0[r0:r0 + rows] = xp.astype(np.float32).reshape(rows, D)
        r0 += rows
    return funcs, x0


def case_reference(groups, D, m):
    """The case runs until every problem has m + 4 accepted steps (the ring has wrapped); those of LARGEST for 6 calls.  tol_grad = 0, so
    that no problem stops on the way."""
    funcs, x0 = case_functions(groups, D)
    if (groups, D, m) in LARGEST:
        trail, opt = reference(funcs, groups, x0, m, 6, tol_grad=0.0)
    else:
        opt = GO.GroupedLBFGS(groups, D, m, np.float32, tol_grad=0.0)
        x, trail = x0.copy(), []
        for call in range(4 * (m + 4) + 20):
            GO.run(opt, funcs, x, 1)
            trail.append((x.copy(), opt.state()))
            if opt.state()["iterations"].min() >= m + 4:
                break
    return dict(funcs=funcs, x0=x0, trail=trail, opt=opt)


@pytest.fixture(scope="module")
def cases():
    return {c: case_reference(*c) for c in CASES}


@pytest.mark.parametrize("groups,D,m", CASES)
def test_bits(cases, groups, D, m):
    c = cases[groups, D, m]
    funcs, x0, trail = c["funcs"], c["x0"], c["trail"]
    it = trail[-1][1]["iterations"]
    assert len(trail) == 6 if (groups, D, m) in LARGEST else it.min() >= m + 4
    assert (trail[-1][1]["status"] == 0).all()
    if (groups, D, m) not in LARGEST and max(groups) * D > 1:  # the ring has wrapped in some problem: more pairs were pushed than it holds
        assert any(a.count == m and a.head != 0 for a in c["opt"].frames)
    assert all("accepted" in log for log in c["opt"].log)
    layouts = [(False, False), (True, False)] + ([(False, True), (True, True)] if D == 72 else [])
    for dev, strided in layouts:
        d = Driver(funcs, groups, x0, m, dev, strided, tol_grad=0.0)
        assert d.opt.info() == dict(n=sum(groups), dim=D, history=m)
        assert d.opt.row_start() == (len(groups), [0] + np.cumsum(groups).tolist())
        for k, want in enumerate(trail):
            assert agrees(d.call(), want), (dev, strided, k)
        assert not strided or d.margins_untouched()


# ---------------------------------------------------------------------------------------------------- 2. alone and in a batch
def test_a_problem_alone_has_the_bits_of_its_slot():
    """The first, the middle and the last problem of a ragged handle, each alone in a handle of its own (P = 1, slot 0, no neighbours) and
    as the middle problem among neighbours of other lengths: the bits of its slot in the ragged handle."""
    groups, D, m, calls = (3, 1, 14, 2, 15), 72, 3, 10
    funcs, x0 = case_functions(groups, D, seed=5)
    trail, ref = reference(funcs, groups, x0, m, calls, tol_grad=0.0)
    assert len(trail) == calls and all("accepted" in log for log in ref.log)
    start = np.concatenate([[0], np.cumsum(groups)])
    other_funcs, other_x0 = case_functions((2, 9), D, seed=9)
    for p in (0, 2, 4):
        rows = slice(int(start[p]), int(start[p + 1]))
        for dev in ((True, False) if p == 0 else (True,)):
            d = Driver(funcs[p:p + 1], groups[p:p + 1], x0[rows], m, dev, tol_grad=0.0)
            for k, want in enumerate(trail):
                assert agrees(d.call(), want, p, rows), (p, dev, k)
        # between a 2-row and a 9-row problem, at offset 3 in rows of 75 floats
        d = Driver([other_funcs[0], funcs[p], other_funcs[1]], (2, groups[p], 9), np.concatenate([other_x0[:2], x0[rows], other_x0[2:]]), m, True, True,
                   tol_grad=0.0)
        for k, want in enumerate(trail):
            x, st = d.call()
            assert agrees((x[2:2 + groups[p]], {key: v[1:2] for key, v in st.items()}), want, p, rows), (p, k)
        assert d.margins_untouched()


# ---------------------------------------------------------------------------------------------------- 3. poisoned rows
def test_ragged_batch_and_poisoned_rows():
    funcs, groups, x0 = GO.ragged_batch(np.float32)
    m, calls, opts = 5, 150, dict(tol_grad=1e-3)
    trail, ref = reference(funcs, groups, x0, m, calls, **opts)
    assert trail[-1][1]["status"].tolist() == [1, 1, 4, 1] and len(trail) < calls
    clean, _ = reference(funcs[:2], groups[:2], x0[:7], m, calls, **opts)  # without the NaN problem and the +inf problem beside them
    start = np.concatenate([[0], np.cumsum(groups)])
    for dev in (False, True):
        d, alone = Driver(funcs, groups, x0, m, dev, **opts), Driver(funcs[:2], groups[:2], x0[:7], m, dev, **opts)
        for k, want in enumerate(trail):
            x, st = d.call(poison=True)
            stopped = trail[k - 1][1]["status"] != 0 if k else np.zeros(4, bool)
            rows = np.repeat(stopped, groups)
            assert (x[rows] == FILL).all()  # no row of a stopped problem is ever written again
            assert np.isnan(_host(d.g)[rows]).all() and np.isnan(_host(d.f)[stopped]).all()
            x[rows] = want[0][rows]
            assert agrees((x, st), want), (dev, k)
            if k < len(clean):
                xa, sa = alone.call()
                live = np.repeat(clean[k - 1][1]["status"] == 0 if k else np.ones(2, bool), groups[:2])
                assert _same(xa[live], x[:7][live]) and agrees((xa, sa), clean[k])
        assert int(_host(d.opt.state(("running",))["running"])[0]) == 0
        assert start[-1] == d.n


# ---------------------------------------------------------------------------------------------------- 4. rejections, best, reset
def rejection_case():
    """Two problems of 2 rows x 4: a stiff quadratic that is +inf outside a small ball, and an easy quadratic."""
    q = LO.Quadratic(8, 4, 11, scale=1000.0)
    q.c = q.c * (0.01 / np.linalg.norm(q.c))
    return [LO.InfOutsideBall(q, 0.05), LO.Quadratic(8, 10, 1)], (2, 2), np.zeros((4, 4), np.float32)


def test_rejection_path():
    funcs, groups, x0 = rejection_case()
    trail, ref = reference(funcs, groups, x0, 5, 14, tol_grad=1e-3)
    log = ref.log
    halves = [k for k in range(len(log[0]) - 3) if log[0][k:k + 4] == ["half"] * 4]
    assert halves and all(w == "accepted" for w in log[1][halves[0]:halves[0] + 4])  # four 0.5-branch rejections while the neighbour accepts
    assert "interpolated" in log[0]  # and the interpolation (f finite, too high)
    for dev in (False, True):
        d = Driver(funcs, groups, x0, 5, dev, tol_grad=1e-3)
        for k, want in enumerate(trail):
            assert agrees(d.call(), want), (dev, k)


def test_best_gives_the_accepted_point_of_a_problem_caught_mid_search():
    funcs, groups, x0 = rejection_case()
    calls = 3  # problem 0 is in its line search, problem 1 has accepted twice
    trail, ref = reference(funcs, groups, x0, 5, calls, tol_grad=1e-3)
    assert ref.frames[0].ls == 2 and ref.frames[0].iterations == 0 and ref.frames[1].iterations == 2
    want_x = ref.best(trail[-1][0].copy())
    assert not _same(want_x[:2], trail[-1][0][:2]) and _same(want_x[:2], x0[:2])
    for dev in (False, True):
        for strided in (False, True):
            d = Driver(funcs, groups, x0, 5, dev, strided, tol_grad=1e-3)
            for _ in range(calls):
                d.call()
            f = d.opt.best(want_f=True)
            assert _same(d.points(), want_x) and _same(f, ref.state()["f_best"]) and (not strided or d.margins_untouched())
    fresh = Driver(funcs, groups, x0 + np.float32(1), 5, True)  # before the first evaluation there is no accepted point: x stays
    fresh.opt.best()
    assert _same(fresh.points(), x0 + np.float32(1))


def test_reset_reproduces_the_first_run():
    groups = (2, 1, 3)
    funcs, x0 = case_functions(groups, 72, seed=3)
    trail, _ = reference(funcs, groups, x0, 3, 12, tol_grad=0.0)
    for dev in (False, True):
        d = Driver(funcs, groups, x0, 3, dev, tol_grad=0.0)
        first = [d.call() for _ in trail]
        assert all(agrees(a, b) for a, b in zip(first, trail))
        d.opt.reset()
        st = {k: _host(v) for k, v in d.opt.state().items()}
        assert all((st[k] == 0).all() and len(st[k]) == 3 for k in KEYS[:-1]) and st["running"][0] == 3
        if dev:
            d.x.copy_(torch.from_numpy(x0))
        else:
            d.x[:] = x0
        d.status = np.zeros(3, np.int32)
        assert all(agrees(d.call(), b) for b in trail)


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals():
    from smplpp_amd import _lib
    from smplpp_amd.optim import BatchedLBFGS

    L = _lib.load()
    n, D, m, P = 6, 5, 4, 3
    good, start0 = (1e-4, 1e-5, 0.0, 20, 1e-10), [0, 2, 3, 6]

    def create(n_=n, D_=D, m_=m, P_=P, start=start0, o=good):
        h = C.c_void_p(7)
        arr = None if start is None else (C.c_int64 * len(start))(*start)
        rc = L.smplpp_lbfgs_create_grouped(0, n_, D_, m_, P_, arr, *o, C.byref(h))
        if rc == 0:
            got_P, got = C.c_int64(), (C.c_int64 * (P_ + 1))()
            assert L.smplpp_lbfgs_groups(h, C.byref(got_P), got) == 0 and got_P.value == P_ and list(got) == list(start)
            L.smplpp_lbfgs_destroy(h)
        else:
            assert h.value is None  # *out = NULL
        return rc

    assert create() == 0 and create(P_=1, start=[0, 6]) == 0 and create(P_=6, start=list(range(7))) == 0 and create(m_=32) == 0
    assert create(P_=0, start=[0]) == 1 and create(P_=-1, start=[0]) == 1 and create(start=None) == 1
    assert create(start=[1, 2, 3, 6]) == 1 and create(start=[0, 2, 3, 5]) == 1 and create(start=[0, 2, 3, 7]) == 1
    assert create(start=[0, 2, 2, 6]) == 1 and create(start=[0, 3, 2, 6]) == 1 and create(start=[0, 2, 6, 6]) == 1
    assert create(n_=0, P_=1, start=[0, 0]) == 1 and create(D_=0) == 1 and create(m_=0) == 1 and create(m_=33) == 1
    assert create(n_=2 ** 20, D_=2 ** 10, m_=2, P_=1, start=[0, 2 ** 20]) == 1
    for i, bad in ((0, 0.0), (1, -1e-9), (2, np.inf), (3, 65), (4, 1.0)):
        o = list(good)
        o[i] = bad
        assert create(o=tuple(o)) == 1, (i, bad)
    assert L.smplpp_lbfgs_create_grouped(0, n, D, m, P, (C.c_int64 * 4)(*start0), *good, None) == 1  # no out
    assert L.smplpp_lbfgs_groups(None, None, None) == 1
    plain = BatchedLBFGS(np.zeros((4, 3), np.float32))  # a handle without groups reports every row as a problem
    assert plain.row_start() == (4, [0, 1, 2, 3, 4])

    groups = (2, 1, 3)
    funcs, x0 = case_functions(groups, D, seed=1)
    for dev in (False, True):
        d = Driver(funcs, groups, x0, m, dev)
        d.call()
        h, space = d.opt.handle, 1 if dev else 0
        put = (lambda a: torch.from_numpy(a).cuda()) if dev else (lambda a: a)
        adr = lambda a: None if a is None else (a.data_ptr() if dev else a.ctypes.data)  # noqa: E731
        x, f, g = put(np.full((n, D), FILL, np.float32)), put(np.ones(P, np.float32)), put(np.ones((n, D), np.float32))
        outs = [put(np.full(P, 7, np.int32)) for _ in range(3)] + [put(np.full(P, FILL, np.float32)) for _ in range(2)] + [put(np.full(1, 7, np.int64))]
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
        torch.cuda.synchronize()
        assert (_host(x) == FILL).all() and (_host(f) == 1).all() and all((_host(a) == 7).all() for a in outs)
        after = {k: _host(v) for k, v in d.opt.state().items()}
        assert all(_same(after[k], before[k]) for k in KEYS)  # the state is untouched
        assert state() == 0 and all(_same(_host(a), before[k]) for a, k in zip(outs, KEYS))
        assert state(o=[None] * 5 + [outs[5]]) == 0 and best(f_=None) == 0
        torch.cuda.synchronize()
        assert (_host(x) != FILL).all()
        with pytest.raises(_lib.SmplppError):  # energies per row where the handle has problems
            d.opt.step_with(put(np.ones(n, np.float32)), g)


# ---------------------------------------------------------------------------------------------------- 6. C++ shim
def test_lbfgs_groups_cpp_shim(tmp_path):
    from smplpp_amd.optim import BatchedLBFGS

    exe = str(tmp_path / "lbfgs_groups_shim")
    libdir = os.path.join(ROOT, "smplpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "lbfgs_groups_shim.cpp"), "-o", exe, "-L" + libdir, "-lsmplpp_hip",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    outp = str(tmp_path / "out.bin")
    r = subprocess.run([exe, outp], stdout=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stdout
    groups, n, P, D, calls, f32 = [2, 1, 3], 6, 3, 5, 12, np.float32
    x = ((np.arange(n * D) % 7 - 3) * f32(0.25)).astype(f32).reshape(n, D)
    i, k = np.arange(n)[:, None], np.arange(D)[None, :]
    lam, c = (f32(1) + (k * (1 + i)).astype(f32)).astype(f32), (f32(0.125) * (k - i).astype(f32)).astype(f32)
    opt = BatchedLBFGS(x, history=3, groups=groups, tol_grad=1e-3)
    start = [0, 2, 3, 6]
    want = []
    for _ in range(calls):
        e = x - c
        terms = ((f32(0.5) * lam) * (e * e)).astype(f32)
        f = np.zeros(P, f32)
        for p in range(P):
            for t in terms[start[p]:start[p + 1]].reshape(-1):  # the rows of the problem, then k, from +0
                f[p] = f[p] + t
        opt.step_with(f, lam * e)
        want.append(x.copy())
    st = opt.state()
    assert st["iterations"].min() >= 3 and len(st["status"]) == P
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


# ---------------------------------------------------------------------------------------------------- 7. a sequence fit
SEQ_T = (6, 4)                # frames of the two sequences; each is a block of T + 1 rows of 75 with beta in the first 10 of its last row
SEQ_GROUPS = [7, 5]
SEQ_VELOCITY, SEQ_BETA = 10.0, 0.01  # the weights of sum_t |J_(t+1) - J_t|^2 (joints in metres) and of |beta|^2
SEQ_SEED = 17
SEQ_BUDGET = 123


def seq_layout(buf):
    """buf [12,75] -> (theta [10,25,3], beta [10,10] (each frame its sequence's), the rows of beta [2,10])."""
    (Ta, Tb) = SEQ_T
    theta = torch.cat([buf[:Ta], buf[Ta + 1:Ta + 1 + Tb]]).reshape(Ta + Tb, 25, 3)
    shared = torch.stack([buf[Ta, :10], buf[Ta + 1 + Tb, :10]])
    return theta, torch.cat([shared[0].expand(Ta, 10), shared[1].expand(Tb, 10)]).contiguous(), shared


def seq_energy(frames, joints, shared):
    """Per problem: the frames' energies, the velocity term on the joints [10,24,3] and the ridge on beta."""
    Ta = SEQ_T[0]
    vel = (joints[1:] - joints[:-1]).pow(2).sum((1, 2))  # [9]: the pair (Ta - 1, Ta) joins the two sequences and is left out
    return torch.stack([frames[:Ta].sum() + SEQ_VELOCITY * vel[:Ta - 1].sum(), frames[Ta:].sum() + SEQ_VELOCITY * vel[Ta:].sum()]) + SEQ_BETA * shared.pow(2).sum(1)


def seq_setup(synth_model):
    """Two sequences on the synthetic model with the 53-row regressor and synthetic_gmm(8, 69, 5): theta linear in time between two poses
    ~N(0, 0.3^2) (rotation and pose; no translation), one beta ~N(0, 1) per sequence, the camera and the confidences of
    test_pose_prior_gpu.fit_setup; detections are the true landmarks' projections.  The float64 graph is restated on the vertices the
    regressor reads."""
    import test_pose_prior_gpu as TP

    n = sum(SEQ_T)
    reg = KP.regressor_53(synth_model)
    V = synth_model["vertices_template"].shape[0]
    mean, mat, offset = PO.gmm_tables(*PO.synthetic_gmm(8, 69, 5))
    p = dict(mean=mean, mat=mat, offset=offset, lo=None, hi=None, weight=None)
    rng = np.random.default_rng(SEQ_SEED)
    theta_true, beta_true = np.zeros((n, 25, 3)), rng.normal(0, 1.0, (2, 10))
    r0 = 0
    for T in SEQ_T:
        a, b = rng.normal(0, 0.3, (2, 24, 3))
        w = np.linspace(0.0, 1.0, T)[:, None, None]
        theta_true[r0:r0 + T, 1:] = (1 - w) * a + w * b
        r0 += T
    cam = np.tile(np.concatenate([np.diag([1.0, -1.0, -1.0]).reshape(9), [0.0, -0.36, 2.5], [500.0, 500.0, 320.0, 240.0]]), (n, 1)).astype(np.float32)
    conf = np.zeros(53, np.float32)
    conf[24:48:2] = 1.0
    used = np.unique(np.concatenate([reg[1][reg[1] < V], np.nonzero(np.abs(synth_model["joint_regressor"]).sum(0))[0]]))
    sub = {k: synth_model[k][used] for k in ("vertices_template", "shape_blend_shapes", "pose_blend_shapes", "weights")}
    sub["joint_regressor"], sub["kinematic_tree"] = synth_model["joint_regressor"][:, used], synth_model["kinematic_tree"]
    m64 = FK.model_tensors(sub, torch.float64)
    A64 = torch.tensor(np.concatenate([KP.dense(reg, V + 24)[:, used], KP.dense(reg, V + 24)[:, V:]], 1))
    cam64, t64 = torch.tensor(cam, dtype=torch.float64), PO.tensors(p, torch.float64)

    def points64(theta, beta):
        out = FK.fk(m64, beta, theta)
        return KP.landmarks_t(A64, out["verts"], out["joints"]), out["joints"]

    true_buf = torch.zeros(n + 2, 75, dtype=torch.float64)
    true_buf[:SEQ_T[0]], true_buf[SEQ_T[0] + 1:n + 1] = torch.tensor(theta_true[:SEQ_T[0]]).reshape(-1, 75), torch.tensor(theta_true[SEQ_T[0]:]).reshape(-1, 75)
    true_buf[SEQ_T[0], :10], true_buf[n + 1, :10] = torch.tensor(beta_true[0]), torch.tensor(beta_true[1])
    with torch.no_grad():
        th, be, _ = seq_layout(true_buf)
        pts_true, _ = points64(th, be)
        uv_true, ok = KP.project_t(pts_true, cam64, TP.NEAR)
    assert bool(ok.all())
    target64 = torch.cat([uv_true, torch.tensor(conf, dtype=torch.float64).expand(n, 53)[..., None]], -1)

    def energies64(buf, target=target64):
        """buf [12,75] float64 -> (the two problems' energies, landmarks [10,53,3], the rows of beta [2,10])."""
        theta, beta, shared = seq_layout(buf)
        pts, joints = points64(theta, beta)
        uv, valid = KP.project_t(pts, cam64, TP.NEAR)
        frames = KP.energy_t(uv, valid, target, TP.FIT_RHO).mean(1) + TP.FIT_PRIOR * PO.energy_t(t64, theta.reshape(n, 75)[:, 6:])[0]
        return seq_energy(frames, joints, shared), pts, shared

    return dict(n=n, reg=reg, prior=p, cam=cam, target64=target64, pts_true=pts_true, beta_true=beta_true, energies64=energies64)


def seq_float64(energies64, budget, record=None):
    """`budget` evaluations of the float64 grouped restatement from 0, then best(): (buf [12,75], f_best [2])."""
    opt = GO.GroupedLBFGS(SEQ_GROUPS, 75, 10, np.float64)
    x = np.zeros((sum(SEQ_GROUPS), 75))
    for k in range(budget):
        buf = torch.tensor(x, requires_grad=True)
        e = energies64(buf)[0]
        e.sum().backward()
        opt.step(x, e.detach().numpy(), buf.grad.numpy())
        if record is not None:
            record.append(opt.state()["f_best"])
    opt.best(x)
    return x, opt.state()["f_best"]


def seq_adam(energies64, steps, lr):
    buf = torch.zeros(sum(SEQ_GROUPS), 75, dtype=torch.float64, requires_grad=True)
    adam = torch.optim.Adam([buf], lr=lr)
    for _ in range(steps):
        adam.zero_grad()
        energies64(buf)[0].sum().backward()
        adam.step()
    with torch.no_grad():
        return energies64(buf)[0].numpy()


def seq_errors(pts, shared, fs):
    """Mean 3-D error of landmarks 24..52 per problem in mm, and |beta - beta_true| per problem."""
    per_frame = 1000 * (pts[:, 24:].double().cpu() - fs["pts_true"][:, 24:]).norm(dim=-1).mean(1).numpy()
    Ta = SEQ_T[0]
    return np.array([per_frame[:Ta].mean(), per_frame[Ta:].mean()]), np.linalg.norm(shared.double().cpu().numpy() - fs["beta_true"], axis=1)


def test_sequence_fit_against_float64(synth_model):
    """Two sequences of T = 6 and T = 4 frames in one handle, groups=[7, 5]: each a [T+1, 75] block of theta rows with beta in the first 10
    coordinates of its last row, all from 0, m = 10.  Energy per problem: sum_t (keypoint mean + 0.01 prior) + 10 sum_t |J_(t+1) - J_t|^2
    + 0.01 |beta|^2 through forward_differentiable -> Landmarks -> project_points_differentiable -> PosePrior, against the same schedule
    of the float64 grouped restatement on the float64 graph.  Measured on the CPU in float64: after 200 Adam steps (lr 0.02) the problems'
    energies are 12.9843 and 5.5274; the L-BFGS is at or below them in both problems from 123 evaluations on (10.1976, 5.4725; at 122
    it is not: 10.2763, 5.5378; at 100: 12.7945, 6.5441), the same with 1 and with 16 threads, so the budget is 123.  On the MI355X after
    123 evaluations: energies 10.2459, 5.4943 (float64: 10.1977, 5.4726; bar 2x + 1e-6), mean 3-D landmark error 112.8, 109.5 mm (112.2,
    110.8; bar 2x), |beta - beta_true| 2.839, 3.820 (2.839, 3.803; bar 2x: twelve 2-D detections a frame hardly determine beta, in either
    precision)."""
    import test_pose_prior_gpu as TP
    from smplpp_amd import smpl as S
    from smplpp_amd.landmarks import Landmarks
    from smplpp_amd.optim import BatchedLBFGS
    from smplpp_amd.priors import PosePrior
    from smplpp_amd.smpl import SMPL

    fs = seq_setup(synth_model)
    n, B, energies64 = fs["n"], SEQ_BUDGET, fs["energies64"]
    # the property of the fixture, in float64 alone
    e_adam = seq_adam(energies64, TP.FIT_STEPS, TP.FIT_LR)
    x64, f64 = seq_float64(energies64, B)
    with torch.no_grad():
        e64, pts64, shared64 = energies64(torch.tensor(x64))
    err64, beta64 = seq_errors(pts64, shared64, fs)
    print("float64: Adam %s, L-BFGS after %d evaluations %s, landmark error %s mm, |beta - beta_true| %s" % (e_adam, B, f64, err64, beta64))
    assert B <= TP.FIT_STEPS and (f64 <= e_adam).all() and np.allclose(e64.numpy(), f64, rtol=1e-12)

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    lm = Landmarks(s, *fs["reg"])
    p = fs["prior"]
    prior = PosePrior("cuda:0", p["mean"], p["mat"], p["offset"])
    dev = torch.device("cuda:0")
    cam32 = torch.from_numpy(fs["cam"]).to(dev)

    def gpu_fit(target64):
        target32 = target64.float().to(dev)
        buf = torch.zeros(sum(SEQ_GROUPS), 75, device=dev, requires_grad=True)
        keep = [None, None]

        def closure():
            theta, beta, shared = seq_layout(buf)
            verts, joints = s.forward_differentiable(beta, theta)
            pts = lm.forward_differentiable(verts, joints)
            _, e, _ = S.project_points_differentiable(pts, cam32, target32, TP.FIT_RHO, TP.NEAR)
            keep[:] = pts, shared
            return seq_energy(e.mean(1) + TP.FIT_PRIOR * prior.forward_differentiable(theta)[0], joints, shared)

        opt = BatchedLBFGS(buf, history=10, groups=SEQ_GROUPS)
        trail = []
        for _ in range(B):
            opt.step(closure)
            trail.append(buf.detach().clone())
        st = opt.run(closure, 0)  # ends with best()
        with torch.no_grad():
            e = closure()
        return e.cpu().numpy(), keep[0].detach(), keep[1].detach(), {k: _host(v) for k, v in st.items()}, torch.stack(trail).cpu().numpy()

    e32, pts32, shared32, st, trail = gpu_fit(fs["target64"])
    err32, beta32 = seq_errors(pts32, shared32, fs)
    print("MI355X: L-BFGS after %d evaluations %s, landmark error %s mm, |beta - beta_true| %s, status %s, iterations %s" %
          (B, e32, err32, beta32, st["status"], st["iterations"]))
    assert (st["evaluations"] == B).all() and np.allclose(e32, st["f_best"], rtol=1e-5)
    assert (trail[:, 6, 10:] == 0).all() and (trail[:, 11, 10:] == 0).all()  # the unused coordinates of the beta rows never move
    assert (e32 <= 2 * f64 + 1e-6).all(), (e32, f64)
    assert (err32 <= 2 * err64).all(), (err32, err64)
    assert (beta32 <= 2 * beta64).all(), (beta32, beta64)

    # NaN detections in the T = 4 sequence: that problem stops at its first evaluation with its rows untouched, and the T = 6 problem's
    # whole trajectory keeps its bits
    target = fs["target64"].clone()
    target[SEQ_T[0]:, :, :2] = float("nan")
    _, _, _, st2, trail2 = gpu_fit(target)
    assert st2["status"][1] == 4 and st2["evaluations"][1] == 1 and (trail2[:, 7:] == 0).all()
    assert st2["evaluations"][0] == B and _same(trail2[:, :7], trail[:, :7])
