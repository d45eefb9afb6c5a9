"""Host-space calls stage their arguments through one arena per handle (csrc/staging.h): slot k holds the k-th staged argument of
whichever call runs.  What that sharing could break is checked here bit for bit against the same calls in device space, which stage
nothing: calls of different features back to back on one handle, an accumulating call behind a larger one, calls that leave
arguments out, a call behind a refused one, a solver and its model by turns, the decoder handle, and the handle-less calls that had
no host-versus-device comparison (the stage calls, the rotation conversion) and the sweep grid."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_raster_oracle as DR  # noqa: E402
from distance_cases import _same_bits  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(a):
    return a  # the converter of a host-space pass


def _flat(r):
    """The arrays of a result (array, tuple or dict; None left out) as numpy, in a fixed order."""
    if isinstance(r, dict):
        r = [r[k] for k in sorted(r)]
    elif not isinstance(r, (tuple, list)):
        r = [r]
    return [a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a) for a in r if a is not None]


def _assert_same(host, dev, what):
    h, d = _flat(host), _flat(dev)
    assert len(h) == len(d) and len(h) > 0, what
    for i, (a, b) in enumerate(zip(h, d)):
        assert a.dtype == b.dtype and _same_bits(a, b), (what, i, a.shape, b.shape)


def _new(synth_model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    return s


@pytest.fixture(scope="module")
def smpl(synth_model):
    return _new(synth_model)


def _verts(s, n, seed, scale=None):
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(n, seed=seed)
    if scale is not None:
        theta[:, 1:] = np.random.default_rng(seed).normal(0, scale, (n, 24, 3)).astype(np.float32)
    return s.launch(beta, theta, want=("verts",))["verts"]


def _cams(verts, H, W):
    return np.stack([DR.look_at_camera((v.min(0) + v.max(0)) / 2, 2.5, 0.3 * i, H, W) for i, v in enumerate(verts)]).astype(np.float32)


def _mask(rng, n, H, W):
    m = (rng.random((n, H, W)) < 0.4).astype(np.uint8)
    m[:, H // 2, W // 2] = 1
    return m


def _points(rng, verts, K):
    return (verts[:, rng.integers(0, verts.shape[1], K)] + rng.normal(0, 0.02, (len(verts), K, 3))).astype(np.float32)


def _pmd_step(s, v, p, g):
    def run(X):
        f, w, c, sq = s.pointMeshDistance(X(v), X(p))
        return (f, w, c, sq) + tuple(s.pointMeshDistanceBackward(X(v), X(p), f, X(g)))
    return run


def test_interleaved_features_on_one_handle(synth_model):
    """Large, then small, then large again at another size, every slot changing element type and length from call to call."""
    from smplpp_amd import model_io

    s = _new(synth_model)
    rng = np.random.default_rng(41)
    V = s.vertex_num
    v3, v1, v2, vsp = _verts(s, 3, 5), _verts(s, 1, 6), _verts(s, 2, 7), _verts(s, 2, 8, scale=0.9)
    p3, p1 = _points(rng, v3, 333), _points(rng, v1, 5)
    cam1, cam2 = _cams(v1, 12, 16), _cams(v2, 8, 8)
    gd, mask = rng.normal(0, 1, (1, 12, 16)).astype(np.float32), _mask(rng, 2, 8, 8)
    gvs, gps = rng.normal(0, 1, (2, V)).astype(np.float32), rng.normal(0, 1, (2, 8, 8)).astype(np.float32)
    ge = rng.normal(0, 1, (2, 64)).astype(np.float32)
    fk = {n: model_io.synthetic_inputs(n, seed=20 + n) + (rng.normal(0, 1, (n, V, 3)).astype(np.float32),
                                                         rng.normal(0, 1, (n, 24, 3)).astype(np.float32)) for n in (5, 1)}
    ids = np.array([0, V - 1, 7, 7, 3], np.int64)

    def raster(X):
        r = s.depthRaster(X(v1), cam1, 12, 16)
        return _flat(r) + [s.depthRasterBackward(X(v1), cam1, 12, 16, r["face"], X(gd))]

    def silhouette(X):
        o = s.silhouette(X(v2), cam2, 8, 8, mask)
        return _flat(o) + [s.silhouetteBackward(X(v2), cam2, 8, 8, o["face"], o["vert_target"], o["pix_source"], X(gvs), X(gps))]

    def selfpen(X):
        pairs, count, e = s.selfPenetration(X(vsp), max_pairs=64, check=False)
        return pairs, count, e, s.selfPenetrationBackward(X(vsp), pairs, count, X(ge))

    def launch(n):
        def run(X):
            beta, theta, gv, gj = fk[n]
            o = s.launch(X(beta), X(theta))
            a = s.launchBackward(X(beta), X(theta), X(gv), X(gj))
            b = s.launchBackward(X(beta), X(theta), X(gv), None, rest=o["rest"])
            return _flat(o) + _flat(a) + _flat(b)
        return run

    def queries(X):  # at the vertices of the launch before (n = 1)
        return (s.calcVertexNormalBatch(ids),) + tuple(s.closestPoints(X(p1)))

    steps = [("pmd 3x333", _pmd_step(s, v3, p3, rng.normal(0, 1, (3, 333)).astype(np.float32))), ("depth raster", raster),
             ("silhouette", silhouette), ("self penetration", selfpen), ("launch 5", launch(5)), ("launch 1", launch(1)),
             ("normals, closest points", queries), ("pmd 1x5", _pmd_step(s, v1, p1, rng.normal(0, 1, (1, 5)).astype(np.float32)))]
    dev = [run(_dev) for _, run in steps]
    torch.cuda.synchronize()
    host = [run(_host) for _, run in steps]
    for (name, _), h, d in zip(steps, host, dev):
        _assert_same(h, d, name)


def test_accumulate_behind_a_larger_call(smpl):
    """The output a call adds into is loaded through a slot that the call before left full of something else."""
    rng = np.random.default_rng(42)
    V = smpl.vertex_num
    v3, v1 = _verts(smpl, 3, 5), _verts(smpl, 1, 6)
    p3, cam = _points(rng, v3, 333), _cams(v1, 12, 16)
    face = smpl.depthRaster(v1, cam, 12, 16)["face"]
    gd, preset = rng.normal(0, 1, (1, 12, 16)).astype(np.float32), rng.normal(0, 1, (1, V, 3)).astype(np.float32)
    ids, gn = np.array([5, 0, V - 1], np.int64), rng.normal(0, 1, (1, 3, 3)).astype(np.float32)
    want = (smpl.depthRasterBackward(_dev(v1), cam, 12, 16, face, _dev(gd), out=_dev(preset)),
            smpl.calcVertexNormalBackward(_dev(v1), ids, _dev(gn), out=_dev(preset)))
    torch.cuda.synchronize()
    smpl.pointMeshDistance(v3, p3)
    got0 = smpl.depthRasterBackward(v1, cam, 12, 16, face, gd, out=preset.copy())
    smpl.pointMeshDistance(v3, p3)
    got1 = smpl.calcVertexNormalBackward(v1, ids, gn, out=preset.copy())
    _assert_same((got0, got1), want, "accumulate")
    assert not _same_bits(got0, preset)


def test_arguments_left_out(smpl):
    """An argument that is not given takes no slot: the ones behind it move up, and compute what they compute in the full call."""
    from smplpp_amd import _lib
    from smplpp_amd._lib import HOST, check
    from smplpp_amd.smpl import _ptr

    rng = np.random.default_rng(43)
    V = smpl.vertex_num
    v2 = _verts(smpl, 2, 7)
    cam, mask = _cams(v2, 8, 8), _mask(rng, 2, 8, 8)
    full = smpl.silhouette(v2, cam, 8, 8, mask)
    only = smpl.silhouette(v2, cam, 8, 8, mask, face=full["face"], want=("pix_sq",))
    assert set(only) == {"pix_sq", "face"} and _same_bits(only["pix_sq"], full["pix_sq"])
    _assert_same(only["pix_sq"], smpl.silhouette(_dev(v2), cam, 8, 8, mask, want=("pix_sq",))["pix_sq"], "pix_sq alone")
    gvs = rng.normal(0, 1, (2, V)).astype(np.float32)
    got = smpl.silhouetteBackward(v2, cam, 8, 8, full["face"], vert_target=full["vert_target"], grad_vert_sq=gvs)
    _assert_same(got, smpl.silhouetteBackward(_dev(v2), cam, 8, 8, full["face"], vert_target=full["vert_target"], grad_vert_sq=_dev(gvs)),
                 "vertex term alone")
    # the vertex term alone is the full call at a zero pixel cotangent (a zero cotangent contributes nothing)
    both = smpl.silhouetteBackward(v2, cam, 8, 8, full["face"], full["vert_target"], full["pix_source"], gvs, np.zeros((2, 8, 8), np.float32))
    assert np.array_equal(got, both)
    p2 = _points(rng, v2, 37)
    whole = smpl.pointMeshSignedDistance(v2, p2)
    face, w, ins, sq = np.empty((2, 37), np.int64), np.empty((2, 37, 3), np.float32), np.empty((2, 37), np.uint8), np.empty((2, 37), np.float32)
    check(_lib.load().smplpp_point_mesh_signed_distance(smpl.handle, 2, _ptr(v2), 37, _ptr(p2), _ptr(face), _ptr(w), None, None, _ptr(ins),
                                                        _ptr(sq), HOST, None))
    _assert_same((face, w, ins.astype(bool), sq), (whole[0], whole[1], whole[4], whole[5]), "signed distance without the optional outputs")
    _assert_same(whole, smpl.pointMeshSignedDistance(_dev(v2), _dev(p2)), "signed distance")


def test_a_valid_call_behind_a_refused_one(smpl, synth_model):
    """Behind a refusal in front of the staging (a face id past the mesh), and behind one in mid-call, with slots taken and uploads
    made (vertices that are not finite, which the sweep grid finds when it reads the bounds back)."""
    import ctypes as C

    from smplpp_amd import _lib
    from smplpp_amd._lib import HOST, SmplppError, check
    from smplpp_amd.smpl import _ptr

    rng = np.random.default_rng(44)
    v2 = _verts(smpl, 2, 7)
    p2, g = _points(rng, v2, 37), rng.normal(0, 1, (2, 37)).astype(np.float32)
    face = smpl.pointMeshDistance(v2, p2)[0]
    want = smpl.pointMeshDistanceBackward(_dev(v2), _dev(p2), face, _dev(g))
    bad = face.copy()
    bad[1, 3] = len(synth_model["face_indices"])  # = F, the first id past the mesh
    with pytest.raises(SmplppError, match="face id out of range"):
        smpl.pointMeshDistanceBackward(v2, p2, bad, g)
    _assert_same(smpl.pointMeshDistanceBackward(v2, p2, face, g), want, "behind a refusal")
    nan = v2[0].copy()
    nan[11, 1] = np.nan
    gmin, gnum, cells = np.zeros(3, np.int32), np.zeros(3, np.int32), C.c_int64(0)
    with pytest.raises(SmplppError, match="non-finite vertices"):
        check(_lib.load().smplpp_sweep_grid(smpl.handle, _ptr(nan), _ptr(gmin), _ptr(gnum), 0, None, None, C.byref(cells), HOST, None))
    _assert_same(smpl.pointMeshDistanceBackward(v2, p2, face, g), want, "behind a refusal in mid-call")


def test_solver_and_model_by_turns(synth_model):
    """The solver stages through an arena of its own: its host-space calls and its model's, by turns, against a second solver on the
    same model that is driven in device space."""
    from smplpp_amd import _lib
    from smplpp_amd._lib import DEVICE, check
    from smplpp_amd.ik import IkSolver, reference_task_faces
    from smplpp_amd.smpl import _ptr, _stream

    s = _new(synth_model)
    rng = np.random.default_rng(45)
    n, K, T = 2, 4, 3
    _, faces = reference_task_faces(K)
    theta0 = np.zeros((n, 25, 3), np.float32)
    theta0[:, 1:] = rng.normal(0, 0.05, (n, 24, 3))
    tp = rng.normal(0, 0.3, (T, n, K, 3)).astype(np.float32)
    valid = np.ones((T, n, K), np.uint8)
    v3 = _verts(s, 3, 5)
    p3 = _points(rng, v3, 333)
    model_want = s.pointMeshDistance(_dev(v3), _dev(p3))
    torch.cuda.synchronize()
    A, B = IkSolver(s, n, K), IkSolver(s, n, K)
    for solver in (A, B):
        solver.setTasks(face_idx=faces, target_pos=tp[0], phi_limit=np.zeros(K))
        solver.setConfig(np.zeros((n, 10), np.float32), theta0)
        if solver is A:
            _assert_same(s.pointMeshDistance(v3, p3), model_want, "model call behind setTasks")
    got = A.solveSequence(tp, valid, warmup_iters=3, iters_per_frame=1)
    _assert_same(s.pointMeshDistance(v3, p3), model_want, "model call behind solveSequence")
    tasks = A.getTasks()
    _assert_same(s.pointMeshDistance(v3, p3), model_want, "model call behind getTasks")
    L = _lib.load()
    tp_d, vl_d = _dev(tp), _dev(valid)
    th_d = torch.empty((T, n, 75), dtype=torch.float32, device="cuda")
    check(L.smplpp_ik_solve_sequence(B._h, T, _ptr(tp_d), _ptr(vl_d), 3, 1, 1, 0, _ptr(th_d), DEVICE, _stream()))
    torch.cuda.synchronize()
    _assert_same(got, th_d, "solveSequence")
    face_d = torch.empty((n, K), dtype=torch.int64, device="cuda")
    vw_d = torch.empty((n, K, 3), dtype=torch.float32, device="cuda")
    check(L.smplpp_ik_get_tasks(B._h, _ptr(face_d), _ptr(vw_d), None, None, None, DEVICE))
    torch.cuda.synchronize()
    _assert_same((tasks["face_idx"], tasks["vertex_weights"]), (face_d, vw_d), "getTasks")


def test_vposer_handle(synth_model):
    from smplpp_amd import _lib
    from smplpp_amd._lib import DEVICE, check
    from smplpp_amd.ik import VPoserDecoder
    from smplpp_amd.smpl import _ptr, _stream

    def empty(*shape):
        return torch.empty(shape, dtype=torch.float32, device="cuda")

    vp = VPoserDecoder(VPoserDecoder.synthetic_params())
    rng = np.random.default_rng(46)
    z, g = rng.normal(0, 1, (3, 32)).astype(np.float32), rng.normal(0, 1, (3, 21, 3)).astype(np.float32)

    host = (_flat(vp.forward(z, want_jac=True)) + _flat(vp.forward(z)) + _flat(vp.launchBackward(z, g, want_out=True))
            + _flat(vp.jacobian(z, want_out=True)) + _flat(vp.launchBackward(z, g)))
    L = _lib.load()
    zd, gd = _dev(z), _dev(g)
    out, jac, out1 = empty(3, 21, 3), empty(3, 63, 32), empty(3, 21, 3)
    check(L.smplpp_vposer_forward_at(vp._h, 3, 0, _ptr(zd), _ptr(out), _ptr(jac), DEVICE, _stream()))
    check(L.smplpp_vposer_forward_at(vp._h, 3, 0, _ptr(zd), _ptr(out1), None, DEVICE, _stream()))
    dev = ([out, jac, out1] + _flat(vp.launchBackward(zd, gd, want_out=True)) + _flat(vp.jacobian(zd, want_out=True))
           + _flat(vp.launchBackward(zd, gd)))
    torch.cuda.synchronize()
    _assert_same(host, dev, "vposer")


def test_handleless_calls():
    """The four stage calls and the rotation conversion stage through temporaries of the call."""
    from smplpp_amd import _lib
    from smplpp_amd import smpl as S
    from smplpp_amd._lib import DEVICE, HOST, check
    from smplpp_amd.ik import convertRotMatToAxisAngle
    from smplpp_amd.smpl import _ptr, _stream

    L = _lib.load()
    rng = np.random.default_rng(47)
    n, V = 3, 37

    def f32(*shape):
        return rng.normal(0, 1, shape).astype(np.float32)

    keep = []

    def dp(a):  # device pointer of a copy that lives to the end of the test
        keep.append(_dev(a))
        return _ptr(keep[-1])

    def empty(*shape):
        return torch.empty(shape, dtype=torch.float32, device="cuda")

    beta, theta24, Sb, Pb = f32(n, 10), f32(n, 24, 3), f32(V, 3, 10), f32(V, 3, 207)
    bs, bp, rot = S.stage_blend_shape(beta, theta24, Sb, Pb)
    d = [empty(n, V, 3), empty(n, V, 3), empty(n, 24, 3, 3)]
    check(L.smplpp_stage_blend_shape(0, V, n, dp(beta), dp(theta24), dp(Sb), dp(Pb), _ptr(d[0]), _ptr(d[1]),
                                     _ptr(d[2]), DEVICE, _stream()))
    _assert_same((bs, bp, rot), d, "blend shape")
    # without pose_rot the rotations live in device memory of the call's own, in either space
    h2 = [np.empty((n, V, 3), np.float32), np.empty((n, V, 3), np.float32)]
    check(L.smplpp_stage_blend_shape(0, V, n, _ptr(beta), _ptr(theta24), _ptr(Sb), _ptr(Pb), _ptr(h2[0]), _ptr(h2[1]), None, HOST, None))
    d2 = [empty(n, V, 3), empty(n, V, 3)]
    check(L.smplpp_stage_blend_shape(0, V, n, dp(beta), dp(theta24), dp(Sb), dp(Pb), _ptr(d2[0]), _ptr(d2[1]),
                                     None, DEVICE, _stream()))
    _assert_same(h2, d2, "blend shape without pose_rot")
    _assert_same(h2, (bs, bp), "blend shape without pose_rot")
    Tm, Jreg = f32(V, 3), f32(24, V)
    rest, joints = S.stage_joint_regression(Tm, Jreg, bs, bp)
    d = [empty(n, V, 3), empty(n, 24, 3)]
    check(L.smplpp_stage_joint_regression(0, V, n, dp(Tm), dp(Jreg), dp(bs), dp(bp), _ptr(d[0]), _ptr(d[1]),
                                          DEVICE, _stream()))
    _assert_same((rest, joints), d, "joint regression")
    kintree = np.maximum(0, (np.arange(24) - 1) // 2).astype(np.int64)
    xf = S.stage_world_transformation(kintree, joints, rot)
    d = empty(n, 24, 4, 4)
    check(L.smplpp_stage_world_transformation(0, n, _ptr(kintree), dp(joints), dp(rot), _ptr(d), DEVICE, _stream()))
    _assert_same(xf, d, "world transformation")
    W, root = np.abs(f32(V, 24)), f32(n, 3)
    out = S.stage_skinning(W, rest, xf, root)
    d = empty(n, V, 3)
    check(L.smplpp_stage_skinning(0, V, n, dp(W), dp(rest), dp(xf), dp(root), _ptr(d), DEVICE, _stream()))
    _assert_same(out, d, "skinning")
    aa = convertRotMatToAxisAngle(rot)
    d = empty(n * 24, 3)
    check(L.smplpp_rotmat_to_axis_angle(0, n * 24, dp(rot), _ptr(d), DEVICE, _stream()))
    _assert_same(aa, d, "rotmat to axis angle")


def test_sweep_grid_spaces(smpl):
    from smplpp_amd import model_io

    beta, theta = model_io.synthetic_inputs(2, seed=9)
    smpl.launch(_dev(beta), _dev(theta), want=("verts",))
    dev = smpl.calcSweepGrid(frame=1)
    smpl.launch(beta, theta, want=("verts",))
    host = smpl.calcSweepGrid(frame=1)
    assert host["winding"].size > 0
    _assert_same(host, dev, "sweep grid")
