"""The four stage calls (smplpp_stage_blend_shape / _joint_regression / _world_transformation / _skinning, csrc/stages.hip) against
the float64 statement of each stage (tests/stage_oracle.py), every element of every output, at the shapes where their kernels
take another path: the 207-term wavefront reduction with a partial last workgroup, the 256-thread strided regression loop on
either side of 256, the per-frame chain on four trees and on either side of a 64-frame workgroup, the homogeneous divide with a
bottom row that is not (0,0,0,1).  Each stage gets independent random inputs, never another stage's GPU output.

Bar, per output array, with E(x) = max_i |x_i - ref64_i| / max_i |ref64_i|:   E(gpu) <= max(4 E(fp32 oracle), 4 * 2^-24),
the project's "4 x an fp32 evaluation of the same graph" taken by elementwise maximum, so one wrong element cannot hide in a norm.
The fp32 oracle's own E on these cases is printed by tests/test_stage_oracle_cpu.py; each test here prints both figures."""
import numpy as np
import pytest

import stage_oracle as so

pytestmark = pytest.mark.gpu


def _held(name, gpu, ref64, ref32):
    assert gpu.dtype == np.float32 and gpu.shape == ref64.shape
    assert np.isfinite(gpu).all(), name
    e, e32 = so.scaled_error(gpu, ref64), so.scaled_error(ref32, ref64)
    print("%-40s E(gpu) = %.3g (%.2f x 2^-24)   E(fp32 oracle) = %.3g (%.2f x 2^-24)" % (name, e, e / so.EPS32, e32, e32 / so.EPS32))
    assert e <= so.bar(e32), (name, e, e32)


@pytest.mark.parametrize("n,V,zero", [(n, V, False) for n, V in so.BLEND_SHAPES] + [(1, 1, True)])
def test_blend_shape(n, V, zero):
    from smplpp_amd import _lib
    from smplpp_amd import smpl as S
    from smplpp_amd._lib import HOST, check
    from smplpp_amd.smpl import _ptr

    c = so.blend_zero_case() if zero else so.blend_case(n, V)
    bs, bp, rot = S.stage_blend_shape(c["beta"], c["theta"], c["S"], c["P"])
    ref = {}
    for dt in (np.float64, np.float32):
        r = so.rodrigues(c["theta"], dt)
        ref[dt] = (r,) + so.blend(c["beta"], r, c["S"], c["P"], dt)
    name = "blend n=%d V=%d%s " % (n, V, " zero" if zero else "")
    _held(name + "rot", rot, ref[np.float64][0], ref[np.float32][0])
    _held(name + "Bs", bs, ref[np.float64][1], ref[np.float32][1])
    _held(name + "Bp", bp, ref[np.float64][2], ref[np.float32][2])
    assert c["zero_frames"] or n == 1
    for f in c["zero_frames"]:  # theta = 0: the rotation is EXACTLY the identity and the pose blend exactly 0
        assert np.array_equal(rot[f], np.tile(np.eye(3, dtype=np.float32), (24, 1, 1)))
        assert np.array_equal(bp[f], np.zeros((V, 3), np.float32))
    # pose_rot = NULL: the rotations live in memory of the call's own, and Bs, Bp keep their bits
    h = [np.full((n, V, 3), np.nan, np.float32), np.full((n, V, 3), np.nan, np.float32)]
    check(_lib.load().smplpp_stage_blend_shape(0, V, n, _ptr(c["beta"]), _ptr(c["theta"]), _ptr(c["S"]), _ptr(c["P"]), _ptr(h[0]),
                                               _ptr(h[1]), None, HOST, None))
    assert np.array_equal(h[0], bs) and np.array_equal(h[1], bp)


@pytest.mark.parametrize("V", so.REGRESS_V)
def test_joint_regression(V):
    from smplpp_amd import smpl as S

    c = so.regress_case(V)
    rest, joints = S.stage_joint_regression(c["T"], c["Jreg"], c["Bs"], c["Bp"])
    r64 = so.joint_regression(c["T"], c["Jreg"], c["Bs"], c["Bp"])
    r32 = so.joint_regression(c["T"], c["Jreg"], c["Bs"], c["Bp"], np.float32)
    _held("joint regression V=%d rest" % V, rest, r64[0], r32[0])
    _held("joint regression V=%d joints" % V, joints, r64[1], r32[1])
    # the joints are regressed from T + Bs: another pose blend moves the rest shape and leaves the joints' bits
    rest2, joints2 = S.stage_joint_regression(c["T"], c["Jreg"], c["Bs"], c["Bp2"])
    assert np.array_equal(joints2, joints) and not np.array_equal(rest2, rest)
    _held("joint regression V=%d rest (Bp2)" % V, rest2, so.joint_regression(c["T"], c["Jreg"], c["Bs"], c["Bp2"])[0],
          so.joint_regression(c["T"], c["Jreg"], c["Bs"], c["Bp2"], np.float32)[0])


@pytest.mark.parametrize("general", [False, True], ids=["rotations", "general"])
@pytest.mark.parametrize("tree", sorted(so.TREES))
@pytest.mark.parametrize("n", so.WORLD_N)
def test_world_transformation(n, tree, general):
    from smplpp_amd import smpl as S

    c = so.world_case(n, tree, general)
    out = S.stage_world_transformation(c["parent"], c["joints"], c["rot"])
    assert out.shape == (n, 24, 4, 4)
    _held("world n=%d %s %s" % (n, tree, "general" if general else "rotations"), out,
          so.world(c["parent"], c["joints"], c["rot"]), so.world(c["parent"], c["joints"], c["rot"], np.float32))
    assert np.array_equal(out[:, :, 3, :], np.broadcast_to(np.array([0, 0, 0, 1], np.float32), (n, 24, 4)))


def test_world_transformation_refuses_a_tree_out_of_order():
    from smplpp_amd import smpl as S
    from smplpp_amd._lib import SmplppError

    c = so.world_case(1, "smpl", False)
    for i, p in ((5, 5), (5, 9), (23, 24), (1, -1)):
        bad = c["parent"].copy()
        bad[i] = p
        with pytest.raises(SmplppError) as ei:
            S.stage_world_transformation(bad, c["joints"], c["rot"])
        assert ei.value.code == 1  # SMPLPP_ERR_INVALID
    S.stage_world_transformation(c["parent"], c["joints"], c["rot"])  # and the next call in order is served


@pytest.mark.parametrize("with_root", [True, False], ids=["root", "no_root"])
@pytest.mark.parametrize("n,V", so.SKIN_SHAPES)
def test_skinning(n, V, with_root):
    from smplpp_amd import smpl as S

    c = so.skin_case(n, V)
    root = c["root"] if with_root else None
    assert np.abs(c["W"].sum(axis=1) - 1).min() > 1 and np.abs(c["G"][..., 3, :3]).max() > 0.05
    out = S.stage_skinning(c["W"], c["rest"], c["G"], root)
    _held("skinning n=%d V=%d %s" % (n, V, "root" if with_root else "no root"), out,
          so.skinning(c["W"], c["rest"], c["G"], root), so.skinning(c["W"], c["rest"], c["G"], root, np.float32))
