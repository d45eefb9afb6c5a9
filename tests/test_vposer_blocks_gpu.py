"""The VPoser decoder on the MI355X, value and Jacobian, held to float64 JOINT BY JOINT (tests/vposer_blocks.py): every (frame,
joint) 3-vector of `out` in absolute radians and every (frame, joint) 3 x 32 slab of d(out)/dz by its own largest entry, within
max(4 x the matching oracle's worst block of the case, 4 x 2^-24).  forward(z, want_jac=True) (vposer_jac2_kernel) against the
fp16x2 oracle's figure, forward(z) (the exact value kernel) against the fp32 oracle's; the value-only twin of the Jacobian kernel
is pinned to its bits by tests/test_vposer_gpu.py.  The cases: one and two frames per workgroup (n = 1, 2, 3, 64 and CUs + 1,
CUs + 2: every frame held), shards that start inside a group and past 2^31, latents over 13 octaves (6 of activation scale) alone
and mixed inside a workgroup, decoders whose layer-0 masks are all ones or all zeros, a decoder whose creation-time scales push
the lo pieces into fp16's subnormals, the axis-angle branch points, and the stand-alone smplpp_rotmat_to_axis_angle around its
128-thread block.  tests/test_vposer_blocks_cpu.py prints the yardsticks; this file prints the kernels' figures beside them (-s).

Measured on an MI355X (256 CUs), units of 2^-24, E of the kernel / yardstick e / bar:
    case family                        out (rad)            jac (of a slab)        value kernel out     old figure
    dense n = 1, 2, 3                  0.2-0.5 / 0.1-0.5 / 4    11.9-12.9 / 8.7 / 34.9   0.1-0.7 / 0.1-0.4 / 4    8e-9 - 1.1e-8
    dense n = 64                       1.3 / 1.0 / 4.2      21.3 / 12.9 / 51.6     0.9 / 1.1 / 4.3      1.9e-8
    dense n = CUs + 1, CUs + 2         1.3 / 1.1 / 4.2      21.3 / 13.5 / 53.9     1.2 / 1.3 / 5.1      1.9e-8
    shard CUs + 1 at 1, 3 at 2^31 + 1  1.2, 0.5 / 1.1, 0.5  19.2, 12.9 / 13.5, 8.7 as dense             1.5e-8, 9e-9
    scale 1e-3, 0.3, 8 (n = 6)         0.2, 0.2, 7.4 / 0.1, 0.2, 3.7   13.7, 11.9, 15.5 / 9.3, 10.3, 9.2   0.2, 0.3, 6.2 / 0.1, 0.2, 5.0
    scale mixed n = CUs + 1            28.1 / 19.5 / 77.9   69.2 / 35.5 / 142      33.2 / 21.2 / 84.6   1.7e-7
    mask, every slope 1                15.0 / 19.6 / 78.5   28.9 / 24.8 / 99.3     17.6 / 9.6 / 38.5    1.5e-7
    mask, every slope 0.01             0.1 / 0.1 / 4        10.7 / 9.4 / 37.6      0.1 / 0.1 / 4        1.6e-10
    range (no cap)                     1.5 / 2.1 / 8.5      722 / 724 / 2896       2.0 / 2.0 / 7.8      5.9e-7
    branch, joints 0, 14-20            0.6 / 0.6 / 4        10.8 / 12.4 / 49.5     0.6 / 0.6 / 4
    branch, joints 8-13 (no cap)       3.64e4 / 3.64e4      1.394e6 / 1.395e6      3.64e4 / 3.64e4      (2.2e-3 rad; 0.08 of a slab)
    branch, joints 1-7 at z ~ 1e-3     as rotations 5.3 / 5.3 / 21          up to sign 2378 / 1352 / 5407 (1.4e-4 of a slab)
    branch, joints 1-7 at z ~ 0.3      as rotations 1728 / 1728 / 6913 (1e-4)   up to sign 3.08e6 / 3.08e6 / 1.2e7 (0.18 of a slab, joints 1-3)
    branch, joints 1-4 at z = 0        as rotations 2.80e4 / 2.32e4 / 9.3e4 (1.7e-3; joint 2)
    branch, joints 5-7 at z = 0        |out| by component 2.1 / 4.0 / 15.9
    branch, joints 4-7 at z = 0                             up to sign 504 / 556 / 2225 (3e-5 of a slab)
    rotmat -> axis-angle n = 127, 128 (129): generic rows 6.0 / 6.0 / 24; towards pi 12.0 / 13.0 / 52 (17.4 / 65.4 / 262); on the
                                       near-pi branch, as vectors, 4.3 / 7.8 / 31; exactly pi, as rotations, 427 / 429 / 1716
Departures from "joints 1-7: R(out) against R(ref), the Jacobian up to sign" (vposer_blocks.BRANCH_CLASSES): joints 1-7 are exactly
at pi in frame 0 only, and ONE class over the three frames would take frame 0's yardstick - 0.98 in a rotation's entries, 1e3 slab
sizes - which nothing can miss; so the frames are held apart.  At z = 0 the float64 and fp32 sign fixes return DIFFERENT rotations
at joints 5-7 (single components of an oblique axis flipped), held by |out| component by component instead, and the slabs of
joints 1-3 (pi about a coordinate axis; the fp32 and fp16x2 oracles are themselves 1 to 1e3 slab sizes from float64, up to sign)
are held to finiteness ONLY.  The stand-alone conversion's rows on the near-pi branch keep the vector form unless they are exactly
pi (to 1e-6), and the generic rows beyond 2.4 rad carry a yardstick of their own (theta / (2 sin theta)).
The old figure is max|d jac| / max(1, max|jac|), which tests/test_vposer_gpu.py holds to 2e-4: max|jac| is 0.02 on the synthetic
decoder, so that bar was an absolute 2e-4, four orders above the kernel.  Slope margins and the share of replaced draws:
vposer_blocks.MARGINS (20 of 257 + 20 dense draws, 13 of 256 + 13 mixed ones, none in the cases of up to six frames).

Value-only mutations of a scratch copy of vposer_jac2_kernel, and what caught them (new = this file, every Jacobian case;
old = test_vposer_gpu.py, test_vposer_jac_exact_gpu.py, test_vposer_vjp_gpu.py without the two 512-frame IK runs):
    0.01 C10 -> 0.0101 C10                         new: E 3500-5300 against bars of 35-54; old: only test_vjp_parity's J^T g cross-check
                                                   (2e-4 of a frame's L2 norm, at n = 257 and 513; n = 1, 7, 64 pass), none of the Jacobian's own
    lo.hi product dropped in layer 2's tangents    new: E 5300-10300; old: test_vjp_parity[7, 64, 257, 513] alone (old figure 4e-6)
    lo piece of T1 zeroed                          new: E 5900-6100; old: test_vjp_parity[7, 64, 257, 513] alone (old figure 4e-6)
    layer-1 slopes of rows r and r + 256 swapped   new and old alike (a gross error: the old Jacobian bars, the latent IK rows)
    0.01 C10 dropped where NF = 2 only             new: the four cases of more frames than CUs (CUs + 1, CUs + 2, the shard at base 1, the mixed
                                                   scales) and no other; old: the two-frame and shard bit tests, test_vjp_parity[257, 513]
    lo piece of the activation vectors zeroed      new: every case, `out` included; old: test_decoder_forward_and_jacobian, the latent IK rows,
                                                   test_vjp_parity
In the first five the decoded angles are untouched and every `out` figure stays where it is.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vposer_blocks as B  # noqa: E402

pytestmark = pytest.mark.gpu
U = B.EPS32

_gpus = {}


def _gpu(which):
    """One decoder handle per parameter set for the module."""
    from smplpp_amd.ik import VPoserDecoder

    if which not in _gpus:
        _gpus[which] = VPoserDecoder({k: v.copy() for k, v in B.decoder(which).items()})
    return _gpus[which]


def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _decode(case, z=None, frame_base=None):
    gpu = _gpu(case["decoder"])
    z = case["z"] if z is None else z
    base = case["frame_base"] if frame_base is None else frame_base
    out, jac = gpu.forward(z, want_jac=True, frame_base=base)
    val = gpu.forward(z, frame_base=base)
    assert out.shape == (len(z), 21, 3) and jac.shape == (len(z), 63, 32) and val.shape == out.shape
    assert out.dtype == np.float32 and jac.dtype == np.float32 and val.dtype == np.float32
    return dict(out=out, jac=jac), dict(out=val, jac=None)


def _held(case, got=None, classes=(B.ALL,)):
    """forward(z, want_jac=True) within bar(fp16x2 oracle) and forward(z) within bar(fp32 oracle), per class of blocks (frames,
    joints, metric of out, metric of jac, name: vposer_blocks.BRANCH_CLASSES).  Prints every figure, then asserts."""
    r64, r32, r16 = B.references(case)
    full, val = _decode(case) if got is None else got
    bad = []
    for cls in classes:
        (eo, ej), (yo, yj) = B.figures(full, r64, cls), B.figures(r16, r64, cls)
        ev, yv = B.figures(val, r64, cls)[0], B.figures(r32, r64, cls)[0]
        rows = [(what, e, y) for what, e, y in (("out", eo, yo), ("jac", ej, yj), ("value kernel out", ev, yv)) if e is not None]
        print("%-22s %-12s %s  (x 2^-24)" % (case["name"], cls[4], " | ".join(
            "%s E %.4g e %.4g bar %.4g" % (what, e / U, y / U, B.bar(y) / U) for what, e, y in rows)))
        for what, e, y in rows:
            if not e <= B.bar(y):
                bad.append((case["name"], cls[4], what, e / U, B.bar(y) / U))
    print("%-22s old figure max|d jac| / max(1, max|jac|) = %.3g (fp16x2 oracle %.3g)"
          % (case["name"], B.old_figure(full["jac"], r64["jac"]), B.old_figure(r16["jac"], r64["jac"])))
    assert np.isfinite(full["out"]).all() and np.isfinite(full["jac"]).all() and np.isfinite(val["out"]).all(), case["name"]
    assert not bad, bad
    return full, val


# ---------------------------------------------------------------------------------------------- dense
@pytest.mark.parametrize("i", range(6), ids=["1", "2", "3", "64", "CUs+1", "CUs+2"])
def test_dense_every_frame_joint_by_joint(i):
    cus = _cus()
    n = B.dense_n(cus)[i]
    assert (n <= cus) if i < 4 else (n > cus and n == cus + i - 3), (n, cus)  # one frame per workgroup | two
    case = B.dense_case(n)
    assert len(case["z"]) == n and not case["z"][0].any()
    _held(case)


# ---------------------------------------------------------------------------------------------- shards
@pytest.mark.parametrize("i", [0, 1], ids=["CUs+1_at_1", "3_at_2^31+1"])
def test_shards_joint_by_joint_and_bit_equal_to_their_global_indices(i):
    """The result may not depend on the base (float64 knows none), and it is the bits of the same latents decoded at base 0
    behind `twin_base` dummy frames: the same instantiation, the same slot of the workgroup, the same group modulo 32."""
    cus = _cus()
    case = B.shard_cases(cus)[i]
    n = len(case["z"])
    assert (n > cus and case["frame_base"] == 1) if i == 0 else (n == 3 <= cus and case["frame_base"] == 2 ** 31 + 1)
    full, val = _held(case)
    t = case["twin_base"]
    zz = np.concatenate([np.full((t, 32), 0.25, np.float32), case["z"]])
    assert (len(zz) > cus) == (n > cus)
    twin, tval = _decode(case, zz, 0)
    assert np.array_equal(twin["out"][t:], full["out"]) and np.array_equal(twin["jac"][t:], full["jac"])
    assert np.array_equal(tval["out"][t:], val["out"])


# ---------------------------------------------------------------------------------------------- latent scale
@pytest.mark.parametrize("i", range(4), ids=["1e-3", "0.3", "8", "mixed"])
def test_latent_scales_joint_by_joint(i):
    cus = _cus()
    case = B.scale_cases(cus)[i]
    assert len(case["z"]) == (cus + 1 if i == 3 else B.SCALE_N)
    _held(case)


# ---------------------------------------------------------------------------------------------- masks, dynamic range
@pytest.mark.parametrize("i", [0, 1], ids=["slope1", "slope001"])
def test_layer0_masks_all_ones_and_all_zeros(i):
    _held(B.mask_cases()[i])


def test_lo_pieces_in_the_fp16_subnormals():
    """The yardstick is this decoder's own fp16x2 oracle (no cap: its Jacobian figure is some 700 x 2^-24); a matrix pipe that
    flushed fp16 subnormals would lose the lo pieces of half the tangent block and exceed it."""
    _held(B.range_case())


# ---------------------------------------------------------------------------------------------- branch points
def test_branch_points_by_joint_class():
    """vposer_blocks.BRANCH_CLASSES.  Joints 0, 14-19 (identity, near it) and 20 (generic): the plain bar.  8-13 (1e-4, 1e-3 rad
    below pi): their own yardstick.  1-7 (exactly pi at z = 0): at z ~ 1e-3 and z ~ 0.3, frame by frame, the decoded angles as
    rotations and the Jacobian up to the sign of each row; at z = 0 joints 1-4 as rotations, joints 5-7 - where one ulp flips single
    components of an oblique axis, which is another rotation - by |out| component by component, the slabs of joints 4-7 up to sign.
    The slabs of joints 1-3 at z = 0 are held to finiteness only (1 to 1e3 slab sizes in the oracles themselves)."""
    _held(B.branch_case(), classes=B.BRANCH_CLASSES)


# ---------------------------------------------------------------------------------------------- rotmat -> axis-angle
@pytest.fixture(scope="module")
def aa_rows():
    R, cls = B.aa_rows()
    return R, cls, B.aa_reference(R.astype(np.float64)), B.aa_reference(R, "float32")


@pytest.mark.parametrize("n", B.AA_N)
def test_rotmat_to_axis_angle_row_by_row(aa_rows, n):
    from smplpp_amd.ik import convertRotMatToAxisAngle

    R, cls, a64, a32 = aa_rows
    aa = convertRotMatToAxisAngle(R[:n])
    assert aa.shape == (n, 3) and aa.dtype == np.float32 and np.isfinite(aa).all()
    E, Y = B.aa_figures(aa, a64[:n], cls[:n]), B.aa_figures(a32[:n], a64[:n], cls[:n])
    print("rotmat -> axis-angle n=%d (x 2^-24): %s" % (n, " | ".join(
        "%s E %.4g e32 %.4g bar %.4g" % (k, e / U, y / U, B.bar(y) / U) for k, e, y in zip(B.AA_CLASSES, E, Y))))
    assert all(e <= B.bar(y) for e, y in zip(E, Y)), (n, [e / U for e in E])
