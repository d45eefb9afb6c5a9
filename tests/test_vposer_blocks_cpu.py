"""The test of tests/test_vposer_blocks_gpu.py's yardsticks (tests/vposer_blocks.py), without a GPU: the float64 reference against
the two torch restatements, the fp32 and fp16x2 oracles through every case (their block-scaled errors, printed in units of 2^-24
with -s, size the bars the kernels are held to), the slope margins (64 x the fp16x2 oracle's pre-activation error per case, layer
and frame; the same slopes in all three oracles; at most 10 % of the draws replaced), the caps of the conditioned cases
(64 x 2^-24 on both outputs), the crafted decoders' slope patterns and scales, the margins of the stand-alone conversion's rows,
and three planted errors that show what the block bar catches.

Measured here (units of 2^-24; fp16x2 oracle out / jac, fp32 oracle out / jac, then the old figure max|d| / max(1, max|jac|)):
    dense n = 1, 2, 3      0.1-0.5 / 8.7     0.1-0.4 / 13.4     7e-9
    dense n = 64           1.0 / 12.9        1.1 / 17.1         1.0e-8
    dense n = 257, 258     1.1 / 13.5        1.3 / 17.5         1.3e-8
    scale 1e-3, 0.3, 8     0.1-3.7 / 9.2-10.3   0.1-5.0 / 14.0-14.5
    scale mixed n = 257    19.5 / 35.5       21.2 / 132         9.2e-8
    mask slope 1 / 0.01    19.6 / 24.8 and 0.1 / 9.4            1.4e-7 and 1.0e-10
    range (no cap)         2.1 / 724         2.0 / 80           5.6e-7
    branch, joints 0, 14-20            0.6 / 12.4
    branch, joints 8-13 (no cap)       3.6e4 / 1.4e6     (2.2e-3 rad; the slab's own size)
    branch, joints 1-7, z ~ 1e-3       5.3 as rotations / 1353 up to sign;  z ~ 0.3: 1728 / 3.1e6 (0.18 of a slab)
    branch, z = 0                      joints 1-4 as rotations 2.3e4; joints 5-7 |out| by component 2.1; slabs 4-7 up to sign 556;
                                       slabs 1-3: 1e3 slab sizes in both oracles (finiteness only); 1-7 as ONE class: 1.6e7 / 1.8e10
    rotmat -> axis-angle rows          generic 6.0, towards pi 13.0 (65.4 with row 129), near-pi branch as vectors 7.8,
                                       exactly pi as rotations 427
Pre-activation error of the fp16x2 oracle: 8.4e-7 (layer 0) and 4.4e-7 (layer 1) at worst on the dense frames; margins and the
share of replaced draws: vposer_blocks.MARGINS (20 of 257 + 20 dense draws, 13 of 256 + 13 mixed ones, none in the small cases);
the measured errors against every case's margins are printed per case (64 x error / margin at worst 0.96, dense)."""
import functools

import numpy as np
import pytest

import vposer_blocks as B

U = B.EPS32
CUS = B.CUS_DEFAULT


def _conditioned():
    return ([B.dense_case(n) for n in B.dense_n(CUS)] + B.scale_cases(CUS) + B.mask_cases())


@functools.lru_cache(maxsize=None)
def _all_cases():
    return _conditioned() + B.shard_cases(CUS) + [B.range_case(), B.branch_case()]


def _ids(cases):
    return [c["name"].replace(" ", "_") for c in cases]


# ------------------------------------------------------------------------------------------------ the float64 reference
def test_float64_reference_against_the_torch_restatements():
    """plain_oracle in float64 = oracle/vposer_torch.py's decoder in float64 (value) and tests/vposer_jac_oracle.jacobian
    (autograd through the whole graph), to 1e-12 of a block's scale, on dense latents and on the branch-point decoder."""
    import torch

    import vposer_jac_oracle as JO
    import vposer_vjp_oracle as VO

    for case in (B.dense_case(3), B.scale_cases(CUS)[2], B.branch_case()):
        p = {k: B.decoder(case["decoder"])[k] for k in B.KEYS}
        dec = VO.decoder(p)
        out = dec(torch.as_tensor(case["z"], dtype=torch.float64)).detach().numpy()
        jac = JO.jacobian(dec, case["z"])
        r64 = B.references(case)[0]
        js = B.PLAIN_JOINTS if case["decoder"] == "branch" else list(range(21))
        eo, ej = B.out_blocks(r64["out"], out)[:, js].max(), B.jac_blocks(r64["jac"], jac)[:, js].max()
        print("%-20s float64 numpy + tail against torch autograd: out %.3g rad, jac %.3g of a slab" % (case["name"], eo, ej))
        assert eo <= 1e-12 and ej <= 1e-12, (case["name"], eo, ej)
        if case["decoder"] == "branch":
            # at and beside pi sqrt(s + eps) multiplies the float64 rounding of the two summation orders by up to 1e7
            js = B.NEAR_PI_JOINTS + B.PI_JOINTS
            eo, ej = B.out_blocks(r64["out"], out)[:, js].max(), B.jac_blocks(r64["jac"], jac)[:, js].max()
            print("%-20s the same on joints 1-13: out %.3g rad, jac %.3g of a slab" % (case["name"], eo, ej))
            assert eo <= 1e-12 and ej <= 1e-7, (case["name"], eo, ej)


# ------------------------------------------------------------------------------------------------ the metric, pinned
def test_block_metrics_are_the_stated_ones():
    ref = np.zeros((1, 63, 32))
    ref[0, 0:3] = 2.0
    ref[0, 3:6] = 1e-3
    x = ref.copy()
    x[0, 4, 7] += 1e-6   # 1e-3 of its own slab, 5e-7 of the frame
    assert B.jac_blocks(x, ref).shape == (1, 21)
    assert B.jac_blocks(x, ref)[0, 1] == pytest.approx(1e-3) and B.jac_blocks(x, ref)[0, 0] == 0
    assert B.old_figure(x, ref) == pytest.approx(5e-7)
    assert B.jac_blocks(x, ref)[0, 2] == 0  # an all-zero slab, exactly zero
    x[0, 8, 0] = 1e-30
    assert B.jac_blocks(x, ref)[0, 2] == np.inf
    x[0, 8, 0] = 0
    y = ref.copy()
    y[0, 1] = -y[0, 1]  # one row of a slab with the other sign
    assert B.jac_blocks(y, ref)[0, 0] == 2.0 and B.jac_blocks_up_to_sign(y, ref)[0, 0] == 0
    y[0, 1, 3] = 0.0    # (not a sign: half a row cannot flip)
    assert B.jac_blocks_up_to_sign(y, ref)[0, 0] == 1.0
    aa = np.array([[0.0, 0, 0], [np.pi, 0, 0], [0.3, -0.2, 0.1]])
    from scipy.spatial.transform import Rotation

    assert np.abs(B.rotation(aa) - Rotation.from_rotvec(aa).as_matrix()).max() < 1e-15
    assert B.rot_blocks([[np.pi, 0, 0]], [[-np.pi, 0, 0]])[0] < 1e-15 and B.out_blocks([[np.pi, 0, 0]], [[-np.pi, 0, 0]])[0] > 6
    assert B.out_blocks([[np.nan, 0, 0]], [[0.0, 0, 0]])[0] == np.inf and B.rot_blocks([[np.nan, 0, 0]], [[0.0, 0, 0]])[0] == np.inf
    assert B.bar(0.0) == 4 * U and B.bar(1e-6) == 4e-6 and B.CAP == 64 * U


# ------------------------------------------------------------------------------------------------ the fp16x2 pieces
def test_fp16x2_pieces_scales_and_subnormals():
    hi, lo = B.split_f16x2(np.array([1000.123, 3.0e-5, 0.1, 16383.9], np.float32))
    assert hi[0] == 1000.0 and abs(hi[0] + lo[0] - np.float32(1000.123)) < 2.0 ** -14
    assert 0 < hi[1] < 2.0 ** -14 and hi[1] == np.round(3.0e-5 * 2 ** 24) / 2 ** 24  # a subnormal hi piece is kept
    assert lo[2] != 0 and abs(lo[2]) < 2.0 ** -14                                     # and so is a subnormal lo piece
    assert lo[2] == np.round((float(np.float32(0.1)) - hi[2]) * 2 ** 24) / 2 ** 24
    assert hi[3] == 16384.0 and lo[3] < 0
    assert B.pow2_under(16384, 1.0) == 16384.0 and B.pow2_under(16384, 1.0001) == 8192.0 and B.pow2_under(16384, 0.0) > 1e30
    p, q = B.decoder("synth"), B.decoder("range")
    s, t = B.scales_of(p), B.scales_of(q)
    m0, m1, m2 = (float(np.abs(p[k]).max()) for k in (B.KEYS[0], B.KEYS[2], B.KEYS[4]))
    for scale, m in zip(s, (m1, m2, m0, 512 * m1 * m0)):
        assert 8192 < scale * m <= 16384 and np.log2(scale) == np.round(np.log2(scale))
    # one entry of each matrix x 2^8: the weight scales drop by 7 or 8 octaves (the entry need not have been the largest), sD2 by
    # 15 or 16: the tangent block T1 sD2, at a few hundred in the synthetic decoder, lies under 2^-6, and the lo pieces of close to half
    # its entries are non-zero fp16 subnormals, against a seventh (rows of slope 0.01) in the synthetic decoder (a matrix pipe that
    # flushed them would leave 11 bits)
    r = [a / b for a, b in zip(s, t)]
    assert all(x in (128.0, 256.0) for x in r[:3]) and r[3] == r[0] * r[2], r
    for which, scale, lo_share, hi_share in (("range", t[3], 0.4, 1.0), ("synth", s[3], 0.0, 0.2)):
        case = B.range_case() if which == "range" else B.dense_case(3)
        _, lo = B.split_f16x2(B.references(case)[2]["T1"] * np.float32(scale))
        sub = ((lo != 0) & (np.abs(lo) < 2.0 ** -14)).mean()
        assert lo_share <= sub <= hi_share, (which, sub)


# ------------------------------------------------------------------------------------------------ margins, slopes, yardsticks
@pytest.mark.parametrize("case", _all_cases(), ids=_ids(_all_cases()))
def test_margins_slopes_and_yardsticks(case):
    p = B.decoder(case["decoder"])
    r64, r32, r16 = B.references(case)
    n = len(case["z"])
    # the draws: at most 10 % replaced; every kept frame (z = 0 included) clears its margins in float64
    draws = n - (1 if case["frame_scales"][0] == 0.0 else 0) + case["replaced"]
    assert case["replaced"] <= 0.1 * draws, (case["name"], case["replaced"], draws)
    m = np.array([B.margins(case["decoder"], s) for s in case["frame_scales"]])
    mh = B.min_preactivation(p, case["z"])
    assert (mh >= m).all(), (case["name"], np.nonzero(mh < m))
    if case["name"].startswith(("dense", "shard")):
        assert not case["z"][0].any() and case["frame_scales"][0] == 0.0
    # 64 x the fp16x2 oracle's pre-activation error <= the margin, per layer and frame; the same slopes in the three oracles
    err = np.stack([np.abs(r16[k] - r64[k]).max(axis=1) for k in ("h0", "h1")], axis=1)
    print("%-22s replaced %d of %d draws; fp16x2 pre-activation error %.3g / %.3g (layers 0 / 1), 64 x error / margin at worst %.2f"
          % (case["name"], case["replaced"], draws, err[:, 0].max(), err[:, 1].max(), (64 * err / m).max()))
    assert (64 * err <= m).all(), (case["name"], (64 * err / m).max())
    for r in (r32, r16):
        for k in ("h0", "h1"):
            assert np.array_equal(r[k] > 0, r64[k] > 0), (case["name"], k)
    # the yardsticks
    assert all(np.isfinite(r[k]).all() for r in (r64, r32, r16) for k in ("out", "jac"))
    (eo16, ej16), (eo32, ej32) = B.figures(r16, r64), B.figures(r32, r64)
    print("%-22s fp16x2 oracle out %.1f jac %.1f   fp32 oracle out %.1f jac %.1f (x 2^-24)   old figure %.3g"
          % (case["name"], eo16 / U, ej16 / U, eo32 / U, ej32 / U, B.old_figure(r16["jac"], r64["jac"])))
    if case["capped"]:
        assert max(eo16, ej16, eo32) <= B.CAP, (case["name"], eo16 / U, ej16 / U, eo32 / U)
        assert not (np.abs(r64["jac"]).reshape(n, 21, -1).max(axis=2) == 0).any()


def test_the_dense_cases_share_one_stream_and_the_two_frame_cases_are_odd_and_even():
    ns = B.dense_n(CUS)
    assert ns == [1, 2, 3, 64, CUS + 1, CUS + 2] and (CUS + 1) % 2 == 1
    big = B.dense_case(ns[-1])["z"]
    for n in ns:
        assert np.array_equal(B.dense_case(n)["z"], big[:n])
    # 64 frames, one per workgroup, walk all 32 rotations 5 x (f / 2) mod 32
    assert sorted({(5 * (f // 2)) & 31 for f in range(64)}) == list(range(32))
    a, b = B.shard_cases(CUS)
    assert a["frame_base"] == 1 and len(a["z"]) == CUS + 1 and b["frame_base"] == 2 ** 31 + 1 and len(b["z"]) == 3
    # the twins: the same groups modulo 32 behind `twin_base` dummy frames at base 0
    for c in (a, b):
        assert all(((c["frame_base"] + f) // 2 - (c["twin_base"] + f) // 2) % 32 == 0 for f in range(len(c["z"])))
        assert c["frame_base"] % 2 == c["twin_base"] % 2


def test_the_mixed_batch_puts_all_three_scales_into_neighbouring_frames():
    c = B.scale_cases(CUS)[3]
    fs = c["frame_scales"]
    pairs = {(fs[f], fs[f + 1]) for f in range(0, len(fs) - 1, 2)}  # the two frames of a workgroup
    assert {(1e-3, 0.3), (8.0, 1e-3), (0.3, 8.0)} <= pairs
    r64 = B.references(c)[0]
    a0 = np.abs(r64["h0"]).max(axis=1)
    assert a0.max() / a0.min() > 2 ** 5  # (the biases keep the activations of a small latent at the biases' size)
    z = np.abs(c["z"]).max(axis=1)[1:]
    assert z.max() / z.min() > 2 ** 12


@pytest.mark.parametrize("i", [0, 1])
def test_mask_decoders_slope_patterns(i):
    c = B.mask_cases()[i]
    r64 = B.references(c)[0]
    assert ((r64["h0"] > 0) == (c["slope0"] == 1.0)).all()
    assert 0.2 < (r64["h1"] > 0).mean() < 0.8
    if c["slope0"] == 0.01:  # the Jacobian is the constant path alone: T1 = s1 (.) 0.01 W1 W0
        p = B.decoder(c["decoder"])
        W0, W1, W2 = (p[k].astype(np.float64) for k in (B.KEYS[0], B.KEYS[2], B.KEYS[4]))
        s1 = np.where(r64["h1"] > 0, 1.0, 0.01)
        T6 = np.einsum("ok,nk,kc->noc", W2, s1, 0.01 * (W1 @ W0))
        assert np.abs(T6 - r64["T6"]).max() <= 1e-12 * np.abs(T6).max()


def test_branch_point_joint_classes():
    """vposer_blocks.BRANCH_CLASSES: the yardstick of every class, printed; the classes of joints 1-7 have yardsticks an error can
    exceed (a rotation matrix's entries differ by at most 2, a slab up to sign by about 1: a yardstick near those holds nothing,
    which is what ONE class of joints 1-7 over the three frames has - 1 rad and 1e3 slabs, from frame 0 alone)."""
    c = B.branch_case()
    r64, r32, r16 = B.references(c)
    th = np.linalg.norm(r64["out"], axis=2)
    assert th[0, 0] < 1e-3 and (th[0, 14:20] < 2e-3).all() and abs(th[0, 20] - 0.7) < 1e-3
    assert (np.abs(th[0, 8:14] - np.pi) < 2e-3).all() and (np.abs(th[0, 1:8] - np.pi) < 1e-3).all()
    fig = {}
    for cls in B.BRANCH_CLASSES:
        f16, f32_ = B.figures(r16, r64, cls), B.figures(r32, r64, cls)
        fig[cls[4]] = f16
        print("branch %-12s out %-5s jac %-5s fp16x2 oracle out %s jac %s   fp32 oracle out %s   (x 2^-24)" % (
            cls[4], cls[2], cls[3], *("-" if v is None else "%.4g" % (v / U) for v in (f16[0], f16[1], f32_[0]))))
        assert all(v is None or np.isfinite(v) for v in f16 + f32_)
    assert max(fig["0, 14-20"]) <= B.CAP
    # every block of joints 1-7 is in a class, bar the slabs of joints 1-3 at z = 0 (finiteness only)
    held_out = {(f, j) for fr, js, ok, _, _ in B.BRANCH_CLASSES if ok for f in (fr or range(3)) for j in js}
    held_jac = {(f, j) for fr, js, _, jk, _ in B.BRANCH_CLASSES if jk for f in (fr or range(3)) for j in js}
    every = {(f, j) for f in range(3) for j in range(21)}
    assert held_out == every and every - held_jac == {(0, 1), (0, 2), (0, 3)}
    # bars that bite: out of joints 1-7 under 0.01 (rotation entries / radians), their slabs up to sign under 1
    for name in ("1-7 z~1e-3", "1-7 z~0.3", "1-4 z=0", "5-7 z=0", "4-7 z=0 jac"):
        eo, ej = fig[name]
        assert eo is None or B.bar(eo) < 0.01, (name, eo)
        assert ej is None or B.bar(ej) < 1.0, (name, ej)
    assert B.bar(fig["1-7 z~1e-3"][1]) < 1e-3 and B.bar(fig["4-7 z=0 jac"][1]) < 1e-3 and B.bar(fig["5-7 z=0"][0]) < 1e-6
    # what the one class would have been, and the slabs left at finiteness
    one = B.figures(r16, r64, (None, B.PI_JOINTS, "rot", "sign", ""))
    left = B.figures(r16, r64, ([0], [1, 2, 3], None, "sign", ""))[1]
    print("branch joints 1-7 as ONE class: out %.3g (rotation entries), jac %.3g slabs; slabs of joints 1-3 at z = 0 up to sign: %.3g"
          % (one[0], one[1], left))
    assert B.bar(one[0]) > 2 and B.bar(one[1]) > 1000 and left > 0.5


# ------------------------------------------------------------------------------------------------ rotmat -> axis-angle
def test_axis_angle_rows_clear_their_branch_thresholds():
    """The 129 rows are picked on purpose (vposer_blocks.aa_rows): distinct, about all three axes, 40 random, in four classes."""
    from test_oracle_vposer import sweep_matrices

    R, cls = B.aa_rows()
    assert R.shape == (129, 3, 3) and R.dtype == np.float32 and len({r.tobytes() for r in R}) == 129
    counts = np.bincount(cls, minlength=4)
    print("rotmat -> axis-angle rows by class %s: %s" % (B.AA_CLASSES, counts))
    assert (counts >= (60, 8, 12, 8)).all(), counts
    # all three axes in the structured rows, and the sweep's random rotations from the 128-thread block's last rows on
    S = sweep_matrices().astype(np.float32)
    rnd = {r.tobytes() for r in S[169:]}
    is_rnd = np.array([r.tobytes() in rnd for r in R])
    assert is_rnd.sum() >= B.AA_RANDOM and is_rnd[-B.AA_RANDOM:].all()
    for axis in range(3):  # a rotation about a coordinate axis keeps that axis: R[axis, axis] = 1 and angle neither 0 nor pi
        about = (R[:, axis, axis] == 1) & (np.abs(R - np.eye(3, dtype=np.float32)).max(axis=(1, 2)) > 0.5) & ~is_rnd
        assert about.sum() >= 6, (axis, about.sum())
    a, b, c = B.aa_predicates(R)
    pi = cls >= 2
    assert (np.abs(a) >= B.AA_MARGIN).all() and (np.abs(b)[~pi] >= B.AA_MARGIN).all()
    # (1 - eps) inside the acos keeps theta 4.9e-4 under pi: the third predicate is never near its threshold
    assert (c <= -3.5e-4).all()
    assert np.array_equal(pi, a < 0) and (b[~pi] < 0).sum() >= 8 and (b[~pi] > 0).sum() >= 60
    # an fp32 evaluation of the trace takes the same branches
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    assert np.array_equal(np.float32(1) + tr < np.float32(B.EPS ** 0.25), pi)
    a64, a32 = B.aa_reference(R.astype(np.float64)), B.aa_reference(R, "float32")
    for n in B.AA_N:
        e = B.aa_figures(a32[:n], a64[:n], cls[:n])
        print("rotmat -> axis-angle n=%d, fp32 oracle (x 2^-24): %s" % (n, ", ".join("%s %.1f" % (k, v / U) for k, v in zip(B.AA_CLASSES, e))))
        assert e[0] <= B.CAP and e[1] <= 128 * U and e[2] <= B.CAP and np.isfinite(e[3])


# ------------------------------------------------------------------------------------------------ the bar bites
def test_planted_errors_the_block_bar_refuses():
    """On the n = 64 dense case, into a copy of the fp16x2 oracle's Jacobian: (a) 1e-4 of its own size on one joint's slab of one
    frame; (b) the 0.01 C10 term left out of one 32-row tile of frame 0's layer-1 tangent block; (c) frame 1's layer-0 mask used
    for frame 0 in one row tile.  The old bar 2e-4 x max(1, max|jac|) accepts (a) and (b) (max|jac| is 0.02: the old bar was an
    absolute 2e-4, 1 % of the largest entry).  It refuses (c), in a whole row tile (4.4e-3) and even in a single 32 x 32 x 16 MFMA tile
    whose masks differ in three rows (3.8e-4): the two frames' masks differ in half their rows, so that departure from the issue's
    expectation is asserted as measured.  The block bar refuses all three by factors of 2e3 to 1e5."""
    case = B.dense_case(64)
    r64, _, r16 = B.references(case)
    p = B.decoder("synth")
    e = B.figures(r16, r64)[1]
    assert np.abs(r64["jac"]).max() < 1.0

    def held(x):
        old, E = B.old_figure(x, r64["jac"]), float(B.jac_blocks(x, r64["jac"]).max())
        return old, E

    a = r16["jac"].copy()
    a[5, 3 * 16:3 * 16 + 3] *= np.float32(1 + 1e-4)
    b = r16["jac"].copy()
    b[0] = B.fp16x2_oracle(p, case["z"][:2], ("no_c10", 7))["jac"][0]
    c = r16["jac"].copy()
    c[0] = B.fp16x2_oracle(p, case["z"][:2], ("next_mask", 7, None))["jac"][0]
    m = r64["h0"][:2] > 0
    c1 = r16["jac"].copy()
    c1[0] = B.fp16x2_oracle(p, case["z"][:2], ("next_mask", 7, 3))["jac"][0]
    assert (m[0, 48:64] != m[1, 48:64]).sum() == 3 and 200 < (m[0] != m[1]).sum() < 312
    figs = {}
    for name, x in (("a", a), ("b", b), ("c", c), ("c, one MFMA tile", c1)):
        figs[name] = held(x)
        print("planted (%s): old figure %.3g against 2e-4; block E %.1f against bar %.1f (x 2^-24)"
              % (name, figs[name][0], figs[name][1] / U, B.bar(e) / U))
    assert figs["a"][0] < 2e-4 and figs["a"][1] > 10 * B.bar(e)
    assert figs["b"][0] < 2e-4 and figs["b"][1] > 1000 * B.bar(e)
    assert figs["c"][0] > 2e-4 and figs["c"][1] > 1000 * B.bar(e)
    assert figs["c, one MFMA tile"][0] > 2e-4 and figs["c, one MFMA tile"][1] > 1000 * B.bar(e)
    assert held(r16["jac"])[1] == e <= B.bar(e)
