"""The block-scaled bar of the VPoser decoder smplpp_vposer_forward (value and d(out)/dz) and of smplpp_rotmat_to_axis_angle, and
the cases it is asserted on (tests/test_vposer_blocks_cpu.py runs the oracles through them, tests/test_vposer_blocks_gpu.py the
kernels).

    output           block                             scale
    out [n,21,3]     each (frame, joint) 3-vector      1 (absolute radians)
    jac [n,63,32]    each (frame, joint) 3 x 32 slab   the slab's largest float64 entry

E = the maximum over ALL blocks of ALL frames of a case, held to bar(e) = max(4 e, 4 x 2^-24) (stage_oracle.bar), e the E of the
MATCHING ORACLE on the same case: the worst block of the case, never a per-block yardstick.  Three statements of the decoder:

    float64   the reference: the MLP and its tangents T6 = W2 diag(s1) W1 diag(s0) W0 analytic in numpy, the rotation tail
              (Gram-Schmidt, convertRotMatToAxisAngle) and its 3 x 6 Jacobian by the torch restatement (oracle/vposer_torch.py).
    fp32      the same graph in float32: the yardstick of the exact value kernel vposer_kernel<false> (forward(z)).
    fp16x2    what the header comment of smplpp_amd/csrc/vposer.hip and smplpp_vposer_create promise (not the kernel's lane
              layout): creation-time scales pow2_under(16384, .), a per-frame activation scale just under 2^14, every operand as
              hi = fp16(x), lo = fp16(x - hi) (subnormals kept), hi.hi + hi.lo + lo.hi per product, accumulated in fp32 once per
              16-wide k-step and piece, layer 0 in fp32, C10 = fp32(W1 W0 in double), T1 = s1 (.) (0.01 C10 + 0.99 acc) formed
              in fp32 and split again at sD2, the tail in fp32: the yardstick of vposer_jac2_kernel (forward(z, want_jac=True)).

A LeakyReLU slope may legitimately differ from float64 where a pre-activation is within rounding of zero, so a latent enters a case
only if every float64 pre-activation of both hidden layers has |h| >= the margin of its layer and scale (MARGINS, `margins`); one
that fails is redrawn from the same seeded stream, so every frame of every batch is still checked.

numpy only at import; the tail (torch) and the branch-point decoder (scipy, torch) are imported when they are called."""
import numpy as np

from stage_oracle import EPS32, bar  # noqa: F401  (bar(e) = max(4 e, 4 x 2^-24); restated nowhere else)
from vjp_blocks import block_errors

HID, LAT, OUT6 = 512, 32, 126
CAP = 64 * EPS32  # the conditioned cases' yardsticks stay under it (tests/test_vposer_blocks_cpu.py)
# The slope margins (layer 0, layer 1) by the scale s of a latent s x N(0,1): 64 x the fp16x2 oracle's worst pre-activation error
# against float64 in that layer, over 1000 such latents of the synthetic decoder and over the frames of the cases below, rounded
# up.  Measured errors (layer 0, layer 1): s = 1e-3: 1.0e-7, 8.4e-8; 0.3: 2.7e-7, 2.1e-7; 1: 8.4e-7, 5.0e-7; 8: 4.6e-6, 4.1e-6 - the
# error grows with the size of a layer's inputs, and the worst of some 10^6 rows is ten times the median's thirty-fold.  5 to 10 %
# of the latents of a scale have a pre-activation inside their margins; one absolute margin for all would turn away a third of
# the small latents, whose pre-activations crowd around the biases.  z = 0 holds the s = 1 margins.  The hidden layers of the
# crafted decoders whose inputs are 4 to 40 instead of about 1 hold 3 to 10 x as much, layer 1 of "slope001" (inputs of 0.04) a
# tenth (MARGIN_FACTORS).  tests/test_vposer_blocks_cpu.py prints the errors and asserts 64 x error <= margin per case, layer
# and frame.  Under the 10 % rule a case of five or six frames can lose no draw, one of 64 at most seven: about every other seed
# holds it, and the cases' seeds are among those (the CPU test asserts it).  The fit is close (64 x error / margin reaches 0.96 on
# the dense frames): after a change to synthetic_params() or to the streams the CPU assertions trip first, and `measured_margins`
# (at the end of this file) says how the numbers are re-derived.
MARGINS = {0.0: (5.6e-5, 3.4e-5), 1e-3: (7.0e-6, 5.8e-6), 0.3: (1.8e-5, 1.4e-5), 1.0: (5.6e-5, 3.4e-5), 8.0: (3.1e-4, 2.8e-4)}
MARGIN_FACTORS = {"slope1": (4.0, 10.0), "slope001": (4.0, 0.1), "range": (3.0, 3.0)}
CUS_DEFAULT = 256  # compute units of an MI355X: what the CPU test takes for the cases cut at "more frames than CUs"
KEYS = ("decoder_net.0.weight", "decoder_net.0.bias", "decoder_net.3.weight", "decoder_net.3.bias", "decoder_net.5.weight",
        "decoder_net.5.bias")
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the metric
def out_blocks(x, ref64):
    """[n,21]: max |x - ref| of each (frame, joint) 3-vector, in radians; inf where x is not finite."""
    d = np.abs(np.asarray(x, np.float64) - np.asarray(ref64, np.float64)).max(axis=-1)
    return np.where(np.isfinite(d), d, np.inf)


def jac_blocks(x, ref64):
    """[n,21]: max |x - ref| / max |ref| of each (frame, joint) 3 x 32 slab; a slab whose reference is zero must be exactly zero."""
    x, ref64 = np.asarray(x, np.float64), np.asarray(ref64, np.float64)
    return block_errors(x.reshape(-1, 21, 3, LAT), ref64.reshape(-1, 21, 3, LAT), (2, 3))


def jac_blocks_up_to_sign(x, ref64):
    """jac_blocks where each of a slab's three rows may carry either sign (at a rotation by pi one ulp picks the axis's sign)."""
    x, r = np.asarray(x, np.float64).reshape(-1, 21, 3, LAT), np.asarray(ref64, np.float64).reshape(-1, 21, 3, LAT)
    err = np.minimum(np.abs(x - r).max(axis=3), np.abs(x + r).max(axis=3)).max(axis=2)
    scale = np.abs(r).max(axis=(2, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale == 0, np.where(np.abs(x).max(axis=(2, 3)) == 0, 0.0, np.inf), err / scale)
    return np.where(np.isfinite(err), e, np.inf)


def rotation(aa):
    """[..., 3] axis-angle -> [..., 3, 3] in float64 (Rodrigues with sin(t)/t and (1 - cos t)/t^2 by series under 1e-4)."""
    aa = np.asarray(aa, np.float64)
    t2 = (aa * aa).sum(-1)
    t = np.sqrt(t2)
    small = t < 1e-4
    ts = np.where(small, 1.0, t)
    a = np.where(small, 1 - t2 / 6, np.sin(ts) / ts)[..., None, None]
    b = np.where(small, 0.5 - t2 / 24, (1 - np.cos(ts)) / (ts * ts))[..., None, None]
    z = np.zeros_like(t)
    K = np.stack([z, -aa[..., 2], aa[..., 1], aa[..., 2], z, -aa[..., 0], -aa[..., 1], aa[..., 0], z], -1).reshape(aa.shape[:-1] + (3, 3))
    return np.eye(3) + a * K + b * (K @ K)


def rot_blocks(x, ref64):
    """max |R(x) - R(ref)| per 3-vector: the decoded angles held as rotations."""
    d = np.abs(rotation(x) - rotation(ref64)).max(axis=(-2, -1))
    return np.where(np.isfinite(d), d, np.inf)


def old_figure(jac, ref64):
    """max |d| / max |jac|: the first-round figure of tests/test_vposer_gpu.py (bar 2e-4), over the whole batch."""
    ref64 = np.asarray(ref64, np.float64)
    return float(np.abs(np.asarray(jac, np.float64) - ref64).max() / max(1.0, np.abs(ref64).max()))


# ------------------------------------------------------------------------------------------------ the rotation tail (torch)
def tail(o6, dtype="float64"):
    """o6 [N,6] -> (aa [N,3], d aa / d o6 [N,3,6]) by the torch restatement of Gram-Schmidt and convertRotMatToAxisAngle in `dtype`."""
    import torch

    from oracle import vposer_torch as VT

    x = torch.as_tensor(np.ascontiguousarray(o6), dtype=getattr(torch, dtype)).clone().requires_grad_(True)
    aa = VT.convert_rotmat_to_axis_angle(VT.continuous_rot_repr_decoder(x))
    J = torch.stack([torch.autograd.grad(aa[:, i].sum(), x, retain_graph=True)[0] for i in range(3)], dim=1)
    return aa.detach().numpy(), J.detach().numpy()


def _through_tail(o6, T6, dtype):
    """o6 [n,126], T6 [n,126,32] -> (out [n,21,3], jac [n,63,32]) in `dtype` (numpy dtype)."""
    n = o6.shape[0]
    aa, J = tail(np.asarray(o6, dtype).reshape(n * 21, 6), np.dtype(dtype).name)
    jac = np.einsum("njik,njkc->njic", J.reshape(n, 21, 3, 6), np.asarray(T6, dtype).reshape(n, 21, 6, LAT))
    assert aa.dtype == dtype and jac.dtype == dtype
    return aa.reshape(n, 21, 3), jac.reshape(n, 63, LAT)


# ------------------------------------------------------------------------------------------------ float64 and fp32
def _weights(params, dtype):
    return [np.asarray(params[k], dtype) for k in KEYS]


def plain_oracle(params, z, dtype=np.float64):
    """The decoder and its Jacobian in `dtype` (float64: the reference; float32: the same graph in fp32).  dict(out [n,21,3],
    jac [n,63,32], h0, h1 [n,512] pre-activations, o6 [n,126], T6 [n,126,32])."""
    W0, b0, W1, b1, W2, b2 = _weights(params, dtype)
    z = np.asarray(z, dtype).reshape(-1, LAT)
    n = z.shape[0]
    one, leak = dtype(1), dtype(0.01)
    h0 = z @ W0.T + b0
    s0 = np.where(h0 > 0, one, leak)
    h1 = (h0 * s0) @ W1.T + b1
    s1 = np.where(h1 > 0, one, leak)
    o6 = (h1 * s1) @ W2.T + b2
    T0 = s0[:, :, None] * W0[None]                                            # [n,512,32]
    T1 = s1[:, :, None] * (W1 @ T0.transpose(1, 0, 2).reshape(HID, n * LAT)).reshape(HID, n, LAT).transpose(1, 0, 2)
    T6 = (W2 @ T1.transpose(1, 0, 2).reshape(HID, n * LAT)).reshape(OUT6, n, LAT).transpose(1, 0, 2)
    out, jac = _through_tail(o6, T6, dtype)
    assert h0.dtype == dtype and T6.dtype == dtype
    return dict(out=out, jac=jac, h0=h0, h1=h1, o6=o6, T6=T6)


def margins(which, scale=1.0):
    """(layer 0, layer 1): the margin a latent of `scale` x N(0,1) holds on decoder `which`."""
    f0, f1 = MARGIN_FACTORS.get(which, (1.0, 1.0))
    return MARGINS[scale][0] * f0, MARGINS[scale][1] * f1


def min_preactivation(params, z):
    """[n,2]: the smallest float64 |h| over the 512 rows of each hidden layer, per latent."""
    W0, b0, W1, b1, _, _ = _weights(params, np.float64)
    h0 = np.asarray(z, np.float64).reshape(-1, LAT) @ W0.T + b0
    h1 = (h0 * np.where(h0 > 0, 1.0, 0.01)) @ W1.T + b1
    return np.stack([np.abs(h0).min(axis=1), np.abs(h1).min(axis=1)], axis=1)


# ------------------------------------------------------------------------------------------------ fp16x2
def pow2_under(bound, m):
    """smplpp_vposer_create's rule: the power of two that puts m just under `bound`."""
    return float(2.0 ** np.floor(np.log2(f32(bound) / max(f32(m), f32(1e-30)))))


def split_f16x2(x):
    """common.h: hi = fp16(x), lo = fp16(x - hi) of an already scaled fp32 array, as float64 arrays; fp16 subnormals kept."""
    x = np.asarray(x, f32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(f32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def scales_of(params):
    """(sW1, sW2, sD1, sD2) fixed at creation from worst-case bounds: |D1| <= max|W0|, |D2| <= 512 max|W1| max|W0|."""
    m0, m1, m2 = (f32(np.abs(params[k]).max()) for k in (KEYS[0], KEYS[2], KEYS[4]))
    return pow2_under(16384, m1), pow2_under(16384, m2), pow2_under(16384, m0), pow2_under(16384, f32(512) * m1 * m0)


def _mm3(A, B):
    """A = (hi, lo) [R,K], B = (hi, lo) [K,C] float64 arrays holding fp16 values -> [R,C] fp32: per 16-wide k-step the three
    products hi.hi, hi.lo, lo.hi, each summed exactly and added to the fp32 accumulator with one rounding."""
    (Ah, Al), (Bh, Bl) = A, B
    acc = np.zeros((Ah.shape[0], Bh.shape[1]), f32)
    tmp = np.empty(acc.shape, np.float64)
    for k in range(0, Ah.shape[1], 16):
        for a, b in ((Ah, Bh), (Ah, Bl), (Al, Bh)):
            np.matmul(a[:, k:k + 16], b[k:k + 16], out=tmp)
            tmp += acc
            acc[...] = tmp
    return acc


def _cols(x):
    """[n,K,C] -> [K, n C]: the frames' columns side by side (they never mix)."""
    return np.ascontiguousarray(x.transpose(1, 0, 2).reshape(x.shape[1], -1))


def _rows(x, n):
    """[R, n C] -> [n,R,C]."""
    return x.reshape(x.shape[0], n, -1).transpose(1, 0, 2)


def _act_scale(a):
    """vscale512: per frame the power of two that puts max |a| just under 2^14 (fp32 arithmetic)."""
    m = np.maximum(np.abs(a).max(axis=1), f32(1e-30)).astype(f32)
    return np.exp2(np.floor(np.log2(f32(16384) / m))).astype(f32)


def _fma(a, b, c):
    """fp32 a * b + c with one rounding (a product of two fp32 numbers is exact in float64)."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def fp16x2_oracle(params, z, plant=None):
    """The documented arithmetic of vposer_jac2_kernel.  Same dict as plain_oracle (float32 arrays).  T1 [n,512,32]: the layer-1
    tangent block before its split at sD2.  `plant` (the planted errors
    of tests/test_vposer_blocks_cpu.py): ("no_c10", tile) leaves the 0.01 C10 term out of rows 32 tile .. 32 tile + 31 of T1;
    ("next_mask", tile, ks) forms those rows of frame f with the layer-0 mask of frame f + 1 (the last frame: of frame 0) in k-step
    ks (rows 16 ks .. 16 ks + 15 of W0: one 32 x 32 x 16 MFMA tile of the layer-1 tangent product with its neighbour's mask) or, ks
    None, in every k-step."""
    W0, b0, W1, b1, W2, b2 = _weights(params, f32)
    z = np.asarray(z, f32).reshape(-1, LAT)
    n = z.shape[0]
    sW1, sW2, sD1, sD2 = scales_of(params)
    W1p, W2p = split_f16x2(W1 * f32(sW1)), split_f16x2(W2 * f32(sW2))
    W0h, W0l = split_f16x2(W0 * f32(sD1))
    C10 = (W1.astype(np.float64) @ W0.astype(np.float64)).astype(f32)
    # layer 0 on the VALU: h = b0, then one fma per latent column
    h0 = np.broadcast_to(b0, (n, HID)).astype(f32)
    for c in range(LAT):
        h0 = _fma(W0[None, :, c], z[:, c:c + 1], h0)
    p0 = h0 > 0
    a0 = (h0 * np.where(p0, f32(1), f32(0.01))).astype(f32)
    # layer 1, value: the activation vector as one more B column, per-frame scale
    sA1 = _act_scale(a0)
    ah, al = split_f16x2(a0 * sA1[:, None])
    acc = _mm3(W1p, (np.ascontiguousarray(ah.T), np.ascontiguousarray(al.T))).T                       # [n,512]
    h1 = _fma(acc, (f32(1.0 / sW1) / sA1)[:, None], b1[None])
    s1 = np.where(h1 > 0, f32(1), f32(0.01))
    a1 = (h1 * s1).astype(f32)
    # layer 1, tangents: W1 . (m (.) W0) with the masked W0 stream, then T1 = s1 (.) (0.01 C10 + 0.99 acc) in fp32
    m = p0.astype(np.float64)[:, :, None]
    accT = _rows(_mm3(W1p, (_cols(m * W0h[None]), _cols(m * W0l[None]))), n)                          # [n,512,32]
    if plant is not None and plant[0] == "next_mask":
        rows = slice(32 * plant[1], 32 * plant[1] + 32)
        mo, ks = m.copy(), (slice(None) if plant[2] is None else slice(16 * plant[2], 16 * plant[2] + 16))
        mo[:, ks] = np.roll(m, -1, axis=0)[:, ks]
        accT = accT.copy()
        accT[:, rows] = _rows(_mm3((W1p[0][rows], W1p[1][rows]), (_cols(mo * W0h[None]), _cols(mo * W0l[None]))), n)
    cc = (f32(0.01) * C10).astype(f32)
    if plant is not None and plant[0] == "no_c10":
        cc = cc.copy()
        cc[32 * plant[1]:32 * plant[1] + 32] = 0
    um = f32(f32(0.99) * f32(1.0 / sW1) / f32(sD1))
    T1 = (s1[:, :, None] * _fma(accT, um, cc[None])).astype(f32)
    # layer 2
    sA2 = _act_scale(a1)
    ah, al = split_f16x2(a1 * sA2[:, None])
    acc = _mm3(W2p, (np.ascontiguousarray(ah.T), np.ascontiguousarray(al.T))).T                       # [n,126]
    o6 = _fma(acc, (f32(1.0 / sW2) / sA2)[:, None], b2[None])
    Dh, Dl = split_f16x2(T1 * f32(sD2))
    T6 = (_rows(_mm3(W2p, (_cols(Dh), _cols(Dl))), n) * f32(f32(1.0 / sW2) / f32(sD2))).astype(f32)
    out, jac = _through_tail(o6, T6, f32)
    return dict(out=out, jac=jac, h0=h0, h1=h1, o6=o6, T6=T6, T1=T1)


# ------------------------------------------------------------------------------------------------ decoders
_decoders = {}


def decoder(which):
    """Parameters of one of the decoders (built once, never modified): "synth" (VPoserDecoder.synthetic_params()); "slope1" and
    "slope001", the synthetic decoder with 4 added to / taken from every layer-0 bias (every layer-0 slope 1 / 0.01 for the cases'
    latents); "range", one entry of each weight matrix multiplied by 2^8 (the creation-time scales drop by 7 or 8 octaves, sD2 by 15 or
    16: the lo pieces of half the layer-1 tangent block are fp16 subnormals); "branch", test_vposer_vjp_gpu.py::_branch_point_decoder()."""
    if which not in _decoders:
        if which == "branch":
            from test_vposer_vjp_gpu import _branch_point_decoder

            p = _branch_point_decoder()
        else:
            from smplpp_amd.ik import VPoserDecoder

            p = VPoserDecoder.synthetic_params()
            if which in ("slope1", "slope001"):
                p[KEYS[1]] = (p[KEYS[1]] + f32(4.0 if which == "slope1" else -4.0)).astype(f32)
            elif which == "range":
                for k, at in ((KEYS[0], (100, 7)), (KEYS[2], (300, 200)), (KEYS[4], (50, 400))):
                    p[k] = p[k].copy()
                    p[k][at] *= f32(256)
            else:
                assert which == "synth", which
        _decoders[which] = {k: np.asarray(p[k], f32) for k in KEYS}
    return _decoders[which]


# ------------------------------------------------------------------------------------------------ cases
def draw(which, n, seed, scales=(1.0,), zero_first=True):
    """(z [n,32] fp32, draws replaced): frame f ~ scales[f % len(scales)] x N(0,1) from one seeded stream, a latent with a
    pre-activation inside the margin redrawn at once; frame 0 is z = 0 (not redrawn: the CPU test asserts that it clears the
    margin).  A longer batch of the same stream starts with the shorter one."""
    rng, p = np.random.default_rng(seed), decoder(which)
    z, replaced = np.zeros((n, LAT), f32), 0
    for f in range(1 if zero_first else 0, n):
        s = scales[f % len(scales)]
        while True:
            cand = (s * rng.standard_normal(LAT)).astype(f32)
            if (min_preactivation(p, cand)[0] >= margins(which, s)).all():
                break
            replaced += 1
        z[f] = cand
    return z, replaced


def _case(name, which, n, seed, scales=(1.0,), frame_base=0, capped=True, zero_first=True, **kw):
    z, replaced = draw(which, n, seed, scales, zero_first)
    fs = [0.0 if zero_first and f == 0 else scales[f % len(scales)] for f in range(n)]
    return dict(name=name, decoder=which, z=z, replaced=replaced, frame_scales=fs, frame_base=frame_base, capped=capped, **kw)


DENSE_SEED = 52
DENSE_ONE = [1, 2, 3, 64]  # one frame per workgroup; 64 frames walk all 32 k-loop rotations (5 x (f / 2) mod 32)


def dense_n(cus=CUS_DEFAULT):
    """One frame per workgroup, then two (n > CUs): CUs + 1 (odd: the last workgroup's spare slot is live) and CUs + 2."""
    return DENSE_ONE + [cus + 1, cus + 2]


def dense_case(n):
    """Synthetic decoder, z = 0 then N(0,1): every dense case is the head of one stream."""
    return _case("dense n=%d" % n, "synth", n, DENSE_SEED)


def shard_cases(cus=CUS_DEFAULT):
    """n = CUs + 1 at frame_base 1 (the first workgroup's slot 0 lies before the shard) and n = 3 at 2^31 + 1.  `twin_base`: the
    latents decoded behind `twin_base` dummy frames at base 0 have the same global groups modulo 32, hence the same bits."""
    return [dict(dense_case(cus + 1), name="shard n=%d base=1" % (cus + 1), frame_base=1, twin_base=1),
            dict(dense_case(3), name="shard n=3 base=2^31+1", frame_base=2 ** 31 + 1, twin_base=1)]


SCALE_N = 6


def scale_cases(cus=CUS_DEFAULT):
    """z x 1e-3, x 0.3, x 8 (13 octaves of latent; the per-frame activation scale, which the biases hold up, moves over 6), and all
    three in neighbouring frames of one two-frame workgroup (n = CUs + 1)."""
    cs = [_case("scale %g n=%d" % (s, SCALE_N), "synth", SCALE_N, 60, (s,)) for s in (1e-3, 0.3, 8.0)]
    return cs + [_case("scale mixed n=%d" % (cus + 1), "synth", cus + 1, 63, (1e-3, 0.3, 8.0))]


MASK_N = 5


def mask_cases():
    """Every layer-0 slope 1 (the full product) or 0.01 (the C10 constant path alone)."""
    return [_case("mask %s n=%d" % (w, MASK_N), w, MASK_N, seed, zero_first=False, slope0=s)
            for w, s, seed in (("slope1", 1.0, 71), ("slope001", 0.01, 70))]


def range_case():
    """The yardstick is this decoder's own fp16x2 oracle, with no cap."""
    return _case("range n=5", "range", 5, 80, capped=False, zero_first=False)


PLAIN_JOINTS, NEAR_PI_JOINTS, PI_JOINTS = [0] + list(range(14, 21)), list(range(8, 14)), list(range(1, 8))


def branch_case():
    """_branch_point_decoder() at z = 0, z ~ 1e-3 and z ~ 0.3."""
    return _case("branch n=3", "branch", 3, 13, (0.0, 1e-3, 0.3), capped=False)


_refs = {}


def references(case):
    """(float64, fp32, fp16x2) oracle dicts of a case, computed once per process and never modified; cases that share latents and a
    decoder (the dense cases are heads of one stream) share the work."""
    key = (case["decoder"], case["z"].shape[0], case["z"].tobytes())
    if key not in _refs:
        big = [k for k in _refs if k[0] == case["decoder"] and k[1] > key[1] and k[2].startswith(key[2])]
        if big:
            n = key[1]
            _refs[key] = tuple({k: v[:n] for k, v in r.items()} for r in _refs[big[0]])
        else:
            p = decoder(case["decoder"])
            _refs[key] = (plain_oracle(p, case["z"]), plain_oracle(p, case["z"], f32), fp16x2_oracle(p, case["z"]))
    return _refs[key]


def abs_blocks(x, ref64):
    """max | |x| - |ref| | per 3-vector, component by component: the decoded angles up to the sign of each component."""
    d = np.abs(np.abs(np.asarray(x, np.float64)) - np.abs(np.asarray(ref64, np.float64))).max(axis=-1)
    return np.where(np.isfinite(d), d, np.inf)


OUT_METRICS = {"plain": out_blocks, "rot": rot_blocks, "abs": abs_blocks}
JAC_METRICS = {"plain": jac_blocks, "sign": jac_blocks_up_to_sign}
ALL = (None, None, "plain", "plain", "all joints")
# The classes of the branch case: (frames, joints, metric of out, metric of jac, name); None: every frame / joint, or not held.
# Joints 0, 14-20: the plain bar.  8-13: their own yardstick.  1-7 sit exactly at pi at z = 0 ONLY: at z ~ 1e-3 and z ~ 0.3 they
# are held, frame by frame, as rotations and up to each row's sign, on yardsticks of 3e-7 and 1e-4 (a single class over the three
# frames would take frame 0's yardstick, 1 rad and 1e3 slabs, which nothing can miss).  At z = 0: joints 1-4 (pi about x, y, z and
# (1,1,0)) as rotations; joints 5-7 (oblique axes), where one fp32 ulp flips single components of the axis - ANOTHER rotation -,
# by |out| component by component; the slabs of joints 4-7 up to sign.  The slabs of joints 1-3 at z = 0 (pi about a coordinate
# axis: s = 0 under the square root, d sqrt(s + eps) = 1 / (2 sqrt(eps)) times the rounding of s, 1 to 1e3 slab sizes in any fp32
# evaluation) are held to finiteness only.
BRANCH_CLASSES = (
    (None, PLAIN_JOINTS, "plain", "plain", "0, 14-20"),
    (None, NEAR_PI_JOINTS, "plain", "plain", "8-13"),
    ([1], PI_JOINTS, "rot", "sign", "1-7 z~1e-3"),
    ([2], PI_JOINTS, "rot", "sign", "1-7 z~0.3"),
    ([0], [1, 2, 3, 4], "rot", None, "1-4 z=0"),
    ([0], [5, 6, 7], "abs", None, "5-7 z=0"),
    ([0], [4, 5, 6, 7], None, "sign", "4-7 z=0 jac"),
)


def figures(got, ref64, cls=ALL):
    """(E_out, E_jac) of got = dict(out, jac or None) over the blocks of class `cls` (see BRANCH_CLASSES); None where the class
    does not hold that output or `got` has no Jacobian."""
    frames, joints, ok, jk, _ = cls
    fs = slice(None) if frames is None else frames
    js = slice(None) if joints is None else joints
    eo = ej = None
    if ok is not None:
        eo = float(OUT_METRICS[ok](got["out"], ref64["out"])[fs][:, js].max())
    if jk is not None and got.get("jac") is not None:
        ej = float(JAC_METRICS[jk](got["jac"], ref64["jac"])[fs][:, js].max())
    return eo, ej


# ------------------------------------------------------------------------------------------------ rotmat -> axis-angle
AA_N = [127, 128, 129]  # around the 128-thread block
AA_MARGIN = 1e-5  # the float64 predicates clear their thresholds by this much (an fp32 trace is good to 3 x 2^-23 = 3.6e-7)
AA_EXACT = 1e-5   # a near-pi row with max |R - R^T| under this is "exactly pi": rounding picks signs there, held as a rotation
AA_RANDOM = 40    # at least this many of the sweep's random rotations
AA_GENERIC = 0.5  # 1 + trace from here on (theta up to 2.4 rad): the generic rows; under it theta / (2 sin theta) grows towards pi
EPS = float(np.finfo(np.float32).eps)


def aa_predicates(R):
    """float64 distances of each matrix from the three branch thresholds of convertRotMatToAxisAngle: (1 + trace) - eps^(1/4),
    |3 - trace| - sqrt(eps), theta - (pi - 1e-4)."""
    tr = np.trace(np.asarray(R, np.float64), axis1=1, axis2=2)
    theta = np.arccos((1 - EPS) * 0.5 * (tr - 1))
    return (1 + tr) - EPS ** 0.25, np.abs(3 - tr) - EPS ** 0.5, theta - (np.pi - 1e-4)


def aa_rows():
    """(R [129,3,3] fp32, cls [129] int), picked from test_oracle_vposer.sweep_matrices() and the branch-point rotations:
      - of the sweep's structured rows (index 1 + ((axis 7 + e) 2 + sign) 4 + base), about ALL THREE axes, the bases 0, pi/4, pi/2,
        pi with eps 0, +-1e-3 and +-1e-1, and +-1e-6 at the bases 0 and pi (1e-12 and 1e-9 collapse onto 0 in fp32, 1e-2 adds no
        branch);
      - the 21 rotations of the branch-point decoder (pi about seven axes, 1e-4 / 1e-3 rad from pi and from the identity, a
        generic one);
      - the sweep's random rotations, in its order, to fill 129 (AA_RANDOM at least),
    without repeats as fp32 matrices, each kept only if its float64 predicates clear AA_MARGIN.
    cls: 0 generic (1 + trace >= AA_GENERIC), held as a vector; 1 towards pi on the generic branch (eps^(1/4) <= 1 + trace <
    AA_GENERIC), a vector on a yardstick of its own; 2 on the near-pi branch with max |R - R^T| >= AA_EXACT (pi -+ 1e-4 ... 1e-1: the
    signs follow R - R^T robustly), a vector on a yardstick of its own; 3 exactly pi (to 1e-6), held as a rotation."""
    from scipy.spatial.transform import Rotation

    from test_oracle_vposer import sweep_matrices

    S = sweep_matrices()
    assert len(S) == 1 + 3 * 7 * 2 * 4 + 10000
    EPS_ABS = (0.0, 1e-12, 1e-9, 1e-6, 1e-3, 1e-2, 1e-1)
    pick = [0]
    for axis in range(3):
        for e, eps_abs in enumerate(EPS_ABS):
            for sgn in range(2):
                for base in range(4):
                    if eps_abs in (0.0, 1e-3, 1e-1) or (eps_abs == 1e-6 and base in (0, 3)):
                        pick.append(1 + ((axis * 7 + e) * 2 + sgn) * 4 + base)
    axes = [np.array(a, np.float64) / np.linalg.norm(a) for a in
            ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, -2, 3], [0.3, 0.5, -0.8], [-1, 0.2, 0.1])]
    extra = [Rotation.from_rotvec(np.pi * a).as_matrix() for a in axes]
    extra += [Rotation.from_rotvec((np.pi - d) * a).as_matrix() for a in axes[:3] for d in (1e-4, 1e-3)]
    extra += [Rotation.from_rotvec(d * a).as_matrix() for a in axes[3:6] for d in (1e-4, 1e-3)]
    extra += [Rotation.from_rotvec(0.7 * axes[4]).as_matrix()]
    R = np.concatenate([S[pick], np.stack(extra), S[169:]]).astype(f32)
    a, b, c = aa_predicates(R)
    keep = (np.abs(a) >= AA_MARGIN) & ((a < 0) | (np.abs(b) >= AA_MARGIN)) & (np.abs(c) >= AA_MARGIN)
    seen, rows = set(), []
    for i in np.nonzero(keep)[0]:
        k = R[i].tobytes()
        if k not in seen:
            seen.add(k)
            rows.append(i)
        if len(rows) == AA_N[-1]:
            break
    assert len(rows) == AA_N[-1]
    R, a = R[rows], a[rows]
    w = np.abs(R.astype(np.float64) - R.astype(np.float64).transpose(0, 2, 1)).max(axis=(1, 2))
    return R, np.where(a >= 0, np.where(a + EPS ** 0.25 >= AA_GENERIC, 0, 1), np.where(w >= AA_EXACT, 2, 3))


def aa_reference(R, dtype="float64"):
    import torch

    from oracle import vposer_torch as VT

    return VT.convert_rotmat_to_axis_angle(torch.as_tensor(np.asarray(R), dtype=getattr(torch, dtype))).numpy()


AA_CLASSES = ("generic, vectors", "towards pi, vectors", "near-pi branch, vectors", "exactly pi, rotations")


def aa_figures(x, ref64, cls):
    """E per class of AA_CLASSES (0.0 for a class without rows)."""
    v, r = out_blocks(x, ref64), rot_blocks(x, ref64)
    return [float(m[cls == c].max()) if (cls == c).any() else 0.0 for c, m in ((0, v), (1, v), (2, v), (3, r))]


# ------------------------------------------------------------------------------------------------ re-deriving the margins
def measured_margins(which="synth", scale=1.0, n=1000, seed=5):
    """(layer 0, layer 1): 64 x the fp16x2 oracle's worst pre-activation error against float64 over n latents scale x N(0,1) on
    decoder `which`: what MARGINS[scale] x MARGIN_FACTORS[which] must not fall under.  MARGINS was set from this (rounded up, and
    raised where a case's own frames measure more: the CPU test prints 64 x error / margin per case).  After a change to
    synthetic_params() or to the latent streams: call this per scale and decoder, write the larger of it and the cases' figures
    into MARGINS / MARGIN_FACTORS, then move a case's seed on if the CPU test reports more than 10 % of its draws replaced."""
    p = decoder(which)
    z = (scale * np.random.default_rng(seed).standard_normal((n, LAT))).astype(f32)
    r64, r16 = plain_oracle(p, z), fp16x2_oracle(p, z)
    return tuple(64 * float(np.abs(r16[k] - r64[k]).max()) for k in ("h0", "h1"))
