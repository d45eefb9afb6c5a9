"""The test of tests/test_vjp_blocks_gpu.py's yardstick (tests/vjp_blocks.py), without a GPU: the fp32 torch evaluation of the
oracle graphs through every case list, whose block-scaled error sizes the bar the kernels are held to.  It is printed here (run
with -s) in units of 2^-24: that is where the yardstick's size is written down.  Each yardstick is finite and below 1e-4 (a sanity
cap on the inputs, not a bar); the float64 reference has no exactly-zero block where a cotangent arrives; and three planted errors
show what the block metric catches that the L2 figure of the existing backward tests lets through."""
import numpy as np
import pytest

import vjp_blocks as B

CAP = 1e-4


def _yardstick(case, r64, r32, outputs, frame_scaled=False):
    """Prints and returns {output: e32}; with frame_scaled also the same rows scaled by their frame's largest entry."""
    live = B.live(case)[case["frames"]]
    out = {}
    for (name, ax), a, b in zip(outputs, r64, r32):
        assert np.isfinite(b).all(), (case["name"], name)
        axes = B.axes_of(ax, a)
        e = B.block_error(b, a, axes)
        line = "%-28s %-5s fp32 oracle E = %.3g (%.1f x 2^-24)" % (case["name"], name, e, e / B.EPS32)
        if frame_scaled:
            ef = B.block_error(b, a, B.frame_axes(a))
            line += "   frame-scaled %.3g (%.1f x 2^-24)" % (ef, ef / B.EPS32)
            assert ef <= e
        print(line)
        assert e < CAP, (case["name"], name, e)
        # a block is exactly zero only where no vertex cotangent reaches it (dL/dbeta: never), and there in both precisions
        zero = B.zero_blocks(a, axes)
        want = np.zeros_like(zero) if name == "beta" else np.broadcast_to((~live).reshape((-1,) + (1,) * (zero.ndim - 1)), zero.shape)
        assert np.array_equal(zero, want), (case["name"], name)
        assert np.array_equal(B.zero_blocks(b, axes), want), (case["name"], name)
        out[name] = e
    return out


def _fk(case, frame_scaled=False):
    return _yardstick(case, B.fk_reference(case), B.fk_reference(case, "float32"), B.FK_OUTPUTS, frame_scaled)


def _rotmat(case, general, frame_scaled=False):
    rot = B.rot_of(case, general)
    c = dict(case, name=case["name"] + (" general" if general else " rotmat"))
    return _yardstick(c, B.rotmat_reference(case, rot), B.rotmat_reference(case, rot, "float32"), B.ROTMAT_OUTPUTS, frame_scaled)


@pytest.mark.parametrize("n", B.DENSE_N + [B.BIG_N])
def test_fp32_yardstick_of_the_dense_cases(n):
    for kind in B.KINDS:
        case = B.dense_case(n, kind)
        assert len(case["frames"]) == (n if n <= 65 else 4)
        _fk(case)
        _rotmat(case, False)
        _rotmat(case, True)


def test_fp32_yardstick_of_the_other_models():
    for which in ("tiny", "eight"):
        _fk(B.dense_case(33, "both", which))


def test_fp32_yardstick_of_the_jacobian_rows():
    """On the synthetic model: block-scaled about 1e-5, the same rows scaled by their frame's largest entry about 2.5e-7 — the small
    (off-chain) blocks are forty times worse conditioned in fp32 than the large ones, which is why the GPU test holds both."""
    for which in B.MODELS:
        case = B.rows_case(which)
        assert B.live(case).all() and (np.count_nonzero(case["gv"].reshape(len(case["frames"]), -1), axis=1) == 1).all()
        e = _fk(case, frame_scaled=True)
        _rotmat(case, False, frame_scaled=True)
        if which == "synth":
            vs = B.row_vertices(which)
            V = 6890
            assert set([0, 1, 31, 32, 33, V - 11, V - 10, V - 1]) <= set(vs) and len(vs) >= 24
            assert e["theta"] > 20 * B.EPS32  # (the off-chain blocks set it)


def test_fp32_yardstick_of_the_sparse_and_silent_cases():
    for case in B.sparse_cases():
        nz = np.abs(case["gv"]).max(axis=2) > 0
        assert (nz.sum(axis=1) < 0.15 * nz.shape[1]).all() and nz.any(axis=1).all()
        _fk(case)
        _rotmat(case, False)
    case = B.silent_case()
    silent = B.silent_frames()
    assert len(silent) == 36 and not B.live(case)[silent].any() and B.live(case).sum() == 64 - 36
    assert set(range(40, 48)) <= set(silent) and 38 not in silent
    _fk(case)
    _rotmat(case, False)


def test_rest_value_moves_the_value_not_the_graph():
    """fk_vjp_oracle.vjp(rest=...) with the graph's own rest is the plain oracle to the bit; a perturbed rest moves dL/dtheta."""
    import fk_vjp_oracle as O

    case = B.dense_case(1, "verts", "tiny")
    m = O.model_tensors(B.model("tiny"))
    t64 = lambda a: O.torch.as_tensor(a, dtype=O.torch.float64)
    rest = O.fk(m, t64(case["beta"]), t64(case["theta"]))["rest"].numpy()
    a = B.fk_reference(case)
    b = B.fk_reference(case, rest=rest)
    c = B.fk_reference(case, rest=rest + 1e-3)
    for x, y, z in zip(a, b, c):
        assert np.abs(x - y).max() <= 1e-15 * np.abs(x).max()
    assert B.block_error(c[1], a[1], B.THETA) > 1e-4


@pytest.mark.parametrize("latent", B.VPOSER_LATENTS)
def test_fp32_yardstick_of_the_vposer_rows(latent):
    from smplpp_amd.ik import VPoserDecoder

    params = VPoserDecoder.synthetic_params()
    case = B.vposer_rows_case(latent)
    assert case["z"].shape == (63, 32) and (case["g"].reshape(63, 63) == np.eye(63)).all()
    _vposer(params, case)


def _vposer(params, case):
    r64, r32 = B.vposer_reference(params, case), B.vposer_reference(params, case, "float32")
    e = B.block_error(r32, r64, B.frame_axes(r64))
    print("%-28s dz    fp32 oracle E = %.3g (%.1f x 2^-24), frame-scaled" % (case["name"], e, e / B.EPS32))
    assert np.isfinite(r32).all() and e < CAP, (case["name"], e)
    assert not B.zero_blocks(r64, B.frame_axes(r64)).any(), case["name"]


def test_fp32_yardstick_of_the_vposer_dense_cases():
    from smplpp_amd.ik import VPoserDecoder

    params = VPoserDecoder.synthetic_params()
    for n in B.VPOSER_DENSE_N:
        _vposer(params, B.vposer_dense_case(n))


def test_vjp_chunks_restatement():
    """The chunk count falls between n = 65 and n = 1024 on a 256-CU device (54 -> 14 on the 6890-vertex model)."""
    assert B.vjp_chunks(256, 65, 6890) == (3, 54, 4)
    assert B.vjp_chunks(256, 1024, 6890) == (32, 14, 16)
    assert B.vjp_chunks(256, 1, 61) == (1, 1, 4)


# ------------------------------------------------------------------------------------------------ the metric, pinned
def test_block_error_is_the_stated_metric():
    ref = np.array([[[3.0, 0, 0], [0, 0.5, 0]], [[0, 0, 0], [1, 2, 4]]])
    x = ref.copy()
    x[0, 1, 2] = 0.05   # 0.1 of its block's scale
    x[1, 1, 0] = 1.2    # 0.05 of its block's scale
    assert B.block_error(x, ref, B.THETA) == pytest.approx(0.1)
    assert B.block_error(x, ref, B.frame_axes(ref)) == pytest.approx(0.05)
    e = B.block_errors(x, ref, B.THETA)
    assert e.shape == (2, 2) and e[1, 0] == 0
    x[1, 0, 1] = -0.0
    assert B.block_error(x, ref, B.THETA) == pytest.approx(0.1)  # a zero block may carry either zero
    x[1, 0, 1] = 1e-30
    assert B.block_error(x, ref, B.THETA) == np.inf
    x[1, 0, 1] = np.nan
    assert B.block_error(x, ref, B.THETA) == np.inf
    assert B.bar(0.0) == 4 * 2.0 ** -24 and B.bar(1e-6) == 4e-6


def test_planted_leaf_joint_error_passes_l2_and_fails_the_blocks():
    """The dense case at seed 1 with row 16 of dL/dtheta multiplied by 1 + 3e-4: inside the old bar max(4 rel(fp32), 1e-5) by L2,
    more than ten times over the block bar."""
    case = B.dense_case(1, "verts", seed=1)
    (_, t64), (_, t32) = B.fk_reference(case), B.fk_reference(case, "float32")
    x = t64.copy()
    x[0, 16] *= 1 + 3e-4
    old, old_bar = B.l2_rel(x, t64), max(4 * B.l2_rel(t32, t64), 1e-5)
    e, e32 = B.block_error(x, t64, B.THETA), B.block_error(t32, t64, B.THETA)
    print("row 16 x (1 + 3e-4): L2 %.3g against %.3g; block E %.3g against %.3g" % (old, old_bar, e, B.bar(e32)))
    assert old_bar == 1e-5 and old < 0.5 * old_bar
    assert e == pytest.approx(3e-4, rel=1e-6) and e > 10 * B.bar(e32)


def test_planted_missing_off_chain_blocks_fail_the_blocks():
    """A one-hot row whose off-chain blocks (the joints that neither carry a weight of the vertex nor lie above one that does: the
    pose-blend columns alone reach them) are zeroed, as a kernel that lost that path would leave them."""
    case = B.rows_case("synth")
    k = 3 * B.row_vertices("synth").index(B.model("synth")["vertices_template"].shape[0] - 10)  # the tail group's first vertex, x
    one = dict(case, frames=[k])
    (_, t64), (_, t32) = B.fk_reference(one), B.fk_reference(one, "float32")
    W = np.asarray(B.model("synth")["weights"])
    parent = np.asarray(B.model("synth")["kinematic_tree"], np.int64)[0]
    chain = set()
    for j in np.nonzero(W[case["row_vertex"][k]])[0]:
        while j not in chain:
            chain.add(int(j))
            if j == 0:
                break
            j = int(parent[j])
    off = [j + 1 for j in range(24) if j not in chain]
    assert 0 < len(off) < 24
    x = t64.copy()
    x[0, off] = 0.0
    old, e, e32 = B.l2_rel(x, t64), B.block_error(x, t64, B.THETA), B.block_error(t32, t64, B.THETA)
    small = np.abs(t64[0, off]).max() / np.abs(t64[0]).max()
    print("%d off-chain blocks zeroed (at most %.3g of the row's largest entry): L2 %.3g; block E %.3g against %.3g"
          % (len(off), small, old, e, B.bar(e32)))
    assert small < 0.05
    assert e == 1.0 and e > B.bar(e32)


def test_planted_leak_into_a_silent_frame_is_infinite():
    case = B.silent_case()
    f = B.silent_frames()[5]
    one = dict(case, frames=[f])
    _, t64 = B.fk_reference(one)
    assert not t64.any()
    x = t64.copy()
    assert B.block_error(x, t64, B.THETA) == 0
    x[0, 9, 1] = 1e-12
    assert B.block_error(x, t64, B.THETA) == np.inf
