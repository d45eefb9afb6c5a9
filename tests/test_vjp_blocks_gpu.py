"""smplpp_fk_vjp, smplpp_fk_rotmat_vjp and smplpp_vposer_vjp on the MI355X, held to float64 autograd BLOCK BY BLOCK
(tests/vjp_blocks.py): every (frame, row) 3-vector of dL/dtheta, every (frame, joint) 3x3 of rot, every frame of dL/dbeta, trans
and dL/dz within max(4 x the fp32 oracle's worst block of the case, 4 x 2^-24) of its own largest entry, so that a leaf joint
cannot hide in a norm the root owns.  The cases: dense cotangents around the 32-frame tile and across the fall of the chunk
count, Jacobian rows (one live vertex per frame, on the group boundaries, each joint's own vertex and the most mixed ones), a few
live vertices, silent frames inside a live tile, the forms that recompute `rest`, and the decoder's transposed Jacobian.
tests/test_vjp_blocks_cpu.py prints the yardsticks; this file prints the kernels' figures beside them (run with -s)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vjp_blocks as B  # noqa: E402

pytestmark = pytest.mark.gpu

_smpls = {}


def _smpl(which, form="default"):
    """One handle per (model, SMPLPP_SKIN form) for the module; the form is read at creation ("default" = unset)."""
    from smplpp_amd.smpl import SMPL

    if (which, form) not in _smpls:
        old = os.environ.pop("SMPLPP_SKIN", None)
        try:
            if form != "default":
                os.environ["SMPLPP_SKIN"] = form
            s = SMPL()
            s.setDevice("cuda:0")
            s.init(B.model(which))
        finally:
            os.environ.pop("SMPLPP_SKIN", None)
            if old is not None:
                os.environ["SMPLPP_SKIN"] = old
        assert s.info()["weights_per_vertex"] == B.MAXW[which]
        _smpls[(which, form)] = s
    return _smpls[(which, form)]


def _held(tag, case, got, r64, r32, outputs, frame_scaled=False):
    """Every output of `got` (full batch) over case["frames"] within bar(e32) block-scaled; with frame_scaled also within its own
    bar when each row is scaled by its frame's largest entry.  Prints every figure, then asserts."""
    fr, bad = case["frames"], []
    for (name, ax), a, b in zip(outputs, r64, r32):
        x = got[name][fr]
        axes = B.axes_of(ax, a)
        figures = [("block", axes)] + ([("frame", B.frame_axes(a))] if frame_scaled and ax is not None else [])
        for what, axs in figures:
            e, e32 = B.block_error(x, a, axs), B.block_error(b, a, axs)
            worst = np.unravel_index(np.argmax(B.block_errors(x, a, axs)), B.block_errors(x, a, axs).shape)
            print("%-44s %-5s %-5s E = %.3g (%.1f x 2^-24) at block %s   fp32 oracle %.3g (%.1f x 2^-24)   bar %.3g"
                  % (case["name"] + " " + tag, name, what, e, e / B.EPS32, tuple(int(i) for i in worst), e32, e32 / B.EPS32, B.bar(e32)))
            if not (np.isfinite(x).all() and e <= B.bar(e32)):
                bad.append((tag, name, what, e, B.bar(e32), worst))
    assert not bad, bad


def _fk_runs(s, case, rests=("given", None)):
    """launchBackward with `rest` passed and with rest = None."""
    for mode in rests:
        rest = s.launch(case["beta"], case["theta"], want=("rest",))["rest"].copy() if mode else None
        yield "rest=%s" % mode, s.launchBackward(case["beta"], case["theta"], grad_verts=case["gv"], grad_joints=case["gj"], rest=rest)


def _rotmat_runs(s, case, rot, rests=("given", None)):
    trans = np.ascontiguousarray(case["theta"][:, 0])
    for mode in rests:
        rest = s.launchRotmat(case["beta"], trans, rot, want=("rest",))["rest"].copy() if mode else None
        yield "rest=%s" % mode, s.launchRotmatBackward(case["beta"], trans, rot, grad_verts=case["gv"], grad_joints=case["gj"], rest=rest)


def _check_fk(s, case, frame_scaled=False, rests=("given", None)):
    r64, r32 = B.fk_reference(case), B.fk_reference(case, "float32")
    for tag, got in _fk_runs(s, case, rests):
        _held("fk " + tag, case, got, r64, r32, B.FK_OUTPUTS, frame_scaled)


def _check_rotmat(s, case, general, frame_scaled=False, rests=("given", None)):
    rot = B.rot_of(case, general)
    r64, r32 = B.rotmat_reference(case, rot), B.rotmat_reference(case, rot, "float32")
    for tag, got in _rotmat_runs(s, case, rot, rests):
        _held(("general " if general else "rotmat ") + tag, case, got, r64, r32, B.ROTMAT_OUTPUTS, frame_scaled)


# ---------------------------------------------------------------------------------------------- a. dense cotangents
@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("n", B.DENSE_N)
@pytest.mark.parametrize("entry", ["fk", "rotmat", "general"])
def test_dense_cotangent_block_by_block(entry, n, kind):
    s, case = _smpl("synth"), B.dense_case(n, kind)
    assert case["frames"] == list(range(n))
    if entry == "fk":
        _check_fk(s, case)
    else:
        _check_rotmat(s, case, entry == "general")


@pytest.mark.parametrize("kind", B.KINDS)
def test_dense_cotangent_where_the_chunk_count_has_fallen(kind):
    """n = 1024: vjp_chain_kernel sums fewer, longer slabs (14 chunks instead of 54 on 256 compute units).  The library exports
    neither its chunk rule nor its compute-unit count, so the rule is restated (vjp_blocks.vjp_chunks, from fk_vjp.hip) and
    evaluated at torch's count of compute units."""
    import torch

    s, case = _smpl("synth"), B.dense_case(B.BIG_N, kind)
    assert case["frames"] == [0, 31, 32, 1023]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert B.vjp_chunks(cus, B.BIG_N, s.vertex_num)[1] < B.vjp_chunks(cus, B.DENSE_N[-1], s.vertex_num)[1], cus
    _check_fk(s, case)
    _check_rotmat(s, case, False)
    _check_rotmat(s, case, True)


@pytest.mark.parametrize("which", ["tiny", "eight"])
def test_dense_cotangent_with_24_and_8_weights_per_vertex(which):
    s, case = _smpl(which), B.dense_case(33, "both", which)
    _check_fk(s, case)
    _check_rotmat(s, case, False)


# ---------------------------------------------------------------------------------------------- b. Jacobian rows
@pytest.mark.parametrize("which", B.MODELS)
def test_jacobian_rows(which):
    """One live vertex per frame.  The off-chain joints' blocks (4e-4 ... 8e-3 of the row's largest entry) come from the pose-blend
    columns of the transposed GEMM alone; they set the block-scaled yardstick, so the frame-scaled figure is held to its own 4 x as
    well and the small blocks' looser fp32 conditioning lends no slack to the large ones."""
    s, case = _smpl(which), B.rows_case(which)
    _check_fk(s, case, frame_scaled=True)
    _check_rotmat(s, case, False, frame_scaled=True)


# ---------------------------------------------------------------------------------------------- c. a few live vertices
@pytest.mark.parametrize("i", [0, 1], ids=["faces", "hand"])
def test_a_few_live_vertices(i):
    s, case = _smpl("synth"), B.sparse_cases()[i]
    _check_fk(s, case)
    _check_rotmat(s, case, False)


# ---------------------------------------------------------------------------------------------- d. silent frames in a live tile
def test_silent_frames_inside_a_live_tile():
    s, case = _smpl("synth"), B.silent_case()
    silent = B.silent_frames()
    alive = [f for f in range(B.SILENT_N) if f not in silent]
    full = dict(case, gv=case["gv_full"])
    trans = np.ascontiguousarray(case["theta"][:, 0])
    rot = B.rot_of(case, False)
    rest = s.launch(case["beta"], case["theta"], want=("rest",))["rest"].copy()
    for mode in (rest, None):
        got = s.launchBackward(case["beta"], case["theta"], grad_verts=case["gv"], grad_joints=case["gj"], rest=mode)
        ref = s.launchBackward(case["beta"], case["theta"], grad_verts=full["gv"], grad_joints=case["gj"], rest=mode)
        assert not got["theta"][silent].any()  # rows 1..24 exactly +0 or -0, row 0 exactly zero
        assert got["beta"][silent].any(axis=1).all()  # (the joints' cotangent still arrives)
        for k in ("beta", "theta"):  # frames do not mix: the live frames' bits do not depend on what the silent ones carry
            assert np.array_equal(got[k][alive], ref[k][alive]), k
            assert not np.array_equal(got[k][silent], ref[k][silent]), k
        gotr = s.launchRotmatBackward(case["beta"], trans, rot, grad_verts=case["gv"], grad_joints=case["gj"], rest=mode)
        refr = s.launchRotmatBackward(case["beta"], trans, rot, grad_verts=full["gv"], grad_joints=case["gj"], rest=mode)
        assert not gotr["rot"][silent].any() and not gotr["trans"][silent].any()
        for k in ("beta", "trans", "rot"):
            assert np.array_equal(gotr[k][alive], refr[k][alive]), k
    # the silent frames' dL/dbeta (and every live block) against the oracle, whose silent frames are its joints-only graph
    _check_fk(s, case)
    _check_rotmat(s, case, False)


# ---------------------------------------------------------------------------------------------- e. the forms that recompute rest
def _check_form(form, case, frame_scaled=False):
    """rest = None under SMPLPP_SKIN = form: the backward recomputes `rest` with that form.  Form h's rest is a 22-bit quantity,
    so its yardstick is the fp32 oracle fed that rest (fk_vjp_oracle.vjp(rest=...)); the reference stays the float64 oracle."""
    s = _smpl("synth", form)
    r64 = B.fk_reference(case)
    rest = s.launch(case["beta"], case["theta"], want=("rest",))["rest"].copy() if form == "h" and case["gv"] is not None else None
    r32 = B.fk_reference(case, "float32", rest=rest)
    got = s.launchBackward(case["beta"], case["theta"], grad_verts=case["gv"], grad_joints=case["gj"])
    _held("form %s rest=None" % form, case, got, r64, r32, B.FK_OUTPUTS, frame_scaled)


@pytest.mark.parametrize("kind", B.KINDS)
@pytest.mark.parametrize("form", B.FORMS)
def test_forms_recompute_rest_dense(form, kind):
    _check_form(form, B.dense_case(33, kind))


@pytest.mark.parametrize("form", B.FORMS)
def test_forms_recompute_rest_jacobian_rows(form):
    _check_form(form, B.rows_case("synth"), frame_scaled=True)


# ---------------------------------------------------------------------------------------------- f. VPoser decoder backward
@pytest.fixture(scope="module")
def vposer():
    from smplpp_amd.ik import VPoserDecoder

    params = VPoserDecoder.synthetic_params()
    return params, VPoserDecoder(params)


def _check_vposer(vposer, case):
    params, gpu = vposer
    r64, r32 = B.vposer_reference(params, case), B.vposer_reference(params, case, "float32")
    gz = gpu.launchBackward(case["z"], case["g"])
    assert gz.shape == r64.shape and gz.dtype == np.float32
    _held("", case, {"dz": gz}, (r64,), (r32,), (("dz", None),))


@pytest.mark.parametrize("latent", B.VPOSER_LATENTS)
def test_vposer_transposed_jacobian(vposer, latent):
    """The 63 one-hot cotangents at one latent: every row of the transposed Jacobian, each scaled by its own largest entry."""
    _check_vposer(vposer, B.vposer_rows_case(latent))


@pytest.mark.parametrize("n", B.VPOSER_DENSE_N)
def test_vposer_dense(vposer, n):
    _check_vposer(vposer, B.vposer_dense_case(n))
