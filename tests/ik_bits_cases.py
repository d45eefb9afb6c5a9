"""The cases whose bits tests/golden/ik_bits.json pins: the IK iteration's host side (ik_iterate_enqueue and the plans of
smplpp_amd/csrc/ik_plan.h) chooses kernels, LDS sizes and a two-stream schedule, and none of that may move a bit.

  solve cases     one per instantiation of ik_solve_kernel, from tests/solve_ref.py's case list (problems by
                  test_ik_solve_gpu.make_problem): three calls of iterate(1), so that the double-buffered mesh, the side stream and
                  the join in front of the next evaluation all take part.
  scan cases      the six branches of the face scan's dispatch, K in {2, 6, 12} with the creation-time switches SMPLPP_SCAN_FORM=0
                  and SMPLPP_SCAN_BLOCKS=n (one chunk per frame, no small chunk); phi locked in half of them (scan beside the solve).
  sequence cases  solve_sequence and solve_sequence_shared in the latent layout, K = 12, phi locked, n = 4, T = 4, warm-up 2, one
                  iteration per frame: the decoder Jacobian made ahead on the side stream, the sequence hook and the frame switch.

inputs() gives every array a case feeds the solver, outputs() what it leaves behind; digest() is the SHA-256 of an array's
little-endian bytes.  tools/record_ik_bits.py wrote the golden file from these, tests/test_ik_bits_gpu.py recomputes and compares."""
import contextlib
import hashlib
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solve_ref as S  # noqa: E402
from test_ik_solve_gpu import make_problem  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ik_bits.json")
SWITCHES = ("SMPLPP_IK_DBG_STOP", "SMPLPP_IK_OVERLAP", "SMPLPP_IK_EVENTS", "SMPLPP_IK_LATENT_SPLIT", "SMPLPP_DEBUG_SYNC",
            "SMPLPP_SCAN_BLOCKS", "SMPLPP_SCAN_FORM")
SOLVE = ("dual_k6_qp", "latent_ntr3_locked_k12", "ntr5_k16_llt", "ntr6_k16_beta_box", "ntr11_k16", "lds_k46_beta")
_BY_NAME = {c["name"]: c for c in S.CASES}


def _scan(name, K, phi, env, form):
    c = S._case(name, "direct", K, False, True, phi=phi, n=4, normals=False)
    return dict(c, env=env, form=form)


# (KPR, NBT) of proj_scan_kernel each case must reach: asserted against the dispatch rule in the test
SCAN = [_scan("scan_k2_pairs", 2, "live", {}, (2, 6)),
        _scan("scan_k6_quads", 6, "locked", {}, (4, 6)),
        _scan("scan_k6_lds_small", 6, "live", {"SMPLPP_SCAN_FORM": "0"}, (0, 3)),
        _scan("scan_k6_lds_one_chunk", 6, "locked", {"SMPLPP_SCAN_FORM": "0", "SMPLPP_SCAN_BLOCKS": "4"}, (0, 6)),
        _scan("scan_k12_small", 12, "locked", {}, (0, 3)),
        _scan("scan_k12_one_chunk", 12, "live", {"SMPLPP_SCAN_BLOCKS": "4"}, (0, 6))]
SEQUENCE = ("sequence_latent_k12", "sequence_shared_latent_k12")
NAMES = SOLVE + tuple(c["name"] for c in SCAN) + SEQUENCE
T_SEQ, WARMUP_SEQ = 4, 2


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()).hexdigest()


def case(name):
    """The solve_ref-style case dict of `name` (scan cases carry `env` and `form` too)."""
    if name in SEQUENCE:
        return dict(_BY_NAME["latent_ntr3_locked_k12"], env={})
    for c in SCAN:
        if c["name"] == name:
            return c
    return dict(_BY_NAME[name], env={})


@contextlib.contextmanager
def switches(env):
    """The creation-time switches of the solver: all cleared, then `env`; put back afterwards."""
    old = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def inputs(name, oracle_model, ref_decoder):
    """Every array the case feeds the solver (host data only)."""
    c = case(name)
    P = make_problem(c, oracle_model, ref_decoder)
    x = {k: np.asarray(P[k]) for k in ("faces", "tp", "pw", "nw", "pl", "beta", "theta")}
    if name in SEQUENCE:
        n, K = c["n"], c["K"]
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        tp = P["tp"][None] + np.cumsum(rng.normal(0, 0.01, (T_SEQ, n, K, 3)), axis=0).astype(np.float32)
        valid = np.ones((T_SEQ, n, K), bool)
        valid[1, :, 3] = False
        valid[2, 1 % n, :2] = False
        if name.startswith("sequence_shared"):  # one capture for every chain
            tp, valid = np.ascontiguousarray(tp[:, 0]), np.ascontiguousarray(valid[:, 0])
        x["seq_tp"] = np.where(valid[..., None], tp, 0.0).astype(np.float32)
        x["seq_valid"] = valid
    return x


def outputs(name, smpl, vposer, x):
    """What the case leaves behind, read through the Python binding in host space."""
    from smplpp_amd.ik import IkSolver

    c = case(name)
    n, K, latent = c["n"], c["K"], c["layout"] == "latent"
    with switches(c["env"]):
        s = IkSolver(smpl, n, K, vposer=vposer if latent else None)
    s.setTasks(face_idx=x["faces"], target_pos=x["tp"], pos_task_weight=x["pw"], normal_task_weight=x["nw"], phi_limit=x["pl"])
    s.setConfig(x["beta"], x["theta"])
    y = {}
    if name in SEQUENCE:
        y["theta_out"] = s.solveSequence(x["seq_tp"], x["seq_valid"], warmup_iters=WARMUP_SEQ, iters_per_frame=1, enable_qp=c["qp"])
    else:
        for _ in range(3):
            y["e2"] = s.iterate(1, enable_qp=c["qp"], optimize_beta_from=0 if c["beta"] else -1)
    y["beta"], y["theta"] = s.getConfig()
    t = s.getTasks()
    y["face_idx"], y["vertex_weights"] = t["face_idx"], t["vertex_weights"]
    y["status"] = s.getStatus()
    y["step"] = s.getStep()
    return y
