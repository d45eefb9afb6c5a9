"""The cases whose bits tests/golden/fk_bits.json pins: the forward pass's host side (smplpp_amd/csrc/fk_plan.h and the launchers of
fk.hip / skin_e.hip / skin_h.hip / skin_b.hip) chooses the form, the grid, each workgroup's run of (frame tile, vertex group) items,
the batch cut and the workspace, and none of that may move a bit.

  forms   a model created under SMPLPP_SKIN unset (e), h, b and v: every fused kernel.
  n       1 (a lone frame), 64 (a full tile), 65 (a tile plus one frame), 257 (five frame tiles: on the synthetic model's 108 vertex
          groups the runs of e and h change their frame tile — tests/test_fk_plan_cpu.py::test_crossing_run shows that they must).
  rest    wanted or not: the two instantiations of every kernel.
  rotmat  launchRotmat at n = 65 on the default form: the rotation-input pose step and the workspace's root image.

inputs() gives the arrays a case feeds the library, outputs() what it returns; digest() is the SHA-256 of an array's little-endian
bytes.  tools/record_fk_bits.py wrote the golden file from these, tests/test_fk_bits_gpu.py recomputes and compares."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fk_bits.json")
FORMS = ("default", "h", "b", "v")
NS = (1, 64, 65, 257)
ROTMAT = "rotmat_default_n65"
NAMES = tuple("%s_n%d_%s" % (f, n, r) for f in FORMS for n in NS for r in ("rest", "norest")) + (ROTMAT,)


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()).hexdigest()


def case(name):
    if name == ROTMAT:
        return {"form": "default", "n": 65, "rest": True, "rotmat": True}
    form, n, rest = name.split("_")
    return {"form": form, "n": int(n[1:]), "rest": rest == "rest", "rotmat": False}


def model(synth_model, form):
    """A model created under SMPLPP_SKIN = form (read at creation; "default" = unset)."""
    from smplpp_amd.smpl import SMPL

    old = os.environ.pop("SMPLPP_SKIN", None)
    try:
        if form != "default":
            os.environ["SMPLPP_SKIN"] = form
        s = SMPL()
        s.setDevice("cuda:0")
        s.init(synth_model)
    finally:
        os.environ.pop("SMPLPP_SKIN", None)
        if old is not None:
            os.environ["SMPLPP_SKIN"] = old
    return s


def inputs(name):
    from smplpp_amd import model_io

    n = case(name)["n"]
    beta, theta = model_io.synthetic_inputs(n, seed=1000 + n)
    return {"beta": beta, "theta": theta}


def outputs(name, smpl, x):
    """What the case returns, through the Python binding in host space (`rest` only where the case wants it)."""
    c = case(name)
    want = ("verts", "joints", "xforms") + (("rest",) if c["rest"] else ())
    if c["rotmat"]:
        rot = smpl.axisAngleToRotmat(x["theta"][:, 1:])
        out = smpl.launchRotmat(x["beta"], np.ascontiguousarray(x["theta"][:, 0]), rot, want=want)
    else:
        out = smpl.launch(x["beta"], x["theta"], want=want)
    return {k: np.asarray(out[k]) for k in want}
