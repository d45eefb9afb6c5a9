"""Models whose kinematic tree the pose kernel's chain table does not cover (model_tables.h, chain_tables: more than CT_LEV levels,
or a level of more than 5 joints) run the kernel's generic loop: FK against the C oracle, under the default forms and SMPLPP_SKIN=h.
Tolerance: that of the tiny-model cases of tests/test_fk_gpu.py."""
import numpy as np
import pytest

from test_fk_gpu import VERT_TOL

pytestmark = pytest.mark.gpu


def _model(tree):
    from smplpp_amd import model_io

    md = model_io.tiny_model(61, seed=7)
    for i in range(1, 24):
        md["kinematic_tree"][0, i] = i - 1 if tree == "chain" else 0
    return md


@pytest.mark.parametrize("form", [None, "h"])
@pytest.mark.parametrize("tree", ["chain", "star"])
def test_fk_on_trees_outside_the_chain_table(tree, form, monkeypatch):
    from oracle.cpu import OracleModel
    from smplpp_amd import model_io
    from smplpp_amd.smpl import SMPL

    if form is None:
        monkeypatch.delenv("SMPLPP_SKIN", raising=False)
    else:
        monkeypatch.setenv("SMPLPP_SKIN", form)
    md = _model(tree)
    s = SMPL()
    s.setDevice("cuda:0")
    s.init(md)
    assert s.info()["weights_per_vertex"] == 24
    beta, theta = model_io.synthetic_inputs(3, seed=61)
    g = s.launch(beta, theta)
    r = OracleModel(md).fk(beta, theta)
    for k in ("verts", "rest", "joints", "xforms"):
        err = float(np.abs(g[k] - r[k]).max())
        print(tree, form, k, err)
        assert err < VERT_TOL, (tree, form, k)


def test_ik_refuses_a_tree_deeper_than_its_tables():
    from smplpp_amd._lib import SmplppError
    from smplpp_amd.ik import IkSolver
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(_model("chain"))
    with pytest.raises(SmplppError, match="smplpp_ik_create: kinematic trees deeper than 12 levels are not supported"):
        IkSolver(s, 2, 4)
