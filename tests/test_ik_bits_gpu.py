"""The bits the IK loop leaves behind (theta, beta, faces, vertex weights, |e|^2, status, the last step) against
tests/golden/ik_bits.json, on the cases of tests/ik_bits_cases.py: one per solve instantiation, one per branch of the face scan's
dispatch, and the two sequence drivers in the latent layout.  The other IK tests hold these results to float64 references within a
bound; this one holds every bit, so an edit of the loop's host side (smplpp_amd/csrc/ik_plan.h, ik_iterate_enqueue) that launches
another instantiation, another LDS size or another schedule shows.  The input digests are asserted first: a drift of numpy's
generators or of the CPU oracle reads as "inputs", not as the solver."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ik_bits_cases as IC  # noqa: E402
import solve_ref as S  # noqa: E402
from test_projection_gpu import _scan_form  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(IC.GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def smpl(synth_model):
    from smplpp_amd.smpl import SMPL

    s = SMPL()
    s.setDevice("cuda:0")
    s.init(synth_model)
    return s


@pytest.fixture(scope="module")
def decoders():
    from oracle import vposer_torch as VT
    from smplpp_amd.ik import VPoserDecoder

    params = VPoserDecoder.synthetic_params()
    return VPoserDecoder(params), VT.VPoserDecoder(params)


@pytest.fixture(scope="module")
def oracle_model(synth_model):
    from oracle import cpu

    return cpu.OracleModel(synth_model)


def _differs(got, want):
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    return [k for k in sorted(want) if IC.digest(got[k]) != want[k]]


def test_the_cases_reach_every_solve_instantiation_and_every_scan_branch(oracle_model):
    assert [S.case_plan(IC.case(n))["kernel"] for n in IC.SOLVE] == ["dual", "ntr3", "ntr5", "ntr6", "ntr11", "ntr6"]
    assert S.case_plan(IC.case("lds_k46_beta"))["first_factor"] == "lds"
    forms = []
    for c in IC.SCAN:
        blocks = int(c["env"]["SMPLPP_SCAN_BLOCKS"]) if "SMPLPP_SCAN_BLOCKS" in c["env"] else None
        chunks, kpr, nbt = _scan_form(c["n"], c["K"], oracle_model.F, blocks, int(c["env"].get("SMPLPP_SCAN_FORM", -1)))
        assert (kpr, nbt) == c["form"], c["name"]
        forms.append((c["K"] <= 8 and "SMPLPP_SCAN_FORM" in c["env"], kpr, nbt))
    assert len(set(forms)) == 6  # (the K <= 8 "many" branches launch the K > 8 instantiations: six branches, four kernels)


@pytest.mark.parametrize("name", IC.NAMES)
def test_ik_bits(golden, smpl, decoders, oracle_model, name):
    x = IC.inputs(name, oracle_model, decoders[1])
    bad = _differs(x, golden[name]["inputs"])
    assert not bad, "inputs differ from the recorded ones (fixture, not solver): %s" % bad
    y = IC.outputs(name, smpl, decoders[0], x)
    assert not y["status"].any(), y["status"]
    bad = _differs(y, golden[name]["outputs"])
    assert not bad, "the IK loop's bits differ from the recorded ones: %s" % bad
