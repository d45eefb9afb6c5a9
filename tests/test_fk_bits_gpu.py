"""The bits smplpp_fk and smplpp_fk_rotmat return (verts, rest, joints, xforms) against tests/golden/fk_bits.json, on the cases of
tests/fk_bits_cases.py: every form of the fused kernel, with and without `rest`, at batch sizes that are a lone frame, a full frame
tile, a tile plus one frame and enough tiles for a workgroup's run to change its frame tile.  The other FK tests hold these results
to the oracle within a bound; this one holds every bit, so an edit of the forward pass's host side (smplpp_amd/csrc/fk_plan.h, the
launchers) that hands a workgroup other items, cuts the batch elsewhere or sizes the workspace differently shows.  The input
digests are asserted first: a drift of numpy's generators reads as "inputs", not as the kernels."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fk_bits_cases as FC  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(FC.GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def models(synth_model):
    return {form: FC.model(synth_model, form) for form in FC.FORMS}


def _differs(got, want):
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    return [k for k in sorted(want) if FC.digest(got[k]) != want[k]]


def test_the_cases_are_the_recorded_ones(golden):
    assert sorted(golden) == sorted(FC.NAMES) and len(FC.NAMES) == 4 * 4 * 2 + 1


@pytest.mark.parametrize("name", FC.NAMES)
def test_fk_bits(golden, models, name):
    x = FC.inputs(name)
    bad = _differs(x, golden[name]["inputs"])
    assert not bad, "inputs differ from the recorded ones (fixture, not kernels): %s" % bad
    y = FC.outputs(name, models[FC.case(name)["form"]], x)
    bad = _differs(y, golden[name]["outputs"])
    assert not bad, "the forward pass's bits differ from the recorded ones: %s" % bad
