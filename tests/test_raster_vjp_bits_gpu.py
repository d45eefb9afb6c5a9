"""The backward bits of the three image-space terms (smplpp_depth_raster_vjp, smplpp_raster_interpolate_vjp, smplpp_silhouette_vjp)
against tests/golden/raster_vjp_bits.json, on the cases of tests/raster_vjp_cases.py.  The other tests hold these gradients to
float64 autograd within a tolerance and to each other; this one holds every bit, so an edit of the face walk, its lane tree, the
channel chunks or the vertex gather that moves one shows.  The input digests are asserted first: a drift of numpy's generators, of a
fixture or of the rasteriser's forward reads as "inputs", not as a gradient."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_vjp_cases as RC  # noqa: E402

import torch  # noqa: E402
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(RC.GOLDEN) as f:
        return json.load(f)["cases"]


def _differs(got, want):
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    return [k for k in sorted(want) if RC.digest(got[k]) != want[k]]


@pytest.mark.parametrize("name", RC.NAMES)
def test_backward_bits(golden, synth_model, name):
    s, v, cams, H, W = RC.scene(name, synth_model)
    x = RC.inputs(name, s, v, cams, H, W)
    bad = _differs(x, golden[name]["inputs"])
    assert not bad, "inputs differ from the recorded ones (fixture, not kernel): %s" % bad
    y = RC.outputs(s, x, H, W)
    assert all(np.abs(a).max() > 0 for a in y.values())
    bad = _differs(y, golden[name]["outputs"])
    assert not bad, "gradient bits differ from the recorded ones: %s" % bad
    if name == "body":  # the same calls on device tensors: the host-space bits
        yd = RC.outputs(s, x, H, W, to=lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda(), back=lambda t: t.cpu().numpy())
        bad = _differs(yd, golden[name]["outputs"])
        assert not bad, "device-space gradient bits differ from the recorded host-space ones: %s" % bad
