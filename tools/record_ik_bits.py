"""Record tests/golden/ik_bits.json: one SHA-256 per input array and per result of every case of tests/ik_bits_cases.py, run
through the Python binding on one MI355X in host space.

The file pins the bits of the library build it was recorded from; tests/test_ik_bits_gpu.py holds every later build to it.  It is
recorded once, from a build whose bits are the ones to keep, and not again after a change to the IK loop's host side or kernels: a
mismatch after such a change is the change's to explain.

    python tools/record_ik_bits.py [--out tests/golden/ik_bits.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ik_bits_cases as IC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=IC.GOLDEN)
    a = ap.parse_args()
    from oracle import cpu
    from oracle import vposer_torch as VT
    from smplpp_amd import model_io
    from smplpp_amd.ik import VPoserDecoder
    from smplpp_amd.smpl import SMPL

    synth = model_io.synthetic_model()
    smpl = SMPL()
    smpl.setDevice("cuda:0")
    smpl.init(synth)
    params = VPoserDecoder.synthetic_params()
    gpu, ref = VPoserDecoder(params), VT.VPoserDecoder(params)
    om = cpu.OracleModel(synth)
    res = {"digest": "sha256 of the array's little-endian bytes", "cases": {}}
    for name in IC.NAMES:
        x = IC.inputs(name, om, ref)
        y = IC.outputs(name, smpl, gpu, x)
        assert not y["status"].any(), (name, y["status"])
        res["cases"][name] = {"inputs": {k: IC.digest(b) for k, b in sorted(x.items())},
                              "outputs": {k: IC.digest(b) for k, b in sorted(y.items())}}
        print("%s: %d inputs, %d outputs" % (name, len(x), len(y)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
