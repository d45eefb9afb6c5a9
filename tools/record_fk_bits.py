"""Record tests/golden/fk_bits.json: one SHA-256 per input array and per result of every case of tests/fk_bits_cases.py, run
through the Python binding on one MI355X in host space.

The file pins the bits of the library build it was recorded from; tests/test_fk_bits_gpu.py holds every later build to it.  It is
recorded once, from a build whose bits are the ones to keep, and not again after a change to the forward pass's host side or
kernels: a mismatch after such a change is the change's to explain.

    python tools/record_fk_bits.py [--out tests/golden/fk_bits.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fk_bits_cases as FC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FC.GOLDEN)
    a = ap.parse_args()
    from smplpp_amd import model_io

    synth = model_io.synthetic_model()
    models = {form: FC.model(synth, form) for form in FC.FORMS}
    res = {"digest": "sha256 of the array's little-endian bytes", "cases": {}}
    for name in FC.NAMES:
        x = FC.inputs(name)
        y = FC.outputs(name, models[FC.case(name)["form"]], x)
        res["cases"][name] = {"inputs": {k: FC.digest(b) for k, b in sorted(x.items())},
                              "outputs": {k: FC.digest(b) for k, b in sorted(y.items())}}
        print("%s: %d inputs, %d outputs" % (name, len(x), len(y)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
