"""Record tests/golden/raster_vjp_bits.json: one SHA-256 per input array and per gradient of every case of
tests/raster_vjp_cases.py, run through the Python binding on one MI355X in host space.

The file pins the bits of the library build it was recorded from; tests/test_raster_vjp_bits_gpu.py holds every later build to it.
It is recorded once, from a build whose backward bits are the ones to keep, and not again after a change to the kernels: a
mismatch after such a change is the change's to explain.

    python tools/record_raster_vjp_bits.py [--out tests/golden/raster_vjp_bits.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import raster_vjp_cases as RC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=RC.GOLDEN)
    a = ap.parse_args()
    from smplpp_amd import model_io

    synth = model_io.synthetic_model()
    res = {"digest": "sha256 of the array's little-endian bytes", "cases": {}}
    for name in RC.NAMES:
        s, v, cams, H, W = RC.scene(name, synth)
        x = RC.inputs(name, s, v, cams, H, W)
        y = RC.outputs(s, x, H, W)
        res["cases"][name] = {"inputs": {k: RC.digest(b) for k, b in sorted(x.items())},
                              "outputs": {k: RC.digest(b) for k, b in sorted(y.items())}}
        print("%s: %d inputs, %d outputs" % (name, len(x), len(y)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
