#!/usr/bin/env python3
"""Generates tests/golden/spmv_bits.json on a machine with an MI355X: for every case of tests/spmv_bits_cases.py the sha256
of the bytes of each output of Spmv.apply, Spmv.fused and Spmv.fused_single (through the C ABI of libgeneopc.so), and the
compiler string of the library that computed them.  Run it with the library built from the commit whose bits are the
reference (the parent of a kernel refactor); tests/test_gpu_spmv_bits.py then holds every later build to them.

    python tests/golden/make_spmv_bits_goldens.py [output.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spmv_bits_cases as sbc                 # noqa: E402
from geneo4petsc_amd import _lib              # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else sbc.GOLDEN
    lib = _lib.load()
    data = {"compiler": sbc.compiler_string(_lib.LIB_PATH), "digests": {}}
    for name in sbc.CASES:
        a, inputs, out = sbc.run_case(lib, name)
        data["digests"][name] = sbc.digests(out)
        print(name, a.shape[0], "rows,", len(out), "outputs", flush=True)
    with open(out_path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out_path, "--", data["compiler"])


if __name__ == "__main__":
    main()
