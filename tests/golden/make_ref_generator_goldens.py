#!/usr/bin/env python3
"""Generates tests/golden/ref_generators.npz: the meshes the reference's own input generators (tst/laplacian, tst/heat,
tst/graph getInput plugins, built into oracle/_ref by oracle/ref_build/Makefile where the reference sources are present)
return for the cases of tests/test_oracle_ref_generators.py -- element pointers, element nodes and element matrices, bit
for bit.  With it the test compares the oracle's and the product's generators with the reference's output anywhere.

    python tests/golden/make_ref_generator_goldens.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_generators as rg      # noqa: E402
import test_oracle_ref_generators as t       # noqa: E402


def main():
    if not rg.available():
        raise SystemExit("oracle/_ref not built: the reference generators are needed to record the golden")
    keys, arrays = [], {}
    for plugin, args in t.golden_cases():
        m = rg.get_input(plugin, args)
        i = len(keys)
        keys.append(t.golden_key(plugin, args))
        arrays["c%d_dims" % i] = np.array([m.nbElem, m.nbNode], dtype=np.int64)
        arrays["c%d_ptr" % i] = np.array(m.elemPtr[:m.nbElem + 1], dtype=np.int64)
        arrays["c%d_idx" % i] = np.array(m.elemIdx, dtype=np.int64)
        arrays["c%d_mat" % i] = np.array([v for e in m.elemSubMat for v in e], dtype=np.float64)
    np.savez_compressed(t.GOLDEN, keys=np.array(keys), **arrays)
    print("%s: %d cases, %d bytes" % (t.GOLDEN, len(keys), os.path.getsize(t.GOLDEN)))


if __name__ == "__main__":
    main()
