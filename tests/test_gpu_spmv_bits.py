"""-m gpu: the single-vector sparse products and every fused epilogue give the recorded bits.

k_spmv_sell, k_spmv_sell_epi, k_spmv_sell_wide, k_spmv_sell_lp (and the epilogues of k_spmv_vec and the SpMM kernels) sum in
a fixed order, so their outputs are reproducible to the bit.  tests/golden/spmv_bits.json holds the sha256 of every output
of the cases in spmv_bits_cases.py, computed by the commit before the four sliced kernels were folded into one traversal
(tests/golden/make_spmv_bits_goldens.py); a change to these kernels that is meant to keep behaviour has to reproduce them.
Bits are promised per compiler, not across compilers: with another compiler string in the library the test skips."""
import json

import numpy as np
import pytest

import spmv_bits_cases as sbc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from geneo4petsc_amd import _lib
    return _lib.load()          # raises if the HIP library is missing: no fallback


@pytest.fixture(scope="module")
def golden():
    from geneo4petsc_amd import _lib
    with open(sbc.GOLDEN) as f:
        data = json.load(f)
    here = sbc.compiler_string(_lib.LIB_PATH)
    if data["compiler"] != here:
        pytest.skip("spmv_bits.json was recorded with another compiler (%s), this library was built with %s: bits are "
                    "promised per compiler" % (data["compiler"], here))
    return data["digests"]


def test_every_case_has_goldens(golden):
    assert sorted(golden) == sorted(sbc.CASES)


@pytest.mark.parametrize("name", list(sbc.CASES))
def test_same_bits_as_recorded(lib, golden, name):
    a, inputs, out = sbc.run_case(lib, name)
    got, want = sbc.digests(out), golden[name]
    assert sorted(got) == sorted(want)
    bad = [k for k in got if got[k] != want[k]]
    if bad:     # the recorded outputs themselves are not kept: say how far each is from the FP64 algebra
        ref = sbc.scipy_products(a, inputs)
        for k in bad:
            print("%s / %s: digest differs; largest |output - scipy| = %.3e" % (name, k, np.abs(out[k] - ref(k)).max()))
    assert not bad, "%s: outputs with other bits than recorded: %s" % (name, bad)
