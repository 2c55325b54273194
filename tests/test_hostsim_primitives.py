"""The serial host twin (tests/hostsim/backend_host.cpp) pinned to numpy primitive by primitive: the cases of
primitive_cases.py on the CPU, and the inventory that keeps every declaration of csrc/backend.h tied to a case."""
import os
import re

import pytest

import primitive_cases as pcases
from hostsim_util import hostsim_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return hostsim_lib()


@pytest.mark.parametrize("case", pcases.CASES, ids=lambda f: f.__name__)
def test_primitive(lib, case):
    case(lib)


def _declared_in_backend_h():
    txt = open(os.path.join(ROOT, "geneo4petsc_amd", "csrc", "backend.h")).read()
    txt = re.sub(r"//[^\n]*", "", txt)
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = txt[txt.index("namespace bk"):]
    txt = re.sub(r"\bstruct\s+\w+\s*\{.*?\n\};", "", txt, flags=re.S)      # data members are not functions
    txt = re.sub(r"\benum\s*\{.*?\};", "", txt, flags=re.S)
    txt = re.sub(r"\{[^{}]*\}", ";", txt)                                    # bodies of inline functions
    return set(re.findall(r"\b([A-Za-z_]\w*)\s*\(", txt))


def test_every_backend_function_has_a_case_or_an_exemption():
    declared = _declared_in_backend_h()
    assert len(declared) > 100 and {"chol_solve", "csr_has_lp", "side_stream_begin", "zero"} <= declared
    missing = sorted(declared - set(pcases.INVENTORY))
    assert not missing, "declared in backend.h without a case or an exemption in primitive_cases.INVENTORY: %s" % missing
    stale = sorted(set(pcases.INVENTORY) - declared)
    assert not stale, "in INVENTORY but no longer declared in backend.h: %s" % stale
    kernels_py = open(os.path.join(ROOT, "tests", "test_gpu_kernels.py")).read()
    listed = {f.__name__ for f in pcases.CASES}
    for fn, entry in pcases.INVENTORY.items():
        if isinstance(entry, tuple):
            assert entry[0] == "exempt" and entry[1] in pcases.EXEMPT_REASONS, (fn, entry)
            continue
        assert entry, fn
        for ref in entry:
            if ref.startswith("test_gpu_kernels.py::"):
                assert re.search(r"^def %s\(" % re.escape(ref.split("::")[1]), kernels_py, flags=re.M), (fn, ref)
            else:
                assert ref in listed and callable(getattr(pcases, ref)), (fn, ref)
