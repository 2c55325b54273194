"""-m gpu: every primitive of csrc/backend.h called alone on the HIP backend and compared with numpy (the cases of
primitive_cases.py, shared with the host twin's runner test_hostsim_primitives.py)."""
import pytest

import primitive_cases as pcases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from geneo4petsc_amd import _lib
    lib = _lib.load()          # raises if the HIP library is missing: no fallback
    assert lib.GeneoBackendName() == b"hip-gfx950"
    return lib


@pytest.mark.parametrize("case", pcases.CASES, ids=lambda f: f.__name__)
def test_primitive(lib, case):
    case(lib)
