"""Worker of tests/test_gpu_block_rhs.py::test_released_memory: the readings of block_rhs_util.memory_readings on the HIP
library in a process of its own (started with GENEO_ALLOC_CACHE=0), one JSON line on stdout."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if __name__ == "__main__":
    import block_rhs_util as U
    from geneo4petsc_amd import _lib
    print("READINGS " + json.dumps(U.memory_readings(_lib.load())))
