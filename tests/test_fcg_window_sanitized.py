"""The window bookkeeping of the flexible CG (geneo4petsc_amd/csrc/fcg_window.h: ring slot, window size, offset in the
doubled pointer table, eta ring) in a stand-alone program with its own main, built with -fsanitize=address,undefined and run
on the host.  Nothing is loaded into Python: the program is what the sanitizers see."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fcg_window_bookkeeping_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fcg_window_check")
    src = os.path.join(ROOT, "tests", "sanitize", "fcg_window_main.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # the runtimes are part of the program
                           "-I", os.path.join(ROOT, "geneo4petsc_amd", "csrc"), src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fcg_window: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
