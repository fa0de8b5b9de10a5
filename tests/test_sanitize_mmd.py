"""The host MMD under AddressSanitizer + UndefinedBehaviorSanitizer (CPU).

`make sanitize_mmd` builds host_mmd.cpp with -fsanitize=address,undefined
into a self-checking stand-alone driver (tests/cpp/sanitize_mmd.cpp) and runs
it; any sanitizer report aborts the driver (-fno-sanitize-recover=all).
Nothing is loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_host_mmd_under_asan_ubsan():
    r = subprocess.run(["make", "-C", ROOT, "sanitize_mmd"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
