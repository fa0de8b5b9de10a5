"""tests/cpp/test_mmd.cpp: SVGD::ComputeMMD (C++ API) of both kernels against
svgd_mmd_host within 1e-12 absolute, the dimension-mismatch exception and the
unknown-kernel std::invalid_argument, N = 300, d = 2.  ``make cpp`` builds it
as build/test_mmd; it runs on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")


def _make_cpp():
    r = subprocess.run(["make", "-s", "-C", ROOT, "cpp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(BUILD, "test_mmd"))


def test_cpp_mmd_builds():
    _make_cpp()


@pytest.mark.gpu
def test_cpp_mmd_matches_the_host_form():
    _make_cpp()
    r = subprocess.run([os.path.join(BUILD, "test_mmd")], capture_output=True, text=True, timeout=300,
                       cwd=BUILD)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
