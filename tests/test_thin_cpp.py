"""tests/cpp/test_thin.cpp: SVGD::Thin (C++ API) against the definition
replayed in long double along the device's own picks, N = 300, d = 2, the
mvn_example target.  ``make cpp`` builds it as build/test_thin; it runs on
the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")


def _make_cpp():
    r = subprocess.run(["make", "-s", "-C", ROOT, "cpp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(BUILD, "test_thin"))


def test_cpp_thin_builds():
    _make_cpp()


@pytest.mark.gpu
def test_cpp_thin_is_a_valid_selection():
    _make_cpp()
    r = subprocess.run([os.path.join(BUILD, "test_thin")], capture_output=True, text=True, timeout=300,
                       cwd=BUILD)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
