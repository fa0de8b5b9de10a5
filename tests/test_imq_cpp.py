"""tests/cpp/test_imq.cpp: the C++ InverseMultiquadricKernel on SVGD's device
path against the generic host path, a manual loop and the logged matrices'
definition.  ``make cpp`` builds it as build/test_imq; it runs on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")


def _make_cpp():
    r = subprocess.run(["make", "-s", "-C", ROOT, "cpp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(BUILD, "test_imq"))


def test_cpp_imq_builds():
    _make_cpp()


@pytest.mark.gpu
def test_cpp_imq_class_on_the_device_path():
    _make_cpp()
    r = subprocess.run([os.path.join(BUILD, "test_imq")], capture_output=True, text=True, timeout=300, cwd=BUILD)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
