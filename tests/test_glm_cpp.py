"""tests/cpp/test_glm.cpp: GeneralizedLinearModel and the SVGD class's
device-model step (C++ API) against a manual loop of the split C calls with
host gradients.  ``make cpp`` builds it as build/test_glm; it runs on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")


def _make_cpp():
    r = subprocess.run(["make", "-s", "-C", ROOT, "cpp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(BUILD, "test_glm"))


def test_cpp_glm_builds():
    _make_cpp()


@pytest.mark.gpu
def test_cpp_glm_device_step_matches_host_gradient_loop():
    _make_cpp()
    r = subprocess.run([os.path.join(BUILD, "test_glm")], capture_output=True, text=True, timeout=300, cwd=BUILD)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
