"""tests/cpp/test_glm_hess.cpp: the C++ SVGD class's device step under the
Hessian scale against a manual loop of the split C calls with the host
Hessian sum and host gradients.  ``make cpp`` builds it as
build/test_glm_hess; it runs on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")


def _make_cpp():
    r = subprocess.run(["make", "-s", "-C", ROOT, "cpp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(BUILD, "test_glm_hess"))


def test_cpp_glm_hess_builds():
    _make_cpp()


@pytest.mark.gpu
def test_cpp_glm_device_hessian_step_matches_split_loop():
    _make_cpp()
    r = subprocess.run([os.path.join(BUILD, "test_glm_hess")], capture_output=True, text=True, timeout=300,
                       cwd=BUILD)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
