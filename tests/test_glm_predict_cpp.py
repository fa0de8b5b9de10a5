"""tests/cpp/test_glm_predict.cpp: the C++ SVGD class's Predict (device)
against GeneralizedLinearModel::Predict (host) at the coordinates Run()
returned, within the bars of tests/_glm_predict.py.  ``make cpp`` builds it as
build/test_glm_predict; it runs on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")


def _make_cpp():
    r = subprocess.run(["make", "-s", "-C", ROOT, "cpp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(BUILD, "test_glm_predict"))


def test_cpp_glm_predict_builds():
    _make_cpp()


@pytest.mark.gpu
def test_cpp_glm_predict_matches_host_model():
    _make_cpp()
    r = subprocess.run([os.path.join(BUILD, "test_glm_predict")], capture_output=True, text=True, timeout=300,
                       cwd=BUILD)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
