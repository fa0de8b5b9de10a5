"""tests/cpp/test_ksd_imq.cpp: SVGD::ComputeKSD(unbiased, SVGD_KERNEL_IMQ) (C++
API) against the direct double-loop formula on the host, N = 300, d = 2, the
mvn_example target.  ``make cpp`` builds it as build/test_ksd_imq; it runs on
the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")


def _make_cpp():
    r = subprocess.run(["make", "-s", "-C", ROOT, "cpp"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(os.path.join(BUILD, "test_ksd_imq"))


def test_cpp_ksd_imq_builds():
    _make_cpp()


@pytest.mark.gpu
def test_cpp_compute_ksd_imq_matches_direct_formula():
    _make_cpp()
    r = subprocess.run([os.path.join(BUILD, "test_ksd_imq")], capture_output=True, text=True, timeout=300,
                       cwd=BUILD)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
