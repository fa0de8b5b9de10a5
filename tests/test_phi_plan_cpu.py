"""The phi plan without a GPU: svgd_plan_phi_name runs the same plan_phi a
context's creation runs (same knobs, same capability answers of the kernel
translation unit) and formats the same name, so the dispatch tables of
tests/_dispatch.py are verified before anything is sent to a GPU
(tests/test_gpu_dim_sweep.py asserts that a context reports the same name).
Also: the knob reader and the documented knob table name the same variables.
"""
import os
import re

import pytest

import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

from _dispatch import F32_TABLE, F32_VARIANTS, F64_TABLE, KNOBS, expected_name, knob_value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    """Every case starts from the library's defaults; a case sets what it needs."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("d", range(1, 65))
@pytest.mark.parametrize("dtype,table", [(C.SVGD_F64, F64_TABLE), (C.SVGD_F32, F32_TABLE)],
                         ids=["f64", "f32"])
def test_plan_dispatch_table(dtype, table, d):
    assert S.plan_phi_name(d, 333, dtype) == expected_name(table, d)


@pytest.mark.parametrize("d,knob,name", [v for v in F32_VARIANTS if v[1]])
def test_plan_f32_knob_rows(monkeypatch, d, knob, name):
    monkeypatch.setenv(knob, knob_value(knob))
    assert S.plan_phi_name(d, 333, C.SVGD_F32) == name


@pytest.mark.parametrize("d,ncb", [(32, 3), (48, 4), (64, 5)])
def test_plan_f64_ones_column(monkeypatch, d, ncb):
    """SVGD_PHI_S1V=0: pick_tiles' NCB (a V column of ones), the non-S1V kernel."""
    monkeypatch.setenv("SVGD_PHI_S1V", "0")
    kp = 32 if d <= 32 else 64
    assert S.plan_phi_name(d, 333, C.SVGD_F64) == "k_phi<double, %d, %d, 8, true, false>" % (kp, ncb)


def test_plan_b3_row_groups(monkeypatch):
    monkeypatch.setenv("SVGD_PHI_B3_RG", "2")
    assert S.plan_phi_name(20, 333, C.SVGD_F32) == "k_phi_b3<32, 2, 8, false, 2>"
    assert S.plan_phi_name(64, 333, C.SVGD_F32) == "k_phi_b3<64, 4, 8, true, 2>"
    assert S.plan_phi_name(16, 333, C.SVGD_F32) == "k_phi_f32s<16, 2>"  # (no bf16 kernel: no effect)
    monkeypatch.setenv("SVGD_PHI_B3_RG", "3")  # anything but 2 is 1
    assert S.plan_phi_name(20, 333, C.SVGD_F32) == "k_phi_b3<32, 2, 8, false, 1>"


@pytest.mark.parametrize("d", [1, 8, 9])
def test_plan_sym_thresholds(monkeypatch, d):
    """The symmetric pass: d <= 8, N >= 32768 and N / P >= 8192; SVGD_PHI_SYM
    replaces the sizes, never the dimension."""
    rows = expected_name(F64_TABLE, d)
    sym = "k_phi_sym<%d>" % d if d <= 8 else rows
    f64 = C.SVGD_F64
    assert S.plan_phi_name(d, 32767, f64) == rows
    assert S.plan_phi_name(d, 32768, f64) == sym
    for rank in (0, 3, 7):
        assert S.plan_phi_name(d, 65536, f64, 8, rank) == sym   # N / P = 8192
        assert S.plan_phi_name(d, 65535, f64, 8, rank) == rows  # N / P = 8191
    monkeypatch.setenv("SVGD_PHI_SYM", "0")
    assert S.plan_phi_name(d, 32768, f64) == rows
    assert S.plan_phi_name(d, 65536, f64, 8, 0) == rows
    for v in ("1", "2"):
        monkeypatch.setenv("SVGD_PHI_SYM", v)
        assert S.plan_phi_name(d, 333, f64) == sym
        assert S.plan_phi_name(d, 65535, f64, 8, 5) == sym
    assert S.plan_phi_name(d, 32768, C.SVGD_F32) == expected_name(F32_TABLE, d)  # fp64 only


def test_plan_unaligned_shard_takes_generic_f32():
    """The streamed F32 kernels (k_phi_f32s, k_phi_b3) give each wave 16-row
    groups of the padded rows, so a shard whose first row is no multiple of
    16 runs the generic fp32 tile kernel -- with the tile class the streamed
    plan chose (NCB = d / 16 at d = 32).  svgd_plan_rows reaches this on
    every rank > 0 whose ceil(n / world) * rank is no multiple of 16: n = 333
    over 2 ranks (rank 1 starts at row 167), n = 1000 over 3 (334, 668)."""
    f32 = C.SVGD_F32
    assert S.plan_phi_name(20, 333, f32, 2, 0) == "k_phi_b3<32, 2, 8, false, 1>"
    assert S.plan_phi_name(20, 333, f32, 2, 1) == "k_phi<float, 32, 2, 4, false, false>"
    assert S.plan_phi_name(32, 333, f32, 2, 1) == "k_phi<float, 32, 2, 4, false, true>"
    assert S.plan_phi_name(16, 333, f32, 2, 1) == "k_phi<float, 16, 2, 4, false, false>"
    assert S.plan_phi_name(50, 1000, f32, 3, 1) == "k_phi<float, 64, 4, 4, false, false>"
    assert S.plan_phi_name(50, 1000, f32, 3, 2) == "k_phi<float, 64, 4, 4, false, false>"
    # 16-aligned shards stay streamed (n = 320 over 2: row 160), and fp64 has no such rule
    assert S.plan_phi_name(20, 320, f32, 2, 1) == "k_phi_b3<32, 2, 8, false, 1>"
    assert S.plan_phi_name(14, 320, f32, 2, 1) == "k_phi_f32s<16, 1>"
    assert S.plan_phi_name(20, 333, C.SVGD_F64, 2, 1) == expected_name(F64_TABLE, 20)


def test_plan_refuses_bad_arguments():
    with pytest.raises(S.DimensionMismatchException):
        S.plan_phi_name(65, 333)
    with pytest.raises(ValueError):
        S.plan_phi_name(8, 333, world=2, rank=2)


def test_knob_reader_matches_documented_table():
    """Every SVGD_* variable the library reads is named once, in read_knobs
    (ctx_create.cpp), and INTEGRATION.md section 7 documents exactly that set."""
    csrc = os.path.join(ROOT, "svgdcpp_amd", "csrc")
    src = open(os.path.join(csrc, "ctx_create.cpp")).read()
    body = src[src.index("Knobs read_knobs()"):]
    body = body[:body.index("\n}\n")]
    read = re.findall(r'"(SVGD_[A-Z0-9_]+)"', body)
    assert len(read) == len(set(read)) >= 20, read
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## 7. Tuning knobs"):]
    sec = sec[:sec.index("\n## ", 1)] if "\n## " in sec[1:] else sec
    rows = re.findall(r"^\| `(SVGD_[A-Z0-9_]+)` \|", sec, flags=re.M)
    assert len(rows) == len(set(rows)), rows
    assert set(rows) == set(read)
    # the environment is read nowhere else in the library
    assert src.count("getenv") == body.count("getenv")
    others = [f for f in sorted(os.listdir(csrc))
              if f.endswith((".cpp", ".hip", ".h", ".inc")) and f != "ctx_create.cpp"]
    assert len(others) >= 30, others
    for f in others:
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f
