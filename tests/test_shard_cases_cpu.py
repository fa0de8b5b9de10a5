"""The sharded-path table of tests/_shard_cases.py against the plan, without a
GPU: every rank of every case plans the kernel the case names and owns the
rows its comment claims, and the table as a whole reaches what it is there
for -- each phi kernel family at row0 != 0 and every S1V tile class in its
float k_phi form (the unaligned-shard kernel).  A later reroute that drops
that coverage turns this red.  The GPU test (tests/test_gpu_shard_paths.py)
asserts each rank's phi_kernel_name() against the same prefixes.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import svgdcpp_amd as S
from svgdcpp_amd import _capi as C

import _shard_cases as T
import _update_cases as U
from _dispatch import KNOBS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    """Every case starts from the library's defaults; a case sets what it needs."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _rows(n, world, rank):
    r0, r1 = ctypes.c_int64(), ctypes.c_int64()
    C.lib().svgd_plan_rows(n, world, rank, ctypes.byref(r0), ctypes.byref(r1))
    return r0.value, r1.value


def _set_env(monkeypatch, case):
    for k, v in case.env.items():
        assert k in KNOBS, k  # (only knobs the fixture clears)
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_case_plans_its_kernels(monkeypatch, case):
    _set_env(monkeypatch, case)
    assert len(case.names) == case.world <= 3
    for rank in range(case.world):
        name = S.plan_phi_name(case.d, case.n, T.dtype_of(case), case.world, rank)
        assert name.startswith(case.names[rank]), (case.id, rank, name)


def test_knob_cases_differ_from_the_defaults():
    """Without its knobs a knob case plans another kernel on rank 1."""
    for case in T.CASES:
        if case.env:
            name = S.plan_phi_name(case.d, case.n, T.dtype_of(case), case.world, 1)
            assert not name.startswith(case.names[1]), (case.id, name)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.id)
def test_case_shards_are_what_it_claims(case):
    shards = [_rows(case.n, case.world, r) for r in range(case.world)]
    assert shards[0][0] == 0 and shards[-1][1] == case.n
    assert all(a[1] == b[0] for a, b in zip(shards, shards[1:]))
    chunk = -(-case.n // case.world)
    if case.shards == "empty":
        assert case.n == 2 and case.world == 3
        assert shards == [(0, 1), (1, 2), (2, 2)]
        return
    assert case.n <= 500 and case.n % 64 != 0 and case.n > 2 * 64  # a padded last tile of several
    assert all(r1 > r0 for r0, r1 in shards)
    wg = 128 if case.dtype == "f64" else 64  # rows per work-group (k_phi<double>: 16 x 8 waves)
    assert any((r1 - r0) % wg for r0, r1 in shards)  # a ragged last work-group
    if case.shards == "unaligned":
        assert all(r0 % 16 for r0, _ in shards[1:])
        want = {2: [(0, 167), (167, 333)], 3: [(0, 167), (167, 334), (334, 500)]}[case.world]
        assert shards == want
    else:
        assert case.shards == "aligned" and case.dtype == "f32"
        assert chunk == 176 == 16 * 11 and shards == [(0, 176), (176, 351)]
        assert (shards[1][1] - shards[1][0]) % 16  # the last 16-row group is ragged too


def test_unaligned_f32_ranks_mix_kernels():
    """An F32 case with an unaligned shard runs the streamed kernel on rank 0
    and the generic one elsewhere (d <= 12 has no streamed kernel); an aligned
    one runs the streamed kernel everywhere."""
    for case in T.CASES:
        if case.dtype != "f32":
            continue
        streamed = [nm.startswith(("k_phi_f32s<", "k_phi_b3<")) for nm in case.names]
        if case.shards == "aligned":
            assert all(streamed), case.id
        else:
            assert streamed[0] == (case.d > 12), case.id
            assert not any(streamed[1:]), case.id
            assert all(nm.startswith("k_phi<float,") for nm in case.names[1:]), case.id


def _tiles_s1v():
    """TILES_S1V of built.h."""
    src = open(os.path.join(ROOT, "svgdcpp_amd", "csrc", "built.h")).read()
    m = re.search(r"TileClass TILES_S1V\[\] = \{(.*?)\};", src, flags=re.S)
    tiles = [(int(a), int(b)) for a, b in re.findall(r"\{(\d+), (\d+)\}", m.group(1))]
    assert len(tiles) >= 3, tiles
    return tiles


def test_table_names_every_float_s1v_class():
    """k_phi<float, KP, NCB, 4, false, true> of every S1V class, each on a
    rank whose shard does not start at row 0 (the only way to reach it)."""
    named = {nm for c in T.CASES for r, nm in enumerate(c.names) if r > 0}
    for kp, ncb in _tiles_s1v():
        assert "k_phi<float, %d, %d, 4, false, true>" % (kp, ncb) in named, (kp, ncb)
        # ... and the fp64 form of the class sharded as well
        assert "k_phi<double, %d, %d, 8, true, true>" % (kp, ncb) in named, (kp, ncb)


def test_table_runs_every_family_off_row_zero():
    fams = {"k_phi<double,": 0, "k_phi<float,": 0, "k_phi_f32s<": 0, "k_phi_b3<": 0}
    for case in T.CASES:
        for rank in range(1, case.world):
            r0, r1 = _rows(case.n, case.world, rank)
            for f in fams:
                if case.names[rank].startswith(f) and r0 != 0 and r1 > r0:
                    fams[f] += 1
    assert all(v > 0 for v in fams.values()), fams
    assert len({c.id for c in T.CASES}) == len(T.CASES)
    # the generic fp32 classes no one-rank knob reaches (tests/test_phi_plan_cpu.py)
    named = {nm for c in T.CASES for nm in c.names}
    for nm in ("k_phi<float, 64, 4, 4, false, false>", "k_phi<float, 16, 1, 4, false, false>"):
        assert nm in named, nm


def test_subsets_name_cases_of_the_table():
    for ids in (T.MATRIX_CASES, T.STEP_CASES, T.BITWISE_CASES):
        assert all(i in T.BY_ID for i in ids)
    assert {T.BY_ID[i].dtype for i in T.MATRIX_CASES} == {"f64", "f32"}
    assert {(T.BY_ID[i].dtype, T.BY_ID[i].shards) for i in T.STEP_CASES} == {
        ("f64", "unaligned"), ("f32", "unaligned"), ("f32", "aligned")}
    # every optimizer on every dtype
    assert {(c.dtype, T.opt_of(c)) for c in T.CASES} == {(t, o) for t in ("f64", "f32") for o in T.OPTS}


def test_inputs_can_exercise_the_bounds(oracle):
    """X_0 at scale 1 against the per-dimension boxes of _update_cases.bounds:
    every bounded dimension starts with particles outside its box, and
    dimension 1 (unbounded) with values beyond every box by more than three
    steps of lr = 0.1 can bring back -- so assert_bounds_exercised can hold
    on the GPU result (with two particles: for some dimension, not every)."""
    import _gpu_shard_rank_worker as W
    for n, d in sorted({(c.n, c.d) for c in T.CASES}):
        X, G, a = W.inputs(n, d)
        assert np.all(G[0] == 0.0) and np.isfinite(a) and a > 0
        lo, up = U.bounds(d)
        fin = [k for k in range(d) if np.isfinite(lo[k])]
        outside = [bool(np.any(X[:, k] < lo[k]) or np.any(X[:, k] > up[k])) for k in fin]
        assert all(outside) if n > 2 else any(outside[:-1]), (n, d)
        assert np.any(X[:, 1] > max(up[k] for k in fin) + 0.3) or np.any(X[:, 1] < min(lo[k] for k in fin) - 0.3), (n, d)
