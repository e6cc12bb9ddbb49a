"""The exact IMPALA cases (impala_util) without a GPU: every case constructs and holds what its
helper asserts -- the any-order exactness bound, the fractions of zeros and of tied pool windows,
their presence on the border and on a tile seam -- and the case lists reach every kernel
instantiation. test_impala_exact_gpu.py runs the kernels on them."""
from __future__ import annotations

import pytest
import torch

import impala_util as U


@pytest.mark.parametrize("case", U.LATTICE_RES_CASES, ids=U.res_id)
def test_resblock_case_holds(case):
    inputs, g, y64, g64, stats = U.lattice_res_case(case)
    print(U.res_id(case), stats)
    assert stats["bound"] < 2 ** 24 and stats["zero_x"] >= 0.05 and stats["zero_mid"] >= 0.01
    assert len(g64) == 5 and all(bool((t == t.round()).all()) for t in [y64, g] + inputs + g64)


@pytest.mark.parametrize("case", U.LATTICE_CP_CASES, ids=U.cp_id)
def test_conv_pool_case_holds(case):
    inputs, g, p64, g64, stats = U.lattice_cp_case(case)
    print(U.cp_id(case), stats)
    H, W, scale = case[3], case[4], case[5]
    assert stats["bound"] < 2 ** 24 and (stats["tied"] >= 0.05 or H * W == 1)
    assert len(g64) == 3 and all(bool((t / scale == (t / scale).round()).all())
                                 for t in [p64] + g64)


def test_case_lists_reach_every_path():
    pairs = {c[1:3] for c in U.LATTICE_CP_CASES}
    assert pairs == {(ci, co) for ci in (1, 2, 3, 4, 16, 32) for co in (16, 32)}
    inst = lambda c: (max(c[1], 4), c[2])  # noqa: E731  (the kernel's template arguments)
    for pair in pairs:
        mine = [c for c in U.LATTICE_CP_CASES if c[1:3] == pair]
        assert {c[3] % 2 for c in mine} == {0, 1} and {c[4] % 2 for c in mine} == {0, 1}, pair
        assert any(c[3] > U.T and c[4] > U.T for c in mine), pair
        assert {c[5] for c in mine} == ({1.0, 0.25} if pair[0] <= 4 else {1.0}), pair
    for i in {inst(c) for c in U.LATTICE_CP_CASES}:
        sizes = {c[3:5] for c in U.LATTICE_CP_CASES if inst(c) == i}
        assert {(1, 1), (2, 3)} <= sizes, i
    assert len({inst(c) for c in U.LATTICE_CP_CASES}) == 6
    assert max(c[0] for c in U.LATTICE_CP_CASES) == 520
    for C in (16, 32):
        sizes = {c[2:4] for c in U.LATTICE_RES_CASES if c[0] == C}
        assert {(1, 1), (2, 3), (13, 13), (14, 14), (15, 15), (17, 23), (29, 29)} <= sizes, C
    assert (16, 520, 2, 3, 0) in U.LATTICE_RES_CASES
    assert max(max(c[3:5]) for c in U.LATTICE_CP_CASES) <= 42
    for ids in (list(map(U.res_id, U.LATTICE_RES_CASES)), list(map(U.cp_id, U.LATTICE_CP_CASES))):
        assert len(set(ids)) == len(ids)


def test_nan_cases_and_the_reporter():
    for pair in U.NAN_CP_CASES:
        inputs, p64 = U.nan_cp_case(pair)
        assert int(inputs[0].isnan().sum()) == 1 and int(p64.isnan().sum()) == 6 * pair[1]
    a = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    U.assert_exact("same", a.float(), a)
    b = a.clone()
    b[1, 0, 2] = -1.0
    b[1, 2, 3] += 2.0 ** -20
    with pytest.raises(AssertionError, match=r"2 of 24 elements differ; first at \(1, 0, 2\): "
                                             r"got -1\.0, twin 14\.0"):
        U.assert_exact("planted", b, a)
