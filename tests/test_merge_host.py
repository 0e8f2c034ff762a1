"""Merged duplicate points without a GPU (include/pccm.h, pccm_merge_duplicates): the NumPy restatement of tests/merge_reference.py
on hand-written cases, the errors of ``check_duplicates``, of the constructor and of the command line -- all before any engine
exists --, the entry points' place in the ABI, and that the summation-order family really tells the order of a sum."""
import os
import re
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.options import check_duplicates
from open_pcc_metric_amd.point_cloud import PointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from merge_reference import drawn_20000, groups, merged, merged_reversed  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_signed_zeros_share_a_key_and_the_representative_keeps_its_bits():
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-0.0, 0.0, 0.0]])
    p, n, c, m = merged(pts, None, None, "drop")
    assert p.shape == (2, 3) and n is None and c is None
    assert m.tolist() == [0, 1, 0] and m.dtype == np.int32
    assert not np.signbit(p[0, 0]) and p.tobytes() == pts[:2].tobytes()
    p, _, _, m = merged(pts[::-1].copy(), None, None, "drop")           # now the -0.0 row comes first: it survives
    assert m.tolist() == [0, 1, 0] and np.signbit(p[0, 0]) and p[1, 0] == 1.0


def test_three_term_average_is_left_to_right_and_one_division():
    a, b, c = 0.1, 0.2, 0.3
    pts = np.array([[5.0, 5.0, 5.0]] * 3 + [[6.0, 5.0, 5.0]])
    col = np.array([[a, b, c], [b, c, a], [c, a, b], [7.0, 8.0, 9.0]])
    nrm = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0], [-0.0, 0.0, 1.0]])
    p, n, cc, m = merged(pts, nrm, col, "average")
    assert m.tolist() == [0, 0, 0, 1] and p.tobytes() == pts[[0, 3]].tobytes()
    assert n.tobytes() == nrm[[0, 3]].tobytes()                          # the representative's normal, never an average
    assert cc[0].tolist() == [((a + b) + c) / 3, ((b + c) + a) / 3, ((c + a) + b) / 3]
    assert ((a + b) + c) / 3 != ((c + b) + a) / 3 or ((b + c) + a) / 3 != ((a + c) + b) / 3    # (the order shows here)
    assert cc[1].tobytes() == col[3].tobytes()
    _, _, cd, _ = merged(pts, nrm, col, "drop")
    assert cd.tobytes() == col[[0, 3]].tobytes()


def test_single_rows_return_the_input_bits():
    rng = np.random.default_rng(3)
    pts = rng.random((50, 3))
    col = rng.random((50, 3)) * 1e-300
    col[0] = [-0.0, np.nan, np.inf]
    nrm = rng.standard_normal((50, 3))
    for mode in ("drop", "average"):
        p, n, c, m = merged(pts, nrm, col, mode)
        assert p.tobytes() == pts.tobytes() and n.tobytes() == nrm.tobytes() and c.tobytes() == col.tobytes()
        assert np.array_equal(m, np.arange(50))


def test_float32_points_are_widened_exactly_and_one_ulp_apart_stays_apart():
    a = np.float32(0.1)
    pts32 = np.array([[a, 0, 0], [a, 0, 0]], dtype=np.float32)
    assert len(merged(pts32, None, None, "drop")[0]) == 1
    pts64 = np.array([[0.1, 0, 0], [np.nextafter(0.1, 1.0), 0, 0]])
    assert pts64.astype(np.float32)[0, 0] == pts64.astype(np.float32)[1, 0]
    assert len(merged(pts64, None, None, "drop")[0]) == 2


def test_groups_are_numbered_by_first_appearance():
    pts = np.array([[3.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0], [2.0, 0, 0], [1.0, 0, 0]])
    mapping, reps = groups(pts)
    assert mapping.tolist() == [0, 1, 0, 2, 1] and reps.tolist() == [0, 1, 3]


def test_check_duplicates_errors():
    for mode in ("keep", "drop", "average"):
        check_duplicates(mode)
    check_duplicates("keep", group=object())
    for bad in ("bogus", "", "AVERAGE", None, 2, True):
        with pytest.raises(ValueError, match="duplicates"):
            check_duplicates(bad)
    for mode in ("drop", "average"):
        with pytest.raises(ValueError, match="group"):
            check_duplicates(mode, group=object())


def test_the_constructor_refuses_before_any_engine_is_acquired(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(nat, "acquire_engine", no_engine)
    a = PointCloud(np.zeros((4, 3), dtype=np.float32))
    b = PointCloud(np.ones((4, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="duplicates"):
        CloudPair(a, b, duplicates="bogus")
    with pytest.raises(ValueError, match="group"):
        CloudPair(a, b, duplicates="average", group=object())


def test_an_engine_that_cannot_merge_is_refused_and_keep_changes_nothing():
    rng = np.random.default_rng(5)
    a, b = rng.random((40, 3), dtype=np.float32), rng.random((30, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="merge duplicate"):
        CloudPair(PointCloud(a), PointCloud(b), extent=[1, 1, 1], duplicates="drop", _engine=OracleEngine())
    pair = CloudPair(PointCloud(a), PointCloud(b), extent=[1, 1, 1], duplicates="keep", _engine=OracleEngine())
    assert pair.duplicates_removed == (0, 0) and pair._merged == [False, False]


def test_cli_flag_and_usage_errors():
    out = CliRunner().invoke(cli, ["--help"])
    assert out.exit_code == 0 and "--duplicates" in out.output
    for bad in ("bogus", "AVERAGE"):
        res = CliRunner().invoke(cli, ["--ocloud", "a.ply", "--pcloud", "b.ply", "--duplicates", bad])
        assert res.exit_code == 2 and "duplicates" in res.output         # a usage error, before any file is read


def test_entry_points_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "pccm.h")) as fh:
        header = fh.read()
    for sym in ("pccm_merge_duplicates", "pccm_get_merge_map", "pccm_get_points", "pccm_get_colors"):
        assert sym in nat.SYMBOLS
        assert re.search(r"int\s+" + sym + r"\s*\(\s*pccm_ctx\s*\*\s*ctx\s*,\s*int\s+which\s*,", header)
    assert re.search(r"#define\s+PCCM_DUP_DROP\s+1\b", header) and re.search(r"#define\s+PCCM_DUP_AVERAGE\s+2\b", header)
    assert nat.DUPLICATES == {"drop": 1, "average": 2}
    lib = nat.load()
    for sym in ("pccm_merge_duplicates", "pccm_get_merge_map", "pccm_get_points", "pccm_get_colors"):
        assert hasattr(lib, sym)
    for meth in ("merge_duplicates", "get_merge_map", "get_points", "get_colors"):
        assert hasattr(nat.Engine, meth)


def test_drawn_family_tells_the_summation_order():
    pts, col = drawn_20000()
    p, _, c, m = merged(pts, None, col, "average")
    _, _, r, m2 = merged_reversed(pts, None, col, "average")
    counts = np.bincount(m)
    moved = np.any(bits(c) != bits(r), axis=1)
    print(f"{len(p)} groups, {(counts >= 3).sum()} with m >= 3, {moved.sum()} rows moved, {moved[counts < 3].sum()} of them with m < 3")
    assert np.array_equal(m, m2) and len(p) == len(counts) == 9721 and (counts >= 3).sum() == 2801
    assert moved.sum() >= 1000 and not moved[counts < 3].any()
