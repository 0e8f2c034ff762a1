"""Carried normals without a GPU (include/pccm.h, pccm_carry_normals): the NumPy restatement of tests/carry_reference.py against
a plain per-row loop, ``CloudPair(..., carry_normals=True)``'s wiring over the CPU test double, the errors of the constructor and
of the command line, and the entry point's place in the ABI."""
import os
import re
import sys

import numpy as np
import pytest
from click.testing import CliRunner

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.point_cloud import PointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from carry_reference import CarryOracleEngine, carried_normals, carried_normals_reversed  # noqa: E402
from oracle_engine import OracleEngine  # noqa: E402
from ties_reference import MeanOracleEngine  # noqa: E402


def loop_carry(src, rows_f, rows_g, n_to):
    """The definition, row by row, in Python floats (IEEE doubles)."""
    out = np.empty((n_to, 3))
    for j in range(n_to):
        members = [i for i in range(len(rows_f)) if rows_f[i] == j]       # ascending
        for c in range(3):
            if not members:
                out[j, c] = src[rows_g[j], c]
                continue
            s = float(src[members[0], c])
            for i in members[1:]:
                s = s + float(src[i, c])
            out[j, c] = s / float(len(members))
    return out


def wild_normals(rng, n):
    return rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))


def test_restatement_follows_the_definition_on_planted_lists():
    rng = np.random.default_rng(0)
    sizes = [0, 1, 2, 5, 0, 3, 1]                              # m per target row
    rows_f = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    src = wild_normals(rng, len(rows_f))
    src[0] = [-0.0, 0.0, -0.0]
    src[1] = [0.0, -0.0, -0.0]
    rows_g = rng.integers(0, len(rows_f), len(sizes))
    got = carried_normals(src, rows_f, rows_g, len(sizes))
    assert got.tobytes() == loop_carry(src, rows_f, rows_g, len(sizes)).tobytes()
    assert np.array_equal(np.bincount(rows_f, minlength=len(sizes)), sizes)


def test_single_rows_and_fallbacks_come_back_bit_for_bit_with_their_signed_zeros():
    src = np.array([[-0.0, 0.0, 1.5], [0.0, -0.0, -0.0], [3.0, -4.0, 5.0]])
    rows_f = np.array([2, 0, 2])                                # target 0 <- row 1; target 1 <- nobody; target 2 <- rows 0, 2
    rows_g = np.array([1, 1, 0])
    got = carried_normals(src, rows_f, rows_g, 3)
    assert got[0].tobytes() == src[1].tobytes()                 # m = 1
    assert got[1].tobytes() == src[1].tobytes()                 # m = 0: the fallback row
    assert got[2].tobytes() == ((src[0] + src[2]) / 2.0).tobytes()
    assert np.signbit(got[0]).tolist() == [False, True, True]


def test_one_point_target_takes_every_row_in_order():
    rng = np.random.default_rng(1)
    src = wild_normals(rng, 300)
    rows_f = np.zeros(300, dtype=np.int64)
    got = carried_normals(src, rows_f, np.array([7]), 1)
    assert got.tobytes() == loop_carry(src, rows_f, [7], 1).tobytes()
    assert got.tobytes() != carried_normals_reversed(src, rows_f, np.array([7]), 1).tobytes()      # the order shows


def test_random_lists_against_the_loop():
    rng = np.random.default_rng(2)
    rows_f = rng.integers(0, 40, 400)
    rows_f[rows_f == 13] = 14                                   # a row nobody matched
    src = wild_normals(rng, 400)
    rows_g = rng.integers(0, 400, 40)
    assert carried_normals(src, rows_f, rows_g, 40).tobytes() == loop_carry(src, rows_f, rows_g, 40).tobytes()


# ---- CloudPair wiring over the test double ----------------------------------------------------------------------------------
def clouds(seed=0, na=60, nb=45):
    rng = np.random.default_rng(seed)
    a, b = rng.random((na, 3)).astype(np.float32), rng.random((nb, 3)).astype(np.float32)
    return a, b, wild_normals(rng, na), wild_normals(rng, nb)


def restated(eng, frm):
    d_f, d_g = (nat.DIR_LEFT, nat.DIR_RIGHT) if frm == 0 else (nat.DIR_RIGHT, nat.DIR_LEFT)
    return carried_normals(eng.nrm[frm], eng.res[d_f][0], eng.res[d_g][0], len(eng.pts[1 - frm]))


def test_both_clouds_have_normals_the_flag_does_nothing():
    a, b, na, nb = clouds()
    eng = CarryOracleEngine()
    pair = CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1, 1, 1], carry_normals=True, _engine=eng)
    pair._require_normals(0)
    pair._require_normals(1)
    assert not [c for c in eng.calls if c[0] in ("carry", "estimate")] and pair._carried == [False, False]


def test_decoded_cloud_without_normals_takes_the_references():
    a, b, na, _ = clouds()
    eng = CarryOracleEngine()
    pair = CloudPair(PointCloud(a, na), PointCloud(b), extent=[1, 1, 1], normal_index="neighbour", carry_normals=True, _engine=eng)
    col = np.asarray(np.square(pair.point_to_plane_column(True)))          # left: projects on cloud 1's normals
    assert [c for c in eng.calls if c[0] in ("carry", "estimate")] == [("carry", 0)]
    assert pair._carried == [False, True] and pair._estimated == [False, False]
    want = restated(eng, 0)
    assert np.asarray(pair.get_normals(1)).tobytes() == want.tobytes()
    ref = CloudPair(PointCloud(a, na), PointCloud(b, want), extent=[1, 1, 1], normal_index="neighbour", _engine=CarryOracleEngine())
    assert col.tobytes() == np.asarray(np.square(ref.point_to_plane_column(True))).tobytes()
    pair._require_normals(1)                                                # already there: no second carry
    assert [c for c in eng.calls if c[0] == "carry"] == [("carry", 0)]


def test_only_the_decoded_cloud_has_normals_they_go_to_cloud_0():
    a, b, _, nb = clouds(1)
    eng = CarryOracleEngine()
    pair = CloudPair(PointCloud(a), PointCloud(b, nb), extent=[1, 1, 1], normal_index="neighbour", carry_normals=True, _engine=eng)
    pair._require_normals(0)
    assert [c for c in eng.calls if c[0] in ("carry", "estimate")] == [("carry", 1)] and pair._carried == [True, False]
    assert np.asarray(pair.get_normals(0)).tobytes() == restated(eng, 1).tobytes()


@pytest.mark.parametrize("first", [0, 1])
def test_neither_cloud_has_normals_cloud_0_is_estimated_and_carried(first):
    a, b, _, _ = clouds(2)
    eng = CarryOracleEngine()
    pair = CloudPair(PointCloud(a), PointCloud(b), extent=[1, 1, 1], normal_index="neighbour", carry_normals=True, _engine=eng)
    pair._require_normals(first)
    pair._require_normals(1 - first)
    assert [c for c in eng.calls if c[0] in ("carry", "estimate")] == [("estimate", 0), ("carry", 0)]
    assert pair._estimated == [True, False] and pair._carried == [False, True]
    assert np.asarray(pair.get_normals(1)).tobytes() == restated(eng, 0).tobytes()


def test_neither_cloud_has_normals_and_no_estimation_raises_as_before():
    a, b, _, _ = clouds(2)
    for flag in (False, True):
        pair = CloudPair(PointCloud(a), PointCloud(b), extent=[1, 1, 1], estimate_normals=False, carry_normals=flag,
                         _engine=CarryOracleEngine())
        with pytest.raises(ValueError, match="has no normals"):
            pair._require_normals(1)


def test_without_the_flag_the_decoded_cloud_is_estimated_as_before():
    a, b, na, _ = clouds()
    eng = CarryOracleEngine()
    pair = CloudPair(PointCloud(a, na), PointCloud(b), extent=[1, 1, 1], _engine=eng)
    pair._require_normals(1)
    assert [c for c in eng.calls if c[0] in ("carry", "estimate")] == [("estimate", 1)]


def test_with_reconst_carries_again():
    a, b, na, _ = clouds()
    b2 = np.random.default_rng(9).random((50, 3)).astype(np.float32)
    eng = CarryOracleEngine()
    pair = CloudPair(PointCloud(a, na), PointCloud(b), extent=[1, 1, 1], normal_index="neighbour", carry_normals=True, _engine=eng)
    pair._require_normals(1)
    nxt = pair.with_reconst(PointCloud(b2))
    assert nxt._carry_normals and nxt._carried == [False, False]
    nxt._require_normals(1)
    assert [c for c in eng.calls if c[0] == "carry"] == [("carry", 0), ("carry", 0)]
    assert np.asarray(nxt.get_normals(1)).shape == (50, 3)
    assert np.asarray(nxt.get_normals(1)).tobytes() == restated(nxt._engine, 0).tobytes()


def test_with_reconst_forgets_normals_carried_from_the_cloud_that_left():
    a, b, _, nb = clouds(3)
    b2, nb2 = np.random.default_rng(8).random((30, 3)).astype(np.float32), wild_normals(np.random.default_rng(7), 30)
    eng = CarryOracleEngine()
    pair = CloudPair(PointCloud(a), PointCloud(b, nb), extent=[1, 1, 1], normal_index="neighbour", carry_normals=True, _engine=eng)
    pair._require_normals(0)
    nxt = pair.with_reconst(PointCloud(b2, nb2))
    assert nxt._carried == [False, False]
    nxt._require_normals(0)
    assert [c for c in eng.calls if c[0] == "carry"] == [("carry", 1), ("carry", 1)]
    assert np.asarray(nxt.get_normals(0)).tobytes() == restated(nxt._engine, 1).tobytes()


def test_the_constructor_refuses_mean_ties_groups_and_engines_that_cannot_carry():
    a, b, na, _ = clouds()
    with pytest.raises(ValueError, match="carry_normals"):
        CloudPair(PointCloud(a, na), PointCloud(b), extent=[1, 1, 1], ties="mean", carry_normals=True, _engine=MeanOracleEngine())
    with pytest.raises(ValueError, match="carry_normals"):
        CloudPair(PointCloud(a, na), PointCloud(b), extent=[1, 1, 1], group=object(), carry_normals=True, _engine=CarryOracleEngine())
    with pytest.raises(ValueError, match="carry normals"):
        CloudPair(PointCloud(a, na), PointCloud(b), extent=[1, 1, 1], carry_normals=True, _engine=OracleEngine())
    CloudPair(PointCloud(a, na), PointCloud(b), extent=[1, 1, 1], _engine=OracleEngine())        # without the flag: as before


def test_cli_flag_and_usage_error():
    out = CliRunner().invoke(cli, ["--help"])
    assert out.exit_code == 0 and "--carry-normals" in out.output
    bad = CliRunner().invoke(cli, ["--ocloud", "a.ply", "--pcloud", "b.ply", "--carry-normals", "--ties", "mean"])
    assert bad.exit_code == 2 and "carry_normals" in bad.output           # a usage error, before any file is read


def test_entry_point_is_declared_and_exported():
    assert "pccm_carry_normals" in nat.SYMBOLS
    with open(os.path.join(ROOT, "include", "pccm.h")) as fh:
        header = fh.read()
    assert re.search(r"int\s+pccm_carry_normals\s*\(\s*pccm_ctx\s*\*\s*ctx\s*,\s*int\s+from\s*,\s*int\s*\*\s*built\s*\)\s*;", header)
    assert "not pinned" in header.lower()
    lib = nat.load()
    assert hasattr(lib, "pccm_carry_normals") and hasattr(nat.Engine, "carry_normals")
