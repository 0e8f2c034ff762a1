"""The planted columns of tests/colsum_planted.py on the host: every column has the property its name claims, and the reference
the GPU tests compare with -- np.add.reduce(axis=0) of an (N, 3) array -- is the plain left-to-right sum on this NumPy build."""
import numpy as np
import pytest

import colsum_planted as cp

COLUMNS = cp.columns()


def test_drift_columns_pull_the_true_sum_and_the_exact_prefix_apart():
    assert len(cp.check_drift()) >= 30
    assert len(cp.check_stall()) >= 40
    assert len(cp.check_behind()) >= 40


@pytest.mark.parametrize("level", list(cp.LANDING_ROWS))
@pytest.mark.parametrize("kind", ["dyadic", "rounded"])
@pytest.mark.parametrize("over", [0, 1])
def test_landings_land_where_they_say(level, kind, over):
    assert cp.check_landing(level, kind, over) == cp.LANDING_ROWS[level]


def test_ties_meet_the_parity_they_name():
    cp.check_ties()


def test_crossings_outnumber_the_flag_list():
    assert len(cp.check_crossings()) > 64


def test_threshold_column_climbs_across_the_limit():
    assert cp.CHUNK < cp.check_threshold() < 2 * cp.CHUNK


def test_every_column_is_a_finite_non_negative_fp64_column_of_at_most_seven_chunks():
    cp.check_all()
    assert len(COLUMNS) == 24


@pytest.mark.parametrize("name", list(COLUMNS))
def test_axis0_reduce_is_the_left_to_right_sum(name):
    x = COLUMNS[name]
    for n in cp.lengths(name, x):
        assert 0 < n <= len(x)
        want = 0.0
        for v in x[:n].tolist():
            want += v
        got = np.add.reduce(np.c_[x[:n], x[:n], x[:n]], axis=0)
        assert got[0] == want == got[1] == got[2] == cp.cumsum(x[:n])[-1], (name, n)
