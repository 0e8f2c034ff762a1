"""bench.py --dump-outputs on the CPU: the arrays are the last step's report rows and the per-point columns behind them, in
float64, within the byte budget, sampled the same way on every run; and --steps is checked before anything starts."""
import numpy as np
import pytest

import bench
import open_pcc_metric_amd.metric as m
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud
from oracle import oracle as orc
from oracle_engine import OracleEngine


def _pair_and_report(n=600):
    a, b, na, nb = bench.synth(n)
    pair = CloudPair(PointCloud(a, na), PointCloud(b, nb), extent=[1.0, 1.0, 1.0], _engine=OracleEngine())
    metrics = transform_options(CalculateOptions(None, False, True))[2:] + [m.GeoHausdorffDistance(True, False),
                                                                            m.GeoHausdorffDistance(False, False)]
    return pair, MetricCalculator(pair).calculate(metrics).as_dict(), (a, b, na, nb)


def test_dump_holds_the_report_and_the_columns_behind_it():
    pair, report, (a, b, na, nb) = _pair_and_report()
    out = bench.last_step_outputs(pair, report)
    assert all(v.dtype == np.float64 for v in out.values())
    rows = {k: v for k, v in out.items() if k.startswith("report.")}
    assert len(rows) == len(report)
    assert rows["report.GeoMSE_True_False"] == report[("GeoMSE", True, False)]
    assert rows["report.SymmetricMetric_GeoPSNR_True_True_GeoPSNR_False_True"] == \
        report[("SymmetricMetric", "GeoPSNR", True, True, "GeoPSNR", False, True)]
    want = orc.OraclePair(a, b, na, nb, method="kdtree")
    assert np.array_equal(out["neighbour_distances_left"], want.nn_d2[0])
    assert np.array_equal(out["neighbour_distances_right"], want.nn_d2[1])
    assert np.array_equal(out["point_to_plane_left"], np.asarray(pair.point_to_plane_column(True)))
    assert np.array_equal(out["point_to_plane_right"], np.asarray(pair.point_to_plane_column(False)))
    assert not any(k.startswith("sample_rows") for k in out)


def test_long_columns_are_sampled_within_the_budget_and_alike_every_run(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", (1 << 20) + 8 * 6 * 100)        # 100 rows per array
    pair, report, _ = _pair_and_report()
    first, second = bench.last_step_outputs(pair, report), bench.last_step_outputs(pair, report)
    assert sum(v.nbytes for v in first.values()) <= bench.DUMP_BYTES
    assert first.keys() == second.keys() and all(np.array_equal(first[k], second[k]) for k in first)
    rows = first["sample_rows_left"].astype(np.int64)
    assert len(rows) == 100 and np.all(np.diff(rows) > 0)
    assert np.array_equal(first["neighbour_distances_left"], np.asarray(pair.get_left_neighbour_distances())[rows])


@pytest.mark.parametrize("steps", ["0", "-3"])
def test_steps_below_one_are_refused(monkeypatch, steps):
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", steps])
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert exc.value.code == 2
