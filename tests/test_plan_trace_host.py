"""What a report asks of the engine, call by call, against the record in tests/golden/plan_trace.json (tests/plan_trace.py says
what the cases are and how the record is made): the launch sequence a report enqueues -- and a ``use_graph`` capture records -- is
decided by Python that every row family passes through, so the whole sequence is pinned, not a family at a time.  No GPU needed."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plan_trace  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "plan_trace.json")) as _file:
    PACKED = json.load(_file)
RECORD = {name: plan_trace.unpack(PACKED, name) for name in PACKED["cases"]}        # (the fixture stores what repeats once)


def test_the_record_covers_every_case():
    assert sorted(RECORD) == sorted(f"{name}, use_graph={g}" for name in plan_trace.CASES for g in (False, True))


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", list(plan_trace.CASES))
def test_engine_calls_rows_and_errors_are_the_recorded_ones(name, use_graph):
    want = RECORD[f"{name}, use_graph={use_graph}"]
    got = plan_trace.run_case(name, use_graph)
    assert got["error"] == want["error"]
    assert got["keys"] == want["keys"]
    for at, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, f"call {at}: {a} where {b} was recorded, after {got['calls'][max(0, at - 3):at]}"
    assert len(got["calls"]) == len(want["calls"])


def test_what_the_record_shows_of_the_planner():
    """The cases are worth their name: the out-of-range left D2 column is left out of every batch and selected on demand, a
    changed report destroys the captured graph, and a pair without normals fails where the record says."""
    calls = RECORD["every, use_graph=False"]["calls"]
    batches = [c[1][0] for c in calls if c[0] == "reduce_prefetch_many"]
    assert batches and not any([0, 1] in batch for batch in batches)                 # (DIR_LEFT, METRIC_D2): 300 rows, 200 normals
    assert ["select_many", [[[0, 1, 150]], "row"]] in calls
    names = [c[0] for c in RECORD["report_change, use_graph=True"]["calls"]]
    assert names.count("graph_destroy") == 2 and names.count("graph_end") == 3
    assert RECORD["every_without_normals, use_graph=True"]["error"][0] == "ValueError"
    late = RECORD["every_but_normal_ssim_without_normals, use_graph=False"]
    assert late["error"][0] == "ValueError" and "reduce_prefetch_many" in [c[0] for c in late["calls"]]
