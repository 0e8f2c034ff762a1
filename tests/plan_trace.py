"""A recording stand-in for the native engine, and the reports whose engine-call traces tests/golden/plan_trace.json pins.

The stand-in answers every engine method a CloudPair may call and writes down ``(method, arguments)`` -- arrays by shape --, so a
whole ``calculate()`` runs on it without a GPU or the native library.  What a report enqueues, in which order and with which
arguments, is then a list that can be compared with the one recorded before a change (tests/golden/make_plan_trace.py records,
tests/test_plan_trace_host.py compares).  The values it answers are made up: only the calls matter."""
import json

import numpy as np

from open_pcc_metric_amd import _native as nat
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

ROWS = {nat.DIR_LEFT: 300, nat.DIR_RIGHT: 200, nat.DIR_SELF: 300}
ONCE = ("ssim_features", "p2d_build", "resolution_build")          # True the first time per argument set, False after
TOTALS = ("reduce_total_many", "reduce_map_total_many", "reduce_density_total_many")


def plain(x):
    """``x`` as JSON would carry it: arrays by shape, tuples as lists, NumPy scalars as Python's."""
    if isinstance(x, np.ndarray):
        return {"shape": list(x.shape)}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    return x


class RecordingEngine:
    keeps_self_search = True

    def __init__(self, hidden=(), record=True):
        self.calls, self._hidden, self._record, self._seen, self._graphs = [], hidden, record, set(), 0

    def _answer(self, name, args):
        if name == "n_iter":
            return ROWS[args[0]]
        if name in ONCE:
            key = repr((name, plain(args)))
            fresh = key not in self._seen
            self._seen.add(key)
            return fresh
        if name == "graph_end":
            self._graphs += 1
            return self._graphs
        if name == "reduce_total":
            return (1.0, 0.5, 2.0)
        if name in TOTALS:
            return [(1.0, 0.5, 2.0)] * len(args[0])
        if name == "select_many":
            return [0.25] * len(args[0])
        if name == "count_many":
            return [7] * len(args[0])
        if name == "color_reduce":
            return np.ones(3), np.full(3, 2.0)
        if name == "obb_frames":
            return np.ones(3), 1.0
        return None

    def __getattr__(self, name):
        if name.startswith("_") or any(h in name for h in self._hidden):
            raise AttributeError(name)

        def call(*args, **kwargs):
            if self._record:
                self.calls.append([name, plain(args)] + ([plain(sorted(kwargs.items()))] if kwargs else []))
            return self._answer(name, args)
        return call


EVERY = dict(color="ycc", hausdorff=True, point_to_plane=True, plane_to_plane=True, point_ssim=("geometry", "normal", "curvature", "color"),
             hausdorff_rank=(0.9, 0.5), point_to_distribution=True, p2d_color=True, resolution_psnr=True, reflectance=True,
             fscore=(0.01, 0.1), chamfer=True, truncate=(0.5, 0.01), dcd=(40.0, 0.0))
REPORTS = {
    "default": {},
    "headline": dict(point_to_plane=True),
    "hausdorff": dict(hausdorff=True, point_to_plane=True),
    "every": EVERY,
    "every_squared": dict(EVERY, dcd_squared=True),
    "every_but_normal_ssim": dict(EVERY, point_ssim=("geometry", "curvature", "color")),
}
# name -> (what the pair is made with, the reports of its steps, engine methods hidden by substring, with_reconst half way)
CASES = {
    "default": ({}, ["default"] * 3, (), False),
    "headline": ({}, ["headline"] * 3, (), False),
    "hausdorff": ({}, ["hausdorff"] * 3, (), False),
    "every": ({}, ["every"] * 3, (), False),
    "every_squared_neighbour": (dict(normal_index="neighbour"), ["every_squared"] * 3, (), False),
    "every_without_normals": (dict(normals=False, estimate_normals=False), ["every"] * 3, (), False),
    "every_but_normal_ssim_without_normals": (dict(normals=False, estimate_normals=False), ["every_but_normal_ssim"] * 3, (), False),
    "report_change": ({}, ["headline"] * 2 + ["every"] * 2 + ["headline"] * 2, (), False),
    "with_reconst": ({}, ["every"] * 3 + ["every"] * 3, (), True),
    "every_per_column_prefetch": ({}, ["every"] * 3, ("reduce_prefetch_many",), False),
    "every_without_prefetch": ({}, ["every"] * 3, ("_prefetch",), False),
}


def cloud(n, seed, normals=True):
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3))
    return PointCloud(rng.random((n, 3)), nrm / np.linalg.norm(nrm, axis=1, keepdims=True) if normals else None,
                      rng.random((n, 3)), rng.random(n))


def make_pair(engine, use_graph, normals=True, **kw):
    return CloudPair(cloud(ROWS[nat.DIR_LEFT], 0, normals), cloud(ROWS[nat.DIR_RIGHT], 1, normals), _engine=engine, use_graph=use_graph, **kw)


def metrics_of(report):
    return transform_options(CalculateOptions(**REPORTS[report]))


def run_case(name, use_graph):
    """The case's record: the engine calls of making the pair and of every step, the rows of every step, and the error that
    ended it, if one did."""
    pair_kw, reports, hidden, reconst = CASES[name]
    engine = RecordingEngine(hidden)
    pair = make_pair(engine, use_graph, **pair_kw)
    out, last_keys = {"calls": None, "keys": [], "error": None}, None
    try:
        for step, report in enumerate(reports):
            if reconst and step == len(reports) // 2:
                engine.calls.append(["-- with_reconst --", []])
                pair = pair.with_reconst(cloud(ROWS[nat.DIR_RIGHT], 2, pair_kw.get("normals", True)))
            engine.calls.append([f"-- step {step}: {report} --", []])
            pair.recompute()
            result = MetricCalculator(pair).calculate(metrics_of(report))
            keys = plain(list(result.as_dict()))
            out["keys"].append("as the step before" if keys == last_keys else keys)
            last_keys = keys
    except Exception as failure:        # noqa: BLE001 -- whatever ends a report is part of its record
        out["error"] = [type(failure).__name__, str(failure)]
    out["calls"] = engine.calls
    return json.loads(json.dumps(out))


def record_all():
    return {f"{name}, use_graph={use_graph}": run_case(name, use_graph) for name in CASES for use_graph in (False, True)}


def _numbered(table, items):
    """The numbers of ``items`` in ``table`` (each distinct item once, in the order met), a run of one number as ``[number, n]``."""
    out = []
    for item in items:
        number = table.setdefault(json.dumps(item), len(table))
        if out and out[-1] == number:
            out[-1] = [number, 2]
        elif out and isinstance(out[-1], list) and out[-1][0] == number:
            out[-1][1] += 1
        else:
            out.append(number)
    return out


def pack(record):
    """``record`` (record_all) with everything that repeats stored once: each distinct call and each distinct row key in a table
    of its own, the calls between two step markers as a named segment of call numbers, the keys of a report by its name."""
    calls, keys, segments, reports, cases = {}, {}, {}, {}, {}
    for name, case in record.items():
        parts = [[None, []]]                                      # (the marker that opens the part, its calls)
        for call in case["calls"]:
            if call[0].startswith("--"):
                parts.append([call[0], []])
            else:
                parts[-1][1].append(call)
        named = [[marker, segments.setdefault(json.dumps(_numbered(calls, part)), f"s{len(segments)}")] for marker, part in parts]
        last = None
        for report, step_keys in zip(_reports_of(named), case["keys"]):
            last = last if step_keys == "as the step before" else step_keys
            assert reports.setdefault(report, _numbered(keys, last)) == _numbered(keys, last)
        cases[name] = {"error": case["error"], "steps_done": len(case["keys"]), "segments": named}
    return {"calls": [json.loads(c) for c in calls], "keys": [json.loads(k) for k in keys], "reports": reports,
            "segments": {number: json.loads(numbers) for numbers, number in segments.items()}, "cases": cases}


def _reports_of(named):
    return [marker.split(": ")[1].split(" ")[0] for marker, _ in named if marker and marker.startswith("-- step")]


def _expanded(table, numbers):
    out = []
    for number in numbers:
        out += [table[number[0]]] * number[1] if isinstance(number, list) else [table[number]]
    return out


def unpack(packed, name):
    """The record of case ``name`` as run_case gives it, from the packed form."""
    case, calls, keys, last = packed["cases"][name], [], [], None
    for marker, segment in case["segments"]:
        if marker is not None:
            calls.append([marker, []])
        calls += _expanded(packed["calls"], packed["segments"][segment])
    for report in _reports_of(case["segments"])[:case["steps_done"]]:
        step_keys = _expanded(packed["keys"], packed["reports"][report])
        keys.append("as the step before" if step_keys == last else step_keys)
        last = step_keys
    return {"calls": calls, "keys": keys, "error": case["error"]}
