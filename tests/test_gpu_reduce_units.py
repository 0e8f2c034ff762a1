"""The leaf reduction's per-leaf and raw-tail outputs (UnitCol::out_units / out_tail, read through Engine.reduce) against the
model of tests/oracle_engine.py on the kd-tree oracle's columns: one np.sum per 128-row leaf of the full chunks, then the raw
values of the partial chunk, element by element, plus minimum and maximum.  Every record layout run_reduce of
tests/variants_check.py walks, unsharded and on each rank of three (shards that begin off a chunk boundary), columns D1, D2
and PROJ.  Lengths: 8192 + 4096 + 128 + 5 (a full chunk; a partial workgroup with two live leaves, one of 5 rows) against 8191
(no full chunk, a last leaf of 127 rows).  The kernels the batches ran on are collected from the path log: every reachable
k_unit_lean of row 'reduce_shapes' (tests/variant_rows.py) by default, k_unit_jobs alone under PCCM_REDUCE_GENERAL=1, which a
child process gets in its environment (`python tests/test_gpu_reduce_units.py` prints one JSON line)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import variant_rows as vr  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (8192 + 4096 + 128 + 5, 8191)
SHARDS = ((0, 1), (0, 3), (1, 3), (2, 3))


def run_check():
    from open_pcc_metric_amd import _native as nat
    from oracle_engine import OracleEngine
    D1, D2, PR = nat.METRIC_D1, nat.METRIC_D2, nat.METRIC_PROJ
    a, b, _ = vr.make_pair(*LENGTHS)
    fail, paths, compared = [], set(), 0
    eng = nat.Engine(0)
    try:
        for shard in SHARDS:
            model = OracleEngine(method="kdtree")
            for e in (eng, model):
                e.set_shard(*shard)
                e.set_cloud(0, a)
                e.set_cloud(1, b)
            for d in (0, 1):
                model.nn(d)
            if shard[1] > 1:
                assert all(model.shard_range(d)[0] % 8192 for d in (0, 1) if shard[0]), "the shards begin on chunk boundaries"
            want = {}                                       # the model's answers, once per (normals, mode, column)
            for engine in ("grid", "brute"):
                for flavour in ("f32", "f64", None):
                    for mode in ("neighbour", "row"):
                        if flavour is None and mode == "row":
                            continue
                        if flavour:
                            # row-indexed normals need a row for every query of the other cloud
                            la, lb = (len(a), len(b)) if mode == "neighbour" else (max(len(a), len(b)),) * 2
                            na, nb = vr._unit(la, 7, flavour == "f64"), vr._unit(lb, 8, flavour == "f64")
                            for e in (eng, model):
                                e.set_normals(0, na)
                                e.set_normals(1, nb)
                        metrics = (D1, D2, PR) if flavour else (D1,)
                        for d in (0, 1):
                            for met in metrics:
                                if (flavour, mode, d, met) not in want:
                                    want[(flavour, mode, d, met)] = model.reduce(d, met, mode)
                        for want_idx in (True, False):
                            for fuse in ((mode, None) if flavour else (None,)):
                                for d in (0, 1):
                                    eng.nn_fuse(d, fuse)
                                eng.nn_want_idx(want_idx)
                                eng.drop_caches()
                                eng.nn_pair(engine)
                                what = f"{engine} {flavour} {mode} idx={want_idx} fuse={fuse} shard={shard}"
                                if shard[1] > 1 and flavour:
                                    # D1 and D2 of a direction in one pass over its records: the two-column kernels (an unsharded
                                    # batch leaves the per-leaf results out, and reduce() would enqueue the column again)
                                    eng.reduce_prefetch_many([(0, D1), (0, D2), (1, D1), (1, D2)], mode)
                                    paths.update(eng.last_path(nat.PATH_REDUCE))
                                for d in (0, 1):
                                    for met in metrics:
                                        xvec, mn, mx = eng.reduce(d, met, mode)
                                        paths.update(eng.last_path(nat.PATH_REDUCE))
                                        wx, wmn, wmx = want[(flavour, mode, d, met)]
                                        compared += len(wx)
                                        if not np.array_equal(xvec, wx):
                                            bad = np.nonzero(xvec != wx)[0]
                                            fail.append(f"{what}: column {(d, met)} differs at {len(bad)} of {len(wx)} elements, first {int(bad[0])}")
                                        if not (mn == wmn and mx == wmx):
                                            fail.append(f"{what}: column {(d, met)}: min / max {mn} / {mx}, model {wmn} / {wmx}")
        eng.nn_want_idx(True)
    finally:
        eng.close()
    return {"fail": fail[:20], "paths": sorted(paths), "compared": compared}


def _unit_kernels(res):
    assert not res["fail"], " | ".join(res["fail"])
    assert res["compared"] > 100_000
    return {k for k in res["paths"] if k.startswith("k_unit_")}


@pytest.mark.parametrize("general", [False, True], ids=["lean", "PCCM_REDUCE_GENERAL=1"])
def test_leaf_and_tail_outputs_match_the_model_on_every_layout(general):
    if not general:
        got = _unit_kernels(run_check())
        missing = [k for k in vr.ROWS["reduce_shapes"]["expect"] if k not in got]
        assert not missing, f"kernels not reached: {missing}; reached {sorted(got)}"
        return
    # the switch is latched once per process: a child gets it in its environment
    child = dict(os.environ, PCCM_REDUCE_GENERAL="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=child, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    assert len(res) == 1
    assert _unit_kernels(res[0]) == {"k_unit_jobs"}


if __name__ == "__main__":
    print(json.dumps(run_check()), flush=True)
