"""Plane-to-plane rows on sharded pairs, on the real kernels: 2 gloo ranks sharing the one GPU split a tie-laden lattice pair by
direction or by query rows, under ties="pick" and ties="mean", and must print the single-process report bit for bit -- the
angular columns' sums travel in the same exchange as every other column (CloudPair._sharded_reduction), and the gathered
per-point columns are the single process's."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.options import CalculateOptions, transform_options

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_ties_mean import lattice_pair  # noqa: E402

WORKER = r'''
import json, os, sys
import numpy as np
import torch, torch.distributed as dist
sys.path.insert(0, os.environ["PCCM_ROOT"]); sys.path.insert(0, os.path.join(os.environ["PCCM_ROOT"], "tests"))
from open_pcc_metric_amd.calculator import MetricCalculator
from open_pcc_metric_amd.cloud_pair import CloudPair
from open_pcc_metric_amd.options import CalculateOptions, transform_options
from test_gpu_ties_mean import lattice_pair
dist.init_process_group("gloo")
a, b = lattice_pair(seed=3, side=32, count=9000)
pair = CloudPair(a, b, extent=[32.0, 32.0, 32.0], device=0, group=dist.group.WORLD, shard_mode=os.environ["PCCM_MODE"],
                 ties=os.environ["PCCM_TIES"])
rows = None
for rep in range(2):
    with np.errstate(divide="ignore"):
        res = MetricCalculator(pair).calculate(transform_options(CalculateOptions("ycc", True, True, plane_to_plane=True))).as_dict()
    now = [[list(map(str, k)), [float(x).hex() for x in np.atleast_1d(v)]] for k, v in res.items()]
    assert rows is None or rows == now
    rows = now
    pair.recompute()
cols = [np.asarray(pair.get_left_angular_similarities()).tobytes().hex(), np.asarray(pair.get_right_angular_similarities()).tobytes().hex()]
with open(os.path.join(os.environ["PCCM_OUT"], f"rank{dist.get_rank()}.json"), "w") as fh:
    json.dump({"rows": rows, "cols": cols, "shards": [list(pair._engine.shard_range(d)) for d in (0, 1, 2)]}, fh)
opts = dist.BarrierOptions()
opts.device = torch.device("cpu")
dist.group.WORLD.barrier(opts=opts).wait()
dist.destroy_process_group()
'''


def _rows(res):
    return [[list(map(str, k)), [float(x).hex() for x in np.atleast_1d(v)]] for k, v in res.items()]


@pytest.mark.parametrize("ties", ["pick", "mean"])
@pytest.mark.parametrize("mode", ["direction", "rows"])
def test_two_ranks_give_the_single_process_report(tmp_path, mode, ties):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, PCCM_ROOT=ROOT, PCCM_OUT=str(tmp_path), PCCM_MODE=mode, PCCM_TIES=ties, MASTER_ADDR="127.0.0.1",
               OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script)]
    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    ranks = [json.load(open(tmp_path / f"rank{r}.json")) for r in range(2)]
    a, b = lattice_pair(seed=3, side=32, count=9000)
    with CloudPair(a, b, extent=[32.0, 32.0, 32.0], ties=ties) as pair:
        with np.errstate(divide="ignore"):
            res = MetricCalculator(pair).calculate(transform_options(CalculateOptions("ycc", True, True, plane_to_plane=True)))
        want = _rows(res.as_dict())
        cols = [np.asarray(pair.get_left_angular_similarities()).tobytes().hex(),
                np.asarray(pair.get_right_angular_similarities()).tobytes().hex()]
    assert any(k[0] == "AngularSimilarity" for k, _ in want)
    for r in ranks:
        assert r["rows"] == want
        assert r["cols"] == cols
    if mode == "rows":
        assert ranks[1]["shards"][0][0] > 0 and ranks[1]["shards"][1][0] > 0       # row shards that start inside the clouds
