"""Run by tests/test_gpu_tail_filed.py in a child process with PCCM_TAIL_FILED=0 (the library reads its switches once per
process): every case of tests/tail_filed_cases.py on the classic graph, what each step read written to the .npz named on the
command line."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import tail_filed_cases as tc  # noqa: E402
from open_pcc_metric_amd import _native as nat  # noqa: E402


def main(out):
    assert os.environ.get("PCCM_TAIL_FILED") == "0"
    keep = {}
    for name in tc.CASES:
        got = tc.run(tc.build(name), nat)
        assert not got.filed, f"{name}: PCCM_TAIL_FILED=0 still left the tail launch out"
        for k, s in enumerate(got.steps):
            keep[f"{name}/{k}/totals"] = s.totals
            for d in (0, 1):
                keep[f"{name}/{k}/idx{d}"] = s.idx[d]
                keep[f"{name}/{k}/d2{d}"] = s.d2[d]
                keep[f"{name}/{k}/stats{d}"] = np.array([s.stats[d]["fallback_queries"], s.stats[d]["tail_queries"]], dtype=np.int64)
    np.savez(out, **keep)
    print("tail filed child ok")


if __name__ == "__main__":
    main(sys.argv[1])
