"""Cost of the colour and joint point-to-distribution columns (CalculateOptions(p2d_color=True)) on a resident 1M + 1M coloured
pair, and the regression guard for the k-NN searches they share with normal estimation and PointSSIM ("Point-to-distribution:
colour and joint").

    python scripts/p2d_color_cost.py [--rounds 15] [--n 1000000] [--k 30] [--baseline-lib PATH/libpccm.so] [--only builds|report]
                                         [--arms normals,ssim,p2d,color_u8,color_f64]

* builds: one context per library, through the C ABI alone, stepped alternately in ONE process (round after round, so that every
  arm sees the same machine state): pccm_estimate_normals (k = 30, cloud 0), pccm_ssim_features (k = 12, all four attributes,
  cloud 0), pccm_p2d_build (geometry, both directions), and -- this library only -- pccm_p2d_build_attrs with PCCM_P2D_COLOR over
  byte colours and over fp64 colours that are no byte quotients.  Every timed build follows an untimed one at another k, so that
  nothing is reused; host clock around pccm_sync.  The libraries take turns in going first.  ``--baseline-lib`` adds the same geometry-only arms on another build of the
  library (the parent commit's), which has to export nothing newer than pccm_p2d_build.  Median, min and max per arm.
* report: two resident pairs under use_graph, stepped alternately: recompute() + the report with the geometry rows only, and with
  the colour and joint rows as well; the difference is what the six to twelve new rows cost.

One JSON line per part.  For the kernels' own times run the builds alone under
``rocprofv3 --kernel-trace --stats -- python scripts/p2d_color_cost.py --only builds --rounds 5 --arms color_u8``: with one
colour arm the launches of k_p2d_geometry and k_p2d_color alternate."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64 = 1
SSIM_ALL = 15
P2D_BOTH = 3


class Ctx:
    """One context of one build of the library, through the calls both builds export."""

    def __init__(self, path, a, b, ca8, cb8):
        self.lib = ctypes.CDLL(path)
        self.ctx = ctypes.c_void_p()
        self.call("pccm_ctx_create", 0, None, ctypes.byref(self.ctx))
        for which, (x, c) in enumerate(((a, ca8), (b, cb8))):
            self.call("pccm_set_cloud", self.ctx, which, x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(x)), F64, 0)
            self.colors_u8(which, c)

    def call(self, name, *args):
        rc = getattr(self.lib, name)(*args)
        if rc:
            self.lib.pccm_last_error.restype = ctypes.c_char_p
            raise RuntimeError(f"{name}: {rc}: {self.lib.pccm_last_error().decode()}")

    def colors_u8(self, which, c):
        self.call("pccm_set_colors_u8", self.ctx, which, c.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(c)))

    def colors_f64(self, which, c):
        self.call("pccm_set_colors", self.ctx, which, c.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(c)), F64, 0)

    def sync(self):
        self.call("pccm_sync", self.ctx)

    def timed(self, fn):
        self.sync()
        t0 = time.perf_counter()
        fn()
        self.sync()
        return 1e3 * (time.perf_counter() - t0)

    def normals(self):
        self.call("pccm_estimate_normals", self.ctx, 0, 29)
        return self.timed(lambda: self.call("pccm_estimate_normals", self.ctx, 0, 30))

    def ssim(self):
        built = ctypes.c_int32()
        self.call("pccm_ssim_features", self.ctx, 0, 13, SSIM_ALL, ctypes.byref(built))
        return self.timed(lambda: self.call("pccm_ssim_features", self.ctx, 0, 12, SSIM_ALL, ctypes.byref(built)))

    def p2d(self, k, attrs=None):
        built = ctypes.c_int32()
        build = (lambda kk: self.call("pccm_p2d_build", self.ctx, kk, ctypes.byref(built))) if attrs is None else \
            (lambda kk: self.call("pccm_p2d_build_attrs", self.ctx, kk, attrs, ctypes.byref(built)))
        build(k + 1 if k < 64 else k - 1)
        ms = self.timed(lambda: build(k))
        assert built.value == 1
        return ms

    def close(self):
        self.lib.pccm_ctx_destroy(self.ctx)


def stats(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(float(np.min(ts)), 4), "max": round(float(np.max(ts)), 4)}


def builds(args):
    try:                                                               # one HIP runtime per process: the one open_pcc_metric_amd binds to
        import torch  # noqa: F401
    except ImportError:
        pass
    rng = np.random.default_rng(7)
    a, b = rng.random((args.n, 3)), rng.random((args.n, 3))
    ca8, cb8 = (rng.integers(0, 256, (args.n, 3), dtype=np.uint8) for _ in range(2))
    ca64, cb64 = rng.random((args.n, 3)), rng.random((args.n, 3))
    libs = {"this": os.path.join(ROOT, "open_pcc_metric_amd", "csrc", "libpccm.so")}
    if args.baseline_lib:
        libs["baseline"] = os.path.abspath(args.baseline_lib)
    ctxs = {name: Ctx(path, a, b, ca8, cb8) for name, path in libs.items()}
    ts = {}
    try:
        arms = args.arms.split(",")
        for r in range(args.rounds + 2):                               # two warm-up rounds
            row = {}
            # alternated, and in alternating order: every arm sees the same machine state, and none always follows the same other
            for name in (list(ctxs) if r % 2 == 0 else list(ctxs)[::-1]):
                c = ctxs[name]
                if "normals" in arms:
                    row[f"{name}.normals_k30"] = c.normals()
                if "ssim" in arms:
                    row[f"{name}.ssim_features_k12"] = c.ssim()
                if "p2d" in arms:
                    row[f"{name}.p2d_geometry"] = c.p2d(args.k)
            c = ctxs["this"]
            if "color_u8" in arms:
                row["this.p2d_geometry_color_u8"] = c.p2d(args.k, P2D_BOTH)
            if "color_f64" in arms:
                c.colors_f64(0, ca64)
                c.colors_f64(1, cb64)
                row["this.p2d_geometry_color_f64"] = c.p2d(args.k, P2D_BOTH)
                c.colors_u8(0, ca8)
                c.colors_u8(1, cb8)
            if r >= 2:
                for key, v in row.items():
                    ts.setdefault(key, []).append(v)
    finally:
        for c in ctxs.values():
            c.close()
    out = {"part": "builds", "points": [args.n, args.n], "k": args.k, "rounds": args.rounds, "unit": "ms"}
    out.update({key: stats(v) for key, v in ts.items()})
    return out


def report(args):
    from open_pcc_metric_amd.calculator import MetricCalculator
    from open_pcc_metric_amd.cloud_pair import CloudPair
    from open_pcc_metric_amd.options import CalculateOptions, transform_options
    from open_pcc_metric_amd.point_cloud import PointCloud
    rng = np.random.default_rng(7)
    a, b = rng.random((args.n, 3)), rng.random((args.n, 3))
    ca8, cb8 = (rng.integers(0, 256, (args.n, 3), dtype=np.uint8) for _ in range(2))

    def cloud(x, c8):
        c = PointCloud(x, colors=c8 / 255.0)
        c.attach_colors_u8(c8)
        return c

    base = dict(hausdorff=True, point_to_distribution=True, p2d_neighbours=args.k)
    runs = {"geometry": CalculateOptions(**base), "geometry_color": CalculateOptions(**base, p2d_color=True)}
    pairs = {name: CloudPair(cloud(a, ca8), cloud(b, cb8), extent=[1.0, 1.0, 1.0], use_graph=True) for name in runs}
    metrics = {name: transform_options(o) for name, o in runs.items()}
    ts, rows = {name: [] for name in runs}, {}
    try:
        for s in range(args.rounds + 5):
            for name in runs:
                t0 = time.perf_counter()
                if s:
                    pairs[name].recompute()
                rows[name] = MetricCalculator(pairs[name]).calculate(metrics[name]).as_dict()
                if s >= 5:
                    ts[name].append(1e3 * (time.perf_counter() - t0))
    finally:
        for p in pairs.values():
            p.close()
    out = {"part": "report", "points": [args.n, args.n], "k": args.k, "rounds": args.rounds, "unit": "ms"}
    out.update({"report_" + name: stats(v) for name, v in ts.items()})
    out["rows"] = {name: len(r) for name, r in rows.items()}
    out["added_ms_median"] = round(out["report_geometry_color"]["median"] - out["report_geometry"]["median"], 4)
    out["other_rows_identical"] = bool(all(np.asarray(rows["geometry_color"][key]).tobytes() == np.asarray(v).tobytes()
                                           for key, v in rows["geometry"].items()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--only", choices=("builds", "report"), default=None)
    ap.add_argument("--arms", default="normals,ssim,p2d,color_u8,color_f64", help="the timed builds to run (comma-separated)")
    args = ap.parse_args()
    if args.only in (None, "builds"):
        print(json.dumps(builds(args)), flush=True)
    if args.only in (None, "report"):
        print(json.dumps(report(args)), flush=True)


if __name__ == "__main__":
    main()
