"""ctypes binding of libpccm.so (include/pccm.h) -- the only door to the GPU.

There is no CPU implementation behind this module: if the shared library is missing, or no
MI355X is visible when an :class:`Engine` is created, it raises.  Build the library with
``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C open_pcc_metric_amd/csrc``.
"""
from __future__ import annotations

import ctypes
import os
import sys
import threading
from typing import Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PCCM_LIB: another build of the same library (tests load a diagnostic build -- make DIAG=1 BUILD=<dir> -- through it)
LIB_PATH = os.environ.get("PCCM_LIB") or os.path.join(_HERE, "csrc", "libpccm.so")

OK, E_ARG, E_NODEV, E_HIP, E_OOM, E_STATE, E_RANGE = 0, -1, -2, -3, -4, -5, -6
F32, F64 = 0, 1
DIR_LEFT, DIR_RIGHT, DIR_SELF = 0, 1, 2
PATH_REDUCE = 3          # Engine.last_path: the last reduction batch
ENGINES = {"auto": 0, "brute": 1, "grid": 2}
NORMAL_MODES = {"row": 0, "neighbour": 1}
TIES = {"pick": 0, "mean": 1}          # PCCM_TIES_PICK / PCCM_TIES_MEAN
DUPLICATES = {"drop": 1, "average": 2}  # PCCM_DUP_DROP / PCCM_DUP_AVERAGE
METRIC_D1, METRIC_D2, METRIC_PROJ = 0, 1, 2
MAP_CLAMP, MAP_ROOT = 1, 2          # Engine.reduce_map_*: PCCM_MAP_*
MAP_DENSITY = 4                     # PCCM_MAP_DENSITY: the map behind Engine.reduce_density_* (reduce_map_* refuses it)
MAP_MOMENT = 8                      # PCCM_MAP_MOMENT: the map behind Engine.reduce_moment_* (likewise)
MAX_OCCUPANCY = 4                   # voxel sizes per Engine.voxel_occupancy call (pccm_voxel_occupancy)
MOMENT_KINDS = 16                   # kinds 0..15 of an alignment moment (include/pccm.h)
METRIC_ANGULAR = 3       # plane-to-plane angular similarity (normal_mode does not apply)
# PointSSIM: feature attributes (PCCM_SSIM_* bit flags) and the similarity column of each (PCCM_METRIC_SSIM_*)
SSIM_ATTRS = {"geometry": 1, "normal": 2, "curvature": 4, "color": 8}
METRIC_SSIM = {"geometry": 4, "normal": 5, "curvature": 6, "color": 7}
METRIC_P2D = 8           # point-to-distribution (Mahalanobis) column of a direction (pccm_p2d_build; normal_mode does not apply)
METRIC_P2D_COLOR = 9     # ... its colour (luma) column and
METRIC_P2D_JOINT = 10    # ... its joint geometry-and-colour column (pccm_p2d_build_attrs with P2D_COLOR)
METRIC_RESOLUTION = 11   # point spacings of the cloud a direction iterates (pccm_resolution_build; normal_mode does not apply)
METRIC_REFLECTANCE = 12  # squared reflectance error against the matched point (pccm_set_reflectance; normal_mode does not apply)
P2D_GEOMETRY, P2D_COLOR = 1, 2      # PCCM_P2D_*: what pccm_p2d_build_attrs builds (P2D_COLOR: the colour and the joint column)
KERNEL_CLASSES = {"ingest": 0, "scan": 1, "refine": 2, "fallback": 3, "point": 4, "reduce": 5,
                  "grid_build": 6, "grid_query": 7, "grid_finish": 8}

# every symbol include/pccm.h declares (tests check that the library exports all of them)
SYMBOLS = (
    "pccm_version", "pccm_last_error", "pccm_device_count", "pccm_ctx_create", "pccm_ctx_destroy", "pccm_ctx_reset",
    "pccm_set_cloud", "pccm_set_normals", "pccm_set_normals_deferred", "pccm_flush_uploads", "pccm_set_io_staged", "pccm_estimate_normals", "pccm_get_normals", "pccm_carry_normals",
    "pccm_merge_duplicates", "pccm_get_merge_map", "pccm_get_points", "pccm_get_colors", "pccm_voxel_occupancy",
    "pccm_ssim_features", "pccm_get_ssim_features", "pccm_p2d_build", "pccm_p2d_build_attrs", "pccm_get_p2d_neighbours",
    "pccm_resolution_build", "pccm_get_resolution", "pccm_set_shard", "pccm_set_shard_dir", "pccm_shard_range", "pccm_nn", "pccm_nn_pair", "pccm_nn_fuse", "pccm_nn_want_idx", "pccm_nn_fetch",
    "pccm_error_vectors", "pccm_point_metric", "pccm_tie_exposure", "pccm_set_ties", "pccm_tie_counts", "pccm_xvec_len", "pccm_reduce_prefetch", "pccm_reduce_prefetch_many", "pccm_reduce", "pccm_finish_sum",
    "pccm_reduce_total", "pccm_reduce_total_many", "pccm_select_prefetch_many", "pccm_select_many", "pccm_count_prefetch_many", "pccm_count_many", "pccm_reduce_map_prefetch_many", "pccm_reduce_map_total_many", "pccm_match_counts", "pccm_reduce_density_prefetch_many", "pccm_reduce_density_total_many", "pccm_reduce_moment_prefetch_many", "pccm_reduce_moment_total_many", "pccm_transform_cloud", "pccm_get_bounds", "pccm_cvec_len", "pccm_reduce_chunks_many", "pccm_finish_chunks",
    "pccm_set_wait", "pccm_wait_counter",
    "pccm_set_reflectance", "pccm_set_reflectance_u16", "pccm_get_reflectance",
    "pccm_set_colors", "pccm_set_colors_u8", "pccm_color_reduce", "pccm_color_rows", "pccm_seq_colsum", "pccm_obb_frames", "pccm_extreme_rows", "pccm_rows_outside",
    "pccm_color_transform", "pccm_lzf_decompress", "pccm_drop_caches", "pccm_graph_begin", "pccm_graph_end", "pccm_graph_launch", "pccm_graph_destroy",
    "pccm_set_tail_filing", "pccm_graph_tail_filed",
    "pccm_sync",
    "pccm_profile_enable", "pccm_profile_reset", "pccm_profile_get", "pccm_nn_stats", "pccm_nn_path", "pccm_grid_geometry",
    "pccm_build_plan", "pccm_build_fetch",
)

# structures a build leaves (pccm_build_plan / pccm_build_fetch) and the fields of a plan, in the order of PCCM_BP_*
BUILD_GRID0, BUILD_GRID1, BUILD_SHARD_LEFT, BUILD_SHARD_RIGHT, BUILD_SHARD_SELF, BUILD_SP0, BUILD_SP1 = range(7)
_BUILD_PLAN_FIELDS = ("rec32", "ncells", "n", "row0", "has_occ", "morton", "bits", "dim0", "dim1", "dim2", "lg", "nbin", "tiles",
                      "tile_rows", "scan", "scan_tiles", "read_sp", "njobs", "job", "job_row0_0", "job_row0_1", "job_n_0", "job_n_1",
                      "has_cs")

COLOR_SCHEMES = {"rgb": 0, "ycc": 1, "yuv": 2}
COLOR_OWN, COLOR_NEIGHBOUR, COLOR_DIFF, COLOR_SQUARE = 0, 1, 2, 3

_lib = None


class NativeLibraryMissing(ImportError):
    pass


class PccmStateError(RuntimeError):
    """PCCM_E_STATE: a call came in the wrong order or hit a stale object (a hipGraph captured before buffers
    changed, a reduction before its search).  The context is intact; callers may recover (CloudPair re-captures)."""


class PccmDeviceError(RuntimeError):
    """PCCM_E_HIP / PCCM_E_NODEV: the HIP runtime reported a failure.  Never retried, never swallowed."""


def load() -> ctypes.CDLL:
    """dlopen libpccm.so and declare the prototypes of include/pccm.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} is not built: open_pcc_metric_amd has no CPU fallback. "
            "Run `make -C open_pcc_metric_amd/csrc` (needs hipcc, --offload-arch=gfx950).")
    # PyTorch ships its own libamdhip64.so.7; loading it first makes libpccm.so bind to that same
    # runtime (one HIP runtime per process), so torch device tensors and streams can be handed in.
    # PCCM_NO_TORCH=1 (the command line sets it for single-process runs): skip the ~1.5 s import; nothing in this
    # process may import torch afterwards and expect to see the GPU.
    if "torch" in sys.modules or os.environ.get("PCCM_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    dp = ctypes.POINTER(ctypes.c_double)
    lib.pccm_version.restype = i32
    lib.pccm_last_error.restype = ctypes.c_char_p
    lib.pccm_device_count.argtypes = [ctypes.POINTER(i32)]
    lib.pccm_ctx_create.argtypes = [i32, vp, ctypes.POINTER(vp)]
    lib.pccm_ctx_destroy.argtypes = [vp]
    lib.pccm_ctx_reset.argtypes = [vp]
    lib.pccm_set_cloud.argtypes = [vp, i32, vp, i64, i32, i32]
    lib.pccm_set_normals.argtypes = [vp, i32, vp, i64, i32, i32]
    lib.pccm_set_normals_deferred.argtypes = [vp, i32, vp, i64, i32]
    lib.pccm_flush_uploads.argtypes = [vp]
    lib.pccm_set_io_staged.argtypes = [vp, i32]
    lib.pccm_set_wait.argtypes = [vp, i32]
    lib.pccm_wait_counter.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.pccm_set_shard.argtypes = [vp, i32, i32]
    lib.pccm_set_shard_dir.argtypes = [vp, i32, i32, i32]
    lib.pccm_estimate_normals.argtypes = [vp, i32, i32]
    lib.pccm_get_normals.argtypes = [vp, i32, vp]
    lib.pccm_carry_normals.argtypes = [vp, i32, ctypes.POINTER(i32)]
    lib.pccm_merge_duplicates.argtypes = [vp, i32, i32, ctypes.POINTER(i64)]
    lib.pccm_get_merge_map.argtypes = [vp, i32, vp, ctypes.POINTER(i64)]
    lib.pccm_get_points.argtypes = [vp, i32, vp]
    lib.pccm_get_colors.argtypes = [vp, i32, vp]
    lib.pccm_voxel_occupancy.argtypes = [vp, i32, dp, ctypes.POINTER(i64)]
    lib.pccm_ssim_features.argtypes = [vp, i32, i32, i32, ctypes.POINTER(i32)]
    lib.pccm_get_ssim_features.argtypes = [vp, i32, i32, vp]
    lib.pccm_p2d_build.argtypes = [vp, i32, ctypes.POINTER(i32)]
    lib.pccm_p2d_build_attrs.argtypes = [vp, i32, i32, ctypes.POINTER(i32)]
    lib.pccm_get_p2d_neighbours.argtypes = [vp, i32, vp, vp]
    lib.pccm_resolution_build.argtypes = [vp, i32, i32, ctypes.POINTER(i32)]
    lib.pccm_get_resolution.argtypes = [vp, i32, vp]
    lib.pccm_shard_range.argtypes = [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.pccm_nn.argtypes = [vp, i32, i32]
    lib.pccm_nn_pair.argtypes = [vp, i32]
    lib.pccm_nn_fuse.argtypes = [vp, i32, i32]
    lib.pccm_nn_want_idx.argtypes = [vp, i32]
    lib.pccm_nn_fetch.argtypes = [vp, i32, vp, vp]
    lib.pccm_error_vectors.argtypes = [vp, i32, vp]
    lib.pccm_point_metric.argtypes = [vp, i32, i32, i32, vp]
    lib.pccm_tie_exposure.argtypes = [vp, i32, i32, dp]
    lib.pccm_set_ties.argtypes = [vp, i32]
    lib.pccm_tie_counts.argtypes = [vp, i32, vp]
    lib.pccm_xvec_len.argtypes = [i64]
    lib.pccm_xvec_len.restype = i64
    lib.pccm_reduce.argtypes = [vp, i32, i32, i32, vp, vp]
    lib.pccm_reduce_prefetch.argtypes = [vp, i32, i32, i32]
    ip = ctypes.POINTER(i32)
    lib.pccm_reduce_prefetch_many.argtypes = [vp, i32, ip, ip, ip]
    lib.pccm_finish_sum.argtypes = [vp, i64, dp]
    lib.pccm_reduce_total.argtypes = [vp, i32, i32, i32, dp]
    lib.pccm_reduce_total_many.argtypes = [vp, i32, ip, ip, ip, dp]
    lp = ctypes.POINTER(i64)
    lib.pccm_select_prefetch_many.argtypes = [vp, i32, ip, ip, ip, lp]
    lib.pccm_select_many.argtypes = [vp, i32, ip, ip, ip, lp, dp]
    lib.pccm_count_prefetch_many.argtypes = [vp, i32, ip, ip, ip, dp]
    lib.pccm_count_many.argtypes = [vp, i32, ip, ip, ip, dp, lp]
    lib.pccm_reduce_map_prefetch_many.argtypes = [vp, i32, ip, ip, ip, ip, dp]
    lib.pccm_reduce_map_total_many.argtypes = [vp, i32, ip, ip, ip, ip, dp, dp]
    lib.pccm_match_counts.argtypes = [vp, i32, vp]
    lib.pccm_reduce_density_prefetch_many.argtypes = [vp, i32, ip, ip, dp]
    lib.pccm_reduce_density_total_many.argtypes = [vp, i32, ip, ip, dp, dp]
    lib.pccm_reduce_moment_prefetch_many.argtypes = [vp, i32, ip, ip, dp, dp]
    lib.pccm_reduce_moment_total_many.argtypes = [vp, i32, ip, ip, dp, dp, dp]
    lib.pccm_transform_cloud.argtypes = [vp, i32, dp]
    lib.pccm_get_bounds.argtypes = [vp, i32, dp, dp]
    lib.pccm_cvec_len.argtypes = [i64]
    lib.pccm_cvec_len.restype = i64
    lib.pccm_reduce_chunks_many.argtypes = [vp, i32, ip, ip, ip, dp, dp]
    lib.pccm_finish_chunks.argtypes = [vp, i64, dp]
    lib.pccm_sync.argtypes = [vp]
    lib.pccm_drop_caches.argtypes = [vp]
    lib.pccm_color_transform.argtypes = [vp, i64, i32, vp]
    lib.pccm_lzf_decompress.argtypes = [vp, i64, vp, i64, ctypes.POINTER(i64)]
    lib.pccm_set_colors.argtypes = [vp, i32, vp, i64, i32, i32]
    lib.pccm_set_colors_u8.argtypes = [vp, i32, vp, i64]
    lib.pccm_set_reflectance.argtypes = [vp, i32, vp, i64, i32, i32]
    lib.pccm_set_reflectance_u16.argtypes = [vp, i32, vp, i64]
    lib.pccm_get_reflectance.argtypes = [vp, i32, vp]
    lib.pccm_color_reduce.argtypes = [vp, i32, i32, ctypes.c_double, vp, i64, dp, dp]
    lib.pccm_seq_colsum.argtypes = [vp, vp, i64, dp]
    lib.pccm_obb_frames.argtypes = [vp, vp, i64, vp, i64, dp, dp]
    lib.pccm_extreme_rows.argtypes = [vp, i32, vp, i32, vp]
    lib.pccm_rows_outside.argtypes = [vp, i32, vp, i32, ctypes.c_double, vp, ctypes.POINTER(i64)]
    lib.pccm_color_rows.argtypes = [vp, i32, i32, ctypes.c_double, i32, vp, i64, vp]
    lib.pccm_graph_begin.argtypes = [vp]
    lib.pccm_graph_end.argtypes = [vp, ctypes.POINTER(i32)]
    lib.pccm_graph_launch.argtypes = [vp, i32]
    lib.pccm_graph_destroy.argtypes = [vp, i32]
    lib.pccm_set_tail_filing.argtypes = [vp, i32]
    lib.pccm_graph_tail_filed.argtypes = [vp, i32, ctypes.POINTER(i32)]
    lib.pccm_profile_enable.argtypes = [vp, i32]
    lib.pccm_profile_reset.argtypes = [vp]
    lib.pccm_profile_get.argtypes = [vp, i32, dp, ctypes.POINTER(i64)]
    lib.pccm_nn_stats.argtypes = [vp, i32, ctypes.POINTER(i64)]
    lib.pccm_nn_path.argtypes = [vp, i32, ctypes.c_char_p, i64, ctypes.POINTER(i64)]
    lib.pccm_grid_geometry.argtypes = [vp, dp, dp, vp]
    lib.pccm_build_plan.argtypes = [vp, i32, lp, dp]
    lib.pccm_build_fetch.argtypes = [vp, i32, vp, vp, vp, vp]
    for name in SYMBOLS:
        fn = getattr(lib, name)
        if name not in ("pccm_last_error", "pccm_xvec_len", "pccm_cvec_len"):
            fn.restype = i32
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc == OK:
        return
    msg = load().pccm_last_error().decode("utf-8", "replace")
    if rc == E_ARG:
        raise ValueError(msg)
    if rc == E_RANGE:
        raise IndexError(msg)
    if rc == E_OOM:
        raise MemoryError(msg)
    if rc == E_STATE:
        raise PccmStateError(f"libpccm error {rc}: {msg}")
    if rc in (E_HIP, E_NODEV):
        raise PccmDeviceError(f"libpccm error {rc}: {msg}")
    raise RuntimeError(f"libpccm error {rc}: {msg}")


def device_count() -> int:
    n = ctypes.c_int(0)
    _check(load().pccm_device_count(ctypes.byref(n)))
    return int(n.value)


def xvec_len(n: int) -> int:
    return int(load().pccm_xvec_len(int(n)))


def cvec_len(n: int) -> int:
    return int(load().pccm_cvec_len(int(n)))


def finish_chunks(cvec: np.ndarray, n: int) -> float:
    """np.sum of the whole per-point column, from its (all-reduced) chunk vector (pccm_reduce_chunks_many)."""
    cvec = np.ascontiguousarray(cvec, dtype=np.float64)
    if cvec.shape[0] != cvec_len(n):
        raise ValueError("chunk vector has the wrong length")
    out = ctypes.c_double(0.0)
    _check(load().pccm_finish_chunks(cvec.ctypes.data_as(ctypes.c_void_p), int(n), ctypes.byref(out)))
    return np.float64(out.value)


def finish_sum(xvec: np.ndarray, n: int) -> float:
    """np.sum of the whole per-point column, from its (all-reduced) exchange vector."""
    xvec = np.ascontiguousarray(xvec, dtype=np.float64)
    if xvec.shape[0] != xvec_len(n):
        raise ValueError("exchange vector has the wrong length")
    out = ctypes.c_double(0.0)
    _check(load().pccm_finish_sum(xvec.ctypes.data_as(ctypes.c_void_p), int(n), ctypes.byref(out)))
    return np.float64(out.value)


def color_transform(colors: np.ndarray, scheme: str) -> np.ndarray:
    """rgb rows -> "ycc" / "yuv" rows (host helper of libpccm; see pccm_color_transform)."""
    src = np.ascontiguousarray(colors, dtype=np.float64)
    if src.ndim != 2 or src.shape[1] != 3:
        raise ValueError("colors must have shape (N, 3)")
    out = np.empty_like(src)
    _check(load().pccm_color_transform(src.ctypes.data_as(ctypes.c_void_p), src.shape[0], {"ycc": 1, "yuv": 2}[scheme],
                                       out.ctypes.data_as(ctypes.c_void_p)))
    return out


def lzf_decompress(data: bytes, size: int) -> bytes:
    """liblzf decompression (host helper of libpccm; PCD binary_compressed bodies)."""
    out = ctypes.create_string_buffer(max(1, int(size)))
    got = ctypes.c_int64()
    _check(load().pccm_lzf_decompress(ctypes.c_char_p(bytes(data)), len(data), out, int(size), ctypes.byref(got)))
    return out.raw[:got.value]


# ---- engine pool ------------------------------------------------------------------------------------------------
# Creating a context is cheap, tearing one down is not (4 ms of hipFree for a 1M-point pair) and a fresh one starts
# with cold allocations (+0.8 ms) and no grid decisions to inherit.  CloudPair therefore borrows its engine here and
# hands it back when it dies; a caller that evaluates one pair after the other pays the work, not the lifecycle.
_POOL: dict = {}
_POOL_MAX = 2
_POOL_LOCK = threading.Lock()      # evaluate_pairs drives the pool from several host threads; __del__ may run on any


def acquire_engine(device: int = 0) -> "Engine":
    while True:
        with _POOL_LOCK:
            pool = _POOL.get(int(device))
            eng = pool.pop() if pool else None
        if eng is None:
            return Engine(device)
        try:
            eng.reset()
            eng.pairs_served = getattr(eng, "pairs_served", 0) + 1      # (a context on its second pair: a loop over pairs, see CloudPair)
            return eng
        except PccmStateError:                 # a context that cannot be reset is not worth keeping
            eng.close()
        # anything else (a HIP failure in particular) propagates: it is not ours to hide


def release_engine(eng: "Engine") -> None:
    if not getattr(eng, "_ctx", None) or not eng._ctx.value:
        return                                 # closed by hand
    with _POOL_LOCK:
        pool = _POOL.setdefault(eng.device, [])
        if eng in pool:
            return
        keep = len(pool) < _POOL_MAX
        if keep:
            pool.append(eng)
    if not keep:
        eng.close()


def drain_pool() -> None:
    while True:
        with _POOL_LOCK:
            eng = next((pool.pop() for pool in _POOL.values() if pool), None)
        if eng is None:
            return
        eng.close()


import atexit  # noqa: E402

atexit.register(drain_pool)


def _as_rows(a, what: str) -> Tuple[object, int, int, int, object]:
    """-> (pointer, n, dtype code, on_device, keepalive) for an (N, 3) f32/f64 array or CUDA tensor."""
    if hasattr(a, "is_cuda") and hasattr(a, "data_ptr"):      # torch tensor
        import torch
        if not a.is_cuda:
            a = a.detach().cpu().numpy()
        else:
            if a.dtype not in (torch.float32, torch.float64):
                a = a.to(torch.float64)
            a = a.contiguous()
            if a.dim() != 2 or a.shape[1] != 3:
                raise ValueError(f"{what} must have shape (N, 3)")
            torch.cuda.current_stream(a.device).synchronize()
            return ctypes.c_void_p(a.data_ptr()), int(a.shape[0]), F32 if a.dtype == torch.float32 else F64, 1, a
    arr = np.asarray(a)
    if arr.dtype != np.float32:
        arr = arr.astype(np.float64, copy=False)
    arr = np.ascontiguousarray(arr)
    if arr.ndim != 2 or arr.shape[1] != 3:
        raise ValueError(f"{what} must have shape (N, 3)")
    return arr.ctypes.data_as(ctypes.c_void_p), int(arr.shape[0]), F32 if arr.dtype == np.float32 else F64, 0, arr


def _modes(normal_mode, k: int):
    """One normal mode for all k requests, or one per request."""
    if isinstance(normal_mode, str):
        return [NORMAL_MODES[normal_mode]] * k
    modes = [NORMAL_MODES[m] for m in normal_mode]
    if len(modes) != k:
        raise ValueError(f"{len(modes)} normal modes for {k} requests")
    return modes


class Engine:
    """One libpccm context = one GPU.  Method names mirror include/pccm.h."""
    keeps_self_search = True      # pccm_set_cloud(1, ...) leaves cloud 0 and its self search untouched (CloudPair.with_reconst)

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._lib = load()
        self._ctx = ctypes.c_void_p()
        _check(self._lib.pccm_ctx_create(int(device), ctypes.c_void_p(stream) if stream else None,
                                         ctypes.byref(self._ctx)))
        self.device = int(device)
        self._n = [0, 0]
        self._p2d_k = 0               # neighbourhood size of the point-to-distribution columns in HBM (0: none)

    def close(self) -> None:
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.pccm_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        """Forget clouds, shard, graphs and profile; keep the device allocations (pccm_ctx_reset)."""
        _check(self._lib.pccm_ctx_reset(self._ctx))
        self._n = [0, 0]
        self._p2d_k = 0

    # -- inputs ---------------------------------------------------------------------------
    def set_cloud(self, which: int, points) -> None:
        ptr, n, dt, dev, keep = _as_rows(points, "points")
        _check(self._lib.pccm_set_cloud(self._ctx, int(which), ptr, n, dt, dev))
        self._n[which] = n
        self._p2d_k = 0               # (new points in either cloud drop both columns)

    def set_normals(self, which: int, normals) -> None:
        ptr, n, dt, dev, keep = _as_rows(normals, "normals")
        self.__dict__.setdefault("_deferred", {}).pop(int(which), None)
        _check(self._lib.pccm_set_normals(self._ctx, int(which), ptr, n, dt, dev))

    def set_normals_deferred(self, which: int, normals) -> None:
        """Announce host normals now, upload them when they are needed or at flush_uploads() -- beside the searches, which do
        not read them (include/pccm.h).  The array is kept alive here until then; device arrays are set at once."""
        ptr, n, dt, dev, keep = _as_rows(normals, "normals")
        if dev:
            _check(self._lib.pccm_set_normals(self._ctx, int(which), ptr, n, dt, dev))
            return
        _check(self._lib.pccm_set_normals_deferred(self._ctx, int(which), ptr, n, dt))
        self.__dict__.setdefault("_deferred", {})[int(which)] = keep

    def set_io_staged(self, on: bool) -> None:
        """Large transfers through the context's own pinned buffers (default) or straight from / to the caller's arrays
        (see pccm_set_io_staged in include/pccm.h)."""
        _check(self._lib.pccm_set_io_staged(self._ctx, 1 if on else 0))

    def set_wait(self, mode: str) -> None:
        """How reductions wait for the GPU: "spin" (default: on the context's completion counter) or "event" (the thread
        sleeps in hipEventSynchronize; see pccm_set_wait in include/pccm.h)."""
        modes = {"spin": 0, "event": 1}
        if mode not in modes:
            raise ValueError(f"wait mode {mode!r}: expected one of {sorted(modes)}")
        _check(self._lib.pccm_set_wait(self._ctx, modes[mode]))

    def wait_counter(self) -> int:
        """Reduction batches whose numbers have reached the host so far (pccm_wait_counter)."""
        out = ctypes.c_uint64(0)
        _check(self._lib.pccm_wait_counter(self._ctx, ctypes.byref(out)))
        return int(out.value)

    def flush_uploads(self) -> None:
        try:
            _check(self._lib.pccm_flush_uploads(self._ctx))
        finally:
            self.__dict__.get("_deferred", {}).clear()

    def set_colors(self, which: int, colors) -> None:
        ptr, n, dt, dev, keep = _as_rows(colors, "colors")
        _check(self._lib.pccm_set_colors(self._ctx, int(which), ptr, n, dt, dev))

    def set_colors_u8(self, which: int, colors_u8) -> None:
        """Colours as (N, 3) uint8; the device widens them as k / 255.0 (what the file readers do on the host)."""
        c = np.ascontiguousarray(colors_u8, dtype=np.uint8)
        if c.ndim != 2 or c.shape[1] != 3:
            raise ValueError("colors_u8 must have shape (N, 3)")
        _check(self._lib.pccm_set_colors_u8(self._ctx, int(which), c.ctypes.data_as(ctypes.c_void_p), c.shape[0]))

    @staticmethod
    def _rows_arg(rows):
        if rows is None:
            return None, 0, None
        keep = np.ascontiguousarray(rows, dtype=np.int32)
        return keep.ctypes.data_as(ctypes.c_void_p), keep.shape[0], keep

    def color_reduce(self, direction: int, scheme: str, scale: float = 1.0, rows=None):
        """-> (column sums in np.add.reduce(axis=0) order, column maxima) of (scale * colour difference)**2."""
        ptr, n, keep = self._rows_arg(rows)
        sums, maxs = (ctypes.c_double * 3)(), (ctypes.c_double * 3)()
        _check(self._lib.pccm_color_reduce(self._ctx, int(direction), COLOR_SCHEMES[scheme], float(scale), ptr, n, sums, maxs))
        return np.array(sums[:], dtype=np.float64), np.array(maxs[:], dtype=np.float64)

    def extreme_rows(self, which: int, directions) -> np.ndarray:
        """Rows of the (about) farthest points of cloud ``which`` along each of <= 1024 directions."""
        d = np.ascontiguousarray(directions, dtype=np.float32)
        out = np.empty(d.shape[0], dtype=np.int32)
        _check(self._lib.pccm_extreme_rows(self._ctx, int(which), d.ctypes.data_as(ctypes.c_void_p), d.shape[0],
                                           out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def rows_outside(self, which: int, planes, margin: float) -> np.ndarray:
        """Rows of cloud ``which`` not strictly inside the polytope ``n.x + off <= 0`` (planes: (F, 4), Qhull's equations)."""
        p = np.ascontiguousarray(planes, dtype=np.float64)
        out = np.empty(self._n[which], dtype=np.int32)
        cnt = ctypes.c_int64()
        _check(self._lib.pccm_rows_outside(self._ctx, int(which), p.ctypes.data_as(ctypes.c_void_p), p.shape[0], float(margin),
                                           out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(cnt)))
        return out[:cnt.value]

    def obb_frames(self, hull_vertices, hull_triangles):
        """-> (extents, volume) of the smallest box over the frames of the hull's triangles (pccm_obb_frames)."""
        v = np.ascontiguousarray(hull_vertices, dtype=np.float64)
        t = np.ascontiguousarray(hull_triangles, dtype=np.float64)
        if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 3 or t.shape[1:] != (3, 3):
            raise ValueError("hull_vertices must be (H, 3) and hull_triangles (T, 3, 3)")
        ext, vol = (ctypes.c_double * 3)(), ctypes.c_double()
        _check(self._lib.pccm_obb_frames(self._ctx, v.ctypes.data_as(ctypes.c_void_p), v.shape[0], t.ctypes.data_as(ctypes.c_void_p),
                                         t.shape[0], ext, ctypes.byref(vol)))
        return np.array(ext[:], dtype=np.float64), vol.value

    def seq_colsum(self, columns) -> np.ndarray:
        """np.add.reduce(a, axis=0) of a non-negative (N, 3) array, bit for bit, on the device."""
        a = np.asarray(columns, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] == 0:
            raise ValueError("columns must have shape (N, 3), N > 0")
        cols = np.ascontiguousarray(a.T)
        out = (ctypes.c_double * 3)()
        _check(self._lib.pccm_seq_colsum(self._ctx, cols.ctypes.data_as(ctypes.c_void_p), a.shape[0], out))
        return np.array(out[:], dtype=np.float64)

    def color_rows(self, direction: int, scheme: str, what: int, scale: float = 1.0, rows=None) -> np.ndarray:
        """(n_iter, 3) rows: what = COLOR_OWN | COLOR_NEIGHBOUR | COLOR_DIFF | COLOR_SQUARE."""
        ptr, n, keep = self._rows_arg(rows)
        out = np.empty((self.n_iter(direction), 3), dtype=np.float64)
        _check(self._lib.pccm_color_rows(self._ctx, int(direction), COLOR_SCHEMES[scheme], float(scale), int(what), ptr, n,
                                         out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def estimate_normals(self, which: int, knn: int = 30) -> None:
        """Open3D-style normals (k-NN covariance, smallest eigenvector) computed and kept on the device."""
        _check(self._lib.pccm_estimate_normals(self._ctx, int(which), int(knn)))

    def carry_normals(self, from_which: int) -> bool:
        """Give the other cloud the normals of cloud ``from_which``, averaged over the points whose nearest neighbour each of
        its points is (pccm_carry_normals: MPEG pc_error's normal carrying); they stay on the device.  True when work was done."""
        built = ctypes.c_int32(0)
        _check(self._lib.pccm_carry_normals(self._ctx, int(from_which), ctypes.byref(built)))
        return bool(built.value)

    def merge_duplicates(self, which: int, mode) -> int:
        """Merge the rows of cloud ``which`` that share their coordinates, in place on the device (pccm_merge_duplicates: MPEG
        pc_error's dropDuplicates).  ``mode``: "drop" (1) keeps the first row's colour, "average" (2) the group's average.  Returns
        the number of rows left; normals and colours that were uploaded follow."""
        if isinstance(mode, str) and mode not in DUPLICATES:
            raise ValueError(f"duplicates mode {mode!r}: expected one of {sorted(DUPLICATES)}")
        m = DUPLICATES[mode] if isinstance(mode, str) else mode      # (an integer goes to the library as it is)
        n_out = ctypes.c_int64(0)
        _check(self._lib.pccm_merge_duplicates(self._ctx, int(which), int(m), ctypes.byref(n_out)))
        self.__dict__.get("_deferred", {}).pop(int(which), None)      # (announced normals were uploaded first)
        if int(n_out.value) != self._n[which]:
            self._n[which] = int(n_out.value)
            self._p2d_k = 0               # (new points in either cloud drop both columns)
        return int(n_out.value)

    def get_merge_map(self, which: int) -> np.ndarray:
        """For every row cloud ``which`` had before merge_duplicates, the merged row of its group (the identity if never merged)."""
        nb = ctypes.c_int64(0)
        _check(self._lib.pccm_get_merge_map(self._ctx, int(which), None, ctypes.byref(nb)))
        out = np.empty(int(nb.value), dtype=np.int32)
        _check(self._lib.pccm_get_merge_map(self._ctx, int(which), out.ctypes.data_as(ctypes.c_void_p), None))
        return out

    def voxel_occupancy(self, voxels) -> list:
        """For each of up to MAX_OCCUPANCY voxel sizes: ``(nA, nB, nAB)`` -- the voxels of the absolute lattice
        floor(coordinate / voxel) that resident cloud 0 occupies, that cloud 1 occupies, and that both do (pccm_voxel_occupancy:
        one table over both clouds per size, every count an integer).  One call, one wait."""
        sizes = np.ascontiguousarray(list(voxels), dtype=np.float64)
        out = np.zeros(3 * max(len(sizes), 1), dtype=np.int64)
        _check(self._lib.pccm_voxel_occupancy(self._ctx, len(sizes), sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                              out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return [(int(out[3 * k]), int(out[3 * k + 1]), int(out[3 * k + 2])) for k in range(len(sizes))]

    def get_points(self, which: int) -> np.ndarray:
        out = np.empty((self._n[which], 3), dtype=np.float64)
        _check(self._lib.pccm_get_points(self._ctx, int(which), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def get_colors(self, which: int) -> np.ndarray:
        out = np.empty((self._n[which], 3), dtype=np.float64)
        _check(self._lib.pccm_get_colors(self._ctx, int(which), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def set_reflectance(self, which: int, reflectance) -> None:
        """One scalar per point of cloud ``which`` (pccm_set_reflectance*): ``uint8`` / ``uint16`` arrays go to the library
        as 16-bit words (pccm_set_reflectance_u16 widens them exactly), ``float32`` as it is, anything else as ``float64``; the
        values are kept as given.  ValueError for a wrong length or a non-finite value."""
        r = np.asarray(reflectance)
        if r.ndim == 2 and r.shape[1] == 1:
            r = r[:, 0]
        if r.ndim != 1:
            raise ValueError("reflectance must have shape (N,)")
        if r.dtype in (np.dtype(np.uint8), np.dtype(np.uint16)):
            r = np.ascontiguousarray(r, dtype=np.uint16)
            _check(self._lib.pccm_set_reflectance_u16(self._ctx, int(which), r.ctypes.data_as(ctypes.c_void_p), r.shape[0]))
            return
        r = np.ascontiguousarray(r, dtype=np.float32 if r.dtype == np.float32 else np.float64)
        _check(self._lib.pccm_set_reflectance(self._ctx, int(which), r.ctypes.data_as(ctypes.c_void_p), r.shape[0],
                                              F32 if r.dtype == np.float32 else F64, 0))

    def get_reflectance(self, which: int) -> np.ndarray:
        """The stored fp64 reflectance column of cloud ``which`` (the merged one after merge_duplicates)."""
        out = np.empty(self._n[which], dtype=np.float64)
        _check(self._lib.pccm_get_reflectance(self._ctx, int(which), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def get_normals(self, which: int) -> np.ndarray:
        out = np.empty((self._n[which], 3), dtype=np.float64)
        _check(self._lib.pccm_get_normals(self._ctx, int(which), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def ssim_features(self, which: int, k: int, attrs) -> bool:
        """Build (or find) cloud ``which``'s PointSSIM feature columns for the attribute names ``attrs`` in HBM; True when work
        was done (pccm_ssim_features)."""
        mask = 0
        for a in attrs:
            mask |= SSIM_ATTRS[a]
        built = ctypes.c_int32()
        _check(self._lib.pccm_ssim_features(self._ctx, int(which), int(k), mask, ctypes.byref(built)))
        return bool(built.value)

    def get_ssim_features(self, which: int, attr: str) -> np.ndarray:
        out = np.empty(self._n[which], dtype=np.float64)
        _check(self._lib.pccm_get_ssim_features(self._ctx, int(which), SSIM_ATTRS[attr], out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def p2d_build(self, k: int, attrs: int = P2D_GEOMETRY) -> bool:
        """Build (or find) the point-to-distribution columns of both directions at neighbourhood size ``k`` in HBM; True when
        work was done (pccm_p2d_build_attrs).  ``attrs``: P2D_GEOMETRY, or P2D_GEOMETRY | P2D_COLOR for the colour and joint
        columns as well (both clouds' colours must be on the device)."""
        built = ctypes.c_int32()
        _check(self._lib.pccm_p2d_build_attrs(self._ctx, int(k), int(attrs), ctypes.byref(built)))
        self._p2d_k = int(k)
        return bool(built.value)

    def get_p2d_neighbours(self, direction: int):
        """-> (rows, counts): per point of the iterating cloud of ``direction`` the rows of its neighbours in the other cloud, in
        ascending (d2, row) order ((n, k) int32, -1 beyond the count), and how many there are (pccm_get_p2d_neighbours)."""
        if not self._p2d_k:
            raise PccmStateError("no point-to-distribution columns (p2d_build)")
        n = self.n_iter(direction)
        rows = np.empty((n, self._p2d_k), dtype=np.int32)
        counts = np.empty(n, dtype=np.int32)
        _check(self._lib.pccm_get_p2d_neighbours(self._ctx, int(direction), rows.ctypes.data_as(ctypes.c_void_p),
                                                 counts.ctypes.data_as(ctypes.c_void_p)))
        return rows, counts

    def resolution_build(self, which: int, k: int) -> bool:
        """Build (or find) cloud ``which``'s point spacings over ``k`` neighbours in HBM; True when work was done
        (pccm_resolution_build)."""
        built = ctypes.c_int32()
        _check(self._lib.pccm_resolution_build(self._ctx, int(which), int(k), ctypes.byref(built)))
        return bool(built.value)

    def get_resolution(self, which: int) -> np.ndarray:
        """Cloud ``which``'s point spacings, n doubles (pccm_get_resolution)."""
        out = np.empty(self._n[which], dtype=np.float64)
        _check(self._lib.pccm_get_resolution(self._ctx, int(which), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def set_shard(self, rank: int, world: int) -> None:
        _check(self._lib.pccm_set_shard(self._ctx, int(rank), int(world)))

    def set_shard_dir(self, direction: int, rank: int, world: int) -> None:
        """This context is number ``rank`` of the ``world`` ranks that share the rows of ``direction``; world 0: it
        owns none of them (pccm_set_shard_dir)."""
        _check(self._lib.pccm_set_shard_dir(self._ctx, int(direction), int(rank), int(world)))

    def shard_range(self, direction: int) -> Tuple[int, int]:
        b, e = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(self._lib.pccm_shard_range(self._ctx, int(direction), ctypes.byref(b), ctypes.byref(e)))
        return int(b.value), int(e.value)

    def n_iter(self, direction: int) -> int:
        return self._n[1] if direction == DIR_RIGHT else self._n[0]

    # -- nearest neighbours -----------------------------------------------------------------
    def nn(self, direction: int, engine: str = "auto") -> None:
        _check(self._lib.pccm_nn(self._ctx, int(direction), ENGINES[engine]))

    def nn_pair(self, engine: str = "auto") -> None:
        """Both directional sweeps of CloudPair.__init__ (cloud_pair.py:67-78) in one call."""
        _check(self._lib.pccm_nn_pair(self._ctx, ENGINES[engine]))

    def nn_fuse(self, direction: int, normal_mode: Optional[str]) -> None:
        """Fuse the D2 projection of ``direction`` into the next searches (pccm_nn_fuse); ``None`` switches it off."""
        _check(self._lib.pccm_nn_fuse(self._ctx, int(direction), -1 if normal_mode is None else NORMAL_MODES[normal_mode]))

    def nn_want_idx(self, on: bool) -> None:
        """Whether the searches store the matched row with every result (pccm_nn_want_idx); off halves the result bytes, and
        whoever asks for the rows later gets them through a repeated search of that direction."""
        _check(self._lib.pccm_nn_want_idx(self._ctx, int(bool(on))))

    def fetch_nn(self, direction: int, want_idx: bool = True, want_d2: bool = True):
        b, e = self.shard_range(direction)
        idx = np.empty(e - b, dtype=np.int32) if want_idx else None
        d2 = np.empty(e - b, dtype=np.float64) if want_d2 else None
        _check(self._lib.pccm_nn_fetch(self._ctx, int(direction),
                                       idx.ctypes.data_as(ctypes.c_void_p) if want_idx else None,
                                       d2.ctypes.data_as(ctypes.c_void_p) if want_d2 else None))
        return idx, d2

    def error_vectors(self, direction: int) -> np.ndarray:
        b, e = self.shard_range(direction)
        out = np.empty((e - b, 3), dtype=np.float64)
        _check(self._lib.pccm_error_vectors(self._ctx, int(direction), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def point_metric(self, direction: int, metric: int, normal_mode: str = "row") -> np.ndarray:
        b, e = self.shard_range(direction)
        out = np.empty(e - b, dtype=np.float64)
        _check(self._lib.pccm_point_metric(self._ctx, int(direction), int(metric), NORMAL_MODES[normal_mode],
                                           out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def tie_exposure(self, direction: int, normal_mode=None) -> dict:
        """Diagnostic of include/pccm.h's pccm_tie_exposure for this shard's rows: how many queries have several
        equidistant nearest neighbours, and the sums of the smallest / largest / chosen squared projection over them
        (``normal_mode`` None: counts only)."""
        out = (ctypes.c_double * 8)()
        _check(self._lib.pccm_tie_exposure(self._ctx, int(direction), -1 if normal_mode is None else NORMAL_MODES[normal_mode], out))
        return {"queries": int(out[0]), "tied": int(out[1]), "sum_min": float(out[2]), "sum_max": float(out[3]), "sum_pick": float(out[4]),
                "not_enumerated": int(out[5]), "max_multiplicity": int(out[6])}

    def set_ties(self, policy: str) -> None:
        """Neighbour policy for exact ties of the next searches (pccm_set_ties): "pick" (smallest row) or "mean"."""
        _check(self._lib.pccm_set_ties(self._ctx, TIES[policy]))

    def tie_counts(self, direction: int) -> np.ndarray:
        """Size of the tie set of every shard row of ``direction`` (pccm_tie_counts; the search ran under "mean")."""
        b, e = self.shard_range(direction)
        out = np.empty(e - b, dtype=np.int32)
        _check(self._lib.pccm_tie_counts(self._ctx, int(direction), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def reduce_prefetch(self, direction: int, metric: int, normal_mode: str = "row") -> None:
        """Enqueue a reduction without waiting; a later reduce() with the same arguments consumes it."""
        _check(self._lib.pccm_reduce_prefetch(self._ctx, int(direction), int(metric), NORMAL_MODES[normal_mode]))

    def reduce_prefetch_many(self, requests, normal_mode: str = "row") -> None:
        """``requests``: up to 8 ``(direction, metric)`` pairs, evaluated and reduced by two launches in all."""
        k = len(requests)
        if k == 0:
            return
        arr = ctypes.c_int * k
        dirs = arr(*[int(r[0]) for r in requests])
        mets = arr(*[int(r[1]) for r in requests])
        modes = arr(*_modes(normal_mode, k))
        _check(self._lib.pccm_reduce_prefetch_many(self._ctx, k, dirs, mets, modes))

    def reduce(self, direction: int, metric: int, normal_mode: str = "row"):
        """-> (xvec, min, max) of this shard; see pccm_reduce() in include/pccm.h."""
        xvec = np.empty(xvec_len(self.n_iter(direction)), dtype=np.float64)
        mm = np.empty(2, dtype=np.float64)
        _check(self._lib.pccm_reduce(self._ctx, int(direction), int(metric), NORMAL_MODES[normal_mode],
                                     xvec.ctypes.data_as(ctypes.c_void_p), mm.ctypes.data_as(ctypes.c_void_p)))
        return xvec, mm[0], mm[1]

    finish_sum = staticmethod(finish_sum)

    def reduce_total(self, direction: int, metric: int, normal_mode: str = "row"):
        """-> (sum, min, max) of the whole column; only when the context is not sharded."""
        out = (ctypes.c_double * 3)()
        _check(self._lib.pccm_reduce_total(self._ctx, int(direction), int(metric), NORMAL_MODES[normal_mode], out))
        return np.float64(out[0]), np.float64(out[1]), np.float64(out[2])

    def reduce_total_many(self, requests, normal_mode: str = "row"):
        """-> [(sum, min, max)] of up to 8 whole columns ``(direction, metric)`` in one call (unsharded contexts)."""
        k = len(requests)
        arr = ctypes.c_int * k
        out = (ctypes.c_double * (3 * k))()
        _check(self._lib.pccm_reduce_total_many(self._ctx, k, arr(*[int(r[0]) for r in requests]), arr(*[int(r[1]) for r in requests]),
                                                arr(*_modes(normal_mode, k)), out))
        return [(np.float64(out[3 * i]), np.float64(out[3 * i + 1]), np.float64(out[3 * i + 2])) for i in range(k)]

    def _select_args(self, requests, normal_mode):
        k = len(requests)
        arr = ctypes.c_int * k
        return (k, arr(*[int(r[0]) for r in requests]), arr(*[int(r[1]) for r in requests]), arr(*_modes(normal_mode, k)),
                (ctypes.c_int64 * k)(*[int(r[2]) for r in requests]))

    def select_prefetch_many(self, requests, normal_mode: str = "row") -> None:
        """``requests``: up to 8 ``(direction, metric, k)``: enqueue the selection of the k-th smallest element (1-based) of each
        D1 / D2 column without waiting (pccm_select_prefetch_many); a later select_many() consumes them."""
        if requests:
            _check(self._lib.pccm_select_prefetch_many(self._ctx, *self._select_args(requests, normal_mode)))

    def select_many(self, requests, normal_mode: str = "row"):
        """-> the k-th smallest element of each of up to 8 columns ``(direction, metric, k)``, ranked in HBM (pccm_select_many):
        bit for bit ``np.partition(column, k - 1)[k - 1]``."""
        if not requests:
            return []
        args = self._select_args(requests, normal_mode)
        out = (ctypes.c_double * args[0])()
        _check(self._lib.pccm_select_many(self._ctx, *args, out))
        return [np.float64(v) for v in out]

    def _count_args(self, requests, normal_mode):
        k = len(requests)
        arr = ctypes.c_int * k
        return (k, arr(*[int(r[0]) for r in requests]), arr(*[int(r[1]) for r in requests]), arr(*_modes(normal_mode, k)),
                (ctypes.c_double * k)(*[float(r[2]) for r in requests]))

    def count_prefetch_many(self, requests, normal_mode: str = "row") -> None:
        """``requests``: up to 8 ``(direction, metric, x)``: enqueue the count of the rows ``<= x`` of each D1 / D2 column without
        waiting (pccm_count_prefetch_many); a later count_many() consumes them."""
        if requests:
            _check(self._lib.pccm_count_prefetch_many(self._ctx, *self._count_args(requests, normal_mode)))

    def count_many(self, requests, normal_mode: str = "row"):
        """-> the number of rows ``<= x`` of each of up to 8 columns ``(direction, metric, x)``, counted in HBM (pccm_count_many):
        ``np.count_nonzero(column <= x)``."""
        if not requests:
            return []
        args = self._count_args(requests, normal_mode)
        out = (ctypes.c_int64 * args[0])()
        _check(self._lib.pccm_count_many(self._ctx, *args, out))
        return [int(v) for v in out]

    def _map_args(self, requests, normal_mode):
        k = len(requests)
        arr = ctypes.c_int * k
        return (k, arr(*[int(r[0]) for r in requests]), arr(*[int(r[1]) for r in requests]), arr(*_modes(normal_mode, k)),
                arr(*[int(r[2]) for r in requests]), (ctypes.c_double * k)(*[float(r[3]) for r in requests]))

    def reduce_map_prefetch_many(self, requests, normal_mode: str = "row") -> None:
        """``requests``: up to 8 ``(direction, metric, map, x)``: enqueue the reduction of ``f(column)`` for each D1 / D2 column
        without waiting (pccm_reduce_map_prefetch_many; ``map``: MAP_CLAMP -- ``min(value, x)`` -- and / or MAP_ROOT -- then the
        square root); a later reduce_map_total_many() consumes them."""
        if requests:
            _check(self._lib.pccm_reduce_map_prefetch_many(self._ctx, *self._map_args(requests, normal_mode)))

    def reduce_map_total_many(self, requests, normal_mode: str = "row"):
        """-> [(sum, min, max)] of ``f(column)`` for up to 8 ``(direction, metric, map, x)``, mapped and summed in HBM
        (pccm_reduce_map_total_many): bit for bit ``np.sum`` / ``np.min`` / ``np.max`` of ``np.sqrt(np.minimum(column, x))``
        with the steps ``map`` names."""
        if not requests:
            return []
        args = self._map_args(requests, normal_mode)
        out = (ctypes.c_double * (3 * args[0]))()
        _check(self._lib.pccm_reduce_map_total_many(self._ctx, *args, out))
        return [(np.float64(out[3 * i]), np.float64(out[3 * i + 1]), np.float64(out[3 * i + 2])) for i in range(args[0])]

    def match_counts(self, direction: int) -> np.ndarray:
        """How many shard rows of ``direction`` (0 or 1) matched each row of the searched cloud (pccm_match_counts):
        ``np.bincount(idx, minlength=n_searched)`` as uint32, counted on the GPU."""
        out = np.empty(self.n_iter(DIR_RIGHT if int(direction) == DIR_LEFT else DIR_LEFT), dtype=np.uint32)
        _check(self._lib.pccm_match_counts(self._ctx, int(direction), out.ctypes.data_as(ctypes.c_void_p)))
        return out

    @staticmethod
    def _density_args(requests):
        k = len(requests)
        arr = ctypes.c_int * k
        return (k, arr(*[int(r[0]) for r in requests]), arr(*[int(bool(r[2])) for r in requests]),
                (ctypes.c_double * k)(*[float(r[1]) for r in requests]))

    def reduce_density_prefetch_many(self, requests, normal_mode: str = "row") -> None:
        """``requests``: up to 8 ``(direction, alpha, squared)``: enqueue the density-aware Chamfer terms of each direction's D1
        column without waiting (pccm_reduce_density_prefetch_many; the match counts are made first where the search's are not
        there yet); a later reduce_density_total_many() consumes them.  ``normal_mode`` does not enter."""
        if requests:
            _check(self._lib.pccm_reduce_density_prefetch_many(self._ctx, *self._density_args(requests)))

    def reduce_density_total_many(self, requests, normal_mode: str = "row"):
        """-> [(sum, min, max)] of ``1 - exp(-alpha * s) / m[idx]`` for up to 8 ``(direction, alpha, squared)``, s the D1 column
        (``squared``) or its root, m the direction's match counts: gathered, mapped and summed in HBM
        (pccm_reduce_density_total_many)."""
        if not requests:
            return []
        args = self._density_args(requests)
        out = (ctypes.c_double * (3 * args[0]))()
        _check(self._lib.pccm_reduce_density_total_many(self._ctx, *args, out))
        return [(np.float64(out[3 * i]), np.float64(out[3 * i + 1]), np.float64(out[3 * i + 2])) for i in range(args[0])]

    @staticmethod
    def _moment_args(requests, pivot):
        k = len(requests)
        arr = ctypes.c_int * k
        return (k, arr(*[int(r[0]) for r in requests]), arr(*[int(r[1]) for r in requests]),
                (ctypes.c_double * k)(*[float(r[2]) for r in requests]), (ctypes.c_double * 3)(*[float(v) for v in pivot]))

    def reduce_moment_prefetch_many(self, requests, pivot) -> None:
        """``requests``: up to 8 ``(direction, kind, cap)``: enqueue the alignment moments of each direction's D1 column
        relative to ``pivot`` without waiting (pccm_reduce_moment_prefetch_many); a later reduce_moment_total_many() with the
        same pivot consumes them."""
        if requests:
            _check(self._lib.pccm_reduce_moment_prefetch_many(self._ctx, *self._moment_args(requests, pivot)))

    def reduce_moment_total_many(self, requests, pivot):
        """-> [(sum, min, max)] of the alignment moment terms for up to 8 ``(direction, kind, cap)``: with w = (d2 <= cap), u the
        row's point and v its matched point, both minus ``pivot``, kinds 0..2 are u_a, 3..5 v_b, 6 + 3 a + b u_a * v_b and 15
        d2, each ``np.where(w, term, 0.0)``; gathered, multiplied and summed in HBM (pccm_reduce_moment_total_many)."""
        if not requests:
            return []
        args = self._moment_args(requests, pivot)
        out = (ctypes.c_double * (3 * args[0]))()
        _check(self._lib.pccm_reduce_moment_total_many(self._ctx, *args, out))
        return [(np.float64(out[3 * i]), np.float64(out[3 * i + 1]), np.float64(out[3 * i + 2])) for i in range(args[0])]

    def transform_cloud(self, which: int, matrix) -> None:
        """Move resident cloud ``which`` by the 3 x 4 (or 4 x 4, whose last row is not read) matrix ``[A | t]``: points become
        ``A x + t``, per-point normals ``A n``, in fp64 on the GPU (pccm_transform_cloud).  Colours, reflectance and the merge map
        stay; search results that touch the cloud go.  The exact identity is a no-op."""
        m = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64)[:3, :4])
        if m.shape != (3, 4):
            raise ValueError("transform_cloud: a 3 x 4 or 4 x 4 matrix expected")
        _check(self._lib.pccm_transform_cloud(self._ctx, int(which), m.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))

    def get_bounds(self, which: int):
        """-> (lo, hi): the bounding box of cloud ``which`` as its ingest found it (pccm_get_bounds), two float64 triples."""
        lo, hi = (ctypes.c_double * 3)(), (ctypes.c_double * 3)()
        _check(self._lib.pccm_get_bounds(self._ctx, int(which), lo, hi))
        return np.array(lo[:]), np.array(hi[:])

    def reduce_chunks_many(self, requests, normal_mode: str = "row"):
        """-> (one float64 array holding the chunk vectors of up to 8 columns ``(direction, metric)`` one after the other,
        their lengths, [(min, max)] of this shard) -- see pccm_reduce_chunks_many() in include/pccm.h."""
        k = len(requests)
        arr = ctypes.c_int * k
        lens = [cvec_len(self.n_iter(int(r[0]))) for r in requests]
        buf = np.empty(sum(lens), dtype=np.float64)
        mm = (ctypes.c_double * (2 * k))()
        dp = ctypes.POINTER(ctypes.c_double)
        _check(self._lib.pccm_reduce_chunks_many(self._ctx, k, arr(*[int(r[0]) for r in requests]), arr(*[int(r[1]) for r in requests]),
                                                 arr(*([NORMAL_MODES[normal_mode]] * k)), buf.ctypes.data_as(dp), mm))
        return buf, lens, [(mm[2 * i], mm[2 * i + 1]) for i in range(k)]

    finish_chunks = staticmethod(finish_chunks)

    # -- housekeeping -------------------------------------------------------------------------
    def sync(self) -> None:
        _check(self._lib.pccm_sync(self._ctx))

    def drop_caches(self) -> None:
        _check(self._lib.pccm_drop_caches(self._ctx))

    # -- hipGraph capture of {drop_caches, nn, reduce_prefetch}* (see include/pccm.h) ----------------
    def graph_begin(self) -> None:
        _check(self._lib.pccm_graph_begin(self._ctx))

    def graph_end(self) -> int:
        gid = ctypes.c_int(-1)
        _check(self._lib.pccm_graph_end(self._ctx, ctypes.byref(gid)))
        return int(gid.value)

    def graph_abort(self) -> None:
        """Leave capture mode after a captured call failed (the partial graph is discarded)."""
        gid = ctypes.c_int(-1)
        self._lib.pccm_graph_end(self._ctx, ctypes.byref(gid))      # reports the failure; nothing to keep

    def set_tail_filing(self, on: bool) -> None:
        """Inside a capture, before its search: ``False`` keeps the tail launch in this capture whatever the eager step showed
        (every capture starts with filing switched on; pccm_set_tail_filing)."""
        _check(self._lib.pccm_set_tail_filing(self._ctx, int(bool(on))))

    def graph_tail_filed(self, graph_id: int) -> bool:
        """Whether the graph was captured without the tail launch (pccm_set_tail_filing)."""
        filed = ctypes.c_int(0)
        _check(self._lib.pccm_graph_tail_filed(self._ctx, int(graph_id), ctypes.byref(filed)))
        return bool(filed.value)

    def graph_launch(self, graph_id: int) -> None:
        _check(self._lib.pccm_graph_launch(self._ctx, int(graph_id)))

    def graph_destroy(self, graph_id: int) -> None:
        _check(self._lib.pccm_graph_destroy(self._ctx, int(graph_id)))

    def profile(self, on: bool) -> None:
        _check(self._lib.pccm_profile_enable(self._ctx, int(bool(on))))

    def profile_reset(self) -> None:
        _check(self._lib.pccm_profile_reset(self._ctx))

    def profile_get(self, kernel_class: str) -> Tuple[float, int]:
        ms, n = ctypes.c_double(0.0), ctypes.c_int64(0)
        _check(self._lib.pccm_profile_get(self._ctx, KERNEL_CLASSES[kernel_class], ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    def nn_stats(self, direction: int) -> dict:
        out = (ctypes.c_int64 * 3)()
        _check(self._lib.pccm_nn_stats(self._ctx, int(direction), out))
        stats = {"fallback_queries": int(out[0]), "splits": int(out[1]), "pairs": int(out[2])}
        _check(self._lib.pccm_nn_stats(self._ctx, int(direction) | 0x10, out))      # PCCM_STATS_TAIL
        stats["tail_queries"] = int(out[0])
        return stats

    def last_path(self, which: int) -> list:
        """Kernels the last search of direction ``which`` (0, 1, 2) or the last reduction batch (``PATH_REDUCE``) enqueued, in
        launch order, named as ``nm -C`` names their host stubs: ["k_grid_query_coop<false>", "k_grid_tail<pccm::Rec32, false>"]."""
        n = ctypes.c_int64(0)
        _check(self._lib.pccm_nn_path(self._ctx, int(which), None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value + 1)
        _check(self._lib.pccm_nn_path(self._ctx, int(which), buf, n.value + 1, ctypes.byref(n)))
        text = buf.value.decode()
        return text.split(";") if text else []

    def grid_geometry(self):
        """(org, h, dim) of the uniform grid the last grid-engine search ran on (pccm_grid_geometry)."""
        org, h = (ctypes.c_double * 3)(), (ctypes.c_double * 3)()
        dim = np.empty(3, dtype=np.int32)
        _check(self._lib.pccm_grid_geometry(self._ctx, org, h, dim.ctypes.data_as(ctypes.c_void_p)))
        return np.array(org[:]), np.array(h[:]), dim

    def build_plan(self, which: int) -> dict:
        """What structure ``which`` (BUILD_*) was last built as: the fields of PCCM_BP_* by name, ``dim``, ``org`` and ``h``
        (pccm_build_plan).  PccmStateError when the structure is not there."""
        plan = (ctypes.c_int64 * len(_BUILD_PLAN_FIELDS))()
        geom = (ctypes.c_double * 6)()
        _check(self._lib.pccm_build_plan(self._ctx, int(which), plan, geom))
        out = {k: int(v) for k, v in zip(_BUILD_PLAN_FIELDS, plan)}
        out["dim"] = np.array([out["dim0"], out["dim1"], out["dim2"]], dtype=np.int64)
        out["org"] = np.array(geom[0:3], dtype=np.float64)
        out["h"] = np.array(geom[3:6], dtype=np.float64)
        return out

    def build_fetch(self, which: int) -> dict:
        """Structure ``which`` as the build left it (pccm_build_fetch): ``plan``, ``rows`` [n], ``xyz`` [n, 3] in stored order,
        ``cell_start`` [ncells + 1] (None when it has been overwritten) and ``occ`` (the bitmap's words, or None)."""
        plan = self.build_plan(which)
        n, ncells = plan["n"], plan["ncells"]
        rows = np.empty(n, dtype=np.int32)
        xyz = np.empty((n, 3), dtype=np.float64)
        cs = np.empty(ncells + 1, dtype=np.uint32) if plan["has_cs"] else None
        occ = np.empty((ncells + 31) // 32, dtype=np.uint32) if plan["has_occ"] else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        _check(self._lib.pccm_build_fetch(self._ctx, int(which), ptr(cs), ptr(rows), ptr(xyz), ptr(occ)))
        return {"plan": plan, "rows": rows, "xyz": xyz, "cell_start": cs, "occ": occ}

    def tie_scan_queries(self, direction: int) -> int:
        """Queries of the last "mean" search of ``direction`` whose tie set the exact scan enumerated (PCCM_STATS_TIES)."""
        out = (ctypes.c_int64 * 3)()
        _check(self._lib.pccm_nn_stats(self._ctx, int(direction) | 0x20, out))
        return int(out[0])
