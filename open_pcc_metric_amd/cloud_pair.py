"""CloudPair on the GPU -- drop-in for ``open_pcc_metric.cloud_pair.CloudPair``.

Reference: open_pcc_metric/cloud_pair.py:45-124.  Same constructor arguments, same attributes
(``clouds``, ``origin_cloud``, ``reconst_cloud``) and the same ten getters; as in the reference
all nearest-neighbour work happens eagerly in ``__init__`` (cloud_pair.py:54-80).  What the
getters return are *device columns*: array-likes that live in HBM, answer ``np.sum`` /
``np.max`` / ``np.min`` / ``np.square`` with fused GPU reductions (bit-identical to what NumPy
returns on the materialised array) and turn into ordinary ``float64`` ndarrays on
``np.asarray``.  The metric DAG above therefore runs unchanged and never copies an N-sized
array to the host unless a caller asks for one.

Differences from the reference, all deliberate:

* inputs are never mutated (quirk Q5).  A cloud without normals gets them estimated on the GPU the
  first time a point-to-plane metric needs them (k = 30 nearest-neighbour covariance, as Open3D's
  ``estimate_normals`` at cloud_pair.py:61-64 does; not bit-pinned, see csrc/pccm_normals.hip) and
  kept inside the pair; ``estimate_normals=False`` raises ``ValueError`` instead;
* ``normal_index="row"`` (default) reproduces the reference's D2, including its ``IndexError``
  when the iterating cloud is larger than the other one (quirk Q1); ``"neighbour"`` uses the
  matched point's normal;
* exact ties go to the smallest row index (Open3D's order is traversal dependent); ``ties="mean"`` replaces the matched
  point of both directional sweeps by the mean of ALL equidistant nearest points (position, colour and -- with
  ``normal_index="neighbour"`` -- normal; include/pccm.h, PCCM_TIES_MEAN), so that D2 and the colour rows no longer
  depend on the order of the points; D1, Hausdorff D1 and the matched rows are the same under either policy;
* ``extent=`` injects ``get_extent()`` (the minimal-OBB is CPU code and not parity-pinned);
* ``group=`` shards the pair over the ranks of a ``torch.distributed`` group: by direction first (half of the ranks
  search cloud_pair.py:67-72, the other half :73-78, so every rank builds one cloud's search structure), then by
  query rows inside each half (``shard_mode="rows"``: every rank takes rows of both directions, as in round 1);
* ``carry_normals=True`` gives a cloud WITHOUT normals the other cloud's normals instead of estimated ones, the way the MPEG
  evaluation procedure treats a decoded cloud (``pc_error``'s normal carrying; include/pccm.h, pccm_carry_normals): each point
  takes the average of the normals of the other cloud's points whose nearest neighbour it is, or -- nobody's nearest neighbour
  -- its own nearest point's normal.  With normals on both clouds the flag does nothing; with normals on neither, cloud 0's are
  estimated and carried to cloud 1.  Not available sharded or under ``ties="mean"`` (``ValueError``);
* ``duplicates="drop"`` / ``"average"`` (default ``"keep"``: nothing changes) merges, on the GPU and before any search, the points
  of each cloud that share their coordinates, as MPEG's ``pc_error`` does with both clouds (dropDuplicates; include/pccm.h,
  pccm_merge_duplicates): one point per position in the order of first appearance, with the first point's normal and the first
  point's colour (``"drop"``) or the group's average colour (``"average"``, pc_error's default).  Every row count, column and
  report then belongs to the merged clouds; ``clouds`` stays the caller's objects, ``duplicates_removed`` says how many rows each
  cloud lost and ``merge_map(which)`` where each original row went.  ``get_extent()`` still measures the given cloud 0: a convex
  hull does not depend on multiplicities.  Not available sharded (``ValueError``);
* a cloud may carry a ``reflectance`` (one scalar per point; ``getattr(cloud, "reflectance", None)``, so Open3D clouds, which have
  none, keep working): it goes up the first time a reflectance row needs it, stays with the origin cloud across
  ``with_reconst`` and is merged by ``duplicates=`` like the colours ("Reflectance").  The rows are not
  available sharded or under ``ties="mean"`` (``ValueError``);
* ``use_graph=True`` lets ``recompute()`` replay the whole sweep + reductions of the previous report
  as one hipGraph launch (for callers that evaluate the same resident pair repeatedly).
"""
from __future__ import annotations

import math
import numbers
import os
import typing

import numpy as np

from . import _native as nat
from .collective import Collective
from .extent import minimal_obb_extent

_REDUCERS = {np.sum: "sum", np.max: "max", np.min: "min", np.amax: "max", np.amin: "min"}


def _plain(x):
    return np.asarray(x) if isinstance(x, _DeviceArray) else x


class _DeviceArray(np.lib.mixins.NDArrayOperatorsMixin):
    """Common array-like plumbing; anything not fused falls back to the materialised ndarray."""
    dtype = np.dtype(np.float64)
    _host: typing.Optional[np.ndarray] = None

    def __array__(self, dtype=None, copy=None):
        if self._host is None:
            self._host = self._materialise()
            self._host.setflags(write=False)
        return self._host if dtype is None else self._host.astype(dtype)

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        fused = self._fused_ufunc(ufunc, method, inputs, kwargs)
        if fused is not NotImplemented:
            return fused
        if "out" in kwargs:
            kwargs["out"] = tuple(_plain(o) for o in kwargs["out"])
        return getattr(ufunc, method)(*[_plain(i) for i in inputs], **kwargs)

    def __array_function__(self, func, types, args, kwargs):
        fused = self._fused_function(func, args, kwargs)
        if fused is not NotImplemented:
            return fused
        return func(*[_plain(a) for a in args], **{k: _plain(v) for k, v in kwargs.items()})

    def _fused_ufunc(self, ufunc, method, inputs, kwargs):
        return NotImplemented

    def _fused_function(self, func, args, kwargs):
        return NotImplemented

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def size(self):
        return int(np.prod(self.shape))

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, key):
        return np.asarray(self)[key]

    def __iter__(self):
        return iter(np.asarray(self))

    def astype(self, dtype, **kw):
        return np.asarray(self).astype(dtype, **kw)

    def tolist(self):
        return np.asarray(self).tolist()

    def __repr__(self):
        return f"<{type(self).__name__} {self._label} shape={self.shape} on GPU>"


class DeviceColumn(_DeviceArray):
    """A per-point float64 column of one direction: ``kind`` is

    ``"d1"``        squared NN distances (NeighbourDistances / D1 EuclideanDistance),
    ``"proj"``      signed point-to-plane projections (ErrorVector, point_to_plane=True),
    ``"d2"``        their squares (D2 EuclideanDistance),
    ``"boundary"``  sqrt of the self-search distances (get_boundary_sqrt_distances),
    ``"angular"``   plane-to-plane angular similarities (get_left/right_angular_similarities; include/pccm.h,
                    PCCM_METRIC_ANGULAR: the own normal against the matched point's, ``normal_index`` does not apply),
    ``"ssim:<attribute>"``  PointSSIM similarities of one attribute (get_left/right_ssim_similarities; PCCM_METRIC_SSIM_*: the
                    own feature against the matched point's, at the neighbourhood size the pair's features were built with),
    ``"p2d"``       point-to-distribution (Mahalanobis) distances (get_left/right_mahalanobis_distances; PCCM_METRIC_P2D: the
                    direction's stored column, at the neighbourhood size the pair's columns were built with),
    ``"p2d_color"`` / ``"p2d_joint"``  its colour and joint columns (get_left/right_color_mahalanobis_distances,
                    get_left/right_joint_mahalanobis_distances; PCCM_METRIC_P2D_COLOR / PCCM_METRIC_P2D_JOINT),
    ``"spacing"``   the point spacings of the cloud the direction iterates (get_left/right_point_spacings;
                    PCCM_METRIC_RESOLUTION: that cloud's stored column, over the neighbours it was built with),
    ``"reflectance"``  squared reflectance differences (get_left/right_reflectance_errors; PCCM_METRIC_REFLECTANCE: the own
                    reflectance against the matched point's, values as given).
    """

    def __init__(self, pair: "CloudPair", direction: int, kind: str):
        self._pair, self._dir, self._kind = pair, direction, kind
        self.shape = (pair._engine.n_iter(direction),)
        self._label = f"{kind}[dir={direction}]"
        self._red = None

    _METRIC = {"d1": nat.METRIC_D1, "boundary": nat.METRIC_D1, "proj": nat.METRIC_PROJ, "d2": nat.METRIC_D2,
               "angular": nat.METRIC_ANGULAR, **{f"ssim:{a}": m for a, m in nat.METRIC_SSIM.items()}, "p2d": nat.METRIC_P2D,
               "p2d_color": nat.METRIC_P2D_COLOR, "p2d_joint": nat.METRIC_P2D_JOINT, "spacing": nat.METRIC_RESOLUTION,
               "reflectance": nat.METRIC_REFLECTANCE}

    def _materialise(self) -> np.ndarray:
        p = self._pair
        if self._kind in ("d1", "boundary"):
            _, col = p._engine.fetch_nn(self._dir, want_idx=False)
        else:
            col = p._engine.point_metric(self._dir, self._METRIC[self._kind], p.normal_index)
        col = p._gather(self._dir, col)
        return np.sqrt(col) if self._kind == "boundary" else col

    def _reduced(self):
        """(sum, min, max) of the whole column: fused on the GPU, exchanged across ranks."""
        if self._red is None:
            p = self._pair
            if p._fast_totals:                            # unsharded, engine with pccm_reduce_total: the usual case
                total, mn, mx = p._total(self._dir, self._METRIC[self._kind])
            elif p._coll.sharded:
                total, mn, mx = p._sharded_reduction(self._dir, self._METRIC[self._kind])
            else:
                xvec, mn, mx = p._engine.reduce(self._dir, self._METRIC[self._kind], p.normal_index)
                total = p._engine.finish_sum(xvec, self.shape[0])
            if self._kind == "boundary":          # sqrt is monotonic: min/max commute with it
                mn, mx, total = np.sqrt(mn), np.sqrt(mx), None
            self._red = (total, np.float64(mn), np.float64(mx))
        return self._red

    def ranked(self, k: int):
        """The k-th smallest element (1-based) of the column: ``np.partition(column, k - 1)[k - 1]``, selected in HBM when the
        engine can (pccm_select_many: D1 and D2 columns) -- no column leaves the GPU then."""
        k = int(k)
        if not 1 <= k <= self.shape[0]:
            raise ValueError(f"rank {k} outside 1..{self.shape[0]}")
        if self._kind in ("d1", "d2"):
            value = self._pair._selected(self._dir, self._METRIC[self._kind], k)
            if value is not None:
                return value
        return np.partition(np.asarray(self), k - 1)[k - 1]

    def count_le(self, x) -> int:
        """The number of elements ``<= x``: ``np.count_nonzero(column <= x)``, counted in HBM when the engine can
        (pccm_count_many: D1 and D2 columns) -- no column leaves the GPU then."""
        x = float(x)
        if x != x:
            raise ValueError("count_le: the threshold is NaN")
        if self._kind in ("d1", "d2"):
            value = self._pair._counted(self._dir, self._METRIC[self._kind], x)
            if value is not None:
                return value
        return int(np.count_nonzero(np.asarray(self) <= x))

    def mapped(self, root: bool = False, clamp=None):
        """``(sum, min, max)`` of ``f(column)``, f = the clamp ``np.minimum(column, clamp)`` (when ``clamp`` is given), then the
        root ``np.sqrt`` (when ``root``): mapped and summed in HBM when the engine can (pccm_reduce_map_total_many: D1 and D2
        columns) -- neither the column nor f(column) leaves the GPU or is stored there.  Bit for bit NumPy on the column."""
        if clamp is not None:
            clamp = float(clamp)
            if clamp != clamp:
                raise ValueError("mapped: the clamp is NaN")
        if not root and clamp is None:
            return self._reduced()
        if self._kind in ("d1", "d2"):
            which = (nat.MAP_CLAMP if clamp is not None else 0) | (nat.MAP_ROOT if root else 0)
            value = self._pair._mapped(self._dir, self._METRIC[self._kind], which, 0.0 if clamp is None else clamp)
            if value is not None:
                return value
        return mapped_on_host(np.asarray(self), root, clamp)

    def density(self, alpha, squared: bool = False):
        """``(sum, min, max)`` of the density-aware Chamfer terms ``1 - exp(-alpha * s) / m[idx]`` of a ``d1`` column: s the
        column (``squared``) or its root, idx the direction's matched rows, m how many rows matched each row of the searched
        cloud (CloudPair.match_counts).  Counted, gathered, mapped and summed in HBM when the engine can
        (pccm_reduce_density_total_many) -- neither the column, the rows nor the terms leave the GPU or are stored there."""
        alpha = float(alpha)
        if not (alpha >= 0.0) or alpha == float("inf"):
            raise ValueError("density: alpha is a finite number >= 0")
        if self._kind != "d1" or self._dir not in (nat.DIR_LEFT, nat.DIR_RIGHT):
            raise ValueError("density: defined on the d1 columns of the two directions")
        value = self._pair._density(self._dir, alpha + 0.0, bool(squared))
        if value is not None:
            return value
        pair = self._pair
        rows = pair._neighbour_index(self._dir)
        counts = np.bincount(rows, minlength=pair._engine.n_iter(nat.DIR_RIGHT if self._dir == nat.DIR_LEFT else nat.DIR_LEFT))
        return density_on_host(np.asarray(self), rows, counts, alpha, squared)

    def _fused_function(self, func, args, kwargs):
        which = _REDUCERS.get(func)
        if which is None or len(args) != 1 or args[0] is not self:
            return NotImplemented
        if set(kwargs) - {"axis"} or kwargs.get("axis", None) not in (None, 0):
            return NotImplemented
        total, mn, mx = self._reduced()
        if which == "sum":
            return NotImplemented if total is None else total
        return mx if which == "max" else mn

    def _fused_ufunc(self, ufunc, method, inputs, kwargs):
        if ufunc is np.square and method == "__call__" and not kwargs and self._kind == "proj":
            return DeviceColumn(self._pair, self._dir, "d2")     # metric.py:179 stays on the GPU
        return NotImplemented


def mapped_on_host(column, root: bool = False, clamp=None):
    """What DeviceColumn.mapped answers, for a column that is a plain array."""
    f = np.asarray(column, dtype=np.float64)
    if clamp is not None:
        f = np.minimum(f, np.float64(clamp))
    if root:
        f = np.sqrt(f)
    return np.sum(f), np.min(f), np.max(f)


def density_on_host(column, rows, counts, alpha, squared: bool = False):
    """What DeviceColumn.density answers, for a column, matched rows and match counts that are plain arrays."""
    d2 = np.asarray(column, dtype=np.float64)
    s = d2 if squared else np.sqrt(d2)
    m = np.asarray(counts)[np.asarray(rows)].astype(np.float64)
    t = 1.0 - np.exp(-np.float64(alpha) * s) / m
    return np.sum(t), np.min(t), np.max(t)


class DeviceFeatures(_DeviceArray):
    """One cloud's PointSSIM feature column of one attribute (get_ssim_features), copied from HBM when asked for."""

    def __init__(self, pair: "CloudPair", which: int, attribute: str):
        self._pair, self._which, self._attribute = pair, which, attribute
        self.shape = (pair._engine.n_iter(nat.DIR_LEFT if which == 0 else nat.DIR_RIGHT),)
        self._label = f"ssim features[{attribute}, cloud {which}]"

    def _materialise(self) -> np.ndarray:
        return self._pair._engine.get_ssim_features(self._which, self._attribute)


class DeviceRows(_DeviceArray):
    """(N, 3) error vectors ``iter[i] - search[nn(i)]`` of one direction (cloud_pair.py:90-100)."""

    def __init__(self, pair: "CloudPair", direction: int):
        self._pair, self._dir = pair, direction
        self.shape = (pair._engine.n_iter(direction), 3)
        self._label = f"error_vector[dir={direction}]"

    def _materialise(self) -> np.ndarray:
        return self._pair._gather(self._dir, self._pair._engine.error_vectors(self._dir))


class DeviceColorRows(_DeviceArray):
    """(N, 3) colour rows of one direction, kept in HBM (metric.py:302-333, 389-427).

    ``what``: ``"neighbour"`` -- colours of the matched points, ``np.take(colors, idx, axis=0)`` of
    cloud_pair.py:120-124;  ``"diff"`` -- ``scale * (T(own) - T(neighbour))`` in ``scheme``;
    ``"square"`` -- its square.  ``np.mean(square, axis=0)`` and ``np.max(square, axis=0)`` are answered
    by pccm_color_reduce (bit-identical to NumPy on the materialised rows); ``255 * diff``,
    ``diff ** 2`` and ``np.square(diff)`` stay on the device; anything else materialises."""
    _WHAT = {"neighbour": nat.COLOR_NEIGHBOUR, "diff": nat.COLOR_DIFF, "square": nat.COLOR_SQUARE}

    def __init__(self, pair: "CloudPair", direction: int, what: str, scheme: str = "rgb", scale: float = 1.0):
        self._pair, self._dir, self._what, self._scheme, self._scale = pair, direction, what, scheme, float(scale)
        self.shape = (pair._engine.n_iter(direction), 3)
        self._label = f"colour {what}[dir={direction}, {scheme}, x{self._scale:g}]"

    def in_scheme(self, scheme: str) -> "DeviceColorRows":
        """own - neighbour in ``scheme`` (the np.subtract of metric.py:326-329 / 417-420)."""
        return DeviceColorRows(self._pair, self._dir, "diff", scheme)

    def _materialise(self) -> np.ndarray:
        p = self._pair
        return p._engine.color_rows(self._dir, self._scheme, self._WHAT[self._what], self._scale, p._colour_rows_arg(self._dir))

    def _fused_ufunc(self, ufunc, method, inputs, kwargs):
        if method != "__call__" or kwargs or self._what != "diff":
            return NotImplemented
        if ufunc is np.square and inputs[0] is self:
            return DeviceColorRows(self._pair, self._dir, "square", self._scheme, self._scale)
        if ufunc is np.power and inputs[0] is self and np.isscalar(inputs[1]) and inputs[1] == 2:
            return DeviceColorRows(self._pair, self._dir, "square", self._scheme, self._scale)
        if ufunc is np.multiply and len(inputs) == 2 and self._scale == 1.0:
            other = inputs[1] if inputs[0] is self else inputs[0]
            if np.isscalar(other) and not isinstance(other, (bool, np.bool_)):
                return DeviceColorRows(self._pair, self._dir, "diff", self._scheme, float(other))
        return NotImplemented

    def _fused_function(self, func, args, kwargs):
        if self._what != "square" or len(args) != 1 or args[0] is not self or set(kwargs) != {"axis"} or kwargs["axis"] != 0:
            return NotImplemented
        if func is np.mean:
            sums, _ = self._pair._colour_reduction(self._dir, self._scheme, self._scale)
            return sums / self.shape[0]                        # np.mean = np.add.reduce(axis=0) / N
        if func in (np.max, np.amax):
            return self._pair._colour_reduction(self._dir, self._scheme, self._scale)[1]
        return NotImplemented


class CloudColorsView(np.ndarray):
    """``np.asarray(cloud.colors)`` that remembers which cloud of which pair it came from."""
    _pccm_origin: typing.Optional[tuple] = None

    def __array_finalize__(self, obj):
        self._pccm_origin = None


class CloudNormalsView(np.ndarray):
    """``np.asarray(cloud.normals)`` that remembers which cloud of which pair it came from, so that
    ErrorVector can keep the projection on the GPU (metric.py:92-98, 146-153)."""
    _pccm_origin: typing.Optional[tuple] = None

    def __array_finalize__(self, obj):
        self._pccm_origin = None      # any derived array is just data


class CloudPair:
    clouds: typing.Tuple[typing.Any, typing.Any]

    def __init__(self, origin_cloud, reconst_cloud, *, device: typing.Optional[int] = None,
                 nn_engine: str = "auto", normal_index: str = "row", extent=None, group=None,
                 use_graph: bool = False, estimate_normals: bool = True, normals_knn: int = 30,
                 shard_mode: str = "direction", _engine=None, _uploads_first: bool = False,
                 staged_io: typing.Optional[bool] = None, ties: str = "pick", carry_normals: bool = False,
                 duplicates: str = "keep", transform=None, align: typing.Optional[str] = None, align_distance=None,
                 align_iterations: int = 30, align_tolerance: float = 1e-6):
        if normal_index not in nat.NORMAL_MODES:
            raise ValueError("normal_index must be 'row' or 'neighbour'")
        if not isinstance(ties, str) or ties not in nat.TIES:
            raise ValueError("ties must be 'pick' or 'mean'")
        if nn_engine not in nat.ENGINES:
            raise ValueError(f"nn_engine must be one of {sorted(nat.ENGINES)}")
        from .options import check_carry_normals, check_duplicates
        check_carry_normals(carry_normals, ties=ties, group=group)       # (ValueError before any GPU work)
        check_duplicates(duplicates, group=group)
        from .align import check_align
        # (transform 4 x 4 or None, "icp" or None, squared distance, iterations, tolerance) -- with_reconst hands them on
        self._align = check_align(align, align_distance, align_iterations, align_tolerance, transform=transform, group=group)
        self.alignment = None                   # align.Alignment once cloud 1 has been moved
        self._moved = [False, False]            # the cloud was moved on the device (transform=, align=): its normals are the engine's
        self.clouds = (origin_cloud, reconst_cloud)
        self.normal_index = normal_index
        self.nn_engine = nn_engine
        self.ties = ties
        self._use_graph = bool(use_graph) and ties == "pick"        # (searches under "mean" are not captured: pccm_set_ties)
        self._estimate_normals, self._normals_knn = bool(estimate_normals), int(normals_knn)
        self._estimated = [False, False]
        self._carry_normals = bool(carry_normals)
        self._carried = [False, False]          # the cloud's normals were carried over from the other cloud (pccm_carry_normals)
        self._duplicates = duplicates
        self._merged = [False, False]           # the cloud lost rows to pccm_merge_duplicates: its arrays are the engine's, not the caller's
        self.duplicates_removed = (0, 0)
        self._drop_results(plan=True)
        # why the searches keep the matched rows (_keep_matched_rows): "carry" (the carry reads them), and the columns a report has asked
        # for that compare a point with its matched point ("angular", "ssim", "reflectance") or count who shares one ("density")
        self._keep_rows = {"carry"} if self._carry_normals else set()
        self._colours_on_device = [False, False]
        self._reflectance_on_device = [False, False]
        self._graph_id = None
        self._last_wanted = None
        self._extent = None if extent is None else np.asarray(extent, dtype=np.float64)
        self._coll = Collective(group)
        self._owns_engine = False
        if _engine is None:
            if device is None:
                device = int(os.environ.get("LOCAL_RANK", "0")) if self._coll.sharded else 0
            _engine = nat.acquire_engine(device)  # raises without libpccm.so or without a GPU; pooled contexts are reused
            self._owns_engine = True
            self._coll.device = device            # the nccl exchange is staged on the same GPU
        self._engine = _engine
        if self._carry_normals and not hasattr(_engine, "carry_normals"):
            raise ValueError("this engine cannot carry normals from one cloud to the other")
        if duplicates != "keep" and not hasattr(_engine, "merge_duplicates"):
            raise ValueError("this engine cannot merge duplicate points")
        if (self._align[0] is not None or self._align[1] is not None) and not hasattr(_engine, "transform_cloud"):
            raise ValueError("this engine cannot move a cloud")
        if hasattr(_engine, "set_ties"):
            _engine.set_ties(ties)                # (every time: a pooled context comes back with the default, pccm_ctx_reset)
        elif ties != "pick":
            raise ValueError("this engine has no tie policy other than 'pick'")
        # ``staged_io``: the clouds' arrays will be FREED while this context is still in use (a sequence of pairs read from files):
        # their bytes then go through the context's own pinned buffers instead of being handed to the HIP runtime, which pins
        # the caller's pages and keeps the mapping -- and whose tear-down, when such an array is freed, stops every GPU queue of
        # the process for 13-27 ms (pccm_set_io_staged).  None: direct for a context's first pair, staged from its second on.
        # A pooled context that has served a pair before means a LOOP over pairs -- whose clouds are normally read, used and
        # freed one after the other -- and takes the staged path unless told otherwise (a loop over fresh 1M-point pairs: 2.2-5 ms
        # per pair staged; direct, every second pair stands still for 30 ms).
        if staged_io is None and self._owns_engine and getattr(_engine, "pairs_served", 0) >= 1:
            staged_io = True
        if staged_io is not None and hasattr(_engine, "set_io_staged"):
            _engine.set_io_staged(bool(staged_io))
        self._fast_totals = not self._coll.sharded and hasattr(_engine, "reduce_total")   # whole columns finished by one call
        # Points first; normals are announced and cross PCIe behind the searches, which do not read them (the reference's
        # constructor orders nothing between the two: cloud_pair.py:61-80) -- see the flush at the end
        deferred = hasattr(_engine, "set_normals_deferred")
        for k, cloud in enumerate(self.clouds):
            _engine.set_cloud(k, cloud.points)
            if duplicates != "keep":
                self._merge_duplicates(k)                 # (its normals and colours go up now: the merge takes them along)
            elif _has_normals(cloud):
                (_engine.set_normals_deferred if deferred else _engine.set_normals)(k, cloud.normals)
        if shard_mode not in ("direction", "rows"):
            raise ValueError("shard_mode must be 'direction' or 'rows'")
        self._plan = shard_plan(self._coll.world, shard_mode if hasattr(_engine, "set_shard_dir") else "rows")
        if self._coll.sharded:
            if hasattr(_engine, "set_shard_dir"):
                for direction in (nat.DIR_LEFT, nat.DIR_RIGHT, nat.DIR_SELF):
                    _engine.set_shard_dir(direction, *self._plan[direction][self._coll.rank])
            else:
                _engine.set_shard(self._coll.rank, self._coll.world)
        self._move_reconst()
        self._update_fusion()
        if deferred and _uploads_first:
            _engine.flush_uploads()                       # (A/B for bench.py: everything uploaded before the first search starts)
        self._colours_for_ties()
        self.recompute()
        if deferred:
            _engine.flush_uploads()                       # (the searches are running: the normals' upload runs beside them)

    def with_reconst(self, reconst_cloud) -> "CloudPair":
        """The pair of THIS pair's origin cloud and another reconstructed cloud -- one reference against several decoded
        versions (BASELINE.json configs[4]; the reference runs its command line once per version, handler.py:57-66, and
        repeats everything).  What belongs to the origin cloud alone is kept: its points, normals (given or estimated,
        cloud_pair.py:61-64) and colours in HBM, its spatial order, ``get_extent()`` (cloud_pair.py:111-112) and the self
        search behind ``get_boundary_sqrt_distances()`` (cloud_pair.py:108-109); only the new cloud is uploaded and the two
        directional searches run.  The GPU context moves to the new pair: this one is closed.  Rows are the same, bit for
        bit, as those of a fresh ``CloudPair(origin_cloud, reconst_cloud)``."""
        eng = self.__dict__.get("_engine")
        if eng is None:
            raise RuntimeError("this CloudPair has been closed")
        if self._coll.sharded or not hasattr(eng, "nn_pair"):
            # (a sharded pair keeps nothing that pays: every rank would have to agree on what is resident)
            kw = dict(nn_engine=self.nn_engine, normal_index=self.normal_index, extent=self._extent, use_graph=self._use_graph,
                      estimate_normals=self._estimate_normals, normals_knn=self._normals_knn, ties=self.ties,
                      carry_normals=self._carry_normals, duplicates=self._duplicates, **self._align_kwargs())
            group, owns = self._coll.group, self._owns_engine
            self.__dict__.pop("_engine")
            if owns:
                nat.release_engine(eng)
                return CloudPair(self.clouds[0], reconst_cloud, group=group, **kw)
            return CloudPair(self.clouds[0], reconst_cloud, group=group, _engine=eng, **kw)
        new = object.__new__(CloudPair)
        new.__dict__.update({k: v for k, v in self.__dict__.items() if k != "_engine"})
        new.clouds = (self.clouds[0], reconst_cloud)
        new._estimated = [self._estimated[0], False]
        new._carried = [False, False]                    # (cloud 0's, if carried, came from the cloud that is leaving: the library
        #                                                   drops them with it, and the next consumer carries from the new one)
        new._colours_on_device = [self._colours_on_device[0], False]
        new._reflectance_on_device = [self._reflectance_on_device[0], False]     # (the origin cloud's column stays in HBM)
        new._moved, new.alignment = [False, False], None # (only cloud 1 ever moves; the new one is moved itself: _move_reconst)
        new._merged = [self._merged[0], False]           # (cloud 0 stays merged and resident: only the new cloud 1 is merged)
        new.duplicates_removed = (self.duplicates_removed[0], 0)
        new._keep_rows = set(self._keep_rows)
        new._drop_results(plan=True)
        new._graph_id, new._last_wanted = None, None
        keep_self = bool(self.__dict__.get("_self_done")) and bool(getattr(eng, "keeps_self_search", False))
        self_total = self.__dict__.get("_totals", {}).get((nat.DIR_SELF, nat.METRIC_D1)) if keep_self else None
        self.__dict__.pop("_engine")                     # moved: this pair is closed, the context is not handed back
        self._owns_engine = False
        new._engine = eng
        if hasattr(eng, "set_io_staged"):
            eng.set_io_staged(True)                              # (the superseded cloud is about to be freed by its owner: see __init__)
        eng.set_cloud(1, reconst_cloud.points)               # (the library keeps cloud 0, everything it owns and its self search)
        deferred = hasattr(eng, "set_normals_deferred")
        if new._duplicates != "keep":
            new._merge_duplicates(1)
        elif _has_normals(reconst_cloud):
            (eng.set_normals_deferred if deferred else eng.set_normals)(1, reconst_cloud.normals)
        new._move_reconst()
        new._update_fusion()
        new._colours_for_ties()
        new.recompute()
        if deferred:
            eng.flush_uploads()
        new._self_done = keep_self
        if self_total is not None:
            new._totals[(nat.DIR_SELF, nat.METRIC_D1)] = self_total
        return new

    def close(self) -> None:
        """Hand the GPU context back (it is reused by the next pair); the pair must not be used afterwards."""
        eng = self.__dict__.pop("_engine", None)
        if eng is not None and self.__dict__.get("_owns_engine"):
            nat.release_engine(eng)

    def __del__(self):
        try:
            self.close()
        except Exception:            # noqa: BLE001 -- interpreter shutdown
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _align_kwargs(self) -> dict:
        """The alignment settings as the constructor takes them."""
        transform, align, tau2, iterations, tolerance = self._align
        return dict(transform=transform, align=align, align_distance=None if math.isinf(tau2) else math.sqrt(tau2),
                    align_iterations=iterations, align_tolerance=tolerance)

    def _move_reconst(self) -> None:
        """``transform=`` and ``align=``: move resident cloud 1 -- after the uploads and the merge of duplicates, before normals
        are estimated or carried and before the pair's searches (align.py).  Without either nothing is called."""
        transform, align, tau2, iterations, tolerance = self._align
        if transform is None and align is None:
            return
        from . import align as al
        eng = self._engine
        if transform is not None:
            eng.transform_cloud(1, transform)
        result = al.Alignment(np.eye(4) if transform is None else transform.copy(), 0, None, None, False)
        if align is not None:
            if self.__dict__.get("_align_pivot") is None:             # (the original never moves: with_reconst keeps it)
                # (the ingest has the box already; np.min over a million rows on the host costs more than the whole alignment)
                self._align_pivot = (al.centre_of(*eng.get_bounds(0)) if hasattr(eng, "get_bounds")
                                     else al.bounding_box_centre(_host_rows(self.clouds[0].points)))
            if self.ties != "pick" and hasattr(eng, "set_ties"):
                eng.set_ties("pick")                                  # (alignment always matches under "pick")
            if hasattr(eng, "nn_want_idx"):
                eng.nn_want_idx(True)                                 # (the moments read the matched rows; _update_fusion follows)
            try:
                result = al.icp(eng, eng.n_iter(nat.DIR_RIGHT), self._align_pivot, tau2, iterations, tolerance,
                                nn_engine=self.nn_engine, start=result.transformation)
            finally:
                if self.ties != "pick" and hasattr(eng, "set_ties"):
                    eng.set_ties(self.ties)
        self.alignment = result
        self._moved[1] = True
        self._occupancy = {}            # (the voxels were counted where the cloud stood: whoever moves resident points drops them)

    def _merge_duplicates(self, which: int) -> None:
        """``duplicates="drop" | "average"``: the cloud's normals and colours go up now, then its rows that share their coordinates
        are merged on the device (pccm_merge_duplicates); every size comes from the engine afterwards."""
        eng, cloud = self._engine, self.clouds[which]
        before = eng.n_iter(nat.DIR_RIGHT if which else nat.DIR_LEFT)
        if _has_normals(cloud):
            eng.set_normals(which, cloud.normals)
        if _has_colors(cloud):
            self._upload_colours(which)
        if _has_reflectance(cloud) and hasattr(eng, "set_reflectance"):
            self._upload_reflectance(which)
        after = eng.merge_duplicates(which, self._duplicates)
        self._merged[which] = after < before
        self._occupancy = {}            # (new rows; the counts would come out the same, but they are the old rows')
        removed = list(self.duplicates_removed)
        removed[which] = before - after
        self.duplicates_removed = tuple(removed)

    def merge_map(self, which: int) -> np.ndarray:
        """For every row of the given cloud ``which``, its row in the merged cloud the pair works on (``duplicates=``); the
        identity when nothing was merged."""
        return self._engine.get_merge_map(which).astype(np.int64)

    def _update_fusion(self) -> None:
        """Let the searches leave the D2 projection next to the distance (pccm_nn_fuse) for every direction whose
        *other* cloud has normals: a report then needs no second pass over the points (metric.py:146-153 fused into
        cloud_pair.py:67-78).  Purely an optimisation; the library ignores what it cannot honour."""
        eng = self._engine
        if not hasattr(eng, "nn_fuse"):
            return
        # (under "mean" the fused projection would be the pick's: the virtual neighbours are formed from the matched rows instead)
        mean = getattr(self, "ties", "pick") == "mean"
        for direction, other in ((nat.DIR_LEFT, 1), (nat.DIR_RIGHT, 0)):
            eng.nn_fuse(direction, self.normal_index if self._normals_ready(other) and not mean else None)
        # the matched rows (cloud_pair.py:34-42) are only read by the colour metrics and the error-vector / neighbour
        # getters: clouds without colours leave them out of the result records (a getter that asks later still gets them)
        # (and so do the columns and passes named in _keep_rows)
        if hasattr(eng, "nn_want_idx"):
            eng.nn_want_idx(mean or bool(self.__dict__.get("_keep_rows")) or any(_has_colors(c) for c in self.clouds))

    def _keep_matched_rows(self, reason: str) -> None:
        """From now on the searches keep the matched rows, for ``reason`` (one of those listed in __init__); the rows of the search
        that has already run are recovered once."""
        if reason not in self._keep_rows:
            self._keep_rows.add(reason)
            self._update_fusion()

    def _drop_results(self, plan: bool = False) -> None:
        """Forget every result read back from the GPU -- new searches are about to run -- and, with ``plan``, which results the last
        report enqueued (the batches they come back in): a new pair."""
        self._idx_cache, self._xchg, self._totals, self._colour_red = {}, {}, {}, {}
        if plan:
            self._xchg_wanted = []
            self._occupancy = {}        # voxel size -> (nA, nB, nAB) of the resident points: kept across recompute(), which searches
            #                             the same points again; dropped by everything that changes them (a new pair here,
            #                             _merge_duplicates, _move_reconst)
        # per row family of _FAMILIES: (the answers by request, the requests the last report enqueued in sorted order)
        self._results = {tag: ({}, [] if plan else self._results[tag][1]) for tag in _FAMILIES}

    def _drop_totals(self, metrics) -> None:
        """Forget the totals of the columns of ``metrics``: what they were reduced from has been built again or replaced."""
        self._totals = {key: v for key, v in self._totals.items() if key[1] not in metrics}

    def _colours_for_ties(self) -> None:
        """Under ``ties="mean"`` the colours go up before the searches, so that the one averaging pass per direction (pccm_set_ties)
        averages them together with the positions and normals instead of walking the tie sets once more for the colour rows."""
        if self.ties == "mean" and all(_has_colors(c) for c in self.clouds) and hasattr(self._engine, "set_colors"):
            self._ensure_colours()

    def recompute(self) -> None:
        """Run both directional sweeps again on the clouds already resident in HBM
        (cloud_pair.py:67-78 does this once, eagerly, in the constructor) and drop cached results."""
        eng = self._engine
        self._drop_results()
        if self._use_graph and self._last_wanted is not None and hasattr(eng, "graph_begin"):
            wants_self = "boundary" in self._last_wanted
            if self._graph_id is not None:
                try:
                    eng.graph_launch(self._graph_id)          # sweeps + the last report's reductions, one launch
                    self._self_done = wants_self
                    return
                except nat.PccmStateError:
                    self._graph_id = None                     # stale (buffers changed): run eagerly, capture again later
                # anything else -- a HIP failure during the replay in particular -- is not retried and not hidden
            else:
                try:
                    eng.graph_begin()
                    self._enqueue_sweeps()
                    self._self_done = False
                    self.prefetch_reductions(self._last_wanted, _remember=False)
                    self._graph_id = eng.graph_end()
                    self._self_done = wants_self
                    return
                except (nat.PccmStateError, ValueError, IndexError):
                    eng.graph_abort()                         # leave capture mode; results were invalidated
                    self._graph_id = None
                    self._use_graph = False                   # capture not possible here: stay eager
                except BaseException:
                    eng.graph_abort()                         # leave capture mode, then let the failure surface
                    self._graph_id = None
                    raise
        self._enqueue_sweeps()
        self._self_done = False

    def _enqueue_sweeps(self) -> None:
        eng = self._engine
        if hasattr(eng, "drop_caches"):
            eng.drop_caches()                                 # search structures are rebuilt, like the KD-trees
        if hasattr(eng, "nn_pair"):
            eng.nn_pair(self.nn_engine)                       # cloud_pair.py:67-78, both directions fused
        else:
            eng.nn(nat.DIR_LEFT, self.nn_engine)
            eng.nn(nat.DIR_RIGHT, self.nn_engine)

    # -- helpers ------------------------------------------------------------------------------
    def _gather(self, direction: int, local: np.ndarray) -> np.ndarray:
        if not self._coll.sharded:
            return local
        n = self._engine.n_iter(direction)
        counts = [_shard_bounds(n, *self._plan[direction][r]) for r in range(self._coll.world)]
        return self._coll.allgather_rows(local, [e - b for b, e in counts])

    def _sharded_reduction(self, direction: int, metric: int):
        """(sum, min, max) of a whole column when the query axis is sharded.

        The exchange vectors of ALL columns the current report asked for (prefetch_reductions) and their
        extrema travel in ONE all-reduce(SUM) per report, however many columns it has.  Every rank calls
        this with the same requests in the same order."""
        key = (direction, metric)
        if key not in self._xchg:
            eng, coll = self._engine, self._coll
            batch = [k for k in self._xchg_wanted if k not in self._xchg]
            if key not in batch:
                batch.append(key)
            parts, ext = [], []
            # shards that start and end on whole 8192-row chunks (every direction of the batch, decided from the row
            # counts and the plan alone: the same answer on every rank) exchange one number per chunk instead of one per
            # 128-row leaf -- 20 KB instead of 0.5 MB per report at 1M points
            chunked = hasattr(eng, "reduce_chunks_many") and len(batch) <= 8 and all(self._chunk_shards(d) for d, _ in batch)
            if chunked:
                buf, lens, mms = eng.reduce_chunks_many(batch, self.normal_index)
                pos = 0
                for ln, (mn, mx) in zip(lens, mms):
                    parts.append(buf[pos:pos + ln])
                    ext += [mx, mn]
                    pos += ln
            else:
                for d, m in batch:
                    xvec, mn, mx = eng.reduce(d, m, self.normal_index)
                    parts.append(xvec)
                    ext += [mx, mn]
            finish = eng.finish_chunks if chunked else eng.finish_sum
            # the extrema ride along: every rank owns one block of slots and leaves the others zero, so the SUM
            # hands every rank all the local extrema unchanged (x + 0 is exact) -- one collective per report
            slots = np.zeros((coll.world, len(ext)), dtype=np.float64)
            slots[coll.rank] = ext
            summed = coll.allreduce(np.concatenate(parts + [slots.ravel()]), "sum")   # x + 0 is exact: bitwise assembly
            ext = summed[len(summed) - slots.size:].reshape(slots.shape)
            pos = 0
            for i, (d, m) in enumerate(batch):
                n = eng.n_iter(d)
                ln = len(parts[i])
                self._xchg[(d, m)] = (finish(summed[pos:pos + ln], n), np.float64(np.min(ext[:, 2 * i + 1])),
                                      np.float64(np.max(ext[:, 2 * i])))
                pos += ln
        return self._xchg[key]

    def _chunk_shards(self, direction: int) -> bool:
        """Do the shards of ``direction`` start and end on 8192-row chunks?  (the rule of pccm_set_shard: whenever the cloud
        has a chunk for every rank that shares the direction)"""
        sub_world = max(w for _, w in self._plan[direction])
        return sub_world >= 1 and self._engine.n_iter(direction) >= sub_world * 8192

    def _total(self, direction: int, metric: int):
        """(sum, min, max) of a whole column, unsharded.  The first column a report asks for brings every column the
        report enqueued (prefetch_reductions) back in ONE call: one wait for the GPU, one trip through ctypes."""
        key = (direction, metric)
        done = self._totals.get(key)
        if done is not None:
            return done
        eng = self._engine
        batch = [k for k in self._xchg_wanted if k not in self._totals]
        if key not in batch:
            batch.append(key)
        if hasattr(eng, "reduce_total_many") and len(batch) > 1:
            batch = batch[:_MAX_REQUESTS]
            for k, v in zip(batch, eng.reduce_total_many(batch, self.normal_index)):
                self._totals[k] = v
        if key not in self._totals:
            self._totals[key] = eng.reduce_total(direction, metric, self.normal_index)
        return self._totals[key]

    def _check_unsharded(self, rows: str) -> None:
        """``rows`` read whole columns on one GPU: ValueError before any GPU work of a report for a sharded pair."""
        if self._coll.sharded:
            raise ValueError(f"{rows} rows are not available for sharded pairs (group=)")

    def _check_density(self) -> None:
        """options.check_dcd for this pair: ValueError before any GPU work of a report."""
        if self.ties == "mean":
            raise ValueError("density-aware Chamfer rows are not defined under ties='mean': a virtual neighbour has no row to count")
        self._check_unsharded("density-aware Chamfer")

    def _consumed(self, tag: str, key):
        """The answer to request ``key`` of row family ``tag`` (_FAMILIES), after the family's check.  The first request a report
        asks for brings back the batch it was enqueued in (prefetch_reductions) in one call.  None: this engine has no such method
        (a test double): the caller works on the materialised column."""
        family = _FAMILIES[tag]
        family.check(self)
        consume = getattr(self._engine, family.consume, None)
        if consume is None:
            return None
        cache, wanted = self._results[tag]
        if key not in cache:
            batch = next((b for b in family.batches(wanted) if key in b), [key])
            cache.update(zip(batch, consume(batch, self.normal_index)))
        return cache[key]

    def _selected(self, direction: int, metric: int, k: int):
        """The k-th smallest element of a whole D1 / D2 column, selected on the GPU."""
        return self._consumed("ranked", (direction, metric, k))

    def _counted(self, direction: int, metric: int, x: float):
        """The number of rows ``<= x`` of a whole D1 / D2 column, counted on the GPU."""
        return self._consumed("within", (direction, metric, x))

    def _mapped(self, direction: int, metric: int, which: int, x: float):
        """``(sum, min, max)`` of f(column) for a whole D1 / D2 column, mapped and reduced on the GPU (``which``: nat.MAP_*, ``x``:
        the clamp)."""
        return self._consumed("mapped", (direction, metric, which, x))

    def _density(self, direction: int, alpha: float, squared: bool):
        """``(sum, min, max)`` of the density-aware Chamfer terms of a whole D1 column, gathered, mapped and reduced on the GPU."""
        return self._consumed("density", (direction, alpha, squared))

    def voxel_occupancy(self, voxel: float) -> typing.Tuple[int, int, int]:
        """``(nA, nB, nAB)``: how many voxels of edge ``voxel`` -- cells of the absolute lattice ``floor(coordinate / voxel)`` --
        the origin cloud occupies, the processed cloud occupies, and both occupy, counted on the GPU's voxel table
        (pccm_voxel_occupancy) over the points as they are compared: after ``duplicates=`` and ``transform=`` / ``align=``.  Python
        ints, kept per voxel size for the life of the pair's points."""
        return self._voxel_occupancy((voxel,))[0]

    def _voxel_occupancy(self, voxels) -> list:
        """The triples of ``voxels``; those the pair does not hold yet come from ONE engine call."""
        self._check_unsharded("voxel-occupancy")
        sizes = []
        for v in voxels:
            if isinstance(v, bool) or type(v).__name__ == "bool_" or not isinstance(v, numbers.Real) \
                    or not math.isfinite(v) or not float(v) > 0.0:
                raise ValueError(f"voxel_occupancy: {v!r} is not a finite voxel size > 0")
            sizes.append(float(v))
        missing = sorted({f for f in sizes if f not in self._occupancy})
        if missing:
            eng = self._engine
            if not hasattr(eng, "voxel_occupancy"):
                raise ValueError("this engine cannot count occupied voxels")
            for at in range(0, len(missing), nat.MAX_OCCUPANCY):
                part = missing[at:at + nat.MAX_OCCUPANCY]
                for f, triple in zip(part, eng.voxel_occupancy(part)):
                    self._occupancy[f] = tuple(int(c) for c in triple)
        return [self._occupancy[f] for f in sizes]

    def match_counts(self, is_left: bool = True) -> np.ndarray:
        """How many points of the iterating cloud (left: the origin cloud) matched each point of the searched cloud:
        ``np.bincount(matched rows, minlength=len(searched cloud))``, counted on the GPU (pccm_match_counts), uint32.  Ties go to
        the smallest row (``ties="pick"``); ``1 - np.count_nonzero(counts) / n`` is the left density row at alpha = 0."""
        self._check_density()
        direction = nat.DIR_LEFT if is_left else nat.DIR_RIGHT
        if hasattr(self._engine, "match_counts"):
            return self._engine.match_counts(direction)
        n_searched = self._engine.n_iter(nat.DIR_RIGHT if is_left else nat.DIR_LEFT)
        return np.bincount(self._neighbour_index(direction), minlength=n_searched).astype(np.uint32)

    def tie_exposure(self, is_left: bool = True, point_to_plane: bool = True) -> dict:
        """Opt-in diagnostic (not part of any report): how far the order of EXACT ties can move the point-to-plane MSE.

        The reference keeps whichever equidistant nearest neighbour nanoflann's traversal meets (cloud_pair.py:22-23),
        this package the smallest row; D1 is identical either way, the projection (metric.py:146-153) is not.  Returns
        for one direction: ``tie_rate`` (queries with >= 2 equidistant nearest neighbours), ``max_multiplicity``, and --
        with ``point_to_plane`` -- ``d2_mse_min <= d2_mse_pick <= d2_mse_max``: the smallest / this package's / the largest
        GeoMSE(point_to_plane=True) any tie rule can produce (the reference's value lies in that interval; on tie-free
        data the three coincide).  Sums are plain fp64 accumulations: a diagnostic, not a bit-pinned metric."""
        direction = nat.DIR_LEFT if is_left else nat.DIR_RIGHT
        mode = None
        if point_to_plane:
            self._require_normals(1 if is_left else 0)
            mode = self.normal_index
        r = self._engine.tie_exposure(direction, mode)      # (the sweeps ran in the constructor / recompute)
        vec = np.array([r["queries"], r["tied"], r["sum_min"], r["sum_max"], r["sum_pick"], r["not_enumerated"]], dtype=np.float64)
        mult = np.array([float(r["max_multiplicity"])])
        if self._coll.sharded:
            vec = self._coll.allreduce(vec, "sum")
            mult = self._coll.allreduce(mult, "max")
        n = self._engine.n_iter(direction)
        out = {"direction": "left" if is_left else "right", "queries": int(vec[0]), "tied_queries": int(vec[1]),
               "tie_rate": float(vec[1] / max(vec[0], 1.0)), "max_multiplicity": int(mult[0]), "not_enumerated": int(vec[5])}
        if point_to_plane:
            out.update(d2_mse_min=float(vec[2] / n), d2_mse_max=float(vec[3] / n), d2_mse_pick=float(vec[4] / n),
                       normal_index=self.normal_index)
        return out

    def tie_counts(self, is_left: bool = True) -> np.ndarray:
        """Under ``ties="mean"``: how many equidistant nearest neighbours every point of the iterating cloud has (1: no tie)."""
        if self.ties != "mean":
            raise ValueError("tie counts exist for ties='mean'")
        direction = nat.DIR_LEFT if is_left else nat.DIR_RIGHT
        return self._gather(direction, self._engine.tie_counts(direction)).astype(np.int64)

    def _neighbour_index(self, direction: int) -> np.ndarray:
        if direction not in self._idx_cache:
            idx, _ = self._engine.fetch_nn(direction, want_d2=False)
            self._idx_cache[direction] = self._gather(direction, idx).astype(np.int64)
        return self._idx_cache[direction]

    def _normals_ready(self, which: int) -> bool:
        return self._estimated[which] or self._carried[which] or _has_normals(self.clouds[which])

    def _require_normals(self, which: int) -> None:
        if self._normals_ready(which):
            return
        if self._carry_normals:
            # the other cloud's normals, given or estimated as below, carried over (with none on either cloud: cloud 0's)
            other = 1 - which
            if not self._normals_ready(other):
                self._estimate(0)
                if which == 0:
                    return                          # (cloud 1 takes them over when somebody needs its normals)
            self._engine.carry_normals(other)                            # stays in HBM; inputs are not touched
            self._carried[which] = True
            self._graph_id = None                                        # device buffers changed
            self._update_fusion()
            return
        self._estimate(which)

    def _estimate(self, which: int) -> None:
        if not (self._estimate_normals and hasattr(self._engine, "estimate_normals")):
            raise ValueError(
                f"cloud {which} has no normals: point-to-plane metrics need them "
                "(the reference would call Open3D's estimate_normals here, cloud_pair.py:61-64)")
        self._engine.estimate_normals(which, self._normals_knn)      # stays in HBM; inputs are not touched
        self._estimated[which] = True
        self._graph_id = None                                        # device buffers changed
        self._update_fusion()                                        # the next sweeps carry the projection along

    # -- reference surface, cloud_pair.py:82-124 -------------------------------------------------
    @property
    def origin_cloud(self):
        return self.clouds[0]

    @property
    def reconst_cloud(self):
        return self.clouds[1]

    def get_left_error_vector(self):
        return DeviceRows(self, nat.DIR_LEFT)

    def get_right_error_vector(self):
        return DeviceRows(self, nat.DIR_RIGHT)

    def get_left_neighbour_distances(self):
        return DeviceColumn(self, nat.DIR_LEFT, "d1")

    def get_right_neighbour_distances(self):
        return DeviceColumn(self, nat.DIR_RIGHT, "d1")

    def get_boundary_sqrt_distances(self):
        if not self._self_done:
            self._engine.nn(nat.DIR_SELF, self.nn_engine)
            self._self_done = True
        return DeviceColumn(self, nat.DIR_SELF, "boundary")

    def get_extent(self):
        if self._extent is None:
            self._extent = minimal_obb_extent(_host_rows(self.clouds[0].points), self._engine)
        return self._extent

    def get_normals(self, which: int):
        """np.asarray(clouds[which].normals), tagged for the fused projection (metric.py:92-98)."""
        self._require_normals(which)
        if self._estimated[which] or self._carried[which] or self._merged[which] or self._moved[which]:
            host = self._engine.get_normals(which)
        else:
            host = np.asarray(_host_rows(self.clouds[which].normals))
        view = host.view(CloudNormalsView)
        view._pccm_origin = (id(self), which)
        return view

    def _own_colours(self, which: int):
        """cloud_pair.py:114-118; tagged so that the colour metrics can recognise the pair's own rows."""
        if self._merged[which]:
            view = self._engine.get_colors(which).view(CloudColorsView)      # (the merged rows: duplicates=)
        else:
            view = np.asarray(_host_rows(self.clouds[which].colors)).view(CloudColorsView)
        view._pccm_origin = (id(self), which)
        return view

    def get_left_colors(self):
        return self._own_colours(0)

    def get_right_colors(self):
        return self._own_colours(1)

    def _upload_colours(self, k: int) -> None:
        cloud = self.clouds[k]
        u8 = getattr(cloud, "colors_u8", None)
        if u8 is not None and hasattr(self._engine, "set_colors_u8"):
            self._engine.set_colors_u8(k, u8)        # file colours: 3 B/point up, the k / 255.0 redone on the device
        else:
            self._engine.set_colors(k, _host_rows(cloud.colors))
        self._colours_on_device[k] = True

    def _ensure_colours(self) -> None:
        for k in range(2):
            if not self._colours_on_device[k]:
                self._upload_colours(k)

    def _colour_rows_arg(self, direction: int):
        """Neighbour rows for the colour kernels: the context's own (None) unless the search was sharded."""
        self._ensure_colours()
        return self._neighbour_index(direction) if self._coll.sharded else None

    def _colour_reduction(self, direction: int, scheme: str, scale: float):
        key = (direction, scheme, scale)
        if key not in self._colour_red:
            self._colour_red[key] = self._engine.color_reduce(direction, scheme, scale, self._colour_rows_arg(direction))
        return self._colour_red[key]

    def _angular_column(self, direction: int) -> DeviceColumn:
        """Plane-to-plane angular similarities of one direction: both clouds' normals (given, or estimated as for point-to-plane)."""
        self._require_normals(0)
        self._require_normals(1)
        return DeviceColumn(self, direction, "angular")

    def get_left_angular_similarities(self):
        """Per point of the origin cloud: the angular similarity of its normal and its nearest reconstructed point's."""
        return self._angular_column(nat.DIR_LEFT)

    def get_right_angular_similarities(self):
        return self._angular_column(nat.DIR_RIGHT)

    # -- PointSSIM ("PointSSIM") ------------------------------------------------------------------------------
    def _check_ssim(self, attributes, k: int) -> None:
        """The ValueErrors of CalculateOptions and options.check_point_ssim, for this pair -- raised before any GPU work of a
        report."""
        from .options import CalculateOptions, check_point_ssim
        check_point_ssim(CalculateOptions(point_ssim=attributes, ssim_neighbours=k), *self.clouds,
                         estimate_normals=self._estimate_normals, ties=self.ties,
                         group=self._coll.group if self._coll.sharded else None)

    def _ensure_ssim(self, attributes, k: int) -> None:
        """Both clouds' feature columns of ``attributes`` at neighbourhood size ``k``, built in HBM where missing
        (pccm_ssim_features; the origin cloud's survive with_reconst), and the matched rows kept by later searches."""
        attributes = tuple(attributes)
        self._check_ssim(attributes, k)
        if "normal" in attributes:
            self._require_normals(0)
            self._require_normals(1)
        if "color" in attributes:
            self._ensure_colours()
        built = False
        for which in (0, 1):
            built = self._engine.ssim_features(which, int(k), attributes) or built
        if built:                                         # totals of earlier features are stale
            self._drop_totals(nat.METRIC_SSIM.values())
        self._keep_matched_rows("ssim")

    def get_ssim_features(self, which: int, attribute: str, k: int = 12):
        """Per point of cloud ``which`` (0 origin, 1 reconstructed): its PointSSIM feature of ``attribute`` over its k
        nearest points (fp64; a device column, copied to the host when asked for)."""
        if which not in (0, 1):
            raise ValueError("which must be 0 or 1")
        self._ensure_ssim((attribute,), k)
        return DeviceFeatures(self, which, attribute)

    def _ssim_column(self, direction: int, attribute: str, k: int) -> DeviceColumn:
        self._ensure_ssim((attribute,), k)
        return DeviceColumn(self, direction, f"ssim:{attribute}")

    def get_left_ssim_similarities(self, attribute: str, k: int = 12):
        """Per point of the origin cloud: the PointSSIM similarity of its ``attribute`` feature and its nearest reconstructed
        point's."""
        return self._ssim_column(nat.DIR_LEFT, attribute, k)

    def get_right_ssim_similarities(self, attribute: str, k: int = 12):
        return self._ssim_column(nat.DIR_RIGHT, attribute, k)

    # -- point-to-distribution ("Point-to-distribution") ------------------------------------------------------
    _P2D_METRICS = (nat.METRIC_P2D, nat.METRIC_P2D_COLOR, nat.METRIC_P2D_JOINT)

    def _check_p2d(self, k: int, color: bool = False) -> None:
        """The ValueErrors of CalculateOptions, options.check_point_to_distribution and -- ``color`` -- options.check_p2d_color,
        for this pair -- raised before any GPU work of a report."""
        from .options import CalculateOptions, check_p2d_color, check_point_to_distribution
        options = CalculateOptions(point_to_distribution=True, p2d_neighbours=k, p2d_color=color)
        group = self._coll.group if self._coll.sharded else None
        check_point_to_distribution(options, group=group)
        check_p2d_color(options, *self.clouds, group=group)

    def _ensure_p2d(self, k: int, color: bool = False) -> None:
        """Both directions' columns at neighbourhood size ``k`` -- ``color``: the colour and joint columns too -- built in HBM
        where missing (pccm_p2d_build_attrs: new points in either cloud -- with_reconst -- drop them, so the next report builds
        them again; new colours drop the colour and joint columns).  Both clouds' colours go up before a build that reads them."""
        self._check_p2d(k, color)
        if not hasattr(self._engine, "p2d_build"):
            raise ValueError("this engine has no point-to-distribution columns")
        if color:
            self._ensure_colours()
        built = self._engine.p2d_build(int(k), nat.P2D_GEOMETRY | (nat.P2D_COLOR if color else 0))
        if built or self.__dict__.get("_p2d_k") != int(k):    # totals of earlier columns are stale
            self._drop_totals(self._P2D_METRICS)
        self._p2d_k = int(k)

    def _p2d_column(self, direction: int, k: int, kind: str = "p2d") -> DeviceColumn:
        self._ensure_p2d(k, color=kind != "p2d")
        return DeviceColumn(self, direction, kind)

    def get_left_mahalanobis_distances(self, k: int = 30):
        """Per point of the origin cloud: its Mahalanobis distance to the distribution of its k nearest reconstructed points
        (fp64; a device column: ``np.asarray`` fetches it, ``np.sum`` / ``np.max`` reduce it on the GPU).  The tie policy of the
        1-NN searches does not enter it."""
        return self._p2d_column(nat.DIR_LEFT, k)

    def get_right_mahalanobis_distances(self, k: int = 30):
        return self._p2d_column(nat.DIR_RIGHT, k)

    def get_left_color_mahalanobis_distances(self, k: int = 30):
        """Per point of the origin cloud: the distance of its luma to the luma distribution of its k nearest reconstructed
        points -- the neighbourhood of get_left_mahalanobis_distances -- in ridged standard deviations (fp64, always finite; a
        device column).  Both clouds need colours."""
        return self._p2d_column(nat.DIR_LEFT, k, "p2d_color")

    def get_right_color_mahalanobis_distances(self, k: int = 30):
        return self._p2d_column(nat.DIR_RIGHT, k, "p2d_color")

    def get_left_joint_mahalanobis_distances(self, k: int = 30):
        """Per point of the origin cloud: sqrt(M_G^2 + M_Y^2) of its geometry and colour point-to-distribution values (inf
        where the geometry value is)."""
        return self._p2d_column(nat.DIR_LEFT, k, "p2d_joint")

    def get_right_joint_mahalanobis_distances(self, k: int = 30):
        return self._p2d_column(nat.DIR_RIGHT, k, "p2d_joint")

    # -- resolution-adaptive PSNR ("Resolution-adaptive PSNR") -------------------------------------------------
    def _check_resolution(self, k: int) -> None:
        """The ValueErrors of CalculateOptions and options.check_resolution_psnr, for this pair -- raised before any GPU work of
        a report.  (``ties="mean"`` is fine: the column does not depend on the policy.)"""
        from .options import CalculateOptions, check_resolution_psnr
        check_resolution_psnr(CalculateOptions(resolution_psnr=True, resolution_neighbours=k),
                              group=self._coll.group if self._coll.sharded else None)

    def _ensure_resolution(self, k: int) -> None:
        """Both clouds' spacing columns over ``k`` neighbours, built in HBM where missing (pccm_resolution_build: the origin
        cloud's survives with_reconst, so only the new cloud's is built then)."""
        self._check_resolution(k)
        if not hasattr(self._engine, "resolution_build"):
            raise ValueError("this engine has no point spacings")
        built = False
        for which in (0, 1):
            built = self._engine.resolution_build(which, int(k)) or built
        if built or self.__dict__.get("_resolution_k") != int(k):     # totals of earlier columns are stale
            self._drop_totals((nat.METRIC_RESOLUTION,))
        self._resolution_k = int(k)

    def _spacing_column(self, direction: int, k: int) -> DeviceColumn:
        self._ensure_resolution(k)
        return DeviceColumn(self, direction, "spacing")

    def get_left_point_spacings(self, k: int = 10):
        """Per point of the origin cloud: the mean distance to its k nearest neighbours in the origin cloud (fp64; a device
        column: ``np.asarray`` fetches it, ``np.sum`` / ``np.max`` reduce it on the GPU).  ``np.sum(...) / n`` is the cloud's
        intrinsic resolution.  Neither the other cloud nor the tie policy enters it."""
        return self._spacing_column(nat.DIR_LEFT, k)

    def get_right_point_spacings(self, k: int = 10):
        """The same for the reconstructed cloud."""
        return self._spacing_column(nat.DIR_RIGHT, k)

    # -- reflectance ("Reflectance") ---------------------------------------------------------------------------
    def _pair_has_reflectance(self, which: int) -> bool:
        return self._reflectance_on_device[which] or _has_reflectance(self.clouds[which])

    def _check_reflectance(self) -> None:
        """The ValueErrors of options.check_reflectance, for this pair -- raised before any GPU work of a report."""
        if self.ties != "pick":
            raise ValueError("reflectance rows are not defined for ties='mean'")
        if self._coll.sharded:
            raise ValueError("reflectance rows are not available for sharded pairs (group=)")
        if not all(self._pair_has_reflectance(k) for k in range(2)):
            raise ValueError("the reflectance rows need the reflectance of both clouds")
        if not hasattr(self._engine, "set_reflectance"):
            raise ValueError("this engine has no reflectance column")

    def _upload_reflectance(self, k: int) -> None:
        self._engine.set_reflectance(k, _host_rows(self.clouds[k].reflectance))   # (uint8 / uint16 go as 16-bit words, widened exactly)
        self._reflectance_on_device[k] = True

    def _ensure_reflectance(self) -> None:
        """Both clouds' reflectance in HBM (uploaded on first need, like the colours), and the matched rows kept by later
        searches."""
        self._check_reflectance()
        for k in range(2):
            if not self._reflectance_on_device[k]:
                self._upload_reflectance(k)
        self._keep_matched_rows("reflectance")

    def set_reflectance(self, which: int, reflectance) -> None:
        """Replace the reflectance the pair holds for cloud ``which`` (the caller's cloud object is not touched): the searches,
        normals, colours and every other column stay as they are; the next report reduces the reflectance columns again.  One value
        per row of the cloud the pair WORKS ON: under ``duplicates=`` that is the merged cloud (``merge_map(which)`` says which
        merged row each given row became), not the cloud that was given; a wrong length raises ``ValueError``."""
        if which not in (0, 1):
            raise ValueError("which must be 0 or 1")
        if not hasattr(self._engine, "set_reflectance"):
            raise ValueError("this engine has no reflectance column")
        values = _host_rows(reflectance)
        rows = self._engine.n_iter(nat.DIR_RIGHT if which else nat.DIR_LEFT)
        if values.shape[0] != rows:
            hint = (f" (duplicates={self._duplicates!r} merged {self.duplicates_removed[which]} of its rows away: pass one value per merged"
                    " row, see merge_map)") if self._merged[which] else ""
            raise ValueError(f"cloud {which} has {rows} rows but {values.shape[0]} reflectance values were given{hint}")
        self._reflectance_on_device[which] = False
        self._drop_totals((nat.METRIC_REFLECTANCE,))
        self._graph_id = None                                        # (a captured point job read the old column)
        self._engine.set_reflectance(which, values)
        self._reflectance_on_device[which] = True

    def get_reflectance(self, which: int) -> np.ndarray:
        """The fp64 reflectance column the pair works on for cloud ``which`` (the merged one under ``duplicates=``)."""
        if which not in (0, 1):
            raise ValueError("which must be 0 or 1")
        if not self._pair_has_reflectance(which):
            raise ValueError(f"cloud {which} has no reflectance")
        if not self._reflectance_on_device[which]:
            self._upload_reflectance(which)
        return self._engine.get_reflectance(which)

    def _reflectance_column(self, direction: int) -> DeviceColumn:
        self._ensure_reflectance()
        return DeviceColumn(self, direction, "reflectance")

    def get_left_reflectance_errors(self):
        """Per point of the origin cloud: the squared difference of its reflectance and its nearest reconstructed point's (fp64;
        a device column: ``np.asarray`` fetches it, ``np.sum`` / ``np.max`` reduce it on the GPU)."""
        return self._reflectance_column(nat.DIR_LEFT)

    def get_right_reflectance_errors(self):
        return self._reflectance_column(nat.DIR_RIGHT)

    def get_left_neighbour_colors(self):
        """cloud_pair.py:120-121: the matched points' colours -- gathered on the device when asked for."""
        return DeviceColorRows(self, nat.DIR_LEFT, "neighbour")

    def get_right_neighbour_colors(self):
        return DeviceColorRows(self, nat.DIR_RIGHT, "neighbour")

    def prefetch_reductions(self, wanted, _remember: bool = True) -> None:
        """Enqueue the fused reductions a report is about to ask for, without waiting for any of them.

        ``wanted``: iterable of ``(is_left, point_to_plane)`` pairs, ``("angular", is_left)``, ``("ssim", attribute, is_left, k)``,
        ``("ranked", is_left, point_to_plane, rank)``, ``("p2d", is_left, k)``, ``("p2d_color", is_left, k)``,
        ``("p2d_joint", is_left, k)``, ``("spacing", is_left, k)``, ``("reflectance", is_left)``, ``("within", is_left, tau)``,
        ``("mapped", is_left, point_to_plane, root, clamp)`` (clamp: a number or None), ``("density", is_left, alpha, squared)``,
        ``("occupancy", voxel)`` and/or the string ``"boundary"``.
        MetricCalculator.calculate() calls this after walking the DAG of the requested metrics, so
        that the host waits for the GPU once per report instead of once per column.  Purely an
        optimisation: columns that were not prefetched are reduced on demand."""
        eng = self._engine
        can_prefetch = hasattr(eng, "reduce_prefetch")
        wanted = list(wanted)
        if _remember and can_prefetch:
            if self._last_wanted is not None and wanted != self._last_wanted and self._graph_id is not None:
                eng.graph_destroy(self._graph_id)             # a different report: capture anew next time
                self._graph_id = None
            self._last_wanted = wanted
        groups = _by_family(wanted)
        self._prepare_families(groups)
        plan = _plan_report(groups, self._prepare_columns(groups.get("column", ())), eng.n_iter)
        self._xchg_wanted = plan.columns
        self._results = {tag: (self._results[tag][0], plan.rows[tag]) for tag in _FAMILIES}
        if can_prefetch:
            self._enqueue(plan)

    def _prepare_families(self, groups) -> None:
        """What a report's row families need before anything is enqueued, family by family: its check (ValueError before any GPU
        work of the family), then what it reads in HBM -- built or uploaded here, eagerly and outside any graph capture, the first
        time a report asks for it, and found there every time after that."""
        if groups.keys() <= {"column"}:
            return                      # (the usual report: D1 / D2, angular and boundary rows only)
        # PointSSIM: both clouds' features, one build per neighbourhood size
        by_k = {}
        for _, attribute, _, k in groups.get("ssim", ()):
            by_k.setdefault(k, []).append(attribute)
        for k, attributes in by_k.items():
            self._check_ssim(attributes, k)
        for k, attributes in by_k.items():
            self._ensure_ssim(sorted(set(attributes)), k)
        # ranked Hausdorff, F-score, Chamfer / truncated and density-aware Chamfer rows: they read the D1 / D2 columns
        for tag, family in _FAMILIES.items():
            if tag in groups:
                family.check(self)
                if family.keeps_rows:
                    self._keep_matched_rows(tag)
        # point-to-distribution: one build per neighbourhood size, with the union of what the report needs at that size
        colour_at = {}
        for kind, _, k in groups.get("p2d", ()):
            colour_at[k] = colour_at.get(k, False) or kind != "p2d"
        for k in sorted(colour_at):
            self._check_p2d(k, colour_at[k])
        for k in sorted(colour_at):
            self._ensure_p2d(k, colour_at[k])
        # point spacings: one build per cloud and neighbour count
        sizes = sorted({item[2] for item in groups.get("spacing", ())})
        for k in sizes:
            self._check_resolution(k)
        for k in sizes:
            self._ensure_resolution(k)
        # reflectance: both clouds' columns in HBM
        if "reflectance" in groups:
            self._ensure_reflectance()
        # voxel occupancy: every size the pair does not hold yet, in one call; a replayed report finds them all held
        if "occupancy" in groups:
            self._voxel_occupancy(sorted({item[1] for item in groups["occupancy"]}))

    def _prepare_columns(self, items):
        """The requests of the columns formed from the searches' results -- ``"boundary"``, ``("angular", is_left)`` and
        ``(is_left, point_to_plane)`` -- in the order given, after what each needs (the self search, normals).  A column that
        cannot be formed is left out: its error surfaces when the column is evaluated."""
        found = (self._boundary_request() if item == "boundary" else self._angular_request(item[1]) if item[0] == "angular"
                 else self._distance_request(*item) for item in items)
        return [request for request in found if request is not None]

    def _boundary_request(self):
        if self._self_done and (nat.DIR_SELF, nat.METRIC_D1) in self._totals:
            return None                                   # inherited with the origin cloud (with_reconst): nothing to reduce again
        if not self._self_done:
            self._engine.nn(nat.DIR_SELF, self.nn_engine)
            self._self_done = True
        return nat.DIR_SELF, nat.METRIC_D1

    def _angular_request(self, is_left: bool):
        try:
            self._require_normals(0)
            self._require_normals(1)
        except ValueError:
            return None
        self._keep_matched_rows("angular")
        return _direction(is_left), nat.METRIC_ANGULAR

    def _distance_request(self, is_left: bool, point_to_plane: bool):
        direction = _direction(is_left)
        if not point_to_plane:
            return direction, nat.METRIC_D1
        other = 1 if is_left else 0
        try:
            self._require_normals(other)
        except ValueError:
            return None
        n_other = self._engine.n_iter(nat.DIR_RIGHT if other else nat.DIR_LEFT) if self._estimated[other] or self._carried[other] \
            or self._merged[other] else len(self.clouds[other].normals)
        if self.normal_index == "row" and self._engine.n_iter(direction) > n_other:
            return None           # row-indexed normals out of range (the WHOLE cloud decides, so that every rank of a sharded
            #                       pair agrees): surfaces, on every rank, where the reference raises
        return direction, nat.METRIC_D2

    def _enqueue(self, plan: "_Plan") -> None:
        """Hand a report's plan to the engine: the column batches in order, then each row family's batches."""
        eng = self._engine
        if not hasattr(eng, "reduce_prefetch_many"):
            for direction, metric in plan.columns:
                eng.reduce_prefetch(direction, metric, self.normal_index)
            return
        for batch in plan.batches:
            eng.reduce_prefetch_many(batch, self.normal_index)
        for tag, rows in plan.rows.items():
            prefetch = getattr(eng, _FAMILIES[tag].prefetch, None) if rows else None
            if prefetch is not None:
                for batch in _FAMILIES[tag].batches(rows):
                    prefetch(batch, self.normal_index)

    # -- fused projection used by metric.ErrorVector ------------------------------------------------
    def point_to_plane_column(self, is_left: bool) -> DeviceColumn:
        self._require_normals(1 if is_left else 0)
        return DeviceColumn(self, nat.DIR_LEFT if is_left else nat.DIR_RIGHT, "proj")


# -- how a report becomes launches ("How a report becomes launches") ----------------------------------------------------
_MAX_REQUESTS = 8       # what one pccm_*_many call takes: every batch below, and every batch read back, has at most eight requests
_MAX_POINT_JOBS = 4     # columns one k_point_jobs launch forms from the matched rows: unfused D2, angular, reflectance, PointSSIM

_GROUP = {"ssim": "ssim", "ranked": "ranked", "within": "within", "mapped": "mapped", "density": "density", "p2d": "p2d",
          "p2d_color": "p2d", "p2d_joint": "p2d", "spacing": "spacing", "reflectance": "reflectance", "occupancy": "occupancy"}


def _by_family(wanted):
    """The items of ``wanted`` (prefetch_reductions) grouped by what prepares them, each group in the order given: the tag's group
    of _GROUP, or "column" for ``"boundary"``, ``("angular", is_left)`` and ``(is_left, point_to_plane)``."""
    groups = {}
    for item in wanted:
        groups.setdefault(_GROUP.get(item[0] if isinstance(item, tuple) else item, "column"), []).append(item)
    return groups


def _direction(is_left: bool) -> int:
    return nat.DIR_LEFT if is_left else nat.DIR_RIGHT


def _side_column(is_left: bool, point_to_plane: bool = False):
    return _direction(is_left), nat.METRIC_D2 if point_to_plane else nat.METRIC_D1


def _selection_batches(selections):
    """Sorted ``(direction, metric, k)`` selections in batches of at most _MAX_REQUESTS that keep the ranks of a column together:
    every pass of a batch streams each of its columns once, whatever the number of ranks.  Counts ``(direction, metric, x)`` are
    batched the same way."""
    batches, current = [], []
    for column in sorted({q[:2] for q in selections}):
        ranks = [q for q in selections if q[:2] == column]
        for at in range(0, len(ranks), _MAX_REQUESTS):
            part = ranks[at:at + _MAX_REQUESTS]
            if current and len(current) + len(part) > _MAX_REQUESTS:
                batches.append(current)
                current = []
            current = current + part
    if current:
        batches.append(current)
    return batches


def _map_batches(maps):
    """Sorted ``(direction, metric, map, x)`` mapped reductions in batches of _MAX_REQUESTS: the order keeps a column's maps next
    to each other, and two of them share one read of the column.  Density maps ``(direction, alpha, squared)`` likewise."""
    return [maps[at:at + _MAX_REQUESTS] for at in range(0, len(maps), _MAX_REQUESTS)]


def _ranked_request(item, column, n_iter):
    from .metric import rank_index
    return column + (rank_index(item[3], n_iter(column[0])),)


def _within_request(item, column, n_iter):
    return column + (float(np.float64(item[2]) * np.float64(item[2])),)       # tau * tau, the product GeoInlierRatio forms


def _mapped_request(item, column, n_iter):
    root, clamp = item[3], item[4]
    return column + ((nat.MAP_CLAMP if clamp is not None else 0) | (nat.MAP_ROOT if root else 0), 0.0 if clamp is None else float(clamp))


def _density_request(item, column, n_iter):
    return column[0], float(item[2]) + 0.0, bool(item[3])


class _Family(typing.NamedTuple):
    """A family of report rows answered from a whole D1 / D2 column by calls of its own, up to _MAX_REQUESTS requests each."""
    check: typing.Callable          # (pair): ValueError where the pair cannot have these rows -- before any GPU work of the family
    column: typing.Callable         # (item) -> the (direction, metric) column the item of ``wanted`` reads
    request: typing.Callable        # (item, column, n_iter) -> the engine's request
    batches: typing.Callable        # (sorted requests) -> the batches they are enqueued and read back in
    prefetch: str                   # the engine method that enqueues a batch
    consume: str                    # ... and the one that brings its answers back
    keeps_rows: bool = False        # the searches have to keep the matched rows


# by the tag of the family's items in ``wanted``; the order is the order of the checks and of the launches
_FAMILIES = {
    "ranked": _Family(lambda pair: pair._check_unsharded("ranked Hausdorff"), lambda item: _side_column(item[1], item[2]),
                      _ranked_request, _selection_batches, "select_prefetch_many", "select_many"),
    "within": _Family(lambda pair: pair._check_unsharded("F-score"), lambda item: _side_column(item[1]),
                      _within_request, _selection_batches, "count_prefetch_many", "count_many"),
    "mapped": _Family(lambda pair: pair._check_unsharded("Chamfer and truncated-distance"), lambda item: _side_column(item[1], item[2]),
                      _mapped_request, _map_batches, "reduce_map_prefetch_many", "reduce_map_total_many"),
    "density": _Family(CloudPair._check_density, lambda item: _side_column(item[1]),
                       _density_request, _map_batches, "reduce_density_prefetch_many", "reduce_density_total_many", keeps_rows=True),
}


class _Plan(typing.NamedTuple):
    """What one report enqueues."""
    batches: list       # the column requests (direction, metric), one reduce_prefetch_many call each, in launch order
    columns: list       # the same requests in the order they are read back in, _MAX_REQUESTS per call (CloudPair._total)
    rows: dict          # per family of _FAMILIES, its requests in sorted order: batched by the family's ``batches``


def _plan_report(groups, requests, n_iter) -> _Plan:
    """The plan of a report from its items by family (_by_family) and the requests of its columns that can be formed
    (CloudPair._prepare_columns).  Asks the engine for nothing but row counts.  Every packing rule is here:

    * a call takes _MAX_REQUESTS requests, and a batch at most _MAX_POINT_JOBS columns formed by point jobs;
    * the reflectance columns join the first batch -- its k_point_jobs launch and its reduction launch -- when it has room for them
      under both limits, and are a batch of their own otherwise;
    * PointSSIM columns, all formed by point jobs, go in batches of _MAX_POINT_JOBS;
    * the stored columns (point-to-distribution, spacings) ride in the first batch when it has room, and follow last otherwise;
    * a row family's requests are those whose column this report reduces (one that was left out surfaces when the row is
      evaluated), sorted, so that a column's ranks stay together and its maps next to each other (_selection_batches, _map_batches)."""
    reduced = set(requests)
    reflectance = [(_direction(item[1]), nat.METRIC_REFLECTANCE) for item in groups.get("reflectance", ())]
    ssim = [(_direction(item[2]), nat.METRIC_SSIM[item[1]]) for item in groups.get("ssim", ())]
    stored = [(_direction(item[1]), DeviceColumn._METRIC[item[0]]) for item in groups.get("p2d", []) + groups.get("spacing", [])]
    first = list(requests)
    if reflectance and len(first) + len(reflectance) <= _MAX_REQUESTS:
        point_jobs = sum(1 for _, m in first if m in (nat.METRIC_D2, nat.METRIC_ANGULAR))
        if point_jobs + len(reflectance) <= _MAX_POINT_JOBS:
            first, reflectance = first + reflectance, []
    columns = first + reflectance + ssim + stored
    ride = len(first) + len(stored) <= _MAX_REQUESTS
    batches = [(first + stored if ride else first)[:_MAX_REQUESTS]]
    if reflectance:
        batches.append(reflectance)
    batches += [ssim[at:at + _MAX_POINT_JOBS] for at in range(0, len(ssim), _MAX_POINT_JOBS)]
    if not ride:
        batches.append(stored)
    rows = {}
    for tag, family in _FAMILIES.items():
        items = groups.get(tag)
        rows[tag] = sorted({family.request(item, column, n_iter) for item in items
                            if (column := family.column(item)) in reduced}) if items else []
    return _Plan(batches, columns, rows)


def _has_normals(cloud) -> bool:
    has = getattr(cloud, "has_normals", None)
    if callable(has):
        return bool(has())
    nrm = getattr(cloud, "normals", None)
    return nrm is not None and len(nrm) > 0


def _has_colors(cloud) -> bool:
    has = getattr(cloud, "has_colors", None)
    if callable(has):
        return bool(has())
    col = getattr(cloud, "colors", None)
    return col is not None and len(col) > 0


def _has_reflectance(cloud) -> bool:
    has = getattr(cloud, "has_reflectance", None)
    if callable(has):
        return bool(has())
    refl = getattr(cloud, "reflectance", None)
    return refl is not None and len(refl) > 0


def _host_rows(a) -> np.ndarray:
    if hasattr(a, "is_cuda"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def shard_plan(world: int, mode: str = "direction"):
    """Who searches what: ``plan[direction][rank] = (sub_rank, sub_world)`` -- rank ``rank`` is number ``sub_rank`` of the
    ``sub_world`` ranks that share the rows of ``direction`` (sub_world 0: it owns none of them).

    "direction" (default, world >= 2): the first half of the ranks takes the left direction (A's rows searched in B:
    they build B's grid only), the second half the right direction and the self search of A (both search A).  The
    replicated part of a step -- the search-structure build -- is halved that way and each half shards its rows; the
    all-gathers of materialised columns concatenate ranks in rank order, which is row order inside each half.
    "rows": every rank takes the same row range of every direction (round 1)."""
    if world <= 1 or mode == "rows":
        same = [(r, world) for r in range(world)]
        return {nat.DIR_LEFT: same, nat.DIR_RIGHT: list(same), nat.DIR_SELF: list(same)}
    nl = (world + 1) // 2
    nr = world - nl
    left = [(r, nl) if r < nl else (0, 0) for r in range(world)]
    right = [(r - nl, nr) if r >= nl else (0, 0) for r in range(world)]
    return {nat.DIR_LEFT: left, nat.DIR_RIGHT: right, nat.DIR_SELF: list(right)}


def _shard_bounds(n: int, rank: int, world: int):
    """Rows of an n-row cloud owned by ``rank``: the rule of pccm_set_shard (whole 8192-row chunks of NumPy's sum when every
    rank can have one, else 128-row leaves); world 0 owns nothing."""
    if world <= 0:
        return 0, 0
    unit = 8192 if n >= world * 8192 else 128
    units = (n + unit - 1) // unit
    return min(n, units * rank // world * unit), min(n, units * (rank + 1) // world * unit)
