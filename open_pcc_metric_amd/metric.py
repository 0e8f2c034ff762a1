"""Metric nodes -- same classes, keys and ``calculate`` signatures as ``open_pcc_metric.metric``.

Reference: open_pcc_metric/metric.py:14-485.  The classes are thin: every N-sized quantity they
pass around is a device column of :mod:`open_pcc_metric_amd.cloud_pair`, so ``np.sum`` in
``GeoMSE``, ``np.max`` in ``GeoHausdorffDistance``, ``np.square`` in ``EuclideanDistance`` and
``np.min``/``np.max`` in ``BoundarySqrtDistances`` run as fused GPU reductions while the code
below reads like the reference's NumPy.  Values injected by hand (as the reference's unit tests
do, tests/unit/test_metric.py:30-70) are plain ndarrays and take the same code path through
NumPy itself.

``_key()`` tuples are both the memo keys of the calculator and the keys of
``CalculateResult.as_dict()`` (metric.py:17-18, 59-60, 70-71, 257-258, 472-473).
"""
from __future__ import annotations

import abc
import fractions
import math
import typing

import numpy as np

from .cloud_pair import CloudPair, CloudNormalsView, DeviceRows


# --------------------------------------------------------------------------- base classes
class AbstractMetric(abc.ABC):                       # metric.py:14-29
    value: typing.Any

    def _key(self) -> typing.Tuple:
        return (type(self).__name__,)

    def _pccm_request(self):
        """What this node asks CloudPair.prefetch_reductions to enqueue ahead of its evaluation -- one of the items listed there --
        or None.  The calculator collects these while it plans a report."""
        return None

    @abc.abstractmethod
    def calculate(self, cloud_pair: CloudPair, **kwargs) -> None:
        raise NotImplementedError("calculate is not implemented")

    def __str__(self) -> str:
        return f"{self._key()}: {self.value}"


class PrimaryMetric(AbstractMetric):                 # metric.py:32-38 -- reads the CloudPair
    _pccm_role = 1          # what the calculator dispatches on (an isinstance on an ABC costs ~1 us)

    @abc.abstractmethod
    def calculate(self, cloud_pair: CloudPair) -> None:
        raise NotImplementedError("calculate is not implemented")


class SecondaryMetric(AbstractMetric):               # metric.py:41-50 -- pure function of its deps
    _pccm_role = 2

    def _get_dependencies(self) -> typing.Dict[str, "AbstractMetric"]:
        return {}

    @abc.abstractmethod
    def calculate(self, **kwargs) -> None:
        raise NotImplementedError("calculate is not implemented")


class DirectionalMetric(AbstractMetric):             # metric.py:53-60
    is_left: bool

    def __init__(self, is_left: bool):
        self.is_left = is_left

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left)


class PointToPlaneable(DirectionalMetric):           # metric.py:63-71
    point_to_plane: bool

    def __init__(self, is_left: bool, point_to_plane: bool):
        super().__init__(is_left)
        self.point_to_plane = point_to_plane

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.point_to_plane)


def _side(metric: DirectionalMetric, left, right):
    return left() if metric.is_left else right()


def _column_reducer(slot: int, on_host):
    """np.sum / np.min / np.max (``on_host``) of a column along axis 0.  A device column answers from ``slot`` of its fused
    (sum, min, max) -- what NumPy would dispatch to, called directly -- unless it has none there (the boundary column's sum); a
    plain array goes to NumPy."""
    def reduce(column):
        fused = getattr(column, "_reduced", None)
        value = fused()[slot] if fused is not None else None
        return on_host(column, axis=0) if value is None else value
    return reduce


_column_sum, _column_min, _column_max = _column_reducer(0, np.sum), _column_reducer(1, np.min), _column_reducer(2, np.max)


# --------------------------------------------------------------------------- primaries
class PrimaryErrorVector(PrimaryMetric, DirectionalMetric):      # metric.py:74-80
    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = _side(self, cloud_pair.get_left_error_vector, cloud_pair.get_right_error_vector)


class NeighbourDistances(PrimaryMetric, DirectionalMetric):      # metric.py:83-89
    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = _side(self, cloud_pair.get_left_neighbour_distances,
                           cloud_pair.get_right_neighbour_distances)


class CloudNormals(PrimaryMetric, DirectionalMetric):            # metric.py:92-98
    def calculate(self, cloud_pair: CloudPair) -> None:
        which = 0 if self.is_left else 1
        if hasattr(cloud_pair, "get_normals"):
            self.value = cloud_pair.get_normals(which)
        else:
            self.value = np.asarray(cloud_pair.clouds[which].normals)


class CloudExtent(PrimaryMetric):                                # metric.py:101-103
    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = cloud_pair.get_extent()


class CloudColors(PrimaryMetric, DirectionalMetric):             # metric.py:106-112
    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = _side(self, cloud_pair.get_left_colors, cloud_pair.get_right_colors)


class NeighbourColors(PrimaryMetric, DirectionalMetric):         # metric.py:115-121
    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = _side(self, cloud_pair.get_left_neighbour_colors,
                           cloud_pair.get_right_neighbour_colors)


class AngularSimilarities(PrimaryMetric, DirectionalMetric):     # no counterpart in the reference (options.py: plane_to_plane)
    """Per point of the iterating cloud, the angular similarity of its normal and its matched neighbour's (include/pccm.h,
    PCCM_METRIC_ANGULAR): 1 - 2 acos(min(|a . b| / (|a| |b|), 1)) / pi, 0 for a zero-length normal."""
    def _pccm_request(self):
        return "angular", self.is_left

    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = _side(self, cloud_pair.get_left_angular_similarities, cloud_pair.get_right_angular_similarities)


class SSIMSimilarities(PrimaryMetric, DirectionalMetric):        # no counterpart in the reference (options.py: point_ssim)
    """Per point of the iterating cloud, the PointSSIM similarity of one attribute's feature and its matched point's
    (include/pccm.h, PCCM_METRIC_SSIM_*): 1 - |a - b| / (max(|a|, |b|) + 2^-52)."""
    def __init__(self, is_left: bool, attribute: str, k: int = 12):
        super().__init__(is_left)
        self.attribute, self.k = attribute, int(k)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.attribute, self.is_left, self.k)

    def _pccm_request(self):
        return "ssim", self.attribute, self.is_left, self.k

    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = _side(self, lambda: cloud_pair.get_left_ssim_similarities(self.attribute, self.k),
                           lambda: cloud_pair.get_right_ssim_similarities(self.attribute, self.k))


class MahalanobisDistances(PrimaryMetric, DirectionalMetric):    # no counterpart in the reference (options.py: point_to_distribution)
    """Per point of the iterating cloud, its Mahalanobis distance to the distribution (mean and ridged covariance) of its k
    nearest points in the OTHER cloud (include/pccm.h, pccm_p2d_build; INTEGRATION.md, "Point-to-distribution")."""
    _pccm_column = "p2d"    # which of the stored columns: the colour and joint subclasses name their own

    def __init__(self, is_left: bool, k: int = 30):
        super().__init__(is_left)
        self.k = int(k)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.k)

    def _pccm_request(self):
        return self._pccm_column, self.is_left, self.k

    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = _side(self, lambda: cloud_pair.get_left_mahalanobis_distances(self.k),
                           lambda: cloud_pair.get_right_mahalanobis_distances(self.k))


class ColorMahalanobisDistances(MahalanobisDistances):           # no counterpart in the reference (options.py: p2d_color)
    """Per point of the iterating cloud, the distance of its luma to the luma distribution of the same k nearest points in the
    OTHER cloud, in ridged standard deviations (include/pccm.h, pccm_p2d_build_attrs; INTEGRATION.md, "Point-to-distribution:
    colour and joint")."""
    _pccm_column = "p2d_color"

    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = _side(self, lambda: cloud_pair.get_left_color_mahalanobis_distances(self.k),
                           lambda: cloud_pair.get_right_color_mahalanobis_distances(self.k))


class JointMahalanobisDistances(MahalanobisDistances):           # no counterpart in the reference (options.py: p2d_color)
    """Per point of the iterating cloud, sqrt(M_G^2 + M_Y^2) of its geometry and colour point-to-distribution values: the
    Mahalanobis distance in (x, y, z, Y) under a block-diagonal covariance."""
    _pccm_column = "p2d_joint"

    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = _side(self, lambda: cloud_pair.get_left_joint_mahalanobis_distances(self.k),
                           lambda: cloud_pair.get_right_joint_mahalanobis_distances(self.k))


class PointSpacings(PrimaryMetric, DirectionalMetric):           # no counterpart in the reference (options.py: resolution_psnr)
    """Per point of ONE cloud -- left: the origin cloud, right: the reconstructed one -- the mean distance to its k nearest
    neighbours in that same cloud (include/pccm.h, pccm_resolution_build; INTEGRATION.md, "Resolution-adaptive PSNR")."""
    def __init__(self, is_left: bool, k: int = 10):
        super().__init__(is_left)
        self.k = int(k)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.k)

    def _pccm_request(self):
        return "spacing", self.is_left, self.k

    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = _side(self, lambda: cloud_pair.get_left_point_spacings(self.k),
                           lambda: cloud_pair.get_right_point_spacings(self.k))


class ReflectanceErrors(PrimaryMetric, DirectionalMetric):       # no counterpart in the reference (options.py: reflectance)
    """Per point of the iterating cloud, the squared difference of its reflectance and its matched point's (include/pccm.h,
    PCCM_METRIC_REFLECTANCE; INTEGRATION.md, "Reflectance"): (a - b)^2 on the values as given."""
    def _pccm_request(self):
        return "reflectance", self.is_left

    def calculate(self, cloud_pair: CloudPair) -> None:
        self.value = _side(self, cloud_pair.get_left_reflectance_errors, cloud_pair.get_right_reflectance_errors)


class MatchedRows(PrimaryMetric, DirectionalMetric):             # no counterpart in the reference (options.py: dcd)
    """Which row of the searched cloud every point of the iterating cloud matched (ties: the smallest row).  For a pair whose
    results live in HBM the value is the direction's lazy DeviceRows -- a handle on the result that is never copied to the host:
    the match counts and the density map read the rows where the search left them -- and for any other pair the plain index
    array."""
    def calculate(self, cloud_pair: CloudPair) -> None:
        getter = getattr(cloud_pair, "get_left_error_vector" if self.is_left else "get_right_error_vector", None)
        rows = getter() if getter is not None else None
        if isinstance(rows, DeviceRows):
            self.value = rows
        else:
            self.value = np.asarray(cloud_pair._neighbour_index(0 if self.is_left else 1))


class BoundarySqrtDistances(PrimaryMetric):                      # metric.py:182-188
    _pccm_waits = True      # reads a reduction back from the GPU: the calculator evaluates these last

    def _pccm_request(self):
        return "boundary"

    def calculate(self, cloud_pair: CloudPair) -> None:
        spacing = cloud_pair.get_boundary_sqrt_distances()
        self.value = (np.min(spacing), np.max(spacing))


# --------------------------------------------------------------------------- geometry secondaries
class ErrorVector(SecondaryMetric, PointToPlaneable):            # metric.py:124-153
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        deps: typing.Dict[str, AbstractMetric] = {"primary_error_vector": PrimaryErrorVector(is_left=self.is_left)}
        if self.point_to_plane:
            # the OTHER cloud's normals, indexed by the iterating row (reference quirk Q1)
            deps["cloud_normals"] = CloudNormals(is_left=not self.is_left)
        return deps

    def calculate(self, primary_error_vector: PrimaryErrorVector,
                  cloud_normals: typing.Optional[CloudNormals] = None) -> None:
        err = primary_error_vector.value
        if not self.point_to_plane:
            err = np.asarray(err)
            # row-wise Euclidean norm (metric.py:138-144); not consumed by any shipped metric
            self.value = np.sqrt(np.einsum("ij,ij->i", err, err))
            return
        nrm = cloud_normals.value
        origin = getattr(nrm, "_pccm_origin", None)
        if isinstance(err, DeviceRows) and isinstance(nrm, CloudNormalsView) and origin == (
                id(err._pair), 1 if self.is_left else 0):
            # both operands live in HBM of the same pair: fused gather + projection on the GPU
            self.value = err._pair.point_to_plane_column(self.is_left)
            return
        # hand-injected arrays: the reference's own row loop, metric.py:146-153
        err, nrm = np.asarray(err), np.asarray(nrm)
        out = np.zeros(shape=(err.shape[0],))
        for i in range(err.shape[0]):
            out[i] = np.dot(err[i], nrm[i])
        self.value = out


class EuclideanDistance(SecondaryMetric, PointToPlaneable):      # metric.py:156-179
    def _pccm_request(self):
        return self.is_left, self.point_to_plane

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        if self.point_to_plane:
            return {"error_vector": ErrorVector(is_left=self.is_left, point_to_plane=True)}
        return {"neighbour_distances": NeighbourDistances(is_left=self.is_left)}

    def calculate(self, neighbour_distances: typing.Optional[NeighbourDistances] = None,
                  error_vector: typing.Optional[ErrorVector] = None) -> None:
        if self.point_to_plane:
            self.value = np.square(error_vector.value)      # stays a device column when it is one
        else:
            self.value = neighbour_distances.value          # the search's own d2, verbatim


class _BoundaryPick(SecondaryMetric):
    _slot = 0

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"boundary_metric": BoundarySqrtDistances()}

    def calculate(self, boundary_metric: BoundarySqrtDistances) -> None:
        self.value = boundary_metric.value[self._slot]


class MinSqrtDistance(_BoundaryPick):                            # metric.py:191-199
    _slot = 0


class MaxSqrtDistance(_BoundaryPick):                            # metric.py:202-210
    _slot = 1


class _OverEuclidean(SecondaryMetric, PointToPlaneable):
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"euclidean_distance": EuclideanDistance(is_left=self.is_left, point_to_plane=self.point_to_plane)}


class GeoMSE(_OverEuclidean):                                    # metric.py:213-228
    _pccm_waits = True      # reads a reduction back from the GPU: the calculator evaluates these last
    def calculate(self, euclidean_distance: EuclideanDistance) -> None:
        column = euclidean_distance.value
        self.value = _column_sum(column) / column.shape[0]


class GeoHausdorffDistance(_OverEuclidean):                      # metric.py:353-366 (a SQUARED distance)
    _pccm_waits = True      # reads a reduction back from the GPU: the calculator evaluates these last
    def calculate(self, euclidean_distance: EuclideanDistance) -> None:
        self.value = _column_max(euclidean_distance.value)


def rank_index(rank: float, n: int) -> int:
    """Nearest-rank index of ``rank`` in (0, 1] over ``n`` points: k = max(1, ceil(R * n)), 1-based, where R is the decimal
    number ``repr(float(rank))`` spells, taken as an exact fraction -- the number the user typed, not the binary double next to
    it (ceil(0.07 * 100) is 8 in fp64 and 7 here)."""
    return max(1, math.ceil(fractions.Fraction(repr(float(rank))) * int(n)))


class GeoRankedHausdorffDistance(_OverEuclidean):                # no counterpart in the reference (options.py: hausdorff_rank)
    """Ranked (generalized) Hausdorff distance of one direction (Javaheri et al., QoMEX 2020; INTEGRATION.md, "Ranked
    Hausdorff"): the rank_index(rank, n)-th smallest element of the column GeoHausdorffDistance takes the maximum of -- a
    SQUARED distance like it, and equal to it bit for bit at rank 1."""
    _pccm_waits = True      # reads a selection back from the GPU: the calculator evaluates these last

    def __init__(self, is_left: bool, point_to_plane: bool, rank: float):
        super().__init__(is_left, point_to_plane)
        self.rank = float(rank)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.point_to_plane, self.rank)

    def _pccm_request(self):
        return "ranked", self.is_left, self.point_to_plane, self.rank

    def calculate(self, euclidean_distance: EuclideanDistance) -> None:
        column = euclidean_distance.value
        k = rank_index(self.rank, column.shape[0])
        ranked = getattr(column, "ranked", None)              # a device column: selected in HBM
        self.value = ranked(k) if ranked is not None else np.partition(np.asarray(column), k - 1)[k - 1]


class GeoInlierRatio(SecondaryMetric, DirectionalMetric):        # no counterpart in the reference (options.py: fscore)
    """The share of one cloud's points that lie within ``threshold`` of the other cloud ("F-score"): the number
    of elements of the D1 column -- squared distances -- that are <= threshold * threshold, over the number of points.  Left
    (origin -> processed) is the recall (completeness) of the processed cloud, right its precision (accuracy)."""
    _pccm_waits = True      # reads a count back from the GPU: the calculator evaluates these last

    def __init__(self, is_left: bool, threshold: float):
        super().__init__(is_left)
        self.threshold = float(threshold)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.threshold)

    def _pccm_request(self):
        return "within", self.is_left, self.threshold

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"euclidean_distance": EuclideanDistance(is_left=self.is_left, point_to_plane=False)}

    def calculate(self, euclidean_distance: EuclideanDistance) -> None:
        column = euclidean_distance.value
        t2 = np.float64(self.threshold) * np.float64(self.threshold)
        count_le = getattr(column, "count_le", None)          # a device column: counted in HBM
        count = count_le(t2) if count_le is not None else np.count_nonzero(np.asarray(column) <= t2)
        self.value = np.float64(count) / np.float64(column.shape[0])


class GeoFScore(SecondaryMetric):                                # no counterpart in the reference (options.py: fscore)
    """F-score at a distance threshold: the harmonic mean of precision (right) and recall (left), 0 when both are 0."""
    def __init__(self, threshold: float):
        self.threshold = float(threshold)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.threshold)

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"precision": GeoInlierRatio(is_left=False, threshold=self.threshold),
                "recall": GeoInlierRatio(is_left=True, threshold=self.threshold)}

    def calculate(self, precision: GeoInlierRatio, recall: GeoInlierRatio) -> None:
        p, r = np.float64(precision.value), np.float64(recall.value)
        self.value = np.float64(0.0) if p + r == 0.0 else ((2.0 * p) * r) / (p + r)


def _mapped_sum(column, root: bool, clamp):
    """np.sum(f(column)), f = np.minimum(., clamp) (when given), then np.sqrt (when ``root``): in HBM for a device column."""
    mapped = getattr(column, "mapped", None)
    if mapped is not None:
        return mapped(root=root, clamp=clamp)[0]
    f = np.asarray(column, dtype=np.float64)
    if clamp is not None:
        f = np.minimum(f, clamp)
    return np.sum(np.sqrt(f) if root else f)


class GeoMeanDistance(_OverEuclidean):                           # no counterpart in the reference (options.py: chamfer)
    """The mean UNSQUARED nearest-neighbour distance of one direction ("Chamfer and truncated distances"):
    np.sum(np.sqrt(column)) / n over the D1 column, or -- point_to_plane -- over the D2 column, where the root of the squared
    projection is its magnitude."""
    _pccm_waits = True      # reads a mapped reduction back from the GPU: the calculator evaluates these last

    def _pccm_request(self):
        return "mapped", self.is_left, self.point_to_plane, True, None

    def calculate(self, euclidean_distance: EuclideanDistance) -> None:
        column = euclidean_distance.value
        self.value = _mapped_sum(column, True, None) / column.shape[0]


class GeoChamferL1(SecondaryMetric):                             # no counterpart in the reference (options.py: chamfer)
    """Chamfer-L1 in PCN's convention (Yuan et al., 3DV 2018): the average of the two directions' mean unsquared distances."""
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"left": GeoMeanDistance(is_left=True, point_to_plane=False), "right": GeoMeanDistance(is_left=False, point_to_plane=False)}

    def calculate(self, left: GeoMeanDistance, right: GeoMeanDistance) -> None:
        self.value = (np.float64(left.value) + np.float64(right.value)) / np.float64(2)


class GeoChamferL2(SecondaryMetric):                             # no counterpart in the reference (options.py: chamfer)
    """Chamfer-L2: the sum of the two directions' mean squared distances, the report's GeoMSE rows (D1)."""
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"left": GeoMSE(is_left=True, point_to_plane=False), "right": GeoMSE(is_left=False, point_to_plane=False)}

    def calculate(self, left: GeoMSE, right: GeoMSE) -> None:
        self.value = np.float64(left.value) + np.float64(right.value)


class GeoTruncatedMSE(SecondaryMetric, DirectionalMetric):       # no counterpart in the reference (options.py: truncate)
    """The mean squared nearest-neighbour distance of one direction with every distance clipped at ``threshold``:
    np.sum(np.minimum(column, threshold * threshold)) / n over the D1 column -- the remedy for partly overlapping clouds, whose
    points without a counterpart otherwise dominate the mean."""
    _pccm_waits = True      # reads a mapped reduction back from the GPU: the calculator evaluates these last
    _root = False

    def __init__(self, is_left: bool, threshold: float):
        super().__init__(is_left)
        self.threshold = float(threshold)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.threshold)

    def _cap(self):
        return np.float64(self.threshold) * np.float64(self.threshold)

    def _pccm_request(self):
        return "mapped", self.is_left, False, self._root, float(self._cap())

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"euclidean_distance": EuclideanDistance(is_left=self.is_left, point_to_plane=False)}

    def calculate(self, euclidean_distance: EuclideanDistance) -> None:
        column = euclidean_distance.value
        self.value = _mapped_sum(column, self._root, self._cap()) / column.shape[0]


class GeoTruncatedMeanDistance(GeoTruncatedMSE):                 # no counterpart in the reference (options.py: chamfer + truncate)
    """... and the mean unsquared distance clipped at ``threshold``: np.sum(np.sqrt(np.minimum(column, threshold * threshold))) / n."""
    _root = True


class GeoDensityAwareDistance(SecondaryMetric, DirectionalMetric):   # no counterpart in the reference (options.py: dcd)
    """One direction of the density-aware Chamfer distance (Wu et al., NeurIPS 2021; INTEGRATION.md, "Density-aware Chamfer
    distance"): the mean over the iterating cloud's points of 1 - exp(-alpha * s) / m, s the distance to the matched point
    (``squared``: its square) and m the number of points that share that matched point.  In [0, 1]; at alpha = 0 it is
    1 - (distinct matched rows) / n."""
    _pccm_waits = True      # reads a mapped reduction back from the GPU: the calculator evaluates these last

    def __init__(self, is_left: bool, alpha: float, squared: bool = False):
        super().__init__(is_left)
        self.alpha = float(alpha) + 0.0
        self.squared = bool(squared)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.alpha, self.squared)

    def _pccm_request(self):
        return "density", self.is_left, self.alpha, self.squared

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"euclidean_distance": EuclideanDistance(is_left=self.is_left, point_to_plane=False),
                "matched_rows": MatchedRows(is_left=self.is_left)}

    def calculate(self, euclidean_distance: EuclideanDistance, matched_rows: MatchedRows) -> None:
        column = euclidean_distance.value
        density = getattr(column, "density", None)            # a device column: counted, gathered and summed in HBM
        if density is not None:
            total = density(self.alpha, self.squared)[0]
        else:
            d2 = np.asarray(column, dtype=np.float64)
            idx = np.asarray(matched_rows.value)
            m = np.bincount(idx)
            s = d2 if self.squared else np.sqrt(d2)
            total = np.sum(1.0 - np.exp(-np.float64(self.alpha) * s) / m[idx].astype(np.float64))
        self.value = total / column.shape[0]


class GeoDensityAwareChamfer(SecondaryMetric):                   # no counterpart in the reference (options.py: dcd)
    """The density-aware Chamfer distance: the average of the two directions' rows."""
    def __init__(self, alpha: float, squared: bool = False):
        self.alpha = float(alpha) + 0.0
        self.squared = bool(squared)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.alpha, self.squared)

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"left": GeoDensityAwareDistance(is_left=True, alpha=self.alpha, squared=self.squared),
                "right": GeoDensityAwareDistance(is_left=False, alpha=self.alpha, squared=self.squared)}

    def calculate(self, left: GeoDensityAwareDistance, right: GeoDensityAwareDistance) -> None:
        self.value = (np.float64(left.value) + np.float64(right.value)) / np.float64(2)


class _AlignmentRow(PrimaryMetric):                              # no counterpart in the reference (options.py: align)
    """A number of the registration that moved the processed cloud (``CloudPair(align="icp")``, align.py), as it stood at ICP's
    last search."""
    _field = ""

    def calculate(self, cloud_pair: CloudPair) -> None:
        alignment = getattr(cloud_pair, "alignment", None)
        value = None if alignment is None else getattr(alignment, self._field)
        if value is None:
            raise ValueError(f"{type(self).__name__}: the pair was not aligned (CloudPair(align='icp'))")
        self.value = np.float64(value)


class AlignmentFitness(_AlignmentRow):
    """The share of the processed cloud's points within ``align_distance`` of the original (1.0 without a distance)."""
    _field = "fitness"


class AlignmentRMSE(_AlignmentRow):
    """The root mean squared distance of those points to their nearest points of the original."""
    _field = "inlier_rmse"


class VoxelCounts(PrimaryMetric):                                # no counterpart in the reference (options.py: occupancy)
    """(nA, nB, nAB): the voxels of edge ``voxel`` on the absolute lattice floor(coordinate / voxel) that the original cloud
    occupies, that the processed cloud occupies, and that both do ("Voxel occupancy") -- Python ints, counted on
    the GPU's voxel table (CloudPair.voxel_occupancy)."""
    _pccm_waits = True      # reads counts back from the GPU: the calculator evaluates these last

    def __init__(self, voxel: float):
        self.voxel = float(voxel)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.voxel)

    def _pccm_request(self):
        return "occupancy", self.voxel

    def calculate(self, cloud_pair: CloudPair) -> None:
        n_a, n_b, n_ab = cloud_pair.voxel_occupancy(self.voxel)
        self.value = (int(n_a), int(n_b), int(n_ab))


class _OverVoxelCounts(SecondaryMetric):
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"voxel_counts": VoxelCounts(voxel=self.voxel)}


class OccupiedVoxels(_OverVoxelCounts, DirectionalMetric):
    """The number of voxels a cloud occupies: the original's (left), the processed cloud's (right)."""
    def __init__(self, is_left: bool, voxel: float):
        super().__init__(is_left)
        self.voxel = float(voxel)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.voxel)

    def calculate(self, voxel_counts: VoxelCounts) -> None:
        n_a, n_b, _ = voxel_counts.value
        self.value = np.float64(n_a if self.is_left else n_b)


class VoxelCoverage(OccupiedVoxels):
    """The share of a cloud's voxels that the other cloud occupies too.  Left: of the original's voxels, those the processed
    cloud reproduced (voxel recall); right: of the processed cloud's voxels, those the original has (voxel precision)."""
    def calculate(self, voxel_counts: VoxelCounts) -> None:
        n_a, n_b, n_ab = voxel_counts.value
        self.value = np.float64(n_ab) / np.float64(n_a if self.is_left else n_b)


class VoxelIoU(_OverVoxelCounts):
    """Intersection over union of the two clouds' occupied voxels (no symmetric row: this is it)."""
    def __init__(self, voxel: float):
        self.voxel = float(voxel)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.voxel)

    def calculate(self, voxel_counts: VoxelCounts) -> None:
        n_a, n_b, n_ab = voxel_counts.value
        self.value = np.float64(n_ab) / np.float64(n_a + n_b - n_ab)


class _OverAngular(SecondaryMetric, DirectionalMetric):
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"angular_similarities": AngularSimilarities(is_left=self.is_left)}


class AngularSimilarity(_OverAngular):
    """Plane-to-plane similarity of one direction: the mean of the per-point values (sum / n, NumPy's pairwise sum)."""
    _pccm_waits = True      # reads a reduction back from the GPU: the calculator evaluates these last
    def calculate(self, angular_similarities: AngularSimilarities) -> None:
        column = angular_similarities.value
        self.value = _column_sum(column) / column.shape[0]


class MinAngularSimilarity(_OverAngular):
    """The worst point of one direction (reported with hausdorff)."""
    _pccm_waits = True      # reads a reduction back from the GPU: the calculator evaluates these last
    def calculate(self, angular_similarities: AngularSimilarities) -> None:
        self.value = _column_min(angular_similarities.value)


class _PointSSIM(SecondaryMetric, DirectionalMetric):
    """PointSSIM of one attribute and direction (Alexiou & Ebrahimi, ICME Workshops 2020; INTEGRATION.md, "PointSSIM"): the
    mean of the per-point similarities (sum / n, NumPy's pairwise sum)."""
    attribute: str
    _pccm_waits = True      # reads a reduction back from the GPU: the calculator evaluates these last

    def __init__(self, is_left: bool, k: int = 12):
        super().__init__(is_left)
        self.k = int(k)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.k)

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"ssim_similarities": SSIMSimilarities(is_left=self.is_left, attribute=self.attribute, k=self.k)}

    def calculate(self, ssim_similarities: SSIMSimilarities) -> None:
        column = ssim_similarities.value
        self.value = _column_sum(column) / column.shape[0]


class GeometrySSIM(_PointSSIM):
    """Variance of the distances to the k - 1 nearest other points."""
    attribute = "geometry"


class NormalSSIM(_PointSSIM):
    """Variance of the angular similarities of the normals of the k - 1 nearest other points with the point's own."""
    attribute = "normal"


class CurvatureSSIM(_PointSSIM):
    """Variance of the curvatures (smallest eigenvalue / trace of the k-NN covariance) over the neighbourhood."""
    attribute = "curvature"


class ColorSSIM(_PointSSIM):
    """Variance of the luma (BT.709 "ycc" Y) over the neighbourhood."""
    attribute = "color"


class _OverMahalanobis(SecondaryMetric, DirectionalMetric):
    _pccm_waits = True      # reads a reduction back from the GPU: the calculator evaluates these last

    def __init__(self, is_left: bool, k: int = 30):
        super().__init__(is_left)
        self.k = int(k)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.k)

    _primary = MahalanobisDistances      # (the colour and joint rows pool their own columns the same way)

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"mahalanobis_distances": self._primary(is_left=self.is_left, k=self.k)}


class MahalanobisDistance(_OverMahalanobis):
    """Point-to-distribution metric of one direction (after Javaheri et al., IEEE SPL 2020): the mean of the per-point
    Mahalanobis distances (sum / n, NumPy's pairwise sum).  Dimensionless; inf when a point's neighbourhood is one location the
    point is not at."""
    def calculate(self, mahalanobis_distances: MahalanobisDistances) -> None:
        column = mahalanobis_distances.value
        self.value = _column_sum(column) / column.shape[0]


class MaxMahalanobisDistance(_OverMahalanobis):
    """The worst point of one direction (reported with hausdorff)."""
    def calculate(self, mahalanobis_distances: MahalanobisDistances) -> None:
        self.value = _column_max(mahalanobis_distances.value)


class ColorMahalanobisDistance(MahalanobisDistance):
    """Colour point-to-distribution metric of one direction (after Javaheri et al., IEEE MMSP 2021): the mean of the per-point
    luma distances.  Dimensionless and always finite."""
    _primary = ColorMahalanobisDistances


class MaxColorMahalanobisDistance(MaxMahalanobisDistance):
    _primary = ColorMahalanobisDistances


class JointMahalanobisDistance(MahalanobisDistance):
    """Joint geometry-and-colour point-to-distribution metric of one direction: the mean of sqrt(M_G^2 + M_Y^2); inf where
    MahalanobisDistance is."""
    _primary = JointMahalanobisDistances


class MaxJointMahalanobisDistance(MaxMahalanobisDistance):
    _primary = JointMahalanobisDistances


SSIM_CLASSES = {"geometry": GeometrySSIM, "normal": NormalSSIM, "curvature": CurvatureSSIM, "color": ColorSSIM}


def _peak_of(cloud_extent):
    """np.max(cloud_extent.value), evaluated once per extent array (a report asks for it four times)."""
    extent = cloud_extent.value
    memo = cloud_extent.__dict__.get("_peak_memo")
    if memo is None or memo[0] is not extent:
        memo = cloud_extent._peak_memo = (extent, np.max(extent))
    return memo[1]


def _psnr(peak, distortion):
    return 10 * np.log10(peak ** 2 / distortion)                 # metric.py:247, 350, 384-386, 443


class GeoPSNR(SecondaryMetric, PointToPlaneable):                # metric.py:231-247
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"cloud_extent": CloudExtent(),
                "geo_mse": GeoMSE(is_left=self.is_left, point_to_plane=self.point_to_plane)}

    def calculate(self, cloud_extent: CloudExtent, geo_mse: GeoMSE) -> None:
        self.value = _psnr(_peak_of(cloud_extent), geo_mse.value)


class GeoHausdorffDistancePSNR(SecondaryMetric, PointToPlaneable):   # metric.py:369-386
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"max_sqrt": MaxSqrtDistance(),
                "hausdorff_distance": GeoHausdorffDistance(is_left=self.is_left,
                                                           point_to_plane=self.point_to_plane)}

    def calculate(self, max_sqrt: MaxSqrtDistance, hausdorff_distance: GeoHausdorffDistance) -> None:
        self.value = _psnr(max_sqrt.value, hausdorff_distance.value)


class GeoRankedHausdorffDistancePSNR(SecondaryMetric, PointToPlaneable):
    """GeoHausdorffDistancePSNR's expression (metric.py:369-386) with the ranked value."""
    def __init__(self, is_left: bool, point_to_plane: bool, rank: float):
        super().__init__(is_left, point_to_plane)
        self.rank = float(rank)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.point_to_plane, self.rank)

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"max_sqrt": MaxSqrtDistance(),
                "ranked_distance": GeoRankedHausdorffDistance(is_left=self.is_left, point_to_plane=self.point_to_plane,
                                                              rank=self.rank)}

    def calculate(self, max_sqrt: MaxSqrtDistance, ranked_distance: GeoRankedHausdorffDistance) -> None:
        self.value = _psnr(max_sqrt.value, ranked_distance.value)


class IntrinsicResolution(SecondaryMetric, DirectionalMetric):   # no counterpart in the reference (options.py: resolution_psnr)
    """Intrinsic resolution of one cloud (after Javaheri et al., ICIP 2020): the mean of its point spacings (sum / n, NumPy's
    pairwise sum).  A property of the cloud, not a comparison: left is the origin cloud, right the reconstructed one."""
    _pccm_waits = True      # reads a reduction back from the GPU: the calculator evaluates these last

    def __init__(self, is_left: bool, k: int = 10):
        super().__init__(is_left)
        self.k = int(k)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.k)

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"point_spacings": PointSpacings(is_left=self.is_left, k=self.k)}

    def calculate(self, point_spacings: PointSpacings) -> None:
        column = point_spacings.value
        self.value = _column_sum(column) / column.shape[0]


class _ResolutionPSNR(SecondaryMetric, PointToPlaneable):
    """A PSNR whose peak is the ORIGIN cloud's intrinsic resolution over k neighbours, for both sides (as GeoPSNR always takes
    the origin's extent): no dependency reaches CloudExtent or MaxSqrtDistance."""
    def __init__(self, is_left: bool, point_to_plane: bool, k: int = 10):
        super().__init__(is_left, point_to_plane)
        self.k = int(k)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.point_to_plane, self.k)


class GeoResolutionPSNR(_ResolutionPSNR):
    """GeoPSNR's expression (metric.py:231-247) with the origin cloud's intrinsic resolution as the peak."""
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"resolution": IntrinsicResolution(is_left=True, k=self.k),
                "geo_mse": GeoMSE(is_left=self.is_left, point_to_plane=self.point_to_plane)}

    def calculate(self, resolution: IntrinsicResolution, geo_mse: GeoMSE) -> None:
        self.value = _psnr(resolution.value, geo_mse.value)


class GeoHausdorffResolutionPSNR(_ResolutionPSNR):
    """GeoHausdorffDistancePSNR's expression (metric.py:369-386) with the origin cloud's intrinsic resolution as the peak."""
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"resolution": IntrinsicResolution(is_left=True, k=self.k),
                "hausdorff_distance": GeoHausdorffDistance(is_left=self.is_left, point_to_plane=self.point_to_plane)}

    def calculate(self, resolution: IntrinsicResolution, hausdorff_distance: GeoHausdorffDistance) -> None:
        self.value = _psnr(resolution.value, hausdorff_distance.value)


# --------------------------------------------------------------------------- reflectance secondaries
class _OverReflectance(SecondaryMetric, DirectionalMetric):
    _pccm_waits = True      # reads a reduction back from the GPU: the calculator evaluates these last

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"reflectance_errors": ReflectanceErrors(is_left=self.is_left)}


class ReflectanceMSE(_OverReflectance):                          # no counterpart in the reference (options.py: reflectance)
    """Reflectance MSE of one direction, as MPEG's pc_error reports beside D1 / D2: the mean of the per-point squared
    differences (sum / n, NumPy's pairwise sum), in the units of the values as given."""
    def calculate(self, reflectance_errors: ReflectanceErrors) -> None:
        column = reflectance_errors.value
        self.value = _column_sum(column) / column.shape[0]


class ReflectanceHausdorffDistance(_OverReflectance):
    """The worst point of one direction (reported with hausdorff): a SQUARED difference, like GeoHausdorffDistance."""
    def calculate(self, reflectance_errors: ReflectanceErrors) -> None:
        self.value = _column_max(reflectance_errors.value)


def _reflectance_psnr(peak: float, distortion):
    """_psnr on float64 operands: identical columns give 0 / inf the way NumPy does, without its divide warning."""
    with np.errstate(divide="ignore"):
        return _psnr(np.float64(peak), np.float64(distortion))


class _ReflectancePSNR(SecondaryMetric, DirectionalMetric):
    """A PSNR whose peak is given (options.py: reflectance_peak; 65535.0 is the full 16-bit range pc_error uses)."""
    _distortion = ReflectanceMSE

    def __init__(self, is_left: bool, peak: float = 65535.0):
        super().__init__(is_left)
        self.peak = float(peak)

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.peak)

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"distortion": self._distortion(is_left=self.is_left)}

    def calculate(self, distortion: AbstractMetric) -> None:
        self.value = _reflectance_psnr(self.peak, distortion.value)


class ReflectancePSNR(_ReflectancePSNR):
    """GeoPSNR's expression (metric.py:231-247) with the reflectance peak and ReflectanceMSE."""


class ReflectanceHausdorffDistancePSNR(_ReflectancePSNR):
    """GeoHausdorffDistancePSNR's expression (metric.py:369-386) with the reflectance peak and ReflectanceHausdorffDistance."""
    _distortion = ReflectanceHausdorffDistance


# --------------------------------------------------------------------------- colour secondaries
class ColorMetric(DirectionalMetric):                            # metric.py:250-258
    color_scheme: str

    def __init__(self, is_left: bool, color_scheme: str):
        super().__init__(is_left)
        self.color_scheme = color_scheme

    def _key(self) -> typing.Tuple:
        return (type(self).__name__, self.is_left, self.color_scheme)


_FROM_RGB = {                                                    # metric.py:270-281
    "ycc": np.array([[0.2126, 0.7152, 0.0722], [-0.1146, -0.3854, 0.5], [0.5, -0.4542, -0.0458]]),
    "yuv": np.array([[0.25, 0.5, 0.25], [1, 0, -1], [-0.5, 1, -0.5]]),
}
_PEAKS = {"rgb": 255.0, "ycc": 1.0, "yuv": 1.0}                  # metric.py:293-299


def transform_colors(colors: np.ndarray, source_scheme: str, target_scheme: str) -> np.ndarray:
    """metric.py:261-290: rows are mapped by the 3x3 matrix of the target scheme."""
    if source_scheme == target_scheme:
        return colors
    if source_scheme != "rgb" or target_scheme not in _FROM_RGB:
        raise TypeError(f"no transform from {source_scheme!r} to {target_scheme!r}")   # the reference fails here too
    colors = np.asarray(colors)
    if not len(colors):
        return colors
    from . import _native
    return _native.color_transform(colors, target_scheme)      # == np.matmul(matrix, row) for every row, in C


def get_color_peak(color_scheme: str) -> np.float64:
    return _PEAKS[color_scheme]


class _ColorPairMetric(SecondaryMetric, ColorMetric):
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"origin_cloud_colors": CloudColors(is_left=self.is_left),
                "neighbour_cloud_colors": NeighbourColors(is_left=self.is_left)}

    def _difference(self, origin_cloud_colors, neighbour_cloud_colors) -> np.ndarray:
        own_rows, other_rows = origin_cloud_colors.value, neighbour_cloud_colors.value
        pair_of = getattr(other_rows, "_pair", None)
        if (pair_of is not None and hasattr(other_rows, "in_scheme")
                and getattr(own_rows, "_pccm_origin", None) == (id(pair_of), 0 if self.is_left else 1)):
            if self.color_scheme not in _PEAKS:
                raise TypeError(f"no transform from 'rgb' to {self.color_scheme!r}")
            return other_rows.in_scheme(self.color_scheme)      # gather, transform and subtract on the GPU
        own = transform_colors(np.copy(origin_cloud_colors.value), "rgb", self.color_scheme)
        other = transform_colors(np.copy(neighbour_cloud_colors.value), "rgb", self.color_scheme)
        return np.subtract(own, other)


class ColorMSE(_ColorPairMetric):                                # metric.py:302-333
    _pccm_waits = True      # reads a reduction back from the GPU: the calculator evaluates these last
    def calculate(self, origin_cloud_colors: CloudColors, neighbour_cloud_colors: NeighbourColors) -> None:
        diff = self._difference(origin_cloud_colors, neighbour_cloud_colors)
        self.value = np.mean(diff ** 2, axis=0)


class ColorHausdorffDistance(_ColorPairMetric):                  # metric.py:389-427
    _pccm_waits = True      # reads a reduction back from the GPU: the calculator evaluates these last
    def calculate(self, origin_cloud_colors: CloudColors, neighbour_cloud_colors: NeighbourColors) -> None:
        diff = self._difference(origin_cloud_colors, neighbour_cloud_colors)
        if self.color_scheme == "rgb":
            diff = 255 * diff                                    # metric.py:422-425
        self.value = np.max(diff ** 2, axis=0)


class ColorPSNR(SecondaryMetric, ColorMetric):                   # metric.py:336-350
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"color_mse": ColorMSE(is_left=self.is_left, color_scheme=self.color_scheme)}

    def calculate(self, color_mse: ColorMSE) -> None:
        self.value = _psnr(get_color_peak(self.color_scheme), color_mse.value)


class ColorHausdorffDistancePSNR(SecondaryMetric, ColorMetric):  # metric.py:430-443
    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"hausdorff_distance": ColorHausdorffDistance(is_left=self.is_left,
                                                             color_scheme=self.color_scheme)}

    def calculate(self, hausdorff_distance: ColorHausdorffDistance) -> None:
        self.value = _psnr(get_color_peak(self.color_scheme), hausdorff_distance.value)


# --------------------------------------------------------------------------- symmetric
class SymmetricMetric(SecondaryMetric):                          # metric.py:446-485
    is_proportional: bool
    metrics: typing.Sequence[DirectionalMetric]

    def __init__(self, metrics: typing.Sequence[DirectionalMetric], is_proportional: bool):
        if len(metrics) != 2:
            raise ValueError("Must be exactly two metrics")
        if type(metrics[0]) is not type(metrics[1]):
            raise ValueError(f"Metrics must be of same class, got: {type(metrics[0])}, {type(metrics[1])}")
        self.metrics = metrics
        self.is_proportional = is_proportional

    def _get_dependencies(self) -> typing.Dict[str, AbstractMetric]:
        return {"lmetric": self.metrics[0], "rmetric": self.metrics[1]}

    def _key(self) -> typing.Tuple:
        return (type(self).__name__,) + self.metrics[0]._key() + self.metrics[1]._key()

    def calculate(self, lmetric: AbstractMetric, rmetric: AbstractMetric) -> None:
        # quality-like metrics (PSNR) report the worse = smaller side, error-like the larger;
        # the left value wins ties in both cases (Python's min/max keep the first extreme).
        # (written out: min / max keep the first extreme, i.e. the right value replaces the left one only when it is strictly
        # smaller / larger -- with NaN keys nothing is, exactly as min([l, r], key=...) behaves)
        left, right = lmetric.value, rmetric.value
        kl, kr = _norm(left), _norm(right)
        if self.is_proportional:
            self.value = right if kr < kl else left
        else:
            self.value = right if kr > kl else left


def _norm(value):
    """np.linalg.norm(value), the reference's comparison key (metric.py:481-485).  For the scalar metrics that is
    sqrt(x . x) = sqrt(x * x) -- evaluated here without NumPy's dispatch, same bits; arrays go to NumPy."""
    if type(value) in (float, np.float64):
        v = float(value)
        return math.sqrt(v * v) if v == v else v
    return np.linalg.norm(value)
