"""Options -> ordered metric list; same order as ``open_pcc_metric.options.transform_options``.

Reference: open_pcc_metric/options.py:16-174.  The order of the returned list is the row order
of the CLI report, so it is part of the contract:

  always                 MinSqrt, MaxSqrt, GeoMSE L/R/sym, GeoPSNR L/R/sym          (options.py:35-56)
  color                  ColorMSE L/R/sym, ColorPSNR L/R/sym                        (options.py:58-82)
  point_to_plane         GeoMSE L/R/sym, GeoPSNR L/R/sym with point_to_plane=True   (options.py:84-104)
  hausdorff              Hausdorff L/R/sym, HausdorffPSNR L/R/sym (D1)              (options.py:106-138)
  hausdorff & p2plane    Hausdorff L/R, HausdorffPSNR L/R, then both symmetric rows (options.py:140-172)

and, with ``plane_to_plane`` (no counterpart in the reference: the angular similarity of Alexiou & Ebrahimi, ICME 2018), after
every row above:

  plane_to_plane         AngularSimilarity L/R/sym
  plane_to_plane & hd    MinAngularSimilarity L/R/sym

and, with ``point_ssim`` (no counterpart in the reference: PointSSIM, Alexiou & Ebrahimi, ICME Workshops 2020), after every row
above and in this order whatever order the caller gave:

  geometry               GeometrySSIM L/R/sym
  normal                 NormalSSIM L/R/sym
  curvature              CurvatureSSIM L/R/sym
  color                  ColorSSIM L/R/sym

and, with ``hausdorff_rank`` (no counterpart in the reference: the generalized Hausdorff distance of Javaheri et al., QoMEX 2020),
after every row above, for each rank in ascending order:

  rank r                 RankedHausdorff L/R/sym, RankedHausdorffPSNR L/R/sym (D1)
  rank r & p2plane       the same six with point_to_plane=True

and, with ``point_to_distribution`` (no counterpart in the reference: the Mahalanobis point-to-distribution metric of Javaheri et
al., IEEE SPL 2020), after every row above, ranked Hausdorff rows included:

  point_to_distribution        MahalanobisDistance L/R/sym
  point_to_distribution & hd   MaxMahalanobisDistance L/R/sym

and, with ``p2d_color`` (which needs ``point_to_distribution``; no counterpart in the reference: the joint geometry-and-colour
point-to-distribution metric after Javaheri et al., IEEE MMSP 2021), after every row above:

  p2d_color                    ColorMahalanobisDistance L/R/sym
  p2d_color                    JointMahalanobisDistance L/R/sym
  p2d_color & hd               MaxColorMahalanobisDistance L/R/sym
  p2d_color & hd               MaxJointMahalanobisDistance L/R/sym

and, with ``resolution_psnr`` (no counterpart in the reference: the resolution-adaptive PSNR after Javaheri et al., ICIP 2020,
whose peak is the origin cloud's intrinsic resolution over ``resolution_neighbours`` neighbours), after every row above:

  resolution_psnr              IntrinsicResolution L, R (the clouds' own resolutions: no symmetric row)
  resolution_psnr              GeoResolutionPSNR L/R/sym (D1)
  resolution_psnr & p2plane    GeoResolutionPSNR L/R/sym with point_to_plane=True
  resolution_psnr & hd         GeoHausdorffResolutionPSNR L/R/sym (D1)
  ... & hd & p2plane           GeoHausdorffResolutionPSNR L/R/sym with point_to_plane=True

and, with ``reflectance`` (no counterpart in the reference: the reflectance rows MPEG's ``pc_error`` reports for LiDAR content,
on the clouds' per-point scalars as given, PSNR against ``reflectance_peak``), after every row above:

  reflectance                  ReflectanceMSE L/R/sym, ReflectancePSNR L/R/sym
  reflectance & hd             ReflectanceHausdorffDistance L/R/sym, ReflectanceHausdorffDistancePSNR L/R/sym

and, with ``fscore`` (no counterpart in the reference: the F-score at a distance threshold of Knapitsch et al., "Tanks and
Temples", ACM TOG 2017, as the reconstruction and completion literature reports it beside the Chamfer distance), after every row
above, for each threshold in ascending order:

  threshold tau                GeoInlierRatio L (recall), GeoInlierRatio R (precision), GeoFScore (no symmetric row: the F-score is it)

and, with ``chamfer`` (no counterpart in the reference: the Chamfer distance of the reconstruction and completion literature, Fan
et al., CVPR 2017; Chamfer-L1 in the convention of PCN, Yuan et al., 3DV 2018), after every row above, F-score rows included:

  chamfer                      GeoMeanDistance L/R/sym (D1: the mean UNSQUARED nearest-neighbour distance)
  chamfer & p2plane            GeoMeanDistance L/R/sym with point_to_plane=True (the mean magnitude of the projection)
  chamfer                      GeoChamferL1 ((L + R) / 2 of the D1 sides), GeoChamferL2 (GeoMSE L + GeoMSE R, D1)

and, with ``truncate`` (no counterpart in the reference: the truncated -- clipped -- mean for partly overlapping clouds, whose
points without a counterpart otherwise dominate every mean), after every row above, for each threshold in ascending order:

  threshold tau                GeoTruncatedMSE L/R/sym (D1: the mean of min(d^2, tau^2))
  threshold tau & chamfer      GeoTruncatedMeanDistance L/R/sym (D1: the mean of min(d, tau))

and, with ``dcd`` (no counterpart in the reference: the density-aware Chamfer distance of Wu et al., NeurIPS 2021 -- every point's
term 1 - exp(-alpha d) / m, m the number of points that share its matched point; ``dcd_squared`` puts d^2 in d's place), after
every row above, truncated rows included, for each alpha in ascending order:

  alpha                        GeoDensityAwareDistance L, GeoDensityAwareDistance R, GeoDensityAwareChamfer ((L + R) / 2; no symmetric row)

and, with ``align`` (no counterpart in the reference: the pair was registered by ``CloudPair(align="icp")``, align.py), after
every row above:

  align                        AlignmentFitness (inliers / points of the processed cloud), AlignmentRMSE (of the inliers)

and, with ``occupancy`` (no counterpart in the reference: the voxel-occupancy numbers of the reconstruction and learned-codec
literature -- 3D-R2N2, occupancy networks -- on the absolute lattice floor(coordinate / voxel); no nearest-neighbour search),
after every row above, alignment rows included, for each voxel size in ascending order:

  voxel v                      OccupiedVoxels L, R (the clouds' occupied voxels)
  voxel v                      VoxelCoverage L (shared / original's voxels: recall), VoxelCoverage R (shared / processed's: precision)
  voxel v                      VoxelIoU (shared / union; no symmetric row: the IoU is it)

``CloudPair(..., duplicates=)`` / ``--duplicates`` (``check_duplicates`` below) merges duplicate points before any of this: it
changes which rows the clouds have, never which report rows there are or their order.
"""
from __future__ import annotations

import typing

import math
import numbers

from .metric import (SSIM_CLASSES, AbstractMetric, AlignmentFitness, AlignmentRMSE, AngularSimilarity, ColorMahalanobisDistance, ColorMSE, ColorPSNR,
                     GeoChamferL1, GeoChamferL2, GeoDensityAwareChamfer, GeoDensityAwareDistance, GeoMeanDistance, GeoTruncatedMeanDistance, GeoTruncatedMSE, GeoFScore, GeoInlierRatio, GeoHausdorffDistance, GeoHausdorffDistancePSNR, GeoHausdorffResolutionPSNR, GeoMSE, GeoPSNR,
                     GeoRankedHausdorffDistance, GeoRankedHausdorffDistancePSNR, GeoResolutionPSNR, IntrinsicResolution,
                     JointMahalanobisDistance, MahalanobisDistance, MaxColorMahalanobisDistance,
                     MaxJointMahalanobisDistance, MaxMahalanobisDistance, MaxSqrtDistance, MinAngularSimilarity, MinSqrtDistance,
                     OccupiedVoxels, ReflectanceHausdorffDistance, ReflectanceHausdorffDistancePSNR, ReflectanceMSE, ReflectancePSNR,
                     SymmetricMetric, VoxelCoverage, VoxelIoU)

SSIM_ATTRIBUTES = ("geometry", "normal", "curvature", "color")     # the row order of transform_options
SSIM_MIN_K, SSIM_MAX_K = 2, 64
MAX_HAUSDORFF_RANKS = 4
MAX_FSCORE_THRESHOLDS = 4
MAX_TRUNCATE_THRESHOLDS = 4
MAX_DCD_ALPHAS = 4
MAX_OCCUPANCY_VOXELS = 4
P2D_MIN_K, P2D_MAX_K = 4, 64
RESOLUTION_MIN_K, RESOLUTION_MAX_K = 1, 63


def _hausdorff_ranks(value) -> typing.Tuple[float, ...]:
    """``hausdorff_rank`` as a sorted tuple of distinct floats in (0, 1]; ValueError for anything else."""
    if value is None:
        return ()
    if isinstance(value, (str, bytes)):
        raise ValueError(f"hausdorff_rank must be a number or an iterable of numbers in (0, 1], not {value!r}")
    items = [value] if isinstance(value, numbers.Real) else list(value) if hasattr(value, "__iter__") else [value]
    ranks = set()
    for r in items:
        if isinstance(r, (bool,)) or type(r).__name__ == "bool_" or not isinstance(r, numbers.Real):
            raise ValueError(f"hausdorff_rank: {r!r} is not a number in (0, 1]")
        f = float(r)
        if math.isnan(f) or not 0.0 < f <= 1.0:
            raise ValueError(f"hausdorff_rank: {r!r} is not in (0, 1]")
        ranks.add(f)
    if len(ranks) > MAX_HAUSDORFF_RANKS:
        raise ValueError(f"hausdorff_rank: at most {MAX_HAUSDORFF_RANKS} ranks per report, not {len(ranks)}")
    return tuple(sorted(ranks))


def _distance_thresholds(value, name: str, most: int) -> typing.Tuple[float, ...]:
    """A distance-threshold option (``fscore``, ``truncate``; the alphas of ``dcd`` obey the same rules) as a sorted tuple of distinct finite floats >= 0; ValueError for
    anything else."""
    if value is None:
        return ()
    if isinstance(value, (str, bytes)):
        raise ValueError(f"{name} must be a number or an iterable of numbers >= 0, not {value!r}")
    items = [value] if isinstance(value, numbers.Real) else list(value) if hasattr(value, "__iter__") else [value]
    thresholds = set()
    for t in items:
        if isinstance(t, (bool,)) or type(t).__name__ == "bool_" or not isinstance(t, numbers.Real):
            raise ValueError(f"{name}: {t!r} is not a finite number >= 0")
        f = float(t)
        if not math.isfinite(f) or f < 0.0:
            raise ValueError(f"{name}: {t!r} is not a finite number >= 0")
        thresholds.add(f + 0.0)                               # (-0.0 is the threshold 0.0)
    if len(thresholds) > most:
        raise ValueError(f"{name}: at most {most} thresholds per report, not {len(thresholds)}")
    return tuple(sorted(thresholds))


def _occupancy_voxels(value) -> typing.Tuple[float, ...]:
    """``occupancy`` as a sorted tuple of distinct finite floats > 0 (voxel sizes in the clouds' units); ValueError for anything
    else."""
    if value is None:
        return ()
    if isinstance(value, (str, bytes)):
        raise ValueError(f"occupancy must be a number or an iterable of numbers > 0, not {value!r}")
    items = [value] if isinstance(value, numbers.Real) else list(value) if hasattr(value, "__iter__") else [value]
    voxels = set()
    for v in items:
        if isinstance(v, (bool,)) or type(v).__name__ == "bool_" or not isinstance(v, numbers.Real):
            raise ValueError(f"occupancy: {v!r} is not a finite number > 0")
        f = float(v)
        if not math.isfinite(f) or not f > 0.0:
            raise ValueError(f"occupancy: {v!r} is not a finite number > 0")
        voxels.add(f)
    if len(voxels) > MAX_OCCUPANCY_VOXELS:
        raise ValueError(f"occupancy: at most {MAX_OCCUPANCY_VOXELS} voxel sizes per report, not {len(voxels)}")
    return tuple(sorted(voxels))


def _fscore_thresholds(value) -> typing.Tuple[float, ...]:
    return _distance_thresholds(value, "fscore", MAX_FSCORE_THRESHOLDS)


def _truncate_thresholds(value) -> typing.Tuple[float, ...]:
    return _distance_thresholds(value, "truncate", MAX_TRUNCATE_THRESHOLDS)


class CalculateOptions:
    def __init__(self, color: typing.Optional[str] = None, hausdorff: bool = False,
                 point_to_plane: bool = False, plane_to_plane: bool = False,
                 point_ssim: typing.Optional[typing.Iterable[str]] = None, ssim_neighbours: int = 12,
                 hausdorff_rank=None, point_to_distribution: bool = False, p2d_neighbours: int = 30,
                 p2d_color: bool = False, resolution_psnr: bool = False, resolution_neighbours: int = 10,
                 reflectance: bool = False, reflectance_peak: float = 65535.0, fscore=None, chamfer: bool = False,
                 truncate=None, dcd=None, dcd_squared: bool = False, align=None, occupancy=None):
        self.color = color
        self.hausdorff = hausdorff
        self.point_to_plane = point_to_plane
        self.plane_to_plane = plane_to_plane
        if isinstance(point_ssim, str):
            point_ssim = (point_ssim,)
        wanted = set(point_ssim or ())
        unknown = sorted(str(a) for a in wanted - set(SSIM_ATTRIBUTES))
        if unknown:
            raise ValueError(f"unknown PointSSIM attribute(s) {', '.join(map(repr, unknown))}: "
                             f"choose from {', '.join(SSIM_ATTRIBUTES)}")
        if isinstance(ssim_neighbours, bool) or int(ssim_neighbours) != ssim_neighbours \
                or not SSIM_MIN_K <= int(ssim_neighbours) <= SSIM_MAX_K:
            raise ValueError(f"ssim_neighbours must be an integer in {SSIM_MIN_K}..{SSIM_MAX_K}, not {ssim_neighbours!r}")
        self.point_ssim = tuple(a for a in SSIM_ATTRIBUTES if a in wanted)
        self.ssim_neighbours = int(ssim_neighbours)
        self.hausdorff_rank = _hausdorff_ranks(hausdorff_rank)
        if isinstance(p2d_neighbours, bool) or type(p2d_neighbours).__name__ == "bool_" or not isinstance(p2d_neighbours, numbers.Real) \
                or int(p2d_neighbours) != p2d_neighbours or not P2D_MIN_K <= int(p2d_neighbours) <= P2D_MAX_K:
            raise ValueError(f"p2d_neighbours must be an integer in {P2D_MIN_K}..{P2D_MAX_K}, not {p2d_neighbours!r}")
        self.point_to_distribution = bool(point_to_distribution)
        self.p2d_neighbours = int(p2d_neighbours)
        if p2d_color and not self.point_to_distribution:
            raise ValueError("p2d_color adds rows to the point-to-distribution metric: it needs point_to_distribution=True")
        self.p2d_color = bool(p2d_color)
        k = resolution_neighbours
        if isinstance(k, bool) or type(k).__name__ == "bool_" or not isinstance(k, numbers.Real) \
                or not math.isfinite(k) or int(k) != k or not RESOLUTION_MIN_K <= int(k) <= RESOLUTION_MAX_K:
            raise ValueError(f"resolution_neighbours must be an integer in {RESOLUTION_MIN_K}..{RESOLUTION_MAX_K}, not {k!r}")
        self.resolution_psnr = bool(resolution_psnr)
        self.resolution_neighbours = int(k)
        peak = reflectance_peak
        if isinstance(peak, bool) or type(peak).__name__ == "bool_" or not isinstance(peak, numbers.Real) \
                or not math.isfinite(peak) or not peak > 0:
            raise ValueError(f"reflectance_peak must be a positive finite number, not {peak!r}")
        self.reflectance = bool(reflectance)
        self.reflectance_peak = float(peak)
        self.fscore = _fscore_thresholds(fscore)
        self.chamfer = bool(chamfer)
        self.truncate = _truncate_thresholds(truncate)
        self.dcd = _distance_thresholds(dcd, "dcd", MAX_DCD_ALPHAS)
        if dcd_squared and not self.dcd:
            raise ValueError("dcd_squared says what the density-aware Chamfer rows are fed: it needs dcd=")
        self.dcd_squared = bool(dcd_squared)
        # the pair was registered (CloudPair(align="icp")): AlignmentFitness and AlignmentRMSE after every other row
        if align is not None and (not isinstance(align, str) or align not in ("icp",)):
            raise ValueError('align must be None or "icp"')
        self.align = align
        self.occupancy = _occupancy_voxels(occupancy)


def check_point_ssim(options: CalculateOptions, origin_cloud, reconst_cloud, *, estimate_normals: bool = True,
                     ties: str = "pick", group=None) -> None:
    """Raise ``ValueError`` when the PointSSIM rows ``options`` asks for cannot be computed for this pair -- before any GPU
    context exists (the command line calls it before it makes the pair; CloudPair checks the same before any GPU work)."""
    attrs = getattr(options, "point_ssim", ())
    if not attrs:
        return
    if ties != "pick":
        raise ValueError("PointSSIM rows are not defined for ties='mean'")
    if group is not None:
        raise ValueError("PointSSIM rows are not available for sharded pairs (group=)")
    from .cloud_pair import _has_colors, _has_normals
    clouds = (origin_cloud, reconst_cloud)
    if "color" in attrs and not all(_has_colors(c) for c in clouds):
        raise ValueError("ColorSSIM needs the colours of both clouds")
    if "normal" in attrs and not estimate_normals and not all(_has_normals(c) for c in clouds):
        raise ValueError("NormalSSIM needs the normals of both clouds (or estimate_normals=True)")


def check_hausdorff_rank(options: CalculateOptions, *, group=None) -> None:
    """Raise ``ValueError`` when the ranked Hausdorff rows ``options`` asks for cannot be computed for this pair -- before any
    GPU work (the command line calls it before it makes the pair; CloudPair checks the same before any GPU work of a report).
    A sharded pair would have to exchange the per-pass histograms across its ranks: not built."""
    if getattr(options, "hausdorff_rank", ()) and group is not None:
        raise ValueError("ranked Hausdorff rows are not available for sharded pairs (group=)")


def check_fscore(options: CalculateOptions, *, group=None) -> None:
    """Raise ``ValueError`` when the F-score rows ``options`` asks for cannot be computed for this pair -- before any GPU work (the
    command line calls it before it makes the pair; CloudPair checks the same before any GPU work of a report).  A sharded pair
    would have to add its ranks' counts up: not built."""
    if getattr(options, "fscore", ()) and group is not None:
        raise ValueError("F-score rows are not available for sharded pairs (group=)")


def check_chamfer(options: CalculateOptions, *, group=None) -> None:
    """Raise ``ValueError`` when the Chamfer rows ``options`` asks for cannot be computed for this pair -- before any GPU work (the
    command line calls it before it makes the pair; CloudPair checks the same before any GPU work of a report).  A sharded pair
    would have to exchange the mapped leaves across its ranks: not built."""
    if getattr(options, "chamfer", False) and group is not None:
        raise ValueError("Chamfer and truncated-distance rows are not available for sharded pairs (group=)")


def check_truncate(options: CalculateOptions, *, group=None) -> None:
    """... and likewise for the truncated-distance rows."""
    if getattr(options, "truncate", ()) and group is not None:
        raise ValueError("Chamfer and truncated-distance rows are not available for sharded pairs (group=)")


def check_dcd(options: CalculateOptions, *, ties: str = "pick", group=None) -> None:
    """Raise ``ValueError`` when the density-aware Chamfer rows ``options`` asks for cannot be computed for this pair -- before any
    GPU work (the command line calls it before it makes the pair; CloudPair checks the same before any GPU work of a report).
    Under ``ties="mean"`` the matched point is a virtual one that has no row to count; a sharded pair would have to add its ranks'
    match counts up: not built."""
    if not getattr(options, "dcd", ()):
        return
    if ties != "pick":
        raise ValueError("density-aware Chamfer rows are not defined under ties='mean': a virtual neighbour has no row to count")
    if group is not None:
        raise ValueError("density-aware Chamfer rows are not available for sharded pairs (group=)")


def check_occupancy(options: CalculateOptions, *, group=None) -> None:
    """Raise ``ValueError`` when the voxel-occupancy rows ``options`` asks for cannot be computed for this pair -- before any GPU
    work (the command line calls it before it makes the pair; CloudPair checks the same before any GPU work of a report).  The
    voxel table holds the rows of both whole clouds on one GPU: a sharded pair is out of scope."""
    if getattr(options, "occupancy", ()) and group is not None:
        raise ValueError("voxel-occupancy rows are not available for sharded pairs (group=)")


def check_point_to_distribution(options: CalculateOptions, *, group=None) -> None:
    """Raise ``ValueError`` when the point-to-distribution rows ``options`` asks for cannot be computed for this pair -- before
    any GPU work (the command line calls it before it makes the pair; CloudPair checks the same before any GPU work of a report).
    The columns need both whole clouds on one GPU: a sharded pair is out of scope."""
    if getattr(options, "point_to_distribution", False) and group is not None:
        raise ValueError("point-to-distribution rows are not available for sharded pairs (group=)")


def check_carry_normals(carry_normals: bool, *, ties: str = "pick", group=None) -> None:
    """The ValueErrors of ``CloudPair(..., carry_normals=True)`` (the command line turns them into usage errors): the carried
    normal averages over matched rows, which ``ties="mean"`` replaces by virtual neighbours, and it needs both whole clouds and
    both searches on one GPU (include/pccm.h, pccm_carry_normals)."""
    if not carry_normals:
        return
    if ties != "pick":
        raise ValueError("carry_normals is not defined under ties='mean' (the carried normal averages over matched rows)")
    if group is not None:
        raise ValueError("carry_normals needs whole clouds on one GPU: it cannot be combined with group=")


DUPLICATES = ("keep", "drop", "average")


def check_duplicates(mode, *, group=None) -> None:
    """The ValueErrors of ``CloudPair(..., duplicates=mode)`` (the command line turns them into usage errors): the mode is "keep"
    (nothing is merged), "drop" or "average" (include/pccm.h, pccm_merge_duplicates), and merging needs each whole cloud on one
    GPU."""
    if not isinstance(mode, str) or mode not in DUPLICATES:
        raise ValueError(f"duplicates must be one of {', '.join(repr(m) for m in DUPLICATES)}")
    if mode != "keep" and group is not None:
        raise ValueError("duplicates other than 'keep' need whole clouds on one GPU: they cannot be combined with group=")


def check_p2d_color(options: CalculateOptions, origin_cloud, reconst_cloud, *, group=None) -> None:
    """Raise ``ValueError`` when the colour and joint point-to-distribution rows ``options`` asks for cannot be computed for this
    pair -- before any GPU work (the command line calls it for every cloud it processes; CloudPair checks the same before any GPU
    work of a report).  Both clouds need colours, and -- like the geometry rows -- both whole clouds on one GPU."""
    if not getattr(options, "p2d_color", False):
        return
    if group is not None:
        raise ValueError("point-to-distribution rows are not available for sharded pairs (group=)")
    from .cloud_pair import _has_colors
    if not all(_has_colors(c) for c in (origin_cloud, reconst_cloud)):
        raise ValueError("the colour and joint point-to-distribution rows (p2d_color) need the colours of both clouds")


def check_resolution_psnr(options: CalculateOptions, *, group=None) -> None:
    """Raise ``ValueError`` when the resolution-adaptive PSNR rows ``options`` asks for cannot be computed for this pair -- before
    any GPU work (the command line calls it before it makes the pair; CloudPair checks the same before any GPU work of a report).
    A cloud's spacings come from a k-NN search of the whole cloud on one GPU: a sharded pair is out of scope."""
    if getattr(options, "resolution_psnr", False) and group is not None:
        raise ValueError("resolution-adaptive PSNR rows are not available for sharded pairs (group=)")


def check_reflectance(options: CalculateOptions, origin_cloud, reconst_cloud, *, ties: str = "pick", group=None) -> None:
    """Raise ``ValueError`` when the reflectance rows ``options`` asks for cannot be computed for this pair -- before any GPU
    work (the command line calls it for every cloud it processes; CloudPair checks the same before any GPU work of a report).
    Both clouds need a reflectance; the rows compare a point with its matched point, which ``ties="mean"`` replaces by a virtual
    neighbour; and the matched rows of a sharded search would have to be gathered: out of scope."""
    if not getattr(options, "reflectance", False):
        return
    if ties != "pick":
        raise ValueError("reflectance rows are not defined for ties='mean'")
    if group is not None:
        raise ValueError("reflectance rows are not available for sharded pairs (group=)")
    from .cloud_pair import _has_reflectance
    if not all(_has_reflectance(c) for c in (origin_cloud, reconst_cloud)):
        raise ValueError("the reflectance rows need the reflectance of both clouds")


def _sides(cls, **kw):
    return [cls(is_left=True, **kw), cls(is_left=False, **kw)]


def _sym(cls, higher_is_better: bool, **kw) -> SymmetricMetric:
    return SymmetricMetric(metrics=tuple(_sides(cls, **kw)), is_proportional=higher_is_better)


def _error_then_psnr(err_cls, psnr_cls, **kw) -> typing.List[AbstractMetric]:
    return (_sides(err_cls, **kw) + [_sym(err_cls, False, **kw)]
            + _sides(psnr_cls, **kw) + [_sym(psnr_cls, True, **kw)])


def transform_options(options: CalculateOptions) -> typing.List[AbstractMetric]:
    metrics: typing.List[AbstractMetric] = [MinSqrtDistance(), MaxSqrtDistance()]
    metrics += _error_then_psnr(GeoMSE, GeoPSNR, point_to_plane=False)
    if options.color is not None:
        metrics += _error_then_psnr(ColorMSE, ColorPSNR, color_scheme=options.color)
    if options.point_to_plane:
        metrics += _error_then_psnr(GeoMSE, GeoPSNR, point_to_plane=True)
    if options.hausdorff:
        metrics += _error_then_psnr(GeoHausdorffDistance, GeoHausdorffDistancePSNR, point_to_plane=False)
    if options.hausdorff and options.point_to_plane:
        kw = dict(point_to_plane=True)
        metrics += (_sides(GeoHausdorffDistance, **kw) + _sides(GeoHausdorffDistancePSNR, **kw)
                    + [_sym(GeoHausdorffDistance, False, **kw), _sym(GeoHausdorffDistancePSNR, True, **kw)])
    if getattr(options, "plane_to_plane", False):
        # higher is better: the symmetric rows report the smaller side
        metrics += _sides(AngularSimilarity) + [_sym(AngularSimilarity, True)]
        if options.hausdorff:
            metrics += _sides(MinAngularSimilarity) + [_sym(MinAngularSimilarity, True)]
    for attribute in SSIM_ATTRIBUTES:
        if attribute in (getattr(options, "point_ssim", None) or ()):
            # higher is better: the symmetric rows report the smaller side
            cls, kw = SSIM_CLASSES[attribute], dict(k=getattr(options, "ssim_neighbours", 12))
            metrics += _sides(cls, **kw) + [_sym(cls, True, **kw)]
    for rank in getattr(options, "hausdorff_rank", None) or ():
        for point_to_plane in (False, True) if options.point_to_plane else (False,):
            metrics += _error_then_psnr(GeoRankedHausdorffDistance, GeoRankedHausdorffDistancePSNR,
                                        point_to_plane=point_to_plane, rank=rank)
    if getattr(options, "point_to_distribution", False):
        # lower is better: the symmetric rows report the larger side
        kw = dict(k=getattr(options, "p2d_neighbours", 30))
        metrics += _sides(MahalanobisDistance, **kw) + [_sym(MahalanobisDistance, False, **kw)]
        if options.hausdorff:
            metrics += _sides(MaxMahalanobisDistance, **kw) + [_sym(MaxMahalanobisDistance, False, **kw)]
        if getattr(options, "p2d_color", False):
            for cls in (ColorMahalanobisDistance, JointMahalanobisDistance):
                metrics += _sides(cls, **kw) + [_sym(cls, False, **kw)]
            if options.hausdorff:
                for cls in (MaxColorMahalanobisDistance, MaxJointMahalanobisDistance):
                    metrics += _sides(cls, **kw) + [_sym(cls, False, **kw)]
    if getattr(options, "resolution_psnr", False):
        k = getattr(options, "resolution_neighbours", 10)
        metrics += _sides(IntrinsicResolution, k=k)
        # higher is better: the symmetric rows report the smaller side
        for cls in (GeoResolutionPSNR, GeoHausdorffResolutionPSNR) if options.hausdorff else (GeoResolutionPSNR,):
            for point_to_plane in (False, True) if options.point_to_plane else (False,):
                kw = dict(point_to_plane=point_to_plane, k=k)
                metrics += _sides(cls, **kw) + [_sym(cls, True, **kw)]
    if getattr(options, "reflectance", False):
        kw = dict(peak=getattr(options, "reflectance_peak", 65535.0))
        metrics += (_sides(ReflectanceMSE) + [_sym(ReflectanceMSE, False)]
                    + _sides(ReflectancePSNR, **kw) + [_sym(ReflectancePSNR, True, **kw)])
        if options.hausdorff:
            metrics += (_sides(ReflectanceHausdorffDistance) + [_sym(ReflectanceHausdorffDistance, False)]
                        + _sides(ReflectanceHausdorffDistancePSNR, **kw) + [_sym(ReflectanceHausdorffDistancePSNR, True, **kw)])
    for threshold in getattr(options, "fscore", None) or ():
        # left: recall (how much of the origin cloud the processed one covers); right: precision; the F-score is the symmetric row
        metrics += _sides(GeoInlierRatio, threshold=threshold) + [GeoFScore(threshold=threshold)]
    chamfer = bool(getattr(options, "chamfer", False))
    if chamfer:
        # lower is better: the symmetric rows report the larger side
        for point_to_plane in (False, True) if options.point_to_plane else (False,):
            metrics += _sides(GeoMeanDistance, point_to_plane=point_to_plane) + [_sym(GeoMeanDistance, False, point_to_plane=point_to_plane)]
        metrics += [GeoChamferL1(), GeoChamferL2()]
    for threshold in getattr(options, "truncate", None) or ():
        for cls in (GeoTruncatedMSE, GeoTruncatedMeanDistance) if chamfer else (GeoTruncatedMSE,):
            metrics += _sides(cls, threshold=threshold) + [_sym(cls, False, threshold=threshold)]
    squared = bool(getattr(options, "dcd_squared", False))
    for alpha in getattr(options, "dcd", None) or ():
        metrics += _sides(GeoDensityAwareDistance, alpha=alpha, squared=squared) + [GeoDensityAwareChamfer(alpha=alpha, squared=squared)]
    if getattr(options, "align", None) is not None:
        metrics += [AlignmentFitness(), AlignmentRMSE()]
    for voxel in getattr(options, "occupancy", None) or ():
        # left: the original's voxels / voxel recall; right: the processed cloud's / voxel precision; the IoU is the symmetric row
        metrics += _sides(OccupiedVoxels, voxel=voxel) + _sides(VoxelCoverage, voxel=voxel) + [VoxelIoU(voxel=voxel)]
    return metrics
