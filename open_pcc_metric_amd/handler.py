"""Command line -- same flags and report text as ``python -m open_pcc_metric`` (handler.py:4-71).

    python -m open_pcc_metric_amd --ocloud A.ply --pcloud B.ply [--pcloud C.ply ...] [--color rgb|ycc] [--hausdorff]
                                  [--point-to-plane] [--plane-to-plane] [--point-ssim ATTR ...] [--hausdorff-rank R ...]
                                  [--point-to-distribution] [--p2d-neighbours K] [--p2d-color] [--carry-normals] [--duplicates keep|drop|average]
                                  [--resolution-psnr] [--resolution-neighbours K] [--reflectance] [--reflectance-peak P] [--fscore TAU ...]
                                  [--chamfer] [--truncate TAU ...] [--dcd ALPHA ...] [--dcd-squared] [--transform FILE] [--align icp]
                                  [--occupancy VOXEL ...] [--csv]

Extra, optional flags (defaults reproduce the reference): ``--device``, ``--engine``,
``--normal-index row|neighbour`` (row = the reference's D2, which raises IndexError when the clouds
differ in size), ``--extent X Y Z`` (inject the PSNR peak box instead of the
Qhull minimal-OBB restatement), ``--tie-exposure`` (diagnostic on stderr: how much of the point-to-plane result hangs
on the order of exact ties, which nanoflann decides by traversal -- cloud_pair.py:22-23), ``--ties pick|mean``
(pick = the smallest row of several equidistant nearest neighbours; mean = their mean, which makes the point-to-plane and
colour rows independent of the order of the points; D1 rows are the same either way).  Files without normals get them estimated on the GPU when
--point-to-plane asks for them (k = 30 covariance normals, as Open3D's estimate_normals does at
cloud_pair.py:61-64).  ``--plane-to-plane`` (no counterpart in the reference) adds the angular similarity rows of Alexiou &
Ebrahimi (ICME 2018) after all others; they compare each point's normal with its matched point's, so they too estimate the
normals files lack.  ``--point-ssim geometry|normal|curvature|color`` (repeatable; no counterpart in the reference) adds the
PointSSIM rows of Alexiou & Ebrahimi (ICME Workshops 2020) after those, over neighbourhoods of ``--ssim-neighbours`` points
("PointSSIM").  ``--hausdorff-rank R`` (repeatable, R in (0, 1]; no counterpart in the reference) adds the ranked
(generalized) Hausdorff rows of Javaheri et al. (QoMEX 2020) after all others: the ceil(R n)-th smallest squared distance of
each direction and its PSNR, for D1 and -- with ``--point-to-plane`` -- D2, selected on the GPU; independent of ``--hausdorff``,
whose rows are those of R = 1 ("Ranked Hausdorff").  ``--point-to-distribution`` (no counterpart in the reference)
adds, after all others, the point-to-distribution rows after Javaheri et al. (IEEE SPL 2020): the mean -- with ``--hausdorff``
also the maximum -- Mahalanobis distance of each point to the distribution of its ``--p2d-neighbours`` nearest points in the other
cloud ("Point-to-distribution").  ``--p2d-color`` (with ``--point-to-distribution``; a usage error without it)
adds, after those, the colour and joint rows after Javaheri et al. (IEEE MMSP 2021): each point's luma against the luma
distribution of the same neighbourhood, and sqrt(geometry^2 + colour^2) per point, pooled like the geometry rows; both clouds need
colours ("Point-to-distribution: colour and joint").  ``--carry-normals`` (no counterpart in the reference) gives
a file WITHOUT normals the other file's normals instead of estimated ones, as the MPEG evaluation procedure does for a decoded
cloud (``pc_error``'s normal carrying): each point takes the average of the normals of the other cloud's points whose nearest
neighbour it is, or its own nearest point's normal when it is nobody's ("Carried normals").  The MPEG-style D2 is
``--point-to-plane --normal-index neighbour --carry-normals``; no default changes, and ``--ties mean`` with it is a usage
error.  ``--duplicates drop|average`` (default ``keep``: nothing changes; no counterpart in the reference) merges, on the GPU and
before anything is searched, the points of each file that share their coordinates, as ``pc_error`` does with both clouds
(dropDuplicates): one point per position, with the first one's normal and the first one's colour (``drop``) or the average colour
(``average``, pc_error's default); a line per cloud on stderr says how many rows were merged away ("Duplicate
points").  ``--resolution-psnr`` (no counterpart in the reference) adds, after all others, the resolution-adaptive PSNR rows after
Javaheri et al. (ICIP 2020): each cloud's intrinsic resolution -- the average distance of a point to its
``--resolution-neighbours`` nearest neighbours in its own cloud -- and the PSNR of the D1 and, with ``--point-to-plane``, D2 errors
(with ``--hausdorff`` also of the Hausdorff distances) against the ORIGINAL cloud's resolution as the peak, instead of its
bounding box ("Resolution-adaptive PSNR").  ``--reflectance`` (no counterpart in the reference) adds, after all
others, the reflectance rows MPEG's ``pc_error`` reports for LiDAR content: the mean -- with ``--hausdorff`` also the maximum --
squared difference between each point's reflectance and its matched point's, on the files' values as given, and their PSNR against
``--reflectance-peak`` (default 65535, the 16-bit range; 255 for 8-bit intensity).  Both files need a reflectance property;
``--ties mean`` with it is a usage error ("Reflectance").  ``--fscore TAU`` (repeatable, TAU >= 0 in the clouds'
units; no counterpart in the reference) adds, after all others, the rows the reconstruction and completion literature reports beside
the Chamfer distance: the share of the original cloud's points within TAU of the processed cloud (recall), the share of the
processed cloud's points within TAU of the original (precision) and their harmonic mean, the F-score -- counted on the GPU, and at
TAU = 0 the share of points reproduced exactly ("F-score").  ``--chamfer`` (no counterpart in the reference) adds,
after those, the mean UNSQUARED nearest-neighbour distance of each direction (with ``--point-to-plane`` also the mean magnitude of
the projection), Chamfer-L1 -- their average over the two directions, PCN's convention -- and Chamfer-L2, the sum of the two D1
GeoMSE rows.  ``--truncate TAU`` (repeatable, TAU >= 0; no counterpart in the reference) adds, last, the mean squared distance with
every distance clipped at TAU -- and with ``--chamfer`` the clipped mean distance --, the remedy for partly overlapping clouds; all
of them are summed inside the reduction kernel, no column is stored ("Chamfer and truncated distances").  ``--dcd ALPHA`` (repeatable, ALPHA >= 0; no counterpart in the reference) adds,
after every other row, the density-aware Chamfer distance of Wu et al. (NeurIPS 2021): per direction the mean of
1 - exp(-ALPHA d) / m over a cloud's points -- d the distance to the matched point, m the number of points that share it, counted on
the GPU -- and the average of the two directions; every row lies in [0, 1], and a cloud that piles its points onto a few places is
penalised where the Chamfer distance is blind.  ``--dcd-squared`` feeds d^2 in d's place; ``--ties mean`` with ``--dcd`` is a usage
error ("Density-aware Chamfer distance").  ``--occupancy VOXEL`` (repeatable, VOXEL > 0 in the clouds' units; no
counterpart in the reference) adds, after every other row, the voxel-occupancy numbers of the reconstruction and learned-codec
literature at that voxel size: the voxels of the lattice floor(coordinate / VOXEL) each cloud occupies, the share of each cloud's
voxels the other occupies too (left: voxel recall, right: voxel precision) and their intersection over union -- counted on a GPU
voxel table, without any search; on integer-voxelised content VOXEL = 2^j reads them at octree level j ("Voxel
occupancy").  Input files: ply, pcd, xyz, xyzn, xyzrgb, pts (io.py; the formats
``o3d.io.read_point_cloud`` picks by extension, handler.py:57).
"""
import click


@click.command()
@click.option("--ocloud", required=True, type=str, help="Original point cloud.")
@click.option("--pcloud", required=True, type=str, multiple=True,
              help="Processed point cloud.  May be given several times: one report per processed cloud, printed one after the other "
                   "exactly as separate runs would print them, with the original cloud read, uploaded and analysed once.")
@click.option("--color", required=False, type=click.Choice(["rgb", "ycc"]), help="Report color distortions as well.")
@click.option("--hausdorff", required=False, is_flag=True,
              help="Report hausdorff metric as well. If --point-to-plane is provided, "
                   "then hausdorff point-to-plane would be reported too")
@click.option("--point-to-plane", required=False, is_flag=True, help="Report point-to-plane distance as well.")
@click.option("--plane-to-plane", required=False, is_flag=True,
              help="Report plane-to-plane angular similarity as well (1: parallel or antiparallel normals, 0: perpendicular), "
                   "after all other rows; with --hausdorff also its worst point.  Compares each point's normal with its matched "
                   "point's normal: --normal-index does not apply.  Normals missing from a file are estimated.")
@click.option("--point-ssim", "point_ssim", type=click.Choice(["geometry", "normal", "curvature", "color"]), multiple=True,
              help="Report the PointSSIM structural similarity of this attribute as well (may be repeated), after all other "
                   "rows: 1 - |F_A - F_B| / max(|F_A|, |F_B|) of each point's neighbourhood variance and its matched point's, "
                   "averaged.  Normals missing from a file are estimated; color needs colours in both files.")
@click.option("--ssim-neighbours", "ssim_neighbours", type=click.IntRange(2, 64), default=12, show_default=True,
              help="Points per PointSSIM neighbourhood (the point itself included).")
@click.option("--hausdorff-rank", "hausdorff_rank", type=float, multiple=True,
              help="Report the ranked (generalized) Hausdorff distance at this rank in (0, 1] as well (may be repeated, at most 4), "
                   "after all other rows: the ceil(R n)-th smallest squared distance of each direction and its PSNR (0.95: the "
                   "distance 95 % of the points stay within; 1: the Hausdorff rows); with --point-to-plane for D2 too.")
@click.option("--point-to-distribution", "point_to_distribution", required=False, is_flag=True,
              help="Report the point-to-distribution metric as well, after all other rows: the Mahalanobis distance of each point "
                   "to the mean and covariance of its nearest points in the other cloud, averaged (lower is better, "
                   "dimensionless); with --hausdorff also its worst point.  Does not depend on --ties.")
@click.option("--p2d-neighbours", "p2d_neighbours", type=click.IntRange(4, 64), default=30, show_default=True,
              help="Points of the other cloud per point-to-distribution neighbourhood.")
@click.option("--p2d-color", "p2d_color", required=False, is_flag=True,
              help="With --point-to-distribution: report its colour rows (each point's luma against the luma distribution of the "
                   "same nearest points) and joint geometry-and-colour rows as well, after all other rows.  Both clouds need "
                   "colours.")
@click.option("--carry-normals", "carry_normals", required=False, is_flag=True,
              help="A cloud without normals takes the other cloud's instead of estimated ones, as MPEG's pc_error does for a "
                   "decoded cloud: per point the average normal of the other cloud's points whose nearest neighbour it is, or its "
                   "own nearest point's normal.  With normals in neither file the original's are estimated and carried over.  "
                   "MPEG-style D2: --point-to-plane --normal-index neighbour --carry-normals.  Not with --ties mean.")
@click.option("--duplicates", type=str, default="keep", show_default=True, metavar="[keep|drop|average]",
              help="Merge the points of each cloud that share their coordinates before comparing, as MPEG's pc_error does "
                   "(dropDuplicates): one point per position, with the first point's normal and the first point's colour (drop) "
                   "or the average colour (average, pc_error's default).  keep: nothing is merged.")
@click.option("--resolution-psnr", "resolution_psnr", required=False, is_flag=True,
              help="Report each cloud's intrinsic resolution (the average distance of a point to its nearest neighbours in its own "
                   "cloud) and PSNR rows whose peak is the original cloud's resolution as well, after all other rows; with "
                   "--point-to-plane for D2 and with --hausdorff for the Hausdorff distances too.  Does not depend on --ties.")
@click.option("--resolution-neighbours", "resolution_neighbours", type=click.IntRange(1, 63), default=10, show_default=True,
              help="Nearest neighbours a point's spacing is averaged over (the point itself not counted).")
@click.option("--reflectance", "reflectance", required=False, is_flag=True,
              help="Report the reflectance MSE and PSNR (LiDAR return intensity, as MPEG's pc_error reports it) as well, after all "
                   "other rows: the squared difference between each point's reflectance and its matched point's, values as given; "
                   "with --hausdorff also its worst point.  Both clouds need a reflectance.  Not with --ties mean.")
@click.option("--reflectance-peak", "reflectance_peak", type=float, default=65535.0, show_default=True,
              help="Peak of the reflectance PSNR rows (65535: 16-bit reflectance; 255: 8-bit intensity).")
@click.option("--fscore", "fscore", type=float, multiple=True, metavar="TAU",
              help="Report precision, recall and F-score at this distance threshold (>= 0, in the clouds' units) as well (may be "
                   "repeated, at most 4), after all other rows: the share of each cloud's points within TAU of the other cloud "
                   "(left: recall, right: precision) and their harmonic mean; TAU = 0 counts the points reproduced exactly.")
@click.option("--chamfer", "chamfer", required=False, is_flag=True,
              help="Report the mean unsquared nearest-neighbour distance of each direction (with --point-to-plane also of the "
                   "projection's magnitude), Chamfer-L1 (their average over both directions) and Chamfer-L2 (the sum of the two "
                   "mean squared distances) as well, after all other rows.")
@click.option("--truncate", "truncate", type=float, multiple=True, metavar="TAU",
              help="Report the mean squared distance with every distance clipped at this threshold (>= 0, in the clouds' units) as "
                   "well (may be repeated, at most 4), after all other rows; with --chamfer also the clipped mean distance.  For "
                   "partly overlapping clouds.")
@click.option("--dcd", "dcd", type=float, multiple=True, metavar="ALPHA",
              help="Report the density-aware Chamfer distance at this alpha (>= 0, in 1 / the clouds' units) as well (may be "
                   "repeated, at most 4), after all other rows: per direction the mean of 1 - exp(-ALPHA d) / m, d the distance "
                   "to the matched point and m the number of points that share it, and the average of both directions; in "
                   "[0, 1], lower is better.  ALPHA = 0: the share of points that share their matched point.  Not with --ties mean.")
@click.option("--dcd-squared", "dcd_squared", required=False, is_flag=True,
              help="With --dcd: feed the squared distance d^2 in d's place.")
@click.option("--transform", "transform", type=str, default=None, metavar="FILE",
              help="Move every processed cloud by the rigid motion in FILE (12 or 16 whitespace-separated numbers: the rows of a "
                   "3 x 4 or 4 x 4 matrix) before comparing, on the GPU; file normals are rotated with it.")
@click.option("--align", "align", type=str, default=None, metavar="[icp]",
              help="Register every processed cloud onto the original before comparing: point-to-point ICP on the GPU's exact "
                   "nearest-neighbour search, starting from --transform (or the identity).  Adds AlignmentFitness and "
                   "AlignmentRMSE after all other rows.")
@click.option("--align-distance", "align_distance", type=float, default=None, metavar="D",
              help="With --align: only points within D of the original take part (for partly overlapping clouds).")
@click.option("--align-iterations", "align_iterations", type=int, default=30, show_default=True, metavar="N",
              help="With --align: at most N searches (1..1000).")
@click.option("--align-tolerance", "align_tolerance", type=float, default=1e-6, show_default=True, metavar="X",
              help="With --align: stop when fitness and inlier RMSE both change by less than X.")
@click.option("--align-out", "align_out", type=str, default=None, metavar="FILE",
              help="Write the 4 x 4 motion each processed cloud was given (--transform included) to FILE, 17 significant digits; "
                   "with several --pcloud the matrices follow one another.")
@click.option("--occupancy", "occupancy", type=float, multiple=True, metavar="VOXEL",
              help="Report the voxel occupancy at this voxel size (> 0, in the clouds' units) as well (may be repeated, at most 4), "
                   "after all other rows: the voxels floor(coordinate / VOXEL) each cloud occupies, the share of each cloud's "
                   "voxels the other occupies too (left: recall, right: precision) and their intersection over union.  Counted "
                   "after --duplicates, --transform and --align; no search involved.")
@click.option("--csv", required=False, is_flag=True, help="Print output in csv format.")
@click.option("--device", type=int, default=0, show_default=True, help="GPU to use.")
@click.option("--engine", type=click.Choice(["auto", "grid", "brute"]), default="auto", show_default=True,
              help="Exact nearest-neighbour engine.")
@click.option("--normal-index", type=click.Choice(["row", "neighbour"]), default="row", show_default=True,
              help="Which normal the point-to-plane projection uses.")
@click.option("--extent", type=float, nargs=3, default=None, help="Extents of the PSNR peak box (skips the min-OBB).")
@click.option("--tie-exposure", is_flag=True,
              help="After the report, print to stderr how many points have several equidistant nearest neighbours and the "
                   "interval of point-to-plane MSE values the order of those ties can produce (diagnostic).")
@click.option("--ties", type=click.Choice(["pick", "mean"]), default="pick", show_default=True,
              help="Neighbour of a point with several equidistant nearest neighbours: the one of the smallest row, or their mean "
                   "(point-to-plane and colour rows then do not depend on the order of the points).")
def cli(ocloud, pcloud, color, hausdorff, point_to_plane, plane_to_plane, point_ssim, ssim_neighbours, hausdorff_rank,
        point_to_distribution, p2d_neighbours, p2d_color, carry_normals, duplicates, resolution_psnr, resolution_neighbours, reflectance, reflectance_peak, fscore, chamfer, truncate, dcd, dcd_squared, transform, align, align_distance, align_iterations, align_tolerance, align_out, occupancy, csv, device, engine, normal_index, extent, tie_exposure,
        ties) -> None:
    from .calculator import MetricCalculator
    from .cloud_pair import CloudPair
    from .io import read_point_cloud
    from .options import (CalculateOptions, check_carry_normals, check_chamfer, check_dcd, check_duplicates, check_fscore, check_hausdorff_rank, check_occupancy, check_p2d_color, check_point_ssim,
                          check_point_to_distribution, check_reflectance, check_resolution_psnr, check_truncate, transform_options)

    try:                                       # (a bad rank: before any file is read and any GPU context exists)
        options = CalculateOptions(color=color, hausdorff=hausdorff, point_to_plane=point_to_plane, plane_to_plane=plane_to_plane,
                                   point_ssim=point_ssim, ssim_neighbours=ssim_neighbours, hausdorff_rank=hausdorff_rank or None,
                                   point_to_distribution=point_to_distribution, p2d_neighbours=p2d_neighbours,
                                   p2d_color=p2d_color, resolution_psnr=resolution_psnr,
                                   resolution_neighbours=resolution_neighbours, reflectance=reflectance,
                                   reflectance_peak=reflectance_peak, fscore=fscore or None, chamfer=chamfer,
                                   truncate=truncate or None, dcd=dcd or None, dcd_squared=dcd_squared, align=align,
                                   occupancy=occupancy or None)
        check_dcd(options, ties=ties)
        from .align import check_align, read_transform_file
        check_align(align, align_distance, align_iterations, align_tolerance)
        if align_distance is not None and align is None:
            raise ValueError("--align-distance needs --align")
        if align_out is not None and align is None and transform is None:
            raise ValueError("--align-out needs --align or --transform")
        check_carry_normals(carry_normals, ties=ties)
        check_duplicates(duplicates)
    except ValueError as exc:
        raise click.UsageError(str(exc))
    check_hausdorff_rank(options)
    check_fscore(options)
    check_chamfer(options)
    check_truncate(options)
    check_point_to_distribution(options)
    check_resolution_psnr(options)
    check_occupancy(options)
    try:                                       # (the one file a usage error may come from: read before any cloud)
        transform_matrix = None if transform is None else read_transform_file(transform)
    except (OSError, ValueError) as exc:
        raise click.UsageError(str(exc))
    ocloud_cloud = read_point_cloud(ocloud)
    cloud_pair = None
    motions = []
    for path in pcloud:
        pcloud_cloud = read_point_cloud(path)
        check_point_ssim(options, ocloud_cloud, pcloud_cloud, ties=ties)       # (before the GPU context, for every processed cloud)
        check_p2d_color(options, ocloud_cloud, pcloud_cloud)
        try:
            check_reflectance(options, ocloud_cloud, pcloud_cloud, ties=ties)
        except ValueError as exc:
            raise click.UsageError(str(exc))
        if cloud_pair is None:
            # (clouds read from files are freed while the GPU context works on -- with several decoded clouds, when the next one
            # is read --: their bytes go through the context's own pinned buffers, see CloudPair's staged_io; 0.6 ms for a pair)
            cloud_pair = CloudPair(ocloud_cloud, pcloud_cloud, device=device, nn_engine=engine, normal_index=normal_index,
                                   extent=list(extent) if extent else None, staged_io=True, ties=ties,
                                   carry_normals=carry_normals, duplicates=duplicates, transform=transform_matrix, align=align,
                                   align_distance=align_distance, align_iterations=align_iterations, align_tolerance=align_tolerance)
            merged_logs = ((0, ocloud, ocloud_cloud), (1, path, pcloud_cloud))
        else:
            cloud_pair = cloud_pair.with_reconst(pcloud_cloud)     # the original cloud stays in HBM with all that belongs to it
            merged_logs = ((1, path, pcloud_cloud),)
        if duplicates != "keep":               # stderr: stdout stays the report
            for which, name, given in merged_logs:
                click.echo(f"duplicates ({duplicates}): {name}: {cloud_pair.duplicates_removed[which]} of {len(given.points)} rows "
                           "merged away", err=True)
        if align_out is not None:
            from .align import write_transform_file
            motions.append(cloud_pair.alignment.transformation)
            write_transform_file(align_out, motions)
        calculator = MetricCalculator(cloud_pair)
        result = calculator.calculate(transform_options(options)).as_df()
        print(result.to_csv() if csv else result.to_string())
        if tie_exposure:                       # stderr: stdout stays byte-identical to the reference's report
            for is_left in (True, False):
                t = cloud_pair.tie_exposure(is_left, point_to_plane)
                line = (f"tie exposure ({t['direction']}): {t['tied_queries']} of {t['queries']} points have several equidistant nearest "
                        f"neighbours ({100.0 * t['tie_rate']:.3f} %, up to {t['max_multiplicity']})")
                if point_to_plane:
                    line += (f"; point-to-plane mse in [{t['d2_mse_min']!r}, {t['d2_mse_max']!r}] over all tie orders, "
                             f"reported {t['d2_mse_pick']!r} (smallest row)")
                click.echo(line, err=True)
    if cloud_pair is not None:
        cloud_pair.close()
