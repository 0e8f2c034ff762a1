"""The reflectance feature without a GPU ("Reflectance"): the NumPy reference pinned on planted cases, the row
lists of the options, file IO, PointCloud's dtype rules, the command line's usage errors, and the staleness event of
csrc/pccm_stale.h through a stand-alone program built with the host sanitizers."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest
from click.testing import CliRunner

import reflectance_reference as ref
from open_pcc_metric_amd.handler import cli
from open_pcc_metric_amd.io import read_point_cloud, write_point_cloud
from open_pcc_metric_amd.options import CalculateOptions, check_reflectance, transform_options
from open_pcc_metric_amd.point_cloud import PointCloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


# ---- the reference on planted cases -------------------------------------------------------------------------------------------
def test_reference_on_a_hand_made_pair():
    a = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [10, 10, 0]], dtype=np.float64)
    b = np.array([[10, 1, 0], [0, 1, 0], [5, 5, 0], [5, 5, 0]], dtype=np.float64)
    ra = np.array([100, 200, 300, 400], dtype=np.uint16)
    rb = np.array([250.0, 90.0, 1000.0, 7.0])
    # a -> b: rows 0 and 1 match b[1] and b[0]; rows 2 and 3 are nearest to the two coincident points, the smaller row (2) wins
    assert ref.column(a, b, ra, rb).tolist() == [100.0, 2500.0, 490000.0, 360000.0]
    # b -> a: b[0] -> a[1], b[1] -> a[0]; b[2] and b[3] are equidistant from all four points of a: row 0
    assert ref.column(b, a, rb, ra).tolist() == [2500.0, 100.0, 810000.0, 8649.0]
    got = ref.rows(a, b, ra, rb, hausdorff=True, peak=1000.0)
    assert list(got) == [
        ("ReflectanceMSE", True), ("ReflectanceMSE", False), ("SymmetricMetric", "ReflectanceMSE", True, "ReflectanceMSE", False),
        ("ReflectancePSNR", True, 1000.0), ("ReflectancePSNR", False, 1000.0),
        ("SymmetricMetric", "ReflectancePSNR", True, 1000.0, "ReflectancePSNR", False, 1000.0),
        ("ReflectanceHausdorffDistance", True), ("ReflectanceHausdorffDistance", False),
        ("SymmetricMetric", "ReflectanceHausdorffDistance", True, "ReflectanceHausdorffDistance", False),
        ("ReflectanceHausdorffDistancePSNR", True, 1000.0), ("ReflectanceHausdorffDistancePSNR", False, 1000.0),
        ("SymmetricMetric", "ReflectanceHausdorffDistancePSNR", True, 1000.0, "ReflectanceHausdorffDistancePSNR", False, 1000.0)]
    mse_l, mse_r = 852600.0 / 4, 821249.0 / 4
    assert got[("ReflectanceMSE", True)] == mse_l and got[("ReflectanceMSE", False)] == mse_r
    assert got[("SymmetricMetric", "ReflectanceMSE", True, "ReflectanceMSE", False)] == mse_l             # the larger side
    assert got[("ReflectancePSNR", True, 1000.0)] == 10 * np.log10(1.0e6 / mse_l)
    assert got[("SymmetricMetric", "ReflectancePSNR", True, 1000.0, "ReflectancePSNR", False, 1000.0)] == 10 * np.log10(1.0e6 / mse_l)
    assert got[("ReflectanceHausdorffDistance", True)] == 490000.0 and got[("ReflectanceHausdorffDistance", False)] == 810000.0
    assert got[("SymmetricMetric", "ReflectanceHausdorffDistancePSNR", True, 1000.0, "ReflectanceHausdorffDistancePSNR", False, 1000.0)] \
        == 10 * np.log10(1.0e6 / 810000.0)
    assert len(ref.rows(a, b, ra, rb)) == 6 and ("ReflectancePSNR", True, 65535.0) in ref.rows(a, b, ra, rb)


@pytest.mark.parametrize("n", [1, 7, 129, 1000])
def test_reference_sums_integer_reflectance_exactly(n):
    """Integers in 0..65535, n <= 1000: every square is below 2^32 and the sum below 2^42 -- all exact in fp64, so np.sum must
    equal the Python-int sum whatever order it adds in."""
    rng = np.random.default_rng(n)
    a, b = rng.random((n, 3)), rng.random((n + 3, 3))
    ra, rb = rng.integers(0, 65536, n).astype(np.uint16), rng.integers(0, 65536, n + 3).astype(np.uint16)
    col = ref.column(a, b, ra, rb)
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
    nn = d2.argmin(axis=1)
    exact = [(int(x) - int(rb[j])) ** 2 for x, j in zip(ra, nn)]
    assert [int(v) for v in col] == exact and all(float(int(v)) == v for v in col)
    assert int(np.sum(col)) == sum(exact) and float(sum(exact)) == np.sum(col)
    assert ref.rows(a, b, ra, rb)[("ReflectanceMSE", True)] == sum(exact) / n


def test_reference_identical_clouds_give_zero_and_inf_without_a_warning(recwarn):
    a = np.random.default_rng(0).random((50, 3))
    r = np.arange(50, dtype=np.uint16)
    got = ref.rows(a, a, r, r, hausdorff=True)
    assert got[("ReflectanceMSE", True)] == 0.0 and got[("ReflectancePSNR", True, 65535.0)] == np.inf
    assert len(recwarn) == 0


def test_reference_merge_rule():
    x = np.array([[1, 1, 1], [2, 2, 2], [1, 1, 1], [3, 3, 3], [1, 1, 1], [2, 2, 2]], dtype=np.float64)
    r = np.array([0.1, 10.0, 0.2, 5.0, 0.4, 20.0])
    assert ref.merged(x, r, "drop").tolist() == [0.1, 10.0, 5.0]
    assert ref.merged(x, r, "average").tolist() == [((0.1 + 0.2) + 0.4) / 3.0, (10.0 + 20.0) / 2.0, 5.0]
    assert ref.merged_points(x).tolist() == [[1, 1, 1], [2, 2, 2], [3, 3, 3]]
    assert ref.merged(x, r.astype(np.float32), "drop").dtype == np.float64


# ---- options ------------------------------------------------------------------------------------------------------------------
EVERYTHING = dict(color="rgb", point_to_plane=True, plane_to_plane=True, point_ssim=("geometry", "normal", "curvature", "color"),
                  hausdorff_rank=[0.5, 0.9], point_to_distribution=True, p2d_color=True, resolution_psnr=True)


def keys(**kw):
    return [m._key() for m in transform_options(CalculateOptions(**kw))]


def reflectance_keys(hausdorff, peak=65535.0):
    names = [("ReflectanceMSE", ()), ("ReflectancePSNR", (peak,))]
    if hausdorff:
        names += [("ReflectanceHausdorffDistance", ()), ("ReflectanceHausdorffDistancePSNR", (peak,))]
    out = []
    for name, extra in names:
        out += [(name, True) + extra, (name, False) + extra, ("SymmetricMetric", name, True) + extra + (name, False) + extra]
    return out


@pytest.mark.parametrize("others", [{}, EVERYTHING], ids=["alone", "with_every_other_option"])
@pytest.mark.parametrize("reflectance,hausdorff", list(itertools.product([False, True], [False, True])))
def test_row_list_and_order(reflectance, hausdorff, others):
    without = keys(hausdorff=hausdorff, **others)
    assert not any("Reflectance" in str(k) for k in without)
    got = keys(hausdorff=hausdorff, reflectance=reflectance, **others)
    want = without + (reflectance_keys(hausdorff) if reflectance else [])
    assert got == want                                                       # (the reflectance rows are last)
    # a peak nobody asked to use changes nothing; one that is used is part of the PSNR keys only
    assert keys(hausdorff=hausdorff, reflectance=False, reflectance_peak=255.0, **others) == without
    if reflectance:
        assert keys(hausdorff=hausdorff, reflectance=True, reflectance_peak=255, **others) == without + reflectance_keys(hausdorff, 255.0)


def test_reports_without_reflectance_have_todays_rows():
    """The row counts of the four reference reports (tests/golden: 8, 14, 14, 26 rows) and their first and last keys."""
    counts = {(h, p): len(keys(hausdorff=h, point_to_plane=p)) for h in (False, True) for p in (False, True)}
    assert counts == {(False, False): 8, (False, True): 14, (True, False): 14, (True, True): 26}
    assert keys()[0] == ("MinSqrtDistance",) and keys()[-1] == ("SymmetricMetric", "GeoPSNR", True, False, "GeoPSNR", False, False)
    assert len(keys(reflectance=True)) == 8 + 6 and len(keys(reflectance=True, hausdorff=True)) == 14 + 12


def test_labels_carry_the_peak():
    from open_pcc_metric_amd.calculator import CalculateResult
    metrics = transform_options(CalculateOptions(reflectance=True, reflectance_peak=255.0))[-6:]
    for m in metrics:
        m.value = 1.0
    labels = CalculateResult(metrics).as_df()["label"].tolist()
    assert labels == ["ReflectanceMSE", "ReflectanceMSE", "ReflectanceMSE(symmetric)", "ReflectancePSNR[255.0]", "ReflectancePSNR[255.0]",
                      "ReflectancePSNR[255.0](symmetric)"]


@pytest.mark.parametrize("peak", [True, False, float("nan"), float("inf"), -float("inf"), 0, 0.0, -1.0, "255", None, np.bool_(True)])
def test_bad_peaks_raise(peak):
    with pytest.raises(ValueError, match="reflectance_peak"):
        CalculateOptions(reflectance=True, reflectance_peak=peak)
    with pytest.raises(ValueError, match="reflectance_peak"):
        CalculateOptions(reflectance_peak=peak)


def test_good_peaks_and_defaults():
    o = CalculateOptions()
    assert o.reflectance is False and o.reflectance_peak == 65535.0
    for peak in (255, 255.0, np.float32(1023.0), 1e-3, 2 ** 40):
        assert CalculateOptions(reflectance=True, reflectance_peak=peak).reflectance_peak == float(peak)


def clouds_4():
    pts = np.arange(12, dtype=np.float64).reshape(4, 3)
    return PointCloud(pts, reflectance=np.arange(4, dtype=np.uint16)), PointCloud(pts + 0.5, reflectance=np.arange(4.0)), PointCloud(pts)


def test_check_reflectance():
    with_a, with_b, bare = clouds_4()
    on, off = CalculateOptions(reflectance=True), CalculateOptions()
    check_reflectance(on, with_a, with_b)
    for pair in ((with_a, bare), (bare, with_b), (bare, bare)):
        with pytest.raises(ValueError, match="reflectance of both clouds"):
            check_reflectance(on, *pair)
        check_reflectance(off, *pair, ties="mean", group=object())       # nothing asked for: nothing to refuse
    with pytest.raises(ValueError, match="ties='mean'"):
        check_reflectance(on, with_a, with_b, ties="mean")
    with pytest.raises(ValueError, match="sharded"):
        check_reflectance(on, with_a, with_b, group=object())

    class Open3dLike:                                                        # (no reflectance attribute at all)
        points = np.zeros((4, 3))
    with pytest.raises(ValueError, match="reflectance of both clouds"):
        check_reflectance(on, with_a, Open3dLike())


# ---- PointCloud ---------------------------------------------------------------------------------------------------------------
def test_point_cloud_dtype_rules():
    pts = np.zeros((5, 3))
    for dtype, kept in ((np.uint8, np.uint8), (np.uint16, np.uint16), (np.float32, np.float32), (np.float64, np.float64),
                        (np.int32, np.float64), (np.uint32, np.float64), (np.int16, np.float64), (np.float16, np.float64)):
        c = PointCloud(pts, reflectance=np.arange(5).astype(dtype))
        assert c.reflectance.dtype == kept and c.reflectance.shape == (5,) and c.has_reflectance()
        assert c.reflectance.tolist() == [0, 1, 2, 3, 4]
    assert PointCloud(pts, reflectance=[1, 2, 3, 4, 5]).reflectance.dtype == np.float64
    assert PointCloud(pts, reflectance=np.uint16([[7], [8], [9], [1], [2]])).reflectance.tolist() == [7, 8, 9, 1, 2]
    assert PointCloud(pts, reflectance=np.uint16([[7], [8], [9], [1], [2]])).reflectance.dtype == np.uint16
    bare = PointCloud(pts)
    assert not bare.has_reflectance() and bare.reflectance.shape == (0,)
    bare.reflectance = np.float32([1, 2, 3, 4, 5])
    assert bare.has_reflectance() and bare.reflectance.dtype == np.float32
    bare.reflectance = None
    assert not bare.has_reflectance()
    for bad in (np.zeros((5, 2)), np.zeros((5, 1, 1)), np.float64(3.0), np.zeros((1, 5))):
        with pytest.raises(ValueError, match="reflectance"):
            PointCloud(pts, reflectance=bad)
    assert PointCloud(pts, None, None).has_reflectance() is False            # (the three positional arguments of before)


# ---- IO -----------------------------------------------------------------------------------------------------------------------
def sample(n=37, seed=3):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)), rng.integers(0, 65536, n).astype(np.uint16)


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "ascii"])
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8, np.float32, np.float64])
def test_write_read_round_trip(tmp_path, dtype, binary):
    pts, r16 = sample()
    values = (r16 % 256).astype(np.uint8) if dtype == np.uint8 else r16.astype(dtype) if dtype == np.uint16 else (r16 / 7.0).astype(dtype)
    path = str(tmp_path / "c.ply")
    write_point_cloud(path, PointCloud(pts, reflectance=values), binary=binary)
    header = open(path, "rb").read().split(b"end_header")[0].decode()
    integral = dtype in (np.uint8, np.uint16)
    assert ("property ushort reflectance" in header) == integral and ("property double reflectance" in header) == (not integral)
    back = read_point_cloud(path)
    assert back.has_reflectance() and back.reflectance.dtype == (np.uint16 if integral else np.float64)
    assert np.array_equal(back.reflectance, values.astype(back.reflectance.dtype))     # (every value is a double: exact)
    assert np.array_equal(np.asarray(back.points), pts)


PLY_TYPES = {"ushort": "u2", "uchar": "u1", "float": "f4", "double": "f8", "int": "i4"}


def hand_ply(path, encoding, prop_type, name, pts, values, with_colour=False):
    """A PLY written here, not by write_point_cloud: any property type and name, any of the three encodings."""
    fields = [("x", "f8"), ("y", "f8"), ("z", "f8")] + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if with_colour else []) \
        + [(name, PLY_TYPES[prop_type])]
    order = {"ascii": "=", "binary_little_endian": "<", "binary_big_endian": ">"}[encoding]
    data = np.zeros(len(pts), dtype=np.dtype([(k, order + v) for k, v in fields]))
    for k, col in zip("xyz", pts.T):
        data[k] = col
    data[name] = values
    rev = {"f8": "double", "u1": "uchar", "u2": "ushort", "f4": "float", "i4": "int"}
    header = ["ply", f"format {encoding} 1.0", f"element vertex {len(pts)}"] + [f"property {rev[v]} {k}" for k, v in fields] + ["end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode())
        if encoding == "ascii":
            for row in data:
                fh.write((" ".join(repr(x.item()) for x in row) + "\n").encode())
        else:
            data.tofile(fh)


@pytest.mark.parametrize("encoding", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("prop_type", ["ushort", "uchar", "float", "double", "int"])
def test_ply_property_types_in_three_encodings(tmp_path, encoding, prop_type):
    pts, r16 = sample()
    values = {"ushort": r16, "uchar": (r16 % 256).astype(np.uint8), "float": (r16 / 3.0).astype(np.float32), "double": r16 / 3.0,
              "int": r16.astype(np.int32) - 30000}[prop_type]
    path = str(tmp_path / "c.ply")
    hand_ply(path, encoding, prop_type, "reflectance", pts, values, with_colour=True)
    back = read_point_cloud(path)
    kept = {"ushort": np.uint16, "uchar": np.uint8, "float": np.float32, "double": np.float64, "int": np.float64}[prop_type]
    assert back.reflectance.dtype == kept and back.reflectance.dtype.isnative
    assert np.array_equal(back.reflectance.astype(np.float64), values.astype(np.float64))
    assert back.has_colors() and np.array_equal(np.asarray(back.points), pts)


@pytest.mark.parametrize("name", ["reflectance", "refc", "intensity", "scalar_intensity", "scalar_Intensity"])
def test_ply_alias_names(tmp_path, name):
    pts, r16 = sample()
    path = str(tmp_path / "c.ply")
    hand_ply(path, "binary_little_endian", "ushort", name, pts, r16)
    assert np.array_equal(read_point_cloud(path).reflectance, r16)


def test_ply_first_present_alias_wins_and_unknown_names_are_not_reflectance(tmp_path):
    pts, r16 = sample(5)
    path = str(tmp_path / "c.ply")
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat ascii 1.0\nelement vertex 5\nproperty double x\nproperty double y\nproperty double z\n"
                 b"property ushort intensity\nproperty ushort reflectance\nproperty ushort confidence\nend_header\n")
        for p, v in zip(pts, r16):
            fh.write(f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {int(v) // 2} {int(v)} 9\n".encode())
    assert np.array_equal(read_point_cloud(path).reflectance, r16)            # "reflectance" comes before "intensity" in the list
    hand_ply(path, "ascii", "ushort", "confidence", pts, r16)
    assert not read_point_cloud(path).has_reflectance()


def test_pcd_ascii_intensity(tmp_path):
    pts, r16 = sample(9)
    for field in ("intensity", "reflectance"):
        path = str(tmp_path / f"{field}.pcd")
        with open(path, "w") as fh:
            fh.write(f"# .PCD v0.7\nVERSION 0.7\nFIELDS x y z {field}\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH 9\nHEIGHT 1\n"
                     "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS 9\nDATA ascii\n")
            for p, v in zip(pts.astype(np.float32), r16):
                fh.write(f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {float(v) / 4!r}\n")
        back = read_point_cloud(path)
        assert back.reflectance.dtype == np.float32 and np.array_equal(back.reflectance, (r16 / 4.0).astype(np.float32))
    path = str(tmp_path / "u2.pcd")
    body = np.zeros(9, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<u2")]))
    body["x"], body["y"], body["z"], body["intensity"] = pts[:, 0], pts[:, 1], pts[:, 2], r16
    with open(path, "wb") as fh:
        fh.write(b"VERSION 0.7\nFIELDS x y z intensity\nSIZE 4 4 4 2\nTYPE F F F U\nCOUNT 1 1 1 1\nWIDTH 9\nHEIGHT 1\nPOINTS 9\nDATA binary\n")
        fh.write(body.tobytes())
    back = read_point_cloud(path)
    assert back.reflectance.dtype == np.uint16 and np.array_equal(back.reflectance, r16)


def test_pts_with_and_without_intensity(tmp_path):
    pts, r16 = sample(6)
    rgb = np.random.default_rng(1).integers(0, 256, (6, 3))

    def write(name, cols):
        path = str(tmp_path / name)
        with open(path, "w") as fh:
            fh.write("6\n")
            for row in cols:
                fh.write(" ".join(repr(float(v)) for v in row) + "\n")
        return read_point_cloud(path)

    xyz = write("xyz.pts", pts)
    assert not xyz.has_reflectance() and not xyz.has_colors()
    xyzi = write("xyzi.pts", np.column_stack([pts, r16]))
    assert xyzi.reflectance.dtype == np.float64 and np.array_equal(xyzi.reflectance, r16.astype(np.float64)) and not xyzi.has_colors()
    xyzrgb = write("xyzrgb.pts", np.column_stack([pts, rgb]))
    assert not xyzrgb.has_reflectance() and xyzrgb.has_colors()
    full = write("full.pts", np.column_stack([pts, r16, rgb]))
    assert np.array_equal(full.reflectance, r16.astype(np.float64)) and np.array_equal(np.asarray(full.colors), rgb / 255.0)


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "ascii"])
def test_a_cloud_without_reflectance_writes_the_same_bytes(tmp_path, binary):
    pts, _ = sample()
    rng = np.random.default_rng(5)
    nrm, col = rng.standard_normal((len(pts), 3)), rng.integers(0, 256, (len(pts), 3)) / 255.0

    class Before:                                                            # what a cloud was before it could hold reflectance
        points, normals, colors = pts, nrm, col
        has_normals = has_colors = staticmethod(lambda: True)

    a, b, c = (str(tmp_path / f"{k}.ply") for k in "abc")
    write_point_cloud(a, PointCloud(pts, nrm, col, reflectance=None), binary=binary)
    write_point_cloud(b, PointCloud(pts, nrm, col), binary=binary)
    write_point_cloud(c, Before(), binary=binary)
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    assert b"reflectance" not in open(a, "rb").read()
    assert not read_point_cloud(a).has_reflectance()


# ---- command line: usage errors before any GPU work ---------------------------------------------------------------------------
@pytest.fixture
def ply_pair(tmp_path):
    with_a, with_b, bare = clouds_4()
    paths = {}
    for name, cloud in (("a", with_a), ("b", with_b), ("bare", bare)):
        paths[name] = str(tmp_path / f"{name}.ply")
        write_point_cloud(paths[name], cloud)
    return paths


def test_cli_usage_errors(ply_pair):
    run = CliRunner().invoke
    r = run(cli, ["--ocloud", ply_pair["a"], "--pcloud", ply_pair["bare"], "--reflectance"])
    assert r.exit_code == 2 and "reflectance of both clouds" in r.output
    r = run(cli, ["--ocloud", ply_pair["bare"], "--pcloud", ply_pair["b"], "--reflectance"])
    assert r.exit_code == 2 and "reflectance of both clouds" in r.output
    r = run(cli, ["--ocloud", ply_pair["a"], "--pcloud", ply_pair["b"], "--reflectance", "--ties", "mean"])
    assert r.exit_code == 2 and "ties='mean'" in r.output
    for peak in ("0", "-5", "nan", "inf"):
        r = run(cli, ["--ocloud", ply_pair["a"], "--pcloud", ply_pair["b"], "--reflectance", "--reflectance-peak", peak])
        assert r.exit_code == 2 and "reflectance_peak" in r.output, (peak, r.output)
    r = run(cli, ["--ocloud", ply_pair["a"], "--pcloud", ply_pair["b"], "--reflectance-peak", "abc"])
    assert r.exit_code == 2


# ---- the staleness event, product by product ----------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_reflectance_changed_moves_exactly_what_the_table_says(tmp_path):
    exe = str(tmp_path / "reflectance_stale_host")
    build = subprocess.run(
        [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
         "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "open_pcc_metric_amd", "csrc"),
         os.path.join(ROOT, "tests", "reflectance_stale_host_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout[-4000:])
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert " checks, 0 failed" in run.stdout
