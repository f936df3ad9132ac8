"""Voxel down-sampling, host side: the C-ABI surface, the build recipe, the two CPU restatements (tests/voxel_restatement.py) held against
each other bit for bit, the host arithmetic of the frame and of the composition, the argument checks that run before any device is asked
for, and the unchanged call path of ``score_mesh`` / ``metrics_3d`` without ``voxel_size``."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import icp, lib, metrics3d, refuse, voxel  # noqa: E402
import icp_restatement as R  # noqa: E402
import voxel_restatement as V  # noqa: E402

NEW_EXPORTS = ("vfn_voxel_keys", "vfn_voxel_means")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the small cases the restatements (and tests/test_hip_voxel.py) share
# ---------------------------------------------------------------------------------------------------------------------------------
def uniform(n, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3))


def face_case():
    """Dyadic coordinates at dyadic h = 1/4: (p - origin) / h is an exact integer for every point on a lattice of pitch 1/4 shifted by
    h / 2 = 1/8 (the origin is the lowest point less 1/8), so the points lie exactly on voxel faces; others lie strictly inside."""
    g = np.random.default_rng(11)
    lattice = g.integers(-8, 9, (200, 3)).astype(np.float64) / 4.0 + 0.125
    lattice[0] = [-2.0, -2.0, -2.0]                     # the lowest corner: origin = -2.125, every lattice point then on a face
    inside = g.integers(-64, 65, (100, 3)).astype(np.float64) / 32.0
    return np.concatenate((lattice, inside)), 0.25


def skewed_case(n, seed):
    """Half the points in one voxel (a cube of edge 0.01 inside a voxel of edge 0.05), the rest spread over [-1, 1]^3."""
    g = np.random.default_rng(seed)
    p = g.uniform(-1, 1, (n, 3))
    p[::2] = np.array([0.512, 0.512, 0.512]) + g.uniform(0, 0.01, (len(p[::2]), 3))
    return p


SMALL = {
    "one": (np.array([[0.3, -0.2, 0.9]]), 0.1),
    "two_same": (np.array([[0.30, 0.30, 0.30], [0.31, 0.32, 0.33]]), 0.1),
    "two_apart": (np.array([[0.3, 0.3, 0.3], [0.9, -0.3, 0.3]]), 0.1),
    "n63": (uniform(63, 63), 0.3), "n64": (uniform(64, 64), 0.3), "n65": (uniform(65, 65), 0.3),
    "n255": (uniform(255, 255), 0.2), "n256": (uniform(256, 256), 0.2), "n257": (uniform(257, 257), 0.2),
    "n4097": (uniform(4097, 4097), 0.1),
    "negative": (uniform(1000, 5, -7.0, -3.0), 0.25),
    "far": (1e6 + uniform(1000, 6, 0.0, 0.01), 0.004),          # sub-voxel spread near 10^6: cancellation in p - origin
    "faces": face_case(),
    "skewed": (skewed_case(2000, 7), 0.05),
    "minus_zero": (np.array([[-0.0, -0.0, -0.0]]), 0.5),
}


def assert_same_sample(got: dict, want: dict, what: str):
    for name in ("points", "normals", "colours"):
        assert (got[name] is None) == (want[name] is None), (what, name)
        if want[name] is not None:
            assert got[name].shape == want[name].shape, (what, name, got[name].shape, want[name].shape)
            assert np.array_equal(bits(got[name]), bits(want[name])), f"{what}: {name} differ in {int((bits(got[name]) != bits(want[name])).sum())} values"
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["voxel_of_point"], want["voxel_of_point"]), what
    assert np.array_equal(bits(got["origin"]), bits(want["origin"])) and tuple(got["dims"]) == tuple(want["dims"]), what


# ---------------------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_voxel_keys"] == ("int", ["const double*", "int64_t", "const double*", "double", "int64_t*", "int64_t*", "void*"])
    assert protos["vfn_voxel_means"] == ("int", ["const double*", "int64_t", "int32_t", "const int64_t*", "int64_t", "double*", "int64_t*",
                                                 "void*"])
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    for name in NEW_EXPORTS:
        assert getattr(handle, name).argtypes is not None
    assert lib.voxel_limits() == (1 << 21, 9) and lib.header_constant("VFN_VOXEL_AXIS_BITS") == V.AXIS_BITS
    # the host-side checks of the exports answer without a device
    assert handle.vfn_voxel_keys(None, 0, None, 1.0, None, None, None) != 0 and b"outside [1, 2^31)" in handle.vfn_last_error()
    assert handle.vfn_voxel_keys(None, 5, None, 1.0, None, None, None) != 0 and b"NULL" in handle.vfn_last_error()
    assert handle.vfn_voxel_means(None, 5, 10, None, 2, None, None, None) != 0 and b"channels 10 outside [1, 9]" in handle.vfn_last_error()
    assert handle.vfn_voxel_means(None, 5, 0, None, 2, None, None, None) != 0
    assert handle.vfn_voxel_means(None, 5, 3, None, 6, None, None, None) != 0 and b"n_voxels" in handle.vfn_last_error()
    assert handle.vfn_voxel_means(None, 5, 3, None, 2, None, None, None) != 0 and b"NULL" in handle.vfn_last_error()


def test_build_recipe_lists_the_unit_in_both_places():
    build = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "build.sh")).read()
    assert re.search(r'^UNITS=".*\bvfn_voxel\b.*"', build, flags=re.M)
    assert re.search(r"\|vfn_voxel[|)].*-ffp-contract=off", build)
    assert os.path.exists(os.path.join(REPO, "vf_nerf_amd", "csrc", "vfn_voxel.hip"))


def test_signature_defaults():
    for fn in (metrics3d.score_mesh, metrics3d.precision_recall_fscore, refuse.metrics_3d):
        assert inspect.signature(fn).parameters["voxel_size"].default is None, fn.__name__
    assert list(inspect.signature(metrics3d.voxel_down_sample).parameters) == ["points", "voxel_size", "normals", "colours", "device"]
    assert list(inspect.signature(icp.align_stages).parameters) == ["source_points", "target_points", "stages", "init", "device"]
    assert metrics3d.VoxelDownSample is voxel.VoxelDownSample
    assert [f.name for f in __import__("dataclasses").fields(voxel.VoxelDownSample)] == ["points", "normals", "colours", "counts",
                                                                                       "voxel_of_point", "origin", "dims"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SMALL))
def test_two_restatements_agree_bit_for_bit(name):
    p, h = SMALL[name]
    g = np.random.default_rng(len(p))
    normals, colours = g.standard_normal(p.shape), g.uniform(0, 1, p.shape)
    a, b = V.down_sample(p, h, normals, colours), V.down_sample_dict(p, h, normals, colours)
    assert_same_sample(a, b, name)
    v = len(a["counts"])
    assert a["counts"].sum() == len(p) and a["counts"].min() >= 1 and a["points"].shape == (v, 3)
    assert a["voxel_of_point"].min() == 0 and a["voxel_of_point"].max() == v - 1
    # voxels in ascending (c_0, c_1, c_2), every mean inside its own voxel's closed box (a mean of points of a convex set), up to rounding
    c = V.cells(p, a["origin"], h)
    first = np.array([np.nonzero(a["voxel_of_point"] == j)[0][0] for j in range(v)])
    cv = c[first]
    assert all(tuple(cv[j]) < tuple(cv[j + 1]) for j in range(v - 1))
    assert (c.max(axis=0) + 1 == np.array(a["dims"])).all() and (c.min(axis=0) == 0).all()
    without = V.down_sample(p, h)
    assert without["normals"] is None and without["colours"] is None and np.array_equal(bits(without["points"]), bits(a["points"]))


def test_restated_properties():
    one = V.down_sample(*SMALL["one"])
    assert np.array_equal(bits(one["points"]), bits(SMALL["one"][0])) and one["dims"] == (1, 1, 1)
    assert len(V.down_sample(*SMALL["two_same"])["counts"]) == 1 and len(V.down_sample(*SMALL["two_apart"])["counts"]) == 2
    # the sign bit of a lone -0.0 survives: the sum starts from the first element, not from +0.0
    z = V.down_sample(*SMALL["minus_zero"])["points"]
    assert np.signbit(z).all() and np.signbit(V.down_sample_dict(*SMALL["minus_zero"])["points"]).all()
    # points exactly on voxel faces: the quotient is an exact integer and the point belongs to the voxel that STARTS there
    p, h = SMALL["faces"]
    origin, _ = V.frame(p, h)
    q = (p[1:200] - np.array(origin)) / h                 # (row 0 is the lowest corner itself: half a voxel above the origin)
    assert np.array_equal(q, np.round(q)) and origin == (-2.125, -2.125, -2.125)
    assert np.array_equal(V.cells(p[1:200], origin, h), q) and q.min() >= 1
    # the skewed case has its heavy voxel
    counts = V.down_sample(*SMALL["skewed"])["counts"]
    assert counts.max() == 1000 and len(counts) > 500
    # near 10^6 the subtraction cancels: the points still spread over several voxels per axis
    assert min(V.down_sample(*SMALL["far"])["dims"]) >= 3
    # a permutation of the rows changes the order of summation inside a voxel, the voxels and their numbering do not move
    p, h = SMALL["n4097"]
    perm = np.random.default_rng(3).permutation(len(p))
    a, b = V.down_sample(p, h), V.down_sample(p[perm], h)
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["voxel_of_point"][perm], b["voxel_of_point"])
    assert np.allclose(a["points"], b["points"], rtol=0, atol=1e-15) and a["origin"] == b["origin"]
    # statuses of the restated keys
    k, status = V.keys(np.array([[0.0, 0.0, np.nan], [0.0, 0.0, 0.0], [np.inf, 0.0, 0.0]]), (-0.5, -0.5, -0.5), 1.0)
    assert status == 1 and k.tolist() == [-1, 0, -1]
    k, status = V.keys(np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]]), (0.5, 0.5, 0.5), 1.0)
    assert status == 2 and k.tolist() == [-1, (0 << 42) | (1 << 21) | 2]
    m = V.serial_means(np.arange(12.0).reshape(4, 3), [0, 2, 2, 5])
    assert np.array_equal(m[0], [1.5, 2.5, 3.5]) and np.isnan(m[1]).all() and np.isnan(m[2]).all()


def test_frame_and_composition_are_the_restatements():
    for name, (p, h) in SMALL.items():
        origin, dims = voxel.frame(p.min(axis=0).tolist(), p.max(axis=0).tolist(), h)
        want = V.frame(p, h)
        assert np.array_equal(bits(origin), bits(want[0])) and dims == want[1], name
    lo, hi = voxel.bounding_box(torch.from_numpy(SMALL["far"][0].astype(np.float32)))
    assert lo == SMALL["far"][0].astype(np.float32).min(axis=0).astype(np.float64).tolist()
    for p in (SMALL["n4097"][0], SMALL["n257"][0], uniform(2048, 1), uniform(10000, 2, -5.0, 9.0)):          # tiled above 2047 rows, with a tail
        assert voxel.bounding_box(torch.from_numpy(p)) == (p.min(axis=0).tolist(), p.max(axis=0).tolist())
    a, b = R.motion(), R.rigid((0.3, -1.0, 0.2), 170.0, (0.5, 0.1, -0.7))
    got = icp.compose(a, b)
    assert np.array_equal(bits(got), bits(V.compose(a, b))) and np.array_equal(got[3], [0, 0, 0, 1])
    assert np.abs(got - a @ b).max() <= 4 * 2.0 ** -53 * 2.0 and np.array_equal(icp.compose(np.eye(4), a), a)


def test_restated_stages_recover_a_small_motion():
    src, tgt = R.transform(R.corner_room(1024, 1), R.rigid((1.0, 2.0, 3.0), 1.0, (0.004, -0.002, 0.003))), R.corner_room(1024, 1)
    out = V.align_stages(src, tgt, [(0.05, 0.1, 5), (None, 0.03, 30)])
    first, last = out["stages"]
    assert first["source_points"] < 1024 and first["target_points"] < 1024 and last["source_points"] == 1024
    assert first["iterations"] == 5 and last["converged"]
    err = np.abs(out["transformation"] @ R.rigid((1.0, 2.0, 3.0), 1.0, (0.004, -0.002, 0.003)) - np.eye(4)).max()
    assert err <= 1e-12, err


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals before a device is asked for
# ---------------------------------------------------------------------------------------------------------------------------------
PTS = uniform(5, 0)
TRI_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.array([[0, 1, 2]])
WIDE = np.array([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])               # 3 / 1e-6 > 2^21 voxels along x


@pytest.mark.parametrize("call", [
    lambda: metrics3d.voxel_down_sample(PTS, 0.0),
    lambda: metrics3d.voxel_down_sample(PTS, -0.1),
    lambda: metrics3d.voxel_down_sample(PTS, float("nan")),
    lambda: metrics3d.voxel_down_sample(PTS, float("inf")),
    lambda: metrics3d.voxel_down_sample(PTS, 1e-200),             # its square is subnormal
    lambda: metrics3d.voxel_down_sample(PTS, "0.1"),
    lambda: metrics3d.voxel_down_sample(PTS, True),
    lambda: metrics3d.voxel_down_sample(WIDE, 1e-6),
    lambda: metrics3d.voxel_down_sample(torch.from_numpy(WIDE), 1e-6),
    lambda: metrics3d.voxel_down_sample(np.zeros((5, 2)), 0.1),
    lambda: metrics3d.voxel_down_sample(np.zeros(15), 0.1),
    lambda: metrics3d.voxel_down_sample(np.zeros((0, 3)), 0.1),
    lambda: metrics3d.voxel_down_sample(PTS, 0.1, normals=np.zeros((4, 3))),
    lambda: metrics3d.voxel_down_sample(PTS, 0.1, colours=np.zeros((5, 4))),
    lambda: metrics3d.voxel_down_sample(PTS, 0.1, colours=np.zeros((5, 3), dtype=bool)),
    lambda: metrics3d.precision_recall_fscore(PTS, PTS, 0.1, voxel_size=0.0),
    lambda: metrics3d.precision_recall_fscore(PTS, PTS, 0.1, voxel_size=float("nan")),
    lambda: metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, voxel_size=-1.0),
    lambda: metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, voxel_size=0.025, normals=True),
    lambda: refuse.metrics_3d(None, None, None, None, 4, 4, voxel_size=0.025, normals=True),
    lambda: refuse.metrics_3d(None, None, None, None, 4, 4, voxel_size=0.0),
    lambda: icp.align_stages(PTS, PTS, []),
    lambda: icp.align_stages(PTS, PTS, [(0.1, 0.2)]),
    lambda: icp.align_stages(PTS, PTS, [(0.0, 0.2, 5)]),
    lambda: icp.align_stages(PTS, PTS, [(None, 0.0, 5)]),
    lambda: icp.align_stages(PTS, PTS, [(None, 0.2, -1)]),
    lambda: icp.align_stages(PTS, PTS, [(None, 0.2, 2.5)]),
    lambda: icp.align_stages(PTS, PTS, 0.1),
    lambda: icp.align_stages(np.zeros((5, 2)), PTS, [(None, 0.2, 5)]),
    lambda: icp.align_stages(PTS, PTS, [(None, 0.2, 5)], init=np.eye(3)),
])
def test_bad_arguments_raise_before_any_device_call(call, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    for module in (voxel, icp, metrics3d):
        monkeypatch.setattr(module, "_device", no_device)
    monkeypatch.setattr(refuse, "reconstruction_meshes", no_device)
    with pytest.raises(ValueError):
        call()


def test_voxel_size_with_normals_says_why():
    with pytest.raises(ValueError, match="normal consistency is not defined"):
        metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, voxel_size=0.025, normals=True)


def test_binding_refuses_channels_and_shapes_before_the_device():
    """More than nine channels, and tables that cannot belong to the rows, are refused on the host tensors they arrive as."""
    start = torch.tensor([0, 5], dtype=torch.int64)
    with pytest.raises(lib.VfnError, match="1 to 9"):
        lib.voxel_means(torch.zeros(5, 10, dtype=torch.float64), start)
    with pytest.raises(lib.VfnError, match="1 to 9"):
        lib.voxel_means(torch.zeros(5, 0, dtype=torch.float64), start)
    with pytest.raises(lib.VfnError, match="entries"):
        lib.voxel_means(torch.zeros(5, 3, dtype=torch.float64), torch.zeros(7, dtype=torch.int64))
    with pytest.raises(lib.VfnError, match="entries"):
        lib.voxel_means(torch.zeros(5, 3, dtype=torch.float64), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(lib.VfnError, match=r"\[n,C\]"):
        lib.voxel_means(torch.zeros(15, dtype=torch.float64), start)
    with pytest.raises(lib.VfnError, match=r"\[n,3\]"):
        lib.voxel_keys(torch.zeros(5, 2, dtype=torch.float64), (0.0, 0.0, 0.0), 1.0)


def test_wrong_container_types_raise_type_error():
    with pytest.raises(TypeError):
        metrics3d.voxel_down_sample([[0.0, 0.0, 0.0]], 0.1)
    with pytest.raises(TypeError):
        metrics3d.voxel_down_sample(PTS, 0.1, normals="normals.npy")


def test_non_finite_box_raises_the_status_error():
    bad = PTS.copy()
    bad[2, 1] = np.nan
    with pytest.raises(lib.VfnError, match="non-finite"):
        metrics3d.voxel_down_sample(bad, 0.1)
    bad[2, 1] = -np.inf
    with pytest.raises(lib.VfnError, match="non-finite"):
        metrics3d.voxel_down_sample(bad, 0.1)
    for row in (7, 4096):                                   # inside a tile of the box's reduction, and in its tail
        big = SMALL["n4097"][0].copy()
        big[row, 2] = np.nan
        with pytest.raises(lib.VfnError, match="non-finite"):
            metrics3d.voxel_down_sample(big, 0.1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is visible: the calls would run")
def test_no_cpu_fallback():
    with pytest.raises(lib.VfnError, match="no GPU"):
        metrics3d.voxel_down_sample(PTS, 0.1)
    with pytest.raises(lib.VfnError, match="no GPU"):
        metrics3d.precision_recall_fscore(PTS, PTS, 0.1, voxel_size=0.05)
    with pytest.raises(lib.VfnError, match="no GPU"):
        icp.align_stages(PTS, PTS, [(0.1, 0.2, 5)])
    with pytest.raises(lib.VfnError):
        lib.voxel_keys(torch.zeros(4, 3, dtype=torch.float64), (0.0, 0.0, 0.0), 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the call paths, the device stood in for
# ---------------------------------------------------------------------------------------------------------------------------------
def test_score_mesh_without_voxel_size_takes_todays_path(monkeypatch):
    calls = []

    def sample(v, f, count, generator=None, uniforms=None, device=None):
        calls.append(("sample", count, generator, uniforms))
        return torch.full((count, 3), float(len(calls))), None

    def both(pred, ref, threshold, device=None, **kw):
        calls.append(("both", float(pred[0, 0]), float(ref[0, 0]), threshold, tuple(pred.shape), kw))
        return np.array([[4.0, 0.0, 2.0, 1.0, 1.0, 4.0, 3.0], [3.0, 0.5, 1.0, 1.0, 1.0, 3.0, 2.0]])

    def no_voxel(*a, **k):
        raise AssertionError("the down-sampling was reached")

    monkeypatch.setattr(metrics3d, "sample_surface", sample)
    monkeypatch.setattr(metrics3d, "_both_directions", both)
    monkeypatch.setattr(metrics3d, "_voxel_pair", no_voxel)
    plain = metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, distance_thresh=0.25, generator="g")
    first = list(calls)
    del calls[:]
    explicit = metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, distance_thresh=0.25, generator="g", voxel_size=None)
    assert plain == explicit and calls == first and "voxel" not in plain
    assert first == [("sample", 10, "g", None), ("sample", 10, "g", None), ("both", 1.0, 2.0, 0.25, (10, 3), {})]
    assert metrics3d.precision_recall_fscore(PTS, PTS, 0.25, voxel_size=None) == metrics3d.precision_recall_fscore(PTS, PTS, 0.25)

    # with a value: the pair goes through the down-sampling after the sampling, and the search keyword still arrives
    def pair(pred, ref, size, device=None):
        calls.append(("voxel", float(pred[0, 0]), float(ref[0, 0]), size))
        return pred[:4] + 10.0, ref[:3] + 10.0, {"size": size, "pred_points": 4, "ref_points": 3}

    monkeypatch.setattr(metrics3d, "_voxel_pair", pair)
    del calls[:]
    out = metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, distance_thresh=0.25, generator="g", voxel_size=0.125,
                               search="grid")
    assert calls[:2] == first[:2] and calls[2] == ("voxel", 1.0, 2.0, 0.125)
    assert calls[3] == ("both", 11.0, 12.0, 0.25, (4, 3), {"search": "grid"})
    assert out["voxel"] == {"size": 0.125, "pred_points": 4, "ref_points": 3}
    assert {k: v for k, v in out.items() if k != "voxel"} == plain


def test_metrics_3d_passes_voxel_size_through(monkeypatch):
    got = []
    monkeypatch.setattr(refuse, "reconstruction_meshes", lambda *a, **k: {name: (torch.zeros(1, 3), name) for name in refuse.MESH_NAMES})
    monkeypatch.setattr(metrics3d, "score_mesh", lambda mesh, gt, **k: got.append(k) or {"mesh": mesh[1]})
    refuse.metrics_3d("tsdf", "gt", None, None, 4, 4, num_points=7)
    assert len(got) == 4 and all("voxel_size" not in k for k in got)
    del got[:]
    refuse.metrics_3d("tsdf", "gt", None, None, 4, 4, num_points=7, voxel_size=0.025)
    assert len(got) == 4 and all(k["voxel_size"] == 0.025 and k["num_points"] == 7 for k in got)
