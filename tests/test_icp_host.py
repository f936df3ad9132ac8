"""Point-set alignment, host side: the CPU restatement (tests/icp_restatement.py) pinned to scipy's cKDTree and to the motion it must
recover, the rigid solve's properties, the C-ABI surface, the argument checks that run before any device call, and the unchanged call
path of ``score_mesh`` / ``metrics_3d`` without ``icp_align``."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import icp, lib, metrics3d, refuse  # noqa: E402
import icp_restatement as R  # noqa: E402

NEW_EXPORTS = ("vfn_transform_points", "vfn_nn_radius", "vfn_icp_accumulate_workspace_bytes", "vfn_icp_accumulate")
M = R.motion()
N_ROOM = 4096


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


_pairs = {}


def room_pair(seed):
    """(source, targets, radius): the seed-1 corner room as targets; the source is M applied to the seed-1 cloud (the same points,
    r = 0.05) or to the seed-2 cloud (another sampling of the same surface, r = 0.1)."""
    if seed not in _pairs:
        _pairs[seed] = (R.transform(R.corner_room(N_ROOM, seed), M), R.corner_room(N_ROOM, 1), 0.05 if seed == 1 else 0.1)
    return _pairs[seed]


_aligned = {}


def restated_align(seed):
    if seed not in _aligned:
        _aligned[seed] = R.align(*room_pair(seed))
    return _aligned[seed]


def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_transform_points"] == ("int", ["const double*", "int64_t", "const double*", "double*", "void*"])
    assert protos["vfn_nn_radius"] == ("int", ["const double*", "int64_t", "const double*", "const double*", "const int64_t*", "int64_t",
                                               "const int32_t*", "const double*", "int32_t", "int32_t", "int32_t", "double", "const int64_t*",
                                               "int32_t", "int64_t*", "double*", "int64_t*", "void*"])
    assert lib.header_abi_version() == 5
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    assert handle.vfn_abi_version() == 5
    for name in NEW_EXPORTS:
        assert getattr(handle, name).argtypes is not None
    # the host-side checks of the exports answer without a device
    assert handle.vfn_icp_accumulate_workspace_bytes(1) == 17 * 8 and handle.vfn_icp_accumulate_workspace_bytes(4097) == 2 * 17 * 8
    assert handle.vfn_icp_accumulate_workspace_bytes(0) == -1 and handle.vfn_icp_accumulate_workspace_bytes(1 << 31) == -1
    assert handle.vfn_nn_radius(None, 0, None, None, None, 5, None, None, 1, 1, 1, 1.0, None, 1, None, None, None, None) != 0
    assert b"outside [1, 2^31)" in handle.vfn_last_error()
    assert handle.vfn_transform_points(None, 1 << 31, None, None, None) != 0
    # the grid's limits are the header's, in the kernels and in the binding alike
    assert lib.icp_grid_limits() == (128, 1.0 + 2.0 ** -20) and (icp.GRID_CAP, icp.GRID_MARGIN) == lib.icp_grid_limits()
    assert lib.icp_sum_levels(4096) == 22 and lib.icp_sum_levels(4096 * 1024 + 5) == 23 and lib.ICP_SUMS == R.SUMS


def test_corner_room_recipe():
    t = R.corner_room(N_ROOM, 1)
    assert t.shape == (N_ROOM, 3)
    back = t + np.array([0.4, 0.3, 0.2])
    assert np.all(np.abs(back[:1024, 2]) < 1e-15) and np.all(np.abs(back[1024:2048, 1]) < 1e-15) and np.all(np.abs(back[2048:3072, 0]) < 1e-15)
    e = (back[3072:] - np.array([0.6, 0.4, 0.3])) / np.array([0.15, 0.105, 0.075])
    assert np.allclose((e * e).sum(axis=1), 1.0, atol=1e-12)
    rot = M[:3, :3]
    assert np.allclose(rot @ rot.T, np.eye(3), atol=1e-15) and abs(np.trace(rot) - (1 + 2 * np.cos(np.radians(5.0)))) < 1e-15
    assert np.allclose(rot @ np.array([1.0, 2.0, 3.0]), [1.0, 2.0, 3.0], atol=1e-15) and np.allclose(M[:3, 3], [0.03, -0.015, 0.021])


@pytest.mark.parametrize("n,m,r", [(3000, 5000, 0.065), (1805, 1037, 0.108), (500, 20000, 0.04)])
def test_restated_search_equals_ckdtree(n, m, r):
    """Indices and distance bits are cKDTree's wherever the nearest distance is not within 1e-12 of r and the minimum is unique;
    scipy's behaviour exactly at r is not relied on."""
    g = np.random.default_rng(7 * n + m)
    q, t = g.uniform(-1, 1, (n, 3)), g.uniform(-1, 1, (m, 3))
    t[-5:] = t[:5]                                         # five coincident pairs of targets: not unique, masked below when they are nearest
    index, sqdist = R.nearest_within(q, t, r)
    free_i, free_d = R.nearest_within(q, t, 1e3)           # the unbounded search
    assert (free_i >= 0).all()
    dist, tree_i = cKDTree(t).query(q, distance_upper_bound=r)
    unique = np.ones(n, dtype=bool)                       # (independent uniform coordinates: the planted pairs are the only ties)
    unique[np.isin(free_i, np.concatenate((np.arange(5), np.arange(m - 5, m))))] = False
    clear = np.abs(np.sqrt(free_d) - r) > 1e-12
    ok = unique & clear
    assert ok.sum() > 0.9 * n
    found = index >= 0
    assert 0.05 * n < found.sum() < 0.95 * n, "the radius should split the queries"
    assert np.array_equal(found[ok], (tree_i < m)[ok])
    both = ok & found
    assert np.array_equal(index[both], tree_i[both])
    assert np.array_equal(bits(np.sqrt(sqdist[both])), bits(dist[both]))
    assert np.all(np.isinf(sqdist[~found])) and np.all(np.isinf(dist[ok & ~found]))
    assert np.array_equal(index[found], free_i[found]) and np.array_equal(bits(sqdist[found]), bits(free_d[found]))
    # the tiling of the restatement does not change a bit; ties go to the lowest index
    again = R.nearest_within(q[:300], t, r, rows=7, tile=333)
    assert np.array_equal(again[0], index[:300]) and np.array_equal(bits(again[1]), bits(sqdist[:300]))
    ti, td = R.nearest_within(t[:5], t, r)
    assert np.array_equal(ti, np.arange(5)) and np.all(td == 0)


def test_restated_align_recovers_the_motion():
    out = restated_align(1)
    first = out["history"][0]
    err = np.abs(out["transformation"] @ M - np.eye(4)).max()
    print(f"seed 1: {first['count']} of {N_ROOM} admitted at first, {out['iterations']} iterations, max|T M - I| = {err:.3g}")
    assert first["count"] == 3982 and first["count"] < N_ROOM            # the bounded search rejects rows: the radius matters
    assert out["converged"] and out["iterations"] == 11
    assert err <= 1e-13
    assert out["history"][-1]["count"] == N_ROOM and out["fitness"] == 1.0


def test_restated_align_on_another_sampling():
    out = restated_align(2)
    err = np.abs(out["transformation"] @ M - np.eye(4)).max()
    print(f"seed 2: {out['iterations']} iterations, rmse {out['inlier_rmse']:.4g}, max|T M - I| = {err:.3g}")
    assert out["converged"] and out["iterations"] <= 30
    assert abs(out["inlier_rmse"] - 0.0115) < 5e-4
    assert err < 2e-2                                                    # a sanity bound on the restatement, not a device tolerance


SOLVES = [pytest.param(lambda p, s: R.solve_pairs(p, s), R.SolveError, id="restatement"),
          pytest.param(lambda p, s: icp.rigid_from_sums(R.sums_of(R.terms(p, None, s, np.arange(len(p)), np.zeros(len(p)), R.bounding_anchor(s))),
                                                        R.bounding_anchor(s)), lib.VfnError, id="package")]


@pytest.mark.parametrize("solve,error", SOLVES)
def test_solve_properties(solve, error):
    g = np.random.default_rng(5)
    p = g.uniform(-1, 1, (200, 3)) + np.array([50.0, -20.0, 10.0])       # far from the origin: the anchor keeps the covariance
    for move in (M, R.rigid((0.3, -1.0, 0.2), 170.0, (0.5, 0.1, -0.7))):
        s = R.transform(p, move)
        u = solve(p, s)
        r = u[:3, :3]
        assert np.abs(r.T @ r - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(r) - 1.0) <= 1e-14
        assert np.abs(u - move).max() < 1e-11 and np.array_equal(u[3], [0, 0, 0, 1])
    # a mirrored configuration: the best ROTATION is returned, never the reflection
    s = p * np.array([1.0, 1.0, -1.0])
    r = solve(p, s)[:3, :3]
    assert abs(np.linalg.det(r) - 1.0) <= 1e-14 and np.abs(r.T @ r - np.eye(3)).max() <= 1e-14
    with pytest.raises(error, match="fewer than 3"):
        solve(p[:2], p[:2])
    line = np.outer(np.linspace(-1, 1, 50), [1.0, 2.0, -0.5]) + 3.0
    with pytest.raises(error, match="collinear"):
        solve(line, line + 0.1)


PTS = np.random.default_rng(0).uniform(-1, 1, (5, 3))
EYE = np.eye(4)
BAD_T = np.eye(4)
BAD_T[1, 2] = np.nan
TRI_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.array([[0, 1, 2]])


@pytest.mark.parametrize("call", [
    lambda: icp.nearest_within(np.zeros((5, 2)), PTS, 0.1),
    lambda: icp.nearest_within(PTS, np.zeros(15), 0.1),
    lambda: icp.nearest_within(np.zeros((0, 3)), PTS, 0.1),
    lambda: icp.nearest_within(PTS, torch.zeros(0, 3), 0.1),
    lambda: icp.nearest_within(PTS, np.zeros((4, 3), dtype=np.int64), 0.1),
    lambda: icp.nearest_within(PTS, PTS, 0.0),
    lambda: icp.nearest_within(PTS, PTS, -1.0),
    lambda: icp.nearest_within(PTS, PTS, float("nan")),
    lambda: icp.nearest_within(PTS, PTS, float("inf")),
    lambda: icp.nearest_within(PTS, PTS, 1e-200),
    lambda: icp.nearest_within(PTS, PTS, "0.1"),
    lambda: icp.nearest_within(PTS, PTS, True),
    lambda: icp.nearest_within(PTS, PTS, 0.1, transform=np.eye(3)),
    lambda: icp.nearest_within(PTS, PTS, 0.1, transform=BAD_T),
    lambda: icp.nearest_within(PTS, PTS, 0.1, transform=np.ones((4, 4))),
    lambda: icp.align(np.zeros((5, 2)), PTS, 0.1),
    lambda: icp.align(PTS, np.zeros((0, 3)), 0.1),
    lambda: icp.align(PTS.astype(np.int32), PTS, 0.1),
    lambda: icp.align(PTS, PTS, 0.0),
    lambda: icp.align(PTS, PTS, float("nan")),
    lambda: icp.align(PTS, PTS, float("inf")),
    lambda: icp.align(PTS, PTS, 0.1, init=BAD_T),
    lambda: icp.align(PTS, PTS, 0.1, init=np.eye(4, dtype=np.int64)),
    lambda: icp.align(PTS, PTS, 0.1, max_iteration=-1),
    lambda: icp.align(PTS, PTS, 0.1, max_iteration=2.5),
    lambda: icp.align(PTS, PTS, 0.1, max_iteration=True),
    lambda: icp.align(PTS, PTS, 0.1, relative_fitness=-1e-6),
    lambda: icp.align(PTS, PTS, 0.1, relative_rmse=float("nan")),
    lambda: icp.transform_points(PTS, None),
    lambda: icp.transform_points(PTS, np.eye(3)),
    lambda: icp.transform_points(np.zeros((3, 4)), EYE),
    lambda: icp.transform_points(PTS, BAD_T),
    lambda: metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, icp_align=True, icp_threshold=0.0),
    lambda: metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, icp_align=True, icp_threshold=float("nan")),
    lambda: metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, icp_align=True, distance_thresh=0.0),
    lambda: metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, icp_align=1),
])
def test_bad_arguments_raise_before_any_device_call(call, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(icp, "_device", no_device)
    monkeypatch.setattr(metrics3d, "_device", no_device)
    with pytest.raises(ValueError):
        call()


def test_wrong_container_types_raise_type_error():
    with pytest.raises(TypeError):
        icp.nearest_within([[0.0, 0.0, 0.0]], PTS, 0.1)
    with pytest.raises(TypeError):
        icp.align(PTS, "cloud.ply", 0.1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is visible: the calls would run")
def test_no_cpu_fallback():
    with pytest.raises(lib.VfnError, match="no GPU"):
        icp.nearest_within(PTS, PTS, 0.1)
    with pytest.raises(lib.VfnError, match="no GPU"):
        icp.align(PTS, PTS, 0.1)
    with pytest.raises(lib.VfnError, match="no GPU"):
        icp.transform_points(PTS, EYE)
    with pytest.raises(lib.VfnError):
        lib.transform_points(torch.zeros(4, 3, dtype=torch.float64), None)


def test_score_mesh_without_icp_takes_todays_path(monkeypatch):
    """The device stood in for: without icp_align (absent or False) score_mesh samples twice, searches once per direction and never
    reaches the alignment; the dictionary has today's keys.  With it, the aligned samples are what is scored."""
    calls = []

    def sample(v, f, count, generator=None, uniforms=None, device=None):
        calls.append(("sample", count, generator, uniforms))
        return torch.full((count, 3), float(len(calls))), None

    def both(pred, ref, threshold, device=None):
        calls.append(("both", float(pred[0, 0]), float(ref[0, 0]), threshold))
        return np.array([[4.0, 0.0, 2.0, 1.0, 1.0, 4.0, 3.0], [3.0, 0.5, 1.0, 1.0, 1.0, 3.0, 2.0]])

    def no_align(*a, **k):
        raise AssertionError("the alignment was reached")

    monkeypatch.setattr(metrics3d, "sample_surface", sample)
    monkeypatch.setattr(metrics3d, "_both_directions", both)
    monkeypatch.setattr(icp, "align", no_align)
    monkeypatch.setattr(icp, "transform_points", no_align)
    plain = metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, distance_thresh=0.25, generator="g")
    first = list(calls)
    del calls[:]
    explicit = metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, distance_thresh=0.25, generator="g", icp_align=False,
                                    icp_threshold=0.5)
    assert plain == explicit and calls == first
    assert first == [("sample", 10, "g", None), ("sample", 10, "g", None), ("both", 1.0, 2.0, 0.25)]
    assert set(plain) == {"chamfer distance", "precision", "recall", "fscore", "pred_within", "ref_within"}
    assert plain["chamfer distance"] == {"mean": 2.0, "median": 2.0, "min": 0.0, "max": 2.0}

    seen = {}

    def align(src, tgt, radius, device=None):
        seen["align"] = (float(src[0, 0]), float(tgt[0, 0]), radius)
        return icp.Result(M.copy(), 0.75, 0.01, 7, True, [])

    def moved(points, transformation, device=None):
        seen["moved"] = transformation
        return points + 40.0

    monkeypatch.setattr(icp, "align", align)
    monkeypatch.setattr(icp, "transform_points", moved)
    del calls[:]
    out = metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, distance_thresh=0.25, generator="g", icp_align=True)
    assert seen["align"] == (1.0, 2.0, 0.25) and np.array_equal(seen["moved"], M)          # icp_threshold None: distance_thresh
    assert calls[:2] == first[:2] and calls[2] == ("both", 41.0, 2.0, 0.25)
    assert out["icp"] == {"transformation": M.tolist(), "fitness": 0.75, "inlier_rmse": 0.01, "iterations": 7}
    assert {k: v for k, v in out.items() if k != "icp"} == plain
    metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, distance_thresh=0.25, icp_align=True, icp_threshold=0.5)
    assert seen["align"][2] == 0.5


def test_metrics_3d_passes_the_keywords_through(monkeypatch):
    got = []
    monkeypatch.setattr(refuse, "reconstruction_meshes", lambda *a, **k: {name: (torch.zeros(1, 3), name) for name in refuse.MESH_NAMES})
    monkeypatch.setattr(metrics3d, "score_mesh", lambda mesh, gt, **k: got.append(k) or {"mesh": mesh[1]})
    out = refuse.metrics_3d("tsdf", "gt", None, None, 4, 4, num_points=7)
    assert list(out) == list(refuse.MESH_NAMES) and all(k["icp_align"] is False and k["icp_threshold"] is None for k in got)
    del got[:]
    refuse.metrics_3d("tsdf", "gt", None, None, 4, 4, num_points=7, icp_align=True, icp_threshold=0.2)
    assert len(got) == 4 and all(k["icp_align"] is True and k["icp_threshold"] == 0.2 and k["num_points"] == 7 for k in got)
