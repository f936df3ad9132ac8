"""Mesh scoring, host side: the CPU restatement (tests/metrics3d_restatement.py) pinned to scipy's cKDTree — the KD-tree the reference
queries (utils/utils.py:351-360) — bit for bit, the hand-computed statistics, the C-ABI surface and the argument checks that run before
any device call."""
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

from vf_nerf_amd import lib, mesh, metrics3d  # noqa: E402
import metrics3d_restatement as R  # noqa: E402

NEW_EXPORTS = ("vfn_nn_sqdist", "vfn_tri_areas", "vfn_cumsum_workspace_bytes", "vfn_cumsum_f64", "vfn_sample_surface",
               "vfn_reduce_stats_workspace_bytes", "vfn_reduce_stats")


def nn_case(name):
    """The three seeded (queries, targets) inputs of the nearest-neighbour contract."""
    if name == "jitter":          # 20 000 x 20 000 uniform in [-1, 1]^3, every query a target moved by 1e-3 noise
        g = np.random.default_rng(101)
        t = g.uniform(-1.0, 1.0, (20000, 3))
        return t[g.permutation(20000)] + 1e-3 * g.standard_normal((20000, 3)), t
    if name == "coincident":      # 30 000 x 10 000 in [-3, 3]^3, 100 queries ON a target, 100 targets stored twice
        g = np.random.default_rng(202)
        t = g.uniform(-3.0, 3.0, (10000, 3))
        t[9900:] = t[g.choice(9900, 100, replace=False)]
        q = g.uniform(-3.0, 3.0, (30000, 3))
        q[g.choice(30000, 100, replace=False)] = t[g.choice(10000, 100, replace=False)]
        return q, t
    if name == "small":           # 5 000 x 40 000 in [-0.05, 0.05]^3
        g = np.random.default_rng(303)
        return g.uniform(-0.05, 0.05, (5000, 3)), g.uniform(-0.05, 0.05, (40000, 3))
    raise KeyError(name)


NN_CASES = ("jitter", "coincident", "small")


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", NN_CASES)
def test_brute_force_equals_ckdtree_bit_for_bit(name):
    q, t = nn_case(name)
    mine = R.nearest_distances(q, t, workers=8)
    tree = cKDTree(t).query(q)[0]
    assert np.array_equal(bits(mine), bits(tree)), f"{name}: {int((bits(mine) != bits(tree)).sum())} of {len(q)} distances differ"
    if name == "coincident":
        assert int((mine == 0).sum()) >= 100 and np.array_equal(mine == 0, tree == 0)
    # the tiling of the restatement does not change a bit
    assert np.array_equal(bits(R.nn_sqdist(q[:700], t, rows=64, tile=333)), bits(R.nn_sqdist(q[:700], t)))


def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_nn_sqdist"] == ("int", ["const double*", "int64_t", "const double*", "int64_t", "double*", "int64_t*", "void*"])
    assert lib.header_abi_version() == 5
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    for name in NEW_EXPORTS:
        assert getattr(handle, name).argtypes is not None
    # the host-side size checks of the exports answer without a device
    assert handle.vfn_cumsum_workspace_bytes(1024) == 0 and handle.vfn_cumsum_workspace_bytes(1025) == 16
    assert handle.vfn_cumsum_workspace_bytes(1024 * 1024 + 1) == 8 * (1025 + 2)
    assert handle.vfn_reduce_stats_workspace_bytes(4097) == 64
    assert handle.vfn_cumsum_workspace_bytes(0) == -1 and handle.vfn_reduce_stats_workspace_bytes(1 << 31) == -1
    assert handle.vfn_nn_sqdist(None, 0, None, 5, None, None, None) != 0 and b"outside [1, 2^31)" in handle.vfn_last_error()
    assert handle.vfn_nn_sqdist(None, 5, None, 1 << 31, None, None, None) != 0
    assert lib.cumsum_levels(1024) == 1 and lib.cumsum_levels(1025) == 2 and lib.cumsum_levels(1 << 20) == 2 and lib.cumsum_levels((1 << 20) + 1) == 3
    assert lib.reduce_sum_levels(2500000) == 22 and lib.reduce_sum_levels(4096 * 1024 + 1) == 23


PTS = np.zeros((5, 3))
TRI_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.array([[0, 1, 2]])


@pytest.mark.parametrize("call", [
    lambda: metrics3d.nearest_distances(np.zeros((5, 2)), PTS),
    lambda: metrics3d.nearest_distances(PTS, np.zeros(15)),
    lambda: metrics3d.nearest_distances(np.zeros((0, 3)), PTS),
    lambda: metrics3d.nearest_distances(PTS, torch.zeros(0, 3)),
    lambda: metrics3d.nearest_distances(PTS, np.zeros((4, 3), dtype=bool)),
    lambda: metrics3d.chamfer_from_points(np.zeros((0, 3)), PTS),
    lambda: metrics3d.chamfer_from_points(PTS, np.zeros((3, 3, 1))),
    lambda: metrics3d.precision_recall_fscore(PTS, PTS, -0.1),
    lambda: metrics3d.precision_recall_fscore(PTS, PTS, float("nan")),
    lambda: metrics3d.precision_recall_fscore(PTS, PTS, float("inf")),
    lambda: metrics3d.precision_recall_fscore(PTS, np.zeros((0, 3)), 0.1),
    lambda: metrics3d.sample_surface(TRI_V, TRI_F.astype(np.float64), 10),
    lambda: metrics3d.sample_surface(TRI_V, np.zeros((0, 3), dtype=np.int64), 10),
    lambda: metrics3d.sample_surface(TRI_V, np.array([0, 1, 2]), 10),
    lambda: metrics3d.sample_surface(TRI_V[:, :2], TRI_F, 10),
    lambda: metrics3d.sample_surface(TRI_V, TRI_F, 0),
    lambda: metrics3d.sample_surface(TRI_V, TRI_F, -3),
    lambda: metrics3d.sample_surface(TRI_V, TRI_F, 2.5),
    lambda: metrics3d.sample_surface(TRI_V, TRI_F, 4, uniforms=np.zeros((5, 3))),
    lambda: metrics3d.chamfer_distance((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=0),
    lambda: metrics3d.chamfer_distance((TRI_V, TRI_F.astype(np.float32)), (TRI_V, TRI_F), num_points=10),
    lambda: metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, np.zeros((0, 3), dtype=np.int64)), num_points=10),
    lambda: metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10, distance_thresh=-1.0),
    lambda: metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=0),
])
def test_bad_arguments_raise_before_any_device_call(call, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(metrics3d, "_device", no_device)
    with pytest.raises(ValueError):
        call()


def test_wrong_container_types_raise_type_error():
    with pytest.raises(TypeError):
        metrics3d.nearest_distances([[0.0, 0.0, 0.0]], PTS)
    with pytest.raises(TypeError):
        metrics3d.score_mesh("mesh.ply", (TRI_V, TRI_F))


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is visible: the calls would run")
def test_no_cpu_fallback():
    with pytest.raises(lib.VfnError, match="no GPU"):
        metrics3d.nearest_distances(PTS, PTS)
    with pytest.raises(lib.VfnError, match="no GPU"):
        metrics3d.score_mesh((TRI_V, TRI_F), (TRI_V, TRI_F), num_points=10)
    with pytest.raises(lib.VfnError):
        lib.nn_sqdist(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64))


def test_a_mesh_tuple_uses_its_scaled_vertices():
    m = mesh.Mesh(torch.zeros(3, 3, dtype=torch.float64), torch.tensor([[0, 1, 2]]), torch.ones(3, 3, dtype=torch.float64))
    v, f = metrics3d._check_mesh(m, "m")
    assert v is not None and torch.equal(v, m.vertices_scaled) and torch.equal(f, m.faces)


# pred has an odd count, ref an even one.  Nearest distances, by hand:
#   ref -> pred:  (0,0,0) 0   (1,0,0) 0   (0,0,3) 3 [to (0,0,0)]   (4,0,0) 3 [to (1,0,0)]      squares 0 0 9 9
#   pred -> ref:  (0,0,0) 0   (1,0,0) 0   (0,2,0) 2 [to (0,0,0)]                              squares 0 0 4
HAND_PRED = np.array([[0.0, 0, 0], [1, 0, 0], [0, 2, 0]])
HAND_REF = np.array([[0.0, 0, 0], [1, 0, 0], [0, 0, 3], [4, 0, 0]])


def test_restatement_statistics_by_hand():
    assert np.array_equal(R.nearest_distances(HAND_REF, HAND_PRED), [0.0, 0.0, 3.0, 3.0])
    assert np.array_equal(R.nearest_distances(HAND_PRED, HAND_REF), [0.0, 0.0, 2.0])
    mean, median, mn, mx = R.chamfer_from_points(HAND_PRED, HAND_REF)
    assert mean == 18.0 / 4.0 + 4.0 / 3.0                   # the sum of the two directions' means
    assert median == (0.0 + 9.0) / 2.0 + 0.0                # even count: the mean of the two middle values; odd count: the middle value
    assert mn == 0.0 and mx == 9.0
    assert R.median([5.0, 1.0, 3.0]) == 3.0 and R.median([4.0, 1.0, 3.0, 2.0]) == 2.5 and R.median([7.0]) == 7.0
    assert R.median(np.arange(10.0)) == np.median(np.arange(10.0)) and R.median(np.arange(11.0)) == np.median(np.arange(11.0))
    # strictly closer than the threshold: at 2.0 the pred point at distance 2 does not count, at 2.5 it does
    r = R.precision_recall_fscore(HAND_PRED, HAND_REF, 2.0)
    assert (r["pred_within"], r["ref_within"]) == (2, 2) and r["precision"] == 2 / 3 and r["recall"] == 0.5
    assert r["fscore"] == 2 * (2 / 3) * 0.5 / (2 / 3 + 0.5)
    r = R.precision_recall_fscore(HAND_PRED, HAND_REF, 2.5)
    assert (r["pred_within"], r["ref_within"]) == (3, 2) and r["precision"] == 1.0 and r["recall"] == 0.5 and r["fscore"] == 2 * 0.5 / 1.5
    r = R.precision_recall_fscore(HAND_PRED, HAND_REF, 3.5)
    assert r["precision"] == r["recall"] == r["fscore"] == 1.0
    r = R.precision_recall_fscore(HAND_PRED, HAND_REF, 0.0)
    assert r["precision"] == r["recall"] == r["fscore"] == 0.0


def test_restatement_sampling_by_hand():
    # a unit right triangle (area 1/2), a degenerate triangle (area 0), a 2 x 2 right triangle (area 2)
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [0, 0, 1], [2, 0, 1], [0, 2, 1]])
    f = np.array([[0, 1, 2], [3, 3, 3], [4, 5, 6]])
    areas = R.tri_areas(v, f)
    assert np.array_equal(areas, [0.5, 0.0, 2.0])
    cum = np.cumsum(areas)
    u = np.array([[0.0, 0.25, 0.25], [0.19, 0.75, 0.75], [0.2, 0.5, 0.0], [0.999, 0.0, 1.0], [0.5, 1.0, 0.5]])
    pts, face = R.sample_surface(v, f, cum, u)
    assert face.tolist() == [0, 0, 2, 2, 2]                 # t = 0.2 x 2.5 = 0.5 is not < cum[0]: the degenerate face is passed over
    assert np.array_equal(pts, [[0.25, 0.25, 0], [0.25, 0.25, 0], [1.0, 0.0, 1.0], [0.0, 2.0, 1.0], [0.0, 1.0, 1.0]])
