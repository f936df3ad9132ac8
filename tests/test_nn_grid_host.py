"""The unbounded grid search without a device: the model of its ring rule (tests/nn_grid_restatement.py) against the definition (brute
force), the leftover counts that tests/test_hip_nn_grid.py then expects of the device, the ABI's declarations, and the argument checks
of the public surface."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, metrics3d, refuse  # noqa: E402
import nn_grid_restatement as G  # noqa: E402
from test_icp_host import bits  # noqa: E402


def model_equals_definition(q, t, cells=None):
    box, dims = G.host_grid(t, cells)
    ring, index, sqdist = G.ring_search(q, t, box, dims)
    want_index, want_sqdist = G.brute(q, t)
    assert np.array_equal(index, want_index), f"{int((index != want_index).sum())} indices differ"
    assert np.array_equal(bits(sqdist), bits(want_sqdist))
    return ring, dims


@pytest.mark.parametrize("n,m", G.UNIFORM_SIZES)
def test_ring_model_equals_brute_force_on_uniform_pairs(n, m):
    a, b = G.uniform_pair(n, m)
    for q, t in ((a, b), (b, a)):
        ring, dims = model_equals_definition(q, t)
        assert G.leftovers(ring, 8) == 0 and ring.max() <= 2, np.bincount(ring)


def test_leftover_counts_of_the_mixed_pair():
    """The numbers the device tests expect: 1037 queries against 1805 targets, default grid 16^3."""
    q, t = G.uniform_pair(*G.MIXED)
    ring, dims = model_equals_definition(q, t)
    assert dims == (16, 16, 16)
    assert (G.leftovers(ring, 0), G.leftovers(ring, 1), G.leftovers(ring, 8)) == (966, 107, 0)
    for cells, want in ((1, 0), (3, 0), (40, 0), (128, 164)):
        ring, dims = model_equals_definition(q, t, cells)
        assert dims == (cells,) * 3 and G.leftovers(ring, 8) == want


def test_ring_model_on_far_queries():
    q, t = G.far_queries()
    ring, _ = model_equals_definition(q, t)
    assert G.leftovers(ring, 8) == 177


def test_ring_model_on_ties():
    q, t, n_mid = G.lattice_ties()
    for cells in (None, 16):
        box, dims = G.host_grid(t, cells)
        ring, index, sqdist = G.ring_search(q, t, box, dims)
        want_index, want_sqdist = G.brute(q, t)
        assert np.array_equal(index, want_index) and np.array_equal(bits(sqdist), bits(want_sqdist))
        assert np.array_equal(sqdist[:n_mid], np.full(n_mid, 3 * 0.0625 ** 2)) and (sqdist[n_mid:] == 0).all()
        if cells == 16:
            assert box[6] == 0.125 * (1.0 + 2.0 ** -20) and dims == (16, 16, 16)
    d2 = ((q[0] - t) ** 2).sum(axis=1)
    assert (d2 == d2.min()).sum() >= 8 and want_index[0] == np.flatnonzero(d2 == d2.min())[0]


@pytest.mark.parametrize("name", ["one", "coincident", "plane", "room"])
def test_ring_model_on_degenerate_targets(name):
    q, t = G.degenerate_cases()[name]
    ring, dims = model_equals_definition(q, t)
    if name in ("one", "coincident"):
        assert dims == (1, 1, 1) and G.host_grid(t)[0][6] == 1.0 and (ring == 0).all()
    if name == "plane":
        assert dims[2] == 1


def test_default_cells():
    cap, margin = lib.icp_grid_limits()
    assert metrics3d.grid_edge((2.0, 4.0, 1.0), 1805) == 4.0 / 16 * margin
    assert metrics3d.grid_edge((2.0, 4.0, 1.0), 1) == 4.0 * margin and metrics3d.grid_edge((2.0, 4.0, 1.0), 8) == 4.0 * margin
    assert metrics3d.grid_edge((2.0, 4.0, 1.0), 9) == 4.0 / 2 * margin
    assert metrics3d.grid_edge((2.0, 4.0, 1.0), 10 ** 7) == 4.0 / cap * margin
    assert metrics3d.grid_edge((0.0, 0.0, 0.0), 5) == 1.0
    assert metrics3d.grid_edge((2.0, 4.0, 1.0), 1805, cells=40) == 4.0 / 40 * margin


def test_exports_and_prototypes():
    assert {"vfn_nn_nearest", "vfn_nn_nearest_list"} <= set(lib.EXPORTS)
    protos = lib.header_prototypes()
    radius, nearest = protos["vfn_nn_radius"][1], protos["vfn_nn_nearest"][1]
    assert protos["vfn_nn_nearest"][0] == "int" and len(nearest) == 19
    # the grid arguments are vfn_nn_radius's, in its order; no transform, no radius; max_rings where the radius was
    assert nearest[:2] == radius[:2] and nearest[2:10] == radius[3:11] and nearest[10] == "int32_t" and nearest[11:13] == radius[12:14]
    assert nearest[13:] == ["int64_t*", "double*", "int64_t*", "int64_t*", "int64_t*", "void*"]
    assert protos["vfn_nn_nearest_list"] == ("int", ["const double*", "int64_t", "const double*", "int64_t", "const int64_t*", "int64_t",
                                                     "int64_t*", "double*", "void*"])
    build = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "build.sh")).read()
    assert re.search(r'^UNITS=".*\bvfn_nn\b.*"', build, flags=re.M) and re.search(r"\|vfn_nn[|)].*-ffp-contract=off", build)


def test_argument_checks():
    q, t = np.zeros((4, 3)), np.ones((5, 3))
    for bad in (np.zeros((4, 2)), np.zeros(3), np.zeros((0, 3)), np.zeros((4, 3), dtype=bool)):
        with pytest.raises(ValueError):
            metrics3d.nearest(bad, t)
        with pytest.raises(ValueError):
            metrics3d.nearest(q, bad)
        with pytest.raises(ValueError):
            metrics3d.nearest_grid(bad)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="max_rings"):
            metrics3d.nearest(q, t, max_rings=bad)
    for bad in (0, 129, 2.0, True):
        with pytest.raises(ValueError, match="cells"):
            metrics3d.nearest(q, t, cells=bad)
        with pytest.raises(ValueError, match="cells"):
            metrics3d.nearest_grid(t, cells=bad)
    mesh = (np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]]))
    for bad in ("kd", None, "GRID"):
        for call in (lambda: metrics3d.nearest_distances(q, t, search=bad), lambda: metrics3d.chamfer_from_points(q, t, search=bad),
                     lambda: metrics3d.chamfer_distance(mesh, mesh, num_points=10, search=bad),
                     lambda: metrics3d.precision_recall_fscore(q, t, 0.1, search=bad),
                     lambda: metrics3d.score_mesh(mesh, mesh, num_points=10, search=bad),
                     lambda: refuse.metrics_3d(mesh, mesh, None, None, 4, 4, search=bad)):
            with pytest.raises(ValueError, match="search"):
                call()
    assert metrics3d.SEARCHES == ("all_pairs", "grid") and metrics3d.MAX_RINGS == 8
