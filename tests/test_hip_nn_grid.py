"""The unbounded grid search on the MI355X (csrc/vfn_nn.hip through vf_nerf_amd/metrics3d.py) against the restatement of its contract
(tests/nn_grid_restatement.py): neighbour indices and squared-distance bits against brute force, the number of leftovers against the
model of the ring rule — so that the all-pairs pass cannot hide a wrong ring pass, nor the other way round."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import icp, lib, metrics3d, refuse  # noqa: E402
import icp_restatement as R  # noqa: E402
import nn_grid_restatement as G  # noqa: E402
import raster_restatement as RR  # noqa: E402
import tsdf_restatement as TR  # noqa: E402
from test_icp_host import bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
W = 16                  # threads of the brute-force restatement


@functools.lru_cache(maxsize=None)
def reference(key):
    """One brute force (and one run of the ring model per grid asked for) per input, shared by the tests."""
    q, t = inputs(key)
    return G.brute(q, t, workers=W)


def inputs(key):
    kind = key[0]
    if kind == "uniform":
        a, b = G.uniform_pair(key[1], key[2])
        return (b, a) if key[3] else (a, b)
    if kind == "far":
        return G.far_queries()
    if kind == "ties":
        return G.lattice_ties()[:2]
    return G.degenerate_cases()[key[1]]


@functools.lru_cache(maxsize=None)
def rings(key, cells=None):
    q, t = inputs(key)
    return G.ring_search(q, t, *G.host_grid(t, cells))[0]


def search(q, t, max_rings=8, cells=None, order=True):
    """-> (index, sqdist, leftover count) as numpy / int, through ``lib.nn_nearest`` on the grid ``metrics3d.nearest_grid`` builds."""
    qd = torch.from_numpy(np.ascontiguousarray(q)).to(DEV)
    grid = metrics3d.nearest_grid(t, cells=cells, device=DEV)
    index, sqdist, left = lib.nn_nearest(qd, grid.nearest_args(), max_rings, order=icp.query_order(qd, None, grid) if order else None)
    assert index.is_cuda and index.dtype == torch.int64 and sqdist.is_cuda and sqdist.dtype == torch.float64
    return index.cpu().numpy(), sqdist.cpu().numpy(), left, grid


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: {int((got[0] != want[0]).sum())} of {len(want[0])} indices differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{what}: {int((bits(got[1]) != bits(want[1])).sum())} squared distances differ"


def check(key, max_rings=8, cells=None, order=True):
    q, t = inputs(key)
    index, sqdist, left, grid = search(q, t, max_rings, cells, order)
    box, dims = G.host_grid(t, cells)
    assert grid.dims == dims and grid.box == box                       # the model speaks about the grid the device searched
    assert_same((index, sqdist), reference(key), f"{key}, max_rings {max_rings}, cells {cells}")
    want_left = G.leftovers(rings(key, cells), max_rings)
    print(f"{key}: grid {dims}, max_rings {max_rings}: {left} leftovers of {len(q)} (model {want_left}), rings {np.bincount(rings(key, cells))}")
    assert left == want_left
    return index, sqdist, left


# ---------------------------------------------------------------------------------------------------------------------------------
# uniform pairs
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swap", [False, True], ids=["forward", "swapped"])
@pytest.mark.parametrize("n,m", G.UNIFORM_SIZES)
def test_uniform_pairs_stop_on_the_ring_path(n, m, swap):
    key = ("uniform", n, m, swap)
    q, t = inputs(key)
    index, sqdist, left = check(key)
    assert left == 0 and rings(key).max() <= 2
    all_pairs = lib.nn_sqdist(torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)).cpu().numpy()
    assert np.array_equal(bits(sqdist), bits(all_pairs))
    # the public surface: the same index, the distance the all-pairs surface reports, from any mix of host and device inputs
    pi, pd = metrics3d.nearest(q, torch.from_numpy(t).to(DEV))
    assert np.array_equal(pi.cpu().numpy(), index)
    assert np.array_equal(bits(pd.cpu().numpy()), bits(metrics3d.nearest_distances(q, t).cpu().numpy()))
    assert np.array_equal(bits(pd.cpu().numpy()), bits(np.sqrt(sqdist)))


def test_ring_budgets_split_the_work_and_change_nothing():
    key = ("uniform",) + G.MIXED + (False,)
    n = G.MIXED[0]
    full = check(key)
    mixed = check(key, max_rings=1)
    assert mixed[2] == 107 and 0 < mixed[2] < n
    none = check(key, max_rings=0)
    assert none[2] == 966
    unordered = check(key, max_rings=1, order=False)
    for other in (mixed, none, unordered):
        assert_same(other, full, "another budget")


@pytest.mark.parametrize("cells", [1, 3, 40, 128])
def test_grid_invariance(cells):
    key = ("uniform",) + G.MIXED + (False,)
    got = check(key, cells=cells)
    assert got[2] == (164 if cells == 128 else 0)
    q, t = inputs(key)
    pi, pd = metrics3d.nearest(q, t, cells=cells)
    assert np.array_equal(pi.cpu().numpy(), reference(key)[0])
    held = metrics3d.nearest(q, metrics3d.nearest_grid(t, cells=cells))                     # a grid built once
    assert np.array_equal(held[0].cpu().numpy(), reference(key)[0]) and torch.equal(held[1], pd)


def test_far_queries_are_clamped():
    got = check(("far",))
    assert got[2] == 177


@pytest.mark.parametrize("cells", [None, 16], ids=["default", "h=spacing"])
def test_ties_go_to_the_lowest_index(cells):
    q, t, n_mid = G.lattice_ties()
    if cells == 16:
        assert G.host_grid(t, 16)[0][6] == 0.125 * (1.0 + 2.0 ** -20)               # the targets sit next to cell faces
    for max_rings in (8, 0):
        index, sqdist, _ = check(("ties",), max_rings=max_rings, cells=cells)
        assert np.array_equal(sqdist[:n_mid], np.full(n_mid, 3 * 0.0625 ** 2)) and (sqdist[n_mid:] == 0).all()
    for i in range(0, len(q), 37):                                                  # from the definition, not the restatement
        d2 = ((q[i] - t) ** 2).sum(axis=1)
        assert index[i] == np.flatnonzero(d2 == d2.min())[0] and (d2 == d2.min()).sum() >= (8 if i < n_mid else 1)


@pytest.mark.parametrize("name", ["one", "coincident", "plane", "room"])
def test_degenerate_targets(name):
    index, sqdist, left = check(("degenerate", name))
    check(("degenerate", name), max_rings=0)
    if name in ("one", "coincident"):
        assert (index == 0).all() and left == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# partial waves, refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_partial_waves():
    """257 queries (one lane into a second workgroup) of which 64 x 3 + 1 are leftovers (one wave into a 49th workgroup of the list
    kernel): chosen with the model from the (1037, 1805) pair at max_rings = 0."""
    key = ("uniform",) + G.MIXED + (False,)
    q, t = inputs(key)
    ring = rings(key)
    pick = np.concatenate((np.flatnonzero(ring > 0)[:193], np.flatnonzero(ring == 0)[:64]))
    pick.sort()
    index, sqdist, left, _ = search(q[pick], t, max_rings=0)
    assert left == 193 and len(pick) == 257
    assert_same((index, sqdist), tuple(x[pick] for x in reference(key)), "257 queries, 193 leftovers")


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_coordinates_are_refused(bad):
    g = np.random.default_rng(3)
    q, t = g.uniform(-1, 1, (300, 3)), g.uniform(-1, 1, (500, 3))
    for which, row, col in ((0, 299, 2), (1, 410, 0), (0, 0, 1)):
        pair = [q.copy(), t.copy()]
        pair[which][row, col] = bad
        with pytest.raises(lib.VfnError, match="non-finite"):
            metrics3d.nearest(pair[0], pair[1])
        with pytest.raises(lib.VfnError, match="non-finite"):
            metrics3d.nearest_distances(pair[0], pair[1], search="grid")
    index, dist = metrics3d.nearest(q, t)
    assert (index >= 0).all() and dist.isfinite().all()


def test_the_library_refuses_what_the_contract_excludes():
    q, t = inputs(("uniform", 3, 7, False))
    qd = torch.from_numpy(q).to(DEV)
    grid = metrics3d.nearest_grid(t, device=DEV)
    with pytest.raises(lib.VfnError, match="max_rings"):
        lib.nn_nearest(qd, grid.nearest_args(), -1)
    args = list(grid.nearest_args())
    args[4] = grid.box[:6] + (float("inf"),)
    with pytest.raises(lib.VfnError, match="cell edge"):
        lib.nn_nearest(qd, tuple(args), 8)
    args[4] = grid.box[:6] + (grid.box[6] / 1000.0,)
    with pytest.raises(lib.VfnError, match="cell edge"):
        lib.nn_nearest(qd, tuple(args), 8)


# ---------------------------------------------------------------------------------------------------------------------------------
# scoring
# ---------------------------------------------------------------------------------------------------------------------------------
def small_meshes():
    ref = RR.icosphere(3, 0.5)
    pred = RR.merged(RR.icosphere(3, 0.5), RR.icosphere(1, 0.1))
    moved = (R.transform(np.asarray(pred[0], dtype=np.float64), R.rigid((1.0, 2.0, 3.0), 2.0, (0.01, -0.005, 0.007))), pred[1])
    return moved, ref


@pytest.mark.parametrize("icp_align", [False, True], ids=["plain", "icp"])
def test_score_mesh_is_the_same_dictionary(icp_align):
    pred, ref = small_meshes()

    def score(**kw):
        return metrics3d.score_mesh(pred, ref, num_points=5000, distance_thresh=0.02, generator=torch.Generator(device=DEV).manual_seed(8),
                                    icp_align=icp_align, icp_threshold=0.1, device=DEV, **kw)

    plain, explicit, grid = score(), score(search="all_pairs"), score(search="grid")
    assert plain == explicit == grid
    assert ("icp" in grid) == icp_align and 0 < grid["precision"] < 1 and grid["chamfer distance"]["mean"] > 0


def test_point_scores_and_distances_are_the_same():
    a, b = inputs(("uniform",) + G.MIXED + (False,))
    assert torch.equal(metrics3d.nearest_distances(a, b, search="grid"), metrics3d.nearest_distances(a, b))
    assert metrics3d.chamfer_from_points(a, b, search="grid") == metrics3d.chamfer_from_points(a, b)
    assert metrics3d.precision_recall_fscore(a, b, 0.2, search="grid") == metrics3d.precision_recall_fscore(a, b, 0.2)
    pred, ref = small_meshes()

    def chamfer(**kw):
        return metrics3d.chamfer_distance(pred, ref, num_points=3000, generator=torch.Generator(device=DEV).manual_seed(2), device=DEV, **kw)

    assert chamfer(search="grid") == chamfer()


def test_metrics_3d_is_the_same_dictionary():
    s = TR.sphere_scene()
    hi = tuple(o + n * s.vl for o, n in zip(s.origin, s.dims))
    mesh = RR.merged(RR.icosphere(3, 0.5), RR.icosphere(1, 0.1))

    def run(**kw):
        return refuse.metrics_3d(mesh, RR.icosphere(3, 0.5), s.intrinsics_matrices(), s.poses, 48, 64, num_points=5000, distance_thresh=0.1,
                                 generator=torch.Generator(device=DEV).manual_seed(3), bounds=(s.origin, hi), voxel_length=s.vl,
                                 sdf_trunc=s.trunc, device=DEV, **kw)

    assert run(search="grid") == run()
