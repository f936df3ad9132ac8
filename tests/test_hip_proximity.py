"""The closest point on a triangle mesh on the MI355X (csrc/vfn_proximity.hip through vf_nerf_amd/metrics3d.py) against the restatement
of its contract (tests/proximity_restatement.py): face, closest point, squared distance and distance bit for bit, by the grid and by
all pairs; the pair, large-face and leftover counts against the model of the grid — so that the all-pairs pass cannot hide a wrong
ring pass, nor the other way round; then the scores built on it."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import icp, lib, meshops, metrics3d  # noqa: E402
import metrics3d_restatement as MR  # noqa: E402
import proximity_restatement as R  # noqa: E402
import simplify_restatement as SR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GOLDEN = os.path.join(REPO, "tests", "golden", "mesh_stages.npz")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


@functools.lru_cache(maxsize=None)
def _shared_matrix(name):
    v, f, q = inputs(name)
    return R.pair_matrix(q, v, f)


def matrix(name):
    """One pair matrix per input, shared by the tests and left unchanged; the recorded meshes' (4096 queries by thousands of faces)
    are computed for their one test and not kept."""
    if isinstance(name, tuple):
        v, f, q = inputs(name)
        return R.pair_matrix(q, v, f)
    return _shared_matrix(name)


@functools.lru_cache(maxsize=None)
def recorded(stage):
    """A recorded mesh; the file numbers its vertices from 1, as the reference writes them."""
    z = np.load(GOLDEN)
    return z[f"{stage}.vs"].astype(np.float64), z[f"{stage}.fs"].astype(np.int64) - 1


@functools.lru_cache(maxsize=None)
def recorded_queries(stage, count=4096):
    """``count`` surface samples of a recorded mesh, the same pushed along their faces' normals by + one voxel and by - one voxel
    (alternating) -> (on [count,3], off [count,3]); a voxel = 1 / 16 of the longest extent."""
    v, f = recorded(stage)
    u = np.random.default_rng(41).uniform(0, 1, (count, 3))
    points, face = metrics3d.sample_surface(v, f, count, uniforms=u, device=DEV)
    normal = meshops.face_normals((v, f), device=DEV)[face].cpu().numpy()
    on = points.cpu().numpy()
    voxel = float((v.max(axis=0) - v.min(axis=0)).max()) / 16.0
    sign = np.where(np.arange(count) % 2 == 0, 1.0, -1.0)[:, None]
    return on, on + sign * voxel * normal


def inputs(name):
    if isinstance(name, tuple):
        stage, kind, step = name
        v, f = recorded(stage)
        return v, f, recorded_queries(stage)[kind == "off"][::step]
    return R.cases()[name]


def search(v, f, q, search="grid", max_rings=8, cells=None, big_face_cells=None, info=None):
    """-> ((face, closest, sqdist) as numpy, leftover count, the grid) through the calls ``closest_point`` makes."""
    with torch.cuda.device(DEV):
        grid = metrics3d._triangle_grid(dev(v), dev(f, torch.int64), cells, metrics3d._check_big_face_cells(big_face_cells), pairs=search == "grid",
                                        info=info)
        face, closest, sqdist, left = metrics3d._closest(dev(q), grid, max_rings if search == "grid" else None, info=info)
    assert face.is_cuda and face.dtype == torch.int64 and closest.dtype == torch.float64 and tuple(closest.shape) == (len(q), 3)
    return (face.cpu().numpy(), closest.cpu().numpy(), sqdist.cpu().numpy()), left, grid


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: {int((got[0] != want[0]).sum())} of {len(want[0])} faces differ"
    assert np.array_equal(bits(got[2]), bits(want[2])), f"{what}: {int((bits(got[2]) != bits(want[2])).sum())} squared distances differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{what}: {int((bits(got[1]) != bits(want[1])).any(axis=1).sum())} closest points differ"


def check(name, **setting):
    """One grid search against the definition and the model of the grid."""
    v, f, q = inputs(name)
    pairs = matrix(name)
    want = R._pick(*pairs)
    got, left, grid = search(v, f, q, **setting)
    assert_same(got, want, f"{name} {setting}")
    box, dims = R.host_grid(v, f, setting.get("cells"))
    big = setting.get("big_face_cells", metrics3d.BIG_FACE_CELLS)
    assert grid.dims == dims and grid.box == box
    ncells = R.cell_ranges(v, f, box, dims)[2]
    assert np.array_equal(grid.ncells.cpu().numpy(), ncells)
    assert (grid.n_pairs, grid.n_large) == R.grid_counts(ncells, big), f"{name} {setting}"
    assert np.array_equal(grid.large.cpu().numpy(), np.flatnonzero(ncells > big))
    ring = R.ring_search(q, v, f, box, dims, big, matrix=pairs)[0]
    assert left == R.leftovers(ring, setting.get("max_rings", 8)), f"{name} {setting}"
    return got, left, grid


# ---------------------------------------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.cases()))
def test_grid_and_all_pairs_equal_the_definition(name):
    """Every shared case: one face with 1, 63, 64, 65 queries; 255, 256, 257 faces with one query; the special positions; degenerate
    faces; a spanning face; two sets; far queries; the cube on its lattice."""
    got = check(name)[0]
    v, f, q = inputs(name)
    listed, left, _ = search(v, f, q, search="all_pairs")
    assert left == len(q)
    assert_same(listed, got, f"{name} all pairs")
    public = metrics3d.closest_point((v, f), q, device=DEV)
    assert_same((public.face.cpu().numpy(), public.points.cpu().numpy(), public.sqdist.cpu().numpy()), got, f"{name} closest_point")
    assert np.array_equal(bits(public.distance.cpu().numpy()), bits(np.sqrt(got[2])))
    assert np.array_equal(bits(metrics3d.surface_distances(q, (v, f), search="all_pairs", device=DEV).cpu().numpy()), bits(np.sqrt(got[2])))


@pytest.mark.parametrize("name", ["spanning", "degenerate", "soup", "far_queries", "two_sets", "cube_lattice"])
def test_the_grid_changes_no_bit(name):
    """cells in {1, 2, 7, 128}, big_face_cells in {0, 1, 8, 10^9}, max_rings in {0, 1, 8}: the same bits, and the counts of the model —
    a 1 x 1 x 1 grid, mostly empty cells at 128, everything large, nothing large, every ring cut off."""
    for setting in R.GRID_SETTINGS:
        _, left, grid = check(name, **setting)
        if setting.get("cells") == 1:
            assert grid.dims == (1, 1, 1) and left == 0
        if setting.get("big_face_cells") == 0:
            assert grid.n_pairs == 0 and grid.n_large == int(R.valid_faces(*inputs(name)[:2]).sum())
        if setting.get("big_face_cells") == 10 ** 9:
            assert grid.n_large == 0


def test_large_faces_and_empty_cells():
    assert check("spanning")[2].n_large == 1                                 # the face from corner to corner, at the default
    assert check("soup", max_rings=0)[1] > 0                                 # queries that ring 0 does not settle
    grid = check("soup", cells=128, max_rings=0)[2]                          # mostly empty cells
    assert max(grid.dims) == 128 and grid.n_pairs < grid.dims[0] * grid.dims[1] * grid.dims[2] // 8


def test_a_built_grid_serves_several_searches():
    v, f, q = inputs("soup")
    grid = metrics3d.triangle_grid((v, f), cells=7, big_face_cells=2, device=DEV)
    box, dims = R.host_grid(v, f, 7)
    assert (grid.n_pairs, grid.n_large) == R.grid_counts(R.cell_ranges(v, f, box, dims)[2], 2) and grid.dims == dims and grid.n_faces == len(f)
    want = R._pick(*matrix("soup"))
    for queries in (q, q[::-1].copy()):
        got = metrics3d.closest_point(grid, queries, max_rings=1)
        k = slice(None) if queries is q else slice(None, None, -1)
        assert_same((got.face.cpu().numpy(), got.points.cpu().numpy(), got.sqdist.cpu().numpy()), tuple(x[k] for x in want), "a built grid")
    with pytest.raises(ValueError, match="the grid's own"):
        metrics3d.closest_point(grid, q, cells=3)


def test_special_positions():
    """On a vertex, on an edge, on the plane inside: distance 0 and the point itself; on the bisector of the two faces through their
    shared edge: the lower face."""
    v, f, q = inputs("special_positions")
    got = check("special_positions")[0]
    assert (got[2][:7] == 0).all() and np.array_equal(got[1][:7], q[:7])
    assert (got[0][[9, 10, 11, 12]] == 0).all()                              # y = z: both faces at the same distance
    c, d2 = matrix("special_positions")
    assert np.array_equal(bits(d2[[9, 10, 11, 12], 0]), bits(d2[[9, 10, 11, 12], 1]))


@pytest.mark.parametrize("name", [("g.random", "on", 1), ("g.random", "off", 1), ("f16", "on", 1), ("f16", "off", 1)])
def test_recorded_meshes(name):
    """The recorded meshes (388 and 2673 faces) with 4096 queries, on the surface and one voxel off it: the definition and the model of
    the grid for all 4096, and the all-pairs kernel beside them."""
    stage, kind, step = name
    v, f = recorded(stage)
    q = recorded_queries(stage)[kind == "off"]
    by_grid, _, _ = search(v, f, q)
    by_list, left, _ = search(v, f, q, search="all_pairs")
    assert left == 4096
    assert_same(by_grid, by_list, f"{name}: grid against all pairs")
    got = check(name)[0]
    assert_same(got, by_grid, f"{name}: one search against the other")
    if kind == "on":
        scale = float(np.abs(v).max())
        assert by_grid[2].max() <= on_surface_bound(scale)


def on_surface_bound(scale: float) -> float:
    """The largest d2 a point SAMPLED on a surface with coordinates up to ``scale`` may have against that surface — by reasoning, not
    by measurement.  The sample (v0 + a e1) + b e2 carries at most 4 roundings a component, each at most half an ulp of a number
    below 4 scale, so it lies within 8 2^-52 scale of the surface per component.  The routine's answer for a query that close is a
    foot q - s n or a segment's P + t d, whose s and t carry a relative error of a few 2^-52 and whose products and sums round again:
    within another 8 2^-52 scale of the query per component.  16 in all; 64 is allowed, and d2 sums three such squares."""
    return 3.0 * (64.0 * 2.0 ** -52 * scale) ** 2


def test_bad_inputs_set_their_bits_and_spare_the_other_rows():
    """A NaN query: bit 1, face -1, +inf; a face index outside the vertices: bit 2, the face is no face and nothing is read through
    it; every other row is the definition's.  The public call raises for either."""
    v, f, q = (x.copy() for x in inputs("soup"))
    f[3, 1], f[7, 0], f[100, 2] = len(v), -1, 2 ** 40
    q[5, 1], q[70, 0] = np.nan, np.inf
    want = R.brute(q, v, f)
    for kw in ({}, {"search": "all_pairs"}, {"max_rings": 0}, {"big_face_cells": 0}):
        info = torch.zeros(1, dtype=torch.int64, device=DEV)
        got, _, grid = search(v, f, q, info=info, **kw)
        assert int(info.cpu()) == 3, kw
        assert got[0][5] == -1 and np.isinf(got[2][5]) and not np.isin(got[0], (3, 7, 100)).any()
        keep = np.delete(np.arange(len(q)), [5, 70])
        assert_same(tuple(x[keep] for x in got), tuple(x[keep] for x in want), f"bad inputs {kw}")
        assert (grid.ncells.cpu().numpy()[[3, 7, 100]] == 0).all()
    with pytest.raises(lib.VfnError, match="face index"):
        metrics3d.closest_point((v, f), inputs("soup")[2], device=DEV)
    with pytest.raises(lib.VfnError, match="non-finite"):
        metrics3d.closest_point(inputs("soup")[:2], q, device=DEV)
    with pytest.raises(lib.VfnError, match="non-finite"):
        metrics3d.closest_point(inputs("soup")[:2], q, search="all_pairs", device=DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
# the scores
# ---------------------------------------------------------------------------------------------------------------------------------
N_SCORE = 2000


def _rows(pred_points, ref_points, pred_mesh, ref_mesh, threshold):
    one = metrics3d._direction(metrics3d.closest_point(pred_mesh, ref_points, device=DEV).distance, threshold).cpu().numpy()
    two = metrics3d._direction(metrics3d.closest_point(ref_mesh, pred_points, device=DEV).distance, threshold).cpu().numpy()
    return one, two


def _entry(one, two):
    mean, median, mn, mx = metrics3d._chamfer(one, two)
    out = {"chamfer distance": {"mean": mean, "median": median, "min": mn, "max": mx}}
    out.update(metrics3d._prf(two, one))
    out["surface"] = "mesh"
    return out


def test_score_mesh_is_its_composition():
    """``score_mesh(..., surface="mesh")`` on two recorded meshes = ``sample_surface``, ``closest_point`` and the module's statistics, key
    by key and bit by bit; with normals, the face's normal at ``face[i]``; with ICP, the ref samples moved by the inverse."""
    pred, ref = recorded("g.random"), recorded("g.ties")
    u = np.random.default_rng(43).uniform(0, 1, (N_SCORE, 3))
    pp, pface = metrics3d.sample_surface(*pred, N_SCORE, uniforms=u, device=DEV)
    rp, rface = metrics3d.sample_surface(*ref, N_SCORE, uniforms=u, device=DEV)
    want = _entry(*_rows(pp, rp, pred, ref, 0.05))
    got = metrics3d.score_mesh(pred, ref, num_points=N_SCORE, distance_thresh=0.05, uniforms=u, device=DEV, surface="mesh")
    assert got == want and list(got) == list(want)
    samples = metrics3d.score_mesh(pred, ref, num_points=N_SCORE, distance_thresh=0.05, uniforms=u, device=DEV)
    assert "surface" not in samples and set(samples) | {"surface"} == set(got)
    # a sample's nearest point of the other SURFACE is no farther than its nearest SAMPLE of it
    assert got["chamfer distance"]["mean"] <= samples["chamfer distance"]["mean"]
    assert metrics3d.chamfer_distance(pred, ref, num_points=50, generator=torch.Generator(DEV).manual_seed(3), device=DEV, surface="mesh")[2] >= 0.0
    # normals
    pn, rn = metrics3d._sample_normals(*pred, pface), metrics3d._sample_normals(*ref, rface)
    towards_ref, towards_pred = metrics3d.closest_point(ref, pp, device=DEV), metrics3d.closest_point(pred, rp, device=DEV)
    a = float(lib.reduce_stats(lib.normal_dots(pn, meshops.face_normals(ref, device=DEV), towards_ref.face), math.inf)[0].cpu()) / N_SCORE
    b = float(lib.reduce_stats(lib.normal_dots(rn, meshops.face_normals(pred, device=DEV), towards_pred.face), math.inf)[0].cpu()) / N_SCORE
    with_normals = metrics3d.score_mesh(pred, ref, num_points=N_SCORE, distance_thresh=0.05, uniforms=u, device=DEV, surface="mesh", normals=True)
    assert with_normals["normal consistency"] == {"pred_to_ref": a, "ref_to_pred": b, "mean": (a + b) / 2.0}
    assert {k: x for k, x in with_normals.items() if k != "normal consistency"} == want
    assert metrics3d.normal_consistency(pred, ref, num_points=N_SCORE, uniforms=u, device=DEV, surface="mesh") == with_normals["normal consistency"]
    # ICP: the moved pred samples against the ref mesh, the ref samples moved back against the pred mesh
    aligned = icp.align(pp, rp, 0.05, device=DEV)
    moved = icp.transform_points(pp, aligned.transformation, device=DEV)
    back = icp.transform_points(rp, metrics3d._rigid_inverse(aligned.transformation), device=DEV)
    with_icp = metrics3d.score_mesh(pred, ref, num_points=N_SCORE, distance_thresh=0.05, uniforms=u, device=DEV, surface="mesh", icp_align=True)
    assert {k: x for k, x in with_icp.items() if k != "icp"} == _entry(*_rows(moved, back, pred, ref, 0.05))
    assert with_icp["icp"]["transformation"] == aligned.transformation.tolist()


def test_the_sampling_floor_is_gone():
    """A surface scored against ITSELF: through the meshes the chamfer mean is 0 up to the rounding of the samples; through the samples
    it is not.  The second mesh lists the same faces in reversed order: given the same ``uniforms`` the two sample sets differ, as two
    samplings of one surface do (with the identical mesh and the same uniforms the two sets are one set, and both scores are 0)."""
    v, f = recorded("g.random")
    u = np.random.default_rng(44).uniform(0, 1, (N_SCORE, 3))
    bound = 2.0 * on_surface_bound(float(np.abs(v).max()))                   # the sum of two means of d2
    for other in ((v, f), (v, f[::-1].copy())):
        mesh = metrics3d.score_mesh((v, f), other, num_points=N_SCORE, distance_thresh=0.01, uniforms=u, device=DEV, surface="mesh")
        print("mesh against itself, chamfer mean:", mesh["chamfer distance"]["mean"], "bound", bound)
        assert 0.0 <= mesh["chamfer distance"]["mean"] <= bound
        assert mesh["precision"] == 1.0 and mesh["recall"] == 1.0
    samples = metrics3d.score_mesh((v, f), (v, f[::-1].copy()), num_points=N_SCORE, distance_thresh=0.01, uniforms=u, device=DEV)
    print("samples against samples, chamfer mean:", samples["chamfer distance"]["mean"])
    assert samples["chamfer distance"]["mean"] > mesh["chamfer distance"]["mean"] and samples["chamfer distance"]["mean"] > bound
    deviation = metrics3d.surface_deviation((v, f), (v, f), num_points=N_SCORE, uniforms=u, device=DEV)
    print("surface_deviation(m, m):", deviation)
    assert set(deviation) == {"mean", "rms", "max", "median"}
    assert 0.0 <= deviation["median"] <= deviation["max"] <= math.sqrt(on_surface_bound(float(np.abs(v).max())))
    assert 0.0 <= deviation["mean"] <= deviation["rms"] <= deviation["max"]


def test_the_deviation_of_a_simplified_cube_equals_the_restatement():
    """``surface_deviation(simplified, original, vertices=True)``: the named vertices of the decimated cube against the cube's surface."""
    original = SR.cube(4)
    simplified = meshops.simplify_edge_collapse(original, target_faces=40, device=DEV)
    sv, sf = simplified.vertices.cpu().numpy(), simplified.faces.cpu().numpy()
    assert 0 < len(sf) < len(original[1])
    got = metrics3d.surface_deviation((sv, sf), original, vertices=True, device=DEV)
    d = np.sqrt(R.brute(sv[np.unique(sf)], *original)[2])
    s = np.sort(d)
    n = len(d)
    want = {"mean": MR.stats_sum(d) / n, "rms": math.sqrt(MR.stats_sum(d * d) / n), "max": float(d.max()), "median": float((s[(n - 1) // 2] + s[n // 2]) / 2.0)}
    assert got == want
    assert got == metrics3d.surface_deviation((sv, sf), original, vertices=True, search="all_pairs", device=DEV)
