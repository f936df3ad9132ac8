"""Point-set alignment on the MI355X (csrc/vfn_icp.hip through vf_nerf_amd/icp.py) against the CPU restatement of its contract
(tests/icp_restatement.py).  Neighbour indices, squared distances, transformed points and counts are compared bit for bit; the sixteen
floating-point sums against math.fsum within the pairwise-summation bound of the tree the kernel builds, and all seventeen bit for bit
against the restatement of that tree (tests/tree_restatement.py); the loop is followed iteration by iteration from the device's own
transformations."""
import math
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
import raster_restatement as RR  # noqa: E402
import tsdf_restatement as TR  # noqa: E402
from test_icp_host import M, N_ROOM, bits, room_pair  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -53          # unit roundoff of float64
W = 16                  # threads of the brute-force restatement
TURN = R.rigid((0.3, -1.0, 0.2), 170.0, (0.5, 0.1, -0.7))


def host(pair):
    index, sqdist = pair
    assert index.is_cuda and index.dtype == torch.int64 and sqdist.is_cuda and sqdist.dtype == torch.float64
    return index.cpu().numpy(), sqdist.cpu().numpy()


def assert_same(got, want, what):
    gi, gd = got
    wi, wd = want
    assert gi.shape == wi.shape and gd.shape == wd.shape
    assert np.array_equal(gi, wi), f"{what}: {int((gi != wi).sum())} of {len(wi)} indices differ"
    assert np.array_equal(bits(gd), bits(wd)), f"{what}: {int((bits(gd) != bits(wd)).sum())} of {len(wd)} squared distances differ"


def half_radius(m):
    """The radius at which a uniform cloud of m points in [-2, 2]^3 leaves about half the queries without a target:
    (4 pi / 3) r^3 m / 64 = ln 2."""
    return (math.log(2.0) * 64.0 * 3.0 / (4.0 * math.pi * m)) ** (1.0 / 3.0)


PLANT_R = 1e-4
PLANT_FACTORS = (1.0 - 1e-3, 1.0 - 1e-9, 1.0 + 1e-9, 1.0 + 1e-3)


def uniform_case(n, m):
    """Uniform in [-2, 2]^3; up to 64 queries are planted next to a target at distances straddling PLANT_R = 1e-4."""
    g = np.random.default_rng(1000 * n + m)
    q, t = g.uniform(-2, 2, (n, 3)), g.uniform(-2, 2, (m, 3))
    k = min(64, n, m)
    d = g.standard_normal((k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    q[:k] = t[m - k:] + d * (PLANT_R * np.array([PLANT_FACTORS[i % 4] for i in range(k)]))[:, None]
    return q, t


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: the search
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1, 1), (3, 7), (1037, 1805), (1024, 8), (2049, 100003)])
def test_search_equals_restatement(n, m):
    """Three radii: one that leaves about half the queries alone, one beyond the diagonal (a single cell: the all-pairs kernel's bits,
    never -1), and 1e-4 against an extent of 4 (40 000 cells an axis asked for, 128 given) with planted pairs either side of it."""
    a, b = uniform_case(n, m)
    for q, t in ((a, b), (b, a)):
        free = R.nearest_within(q, t, 1e3, workers=W)                      # one brute force per direction
        for radius in (half_radius(len(t)), 8.0, PLANT_R):
            want = R.bounded(*free, radius)
            got = host(icp.nearest_within(q, t, radius))
            assert_same(got, want, f"{len(q)} x {len(t)}, r = {radius:.4g}")
            again = host(icp.nearest_within(torch.from_numpy(q).to(DEV), torch.from_numpy(t), radius))
            assert_same(again, got, "second run")
            found = int((got[0] >= 0).sum())
            if radius == 8.0:
                assert found == len(q)
                all_pairs = lib.nn_sqdist(torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)).cpu().numpy()
                assert np.array_equal(bits(got[1]), bits(all_pairs))
            elif radius == PLANT_R:
                k = min(64, n, m)
                if q is a and k >= 4:
                    assert k // 2 <= found < k + 4 and (got[0][:k][np.arange(k) % 4 < 2] >= 0).all()
                    assert (got[0][:k][np.arange(k) % 4 >= 2] == -1).all()
            elif min(len(q), len(t)) > 1000:
                assert 0.3 * len(q) < found < 0.7 * len(q), found
    # the restatement's own bounded search is the lemma `bounded` (checked on the smaller direction)
    q, t = (a, b) if n * m <= 4e6 else (a[:200], b)
    assert_same(R.nearest_within(q, t, half_radius(len(t)), workers=W), R.bounded(*R.nearest_within(q, t, 1e3, workers=W), half_radius(len(t))),
                "lemma")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2: the boundary of the radius, ties
# ---------------------------------------------------------------------------------------------------------------------------------
def lattice_case(reverse):
    """The `at` / `beyond` queries lie OUTSIDE the targets' box (on a lattice of spacing r an interior point exactly r from one lattice
    point is another lattice point): they exercise the clamp, and after it a query shares its partner's cell, so the pair admitted at
    exactly r never crosses a cell here.  test_exact_radius_across_cells is the case where it does."""
    r = 0.125
    axis = np.arange(-8, 9) * r
    lattice = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)            # 17^3 = 4913 points
    g = np.random.default_rng(11)
    dup = lattice[g.choice(len(lattice), 200, replace=False)]
    targets = np.concatenate((lattice, dup))                                                           # 200 positions stored twice
    if reverse:
        targets = targets[::-1].copy()
    at, beyond = [], []
    for ax in range(3):
        for sign in (-1.0, 1.0):
            face = lattice[lattice[:, ax] == sign * 1.0]
            pick = face[g.choice(len(face), 40, replace=False)]
            on = pick.copy()
            on[:, ax] = sign * 1.125                    # exactly r outside the face: the next lattice points are r sqrt(2) away
            far = on.copy()
            far[:, ax] = np.nextafter(on[:, ax], sign * np.inf)
            at.append(on)
            beyond.append(far)
    at, beyond = np.concatenate(at), np.concatenate(beyond)
    mid = []
    for ax in range(3):
        base = lattice[g.choice(len(lattice), 300, replace=False)]
        base = base[base[:, ax] < 1.0].copy()
        base[:, ax] += r / 2                            # midway between two lattice points r / 2 either side
        mid.append(base)
    mid = np.concatenate(mid)
    return r, targets, at, beyond, mid, dup


@pytest.mark.parametrize("reverse", [False, True], ids=["ascending", "reversed"])
def test_boundary_and_ties(reverse):
    r, targets, at, beyond, mid, dup = lattice_case(reverse)
    queries = np.concatenate((at, beyond, mid, dup))
    want = R.nearest_within(queries, targets, r, workers=W)
    got = host(icp.nearest_within(queries, targets, r))
    assert_same(got, want, "lattice")
    assert_same(host(icp.nearest_within(queries, targets, r)), got, "second run")
    n_at, n_mid = len(at), len(mid)
    i_at, d_at = got[0][:n_at], got[1][:n_at]
    assert (i_at >= 0).all() and np.array_equal(d_at, np.full(n_at, r * r))                            # d2 == r r: admitted
    i_far = got[0][n_at:2 * n_at]
    assert np.array_equal(i_far, want[0][n_at:2 * n_at]) and (i_far == -1).sum() > 0.9 * n_at           # one ulp farther: rejected
    i_mid, d_mid = got[0][2 * n_at:2 * n_at + n_mid], got[1][2 * n_at:2 * n_at + n_mid]
    assert np.array_equal(d_mid, np.full(n_mid, (r / 2) ** 2))
    i_dup, d_dup = got[0][2 * n_at + n_mid:], got[1][2 * n_at + n_mid:]
    assert (d_dup == 0).all()
    # the lowest index among the targets at the minimum, from the definition
    for i, qi in list(zip(i_mid, mid))[::7] + list(zip(i_dup, dup))[::5] + list(zip(i_at, at))[::9]:
        d2 = ((qi - targets) ** 2).sum(axis=1)
        assert i == int(np.flatnonzero(d2 == d2.min())[0])
    twice = np.array([int((np.abs(targets - p).sum(axis=1) == 0).sum()) for p in dup[:20]])
    assert (twice == 2).all()


@pytest.mark.parametrize("reverse", [False, True], ids=["ascending", "reversed"])
def test_exact_radius_across_cells(reverse):
    """Targets on the coarse lattice 0.5 Z^3 in [-1, 1]^3 (125 points, 4 r apart), r = 0.125; queries exactly r from a target along
    +-x, +-y, +-z INSIDE the box (dyadic coordinates: d2 == r r to the bit, every other target at least 3 r away).  The cell edge is
    r (1 + 2^-20), so a query r from its partner lies in the neighbouring cell along that axis: the pair admitted at exactly the
    radius is found across a cell boundary — where a grid of edge r could lose it.  One ulp farther is rejected."""
    r = 0.125
    axis = np.arange(-2, 3) * 0.5
    targets = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(-1, 3)
    if reverse:
        targets = targets[::-1].copy()
    at, beyond, partner = [], [], []
    for ax in range(3):
        for sign in (-1.0, 1.0):
            inside = np.flatnonzero(np.abs(targets[:, ax] + sign * r) <= 1.0)
            on = targets[inside].copy()
            on[:, ax] += sign * r
            far = on.copy()
            far[:, ax] = np.nextafter(on[:, ax], sign * np.inf)          # away from the partner
            at.append(on)
            beyond.append(far)
            partner.append(inside)
    at, beyond, partner = np.concatenate(at), np.concatenate(beyond), np.concatenate(partner)
    queries = np.concatenate((at, beyond))
    want = R.nearest_within(queries, targets, r)
    got = host(icp.nearest_within(queries, targets, r))
    assert_same(got, want, "coarse lattice")
    n = len(at)
    assert np.array_equal(got[0][:n], partner) and np.array_equal(got[1][:n], np.full(n, r * r))
    assert (got[0][n:] == -1).all() and np.isinf(got[1][n:]).all()
    # the admitted pairs do cross cells: the keys of a query and of its partner differ for all but the 75 queries r above a target
    # on the box's lower faces (a quotient of 1 / (1 + 2^-20) stays in cell 0)
    grid = icp.build_grid(torch.from_numpy(targets).to(DEV), r)
    key_q = icp._cells(torch.from_numpy(at).to(DEV), grid.box, grid.dims, DEV).cpu().numpy()
    key_t = icp._cells(torch.from_numpy(targets).to(DEV), grid.box, grid.dims, DEV).cpu().numpy()[partner]
    crossing = int((key_q != key_t).sum())
    print(f"{crossing} of {n} pairs at exactly r lie in different cells; grid {grid.dims}")
    assert n == 600 and crossing == 525 and grid.dims == (16, 16, 16)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: the transform on the fly
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("move", [M, TURN], ids=["M", "170deg"])
def test_transform_on_the_fly(move):
    q, t = uniform_case(1037, 1805)
    radius = half_radius(1805)
    want = R.nearest_within(q, t, radius, move, workers=W)
    got = host(icp.nearest_within(q, t, radius, transform=move))
    assert_same(got, want, "transformed")
    assert 0.2 * len(q) < (got[0] >= 0).sum() < 0.8 * len(q)
    moved = icp.transform_points(q, move)
    assert moved.is_cuda and moved.dtype == torch.float64 and tuple(moved.shape) == q.shape
    assert np.array_equal(bits(moved.cpu().numpy()), bits(R.transform(q, move)))
    # the same search on the materialised points, without a transform
    assert_same(host(icp.nearest_within(moved, t, radius)), got, "materialised")
    assert_same(host(icp.nearest_within(moved, t, radius, transform=None)), got, "transform=None")
    assert np.array_equal(bits(lib.transform_points(moved, None).cpu().numpy()), bits(moved.cpu().numpy()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: refusals on the device
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_coordinates_are_refused(bad):
    g = np.random.default_rng(3)
    q, t = g.uniform(-1, 1, (3000, 3)), g.uniform(-1, 1, (5000, 3))
    for which, row, col in ((0, 2999, 2), (1, 4100, 0), (0, 0, 1)):
        pair = [q.copy(), t.copy()]
        pair[which][row, col] = bad
        with pytest.raises(lib.VfnError, match="non-finite"):
            icp.nearest_within(pair[0], pair[1], 0.1)
        with pytest.raises(lib.VfnError, match="non-finite"):
            icp.align(pair[0], pair[1], 0.1)
    index, sqdist = icp.nearest_within(q, t, 0.1)
    assert (index >= 0).any() and sqdist[index >= 0].isfinite().all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: the sums
# ---------------------------------------------------------------------------------------------------------------------------------
def check_sums(q, move, t, index, sqdist, anchor):
    """index / sqdist are device tensors.  All 17 sums equal the restatement of the fixed tree (lane order "near") bit for bit; the count
    is exact; every other sum is within L u sum|term| of math.fsum, L = the addition levels include/vfn.h states; two runs give equal
    bits."""
    n = len(q)
    qd, td = torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)
    twelve = icp._twelve(move)
    got = lib.icp_accumulate(qd, twelve, td, index, sqdist, tuple(anchor)).cpu().numpy()
    again = lib.icp_accumulate(qd, twelve, td, index, sqdist, tuple(anchor)).cpu().numpy()
    assert got.shape == (17,) and np.array_equal(bits(got), bits(again))
    placed = R.placed_terms(q, move, t, index.cpu().numpy(), sqdist.cpu().numpy(), anchor)
    assert np.array_equal(bits(got), bits(R.sums_of(placed, "tree")))
    rows = placed[index.cpu().numpy() >= 0]
    exact = R.sums_of(rows)
    assert got[0] == exact[0] == len(rows)
    L = lib.icp_sum_levels(n)
    p = -(-n // 4096)
    assert L == 4 + 8 + (-(-p // 1024) - 1) + 10
    scale = np.abs(rows).sum(axis=0) * (1.0 - 2.0 ** -40)          # (numpy's sum of the magnitudes, shaved: never above the exact one)
    err = np.abs(got - exact)
    worst = float(np.max(err[1:] / np.where(scale[1:] > 0, scale[1:], 1.0))) / U
    print(f"n={n}: {len(rows)} rows, worst sum error {worst:.2f} x 2^-53 of sum|term|, bound {L}")
    assert np.all(err[1:] <= L * U * scale[1:])
    return got


@pytest.mark.parametrize("n,m", [(1, 1), (257, 130), (4097, 1805), (100003, 2049)])
def test_accumulate_on_searched_pairs(n, m):
    q, t = uniform_case(n, m)
    q = q + 100.0
    t = t + 100.0                                          # far from the origin: the anchor is what keeps the products small
    radius = half_radius(m) if n > 1 else 8.0
    anchor = R.bounding_anchor(R.transform(t, None))
    move = R.rigid((1.0, 2.0, 3.0), 0.01, (1e-3, -2e-3, 5e-4)) if n > 1 else None
    index, sqdist = icp.nearest_within(q, t, radius, transform=move)
    got = check_sums(q, move, t, index, sqdist, anchor)
    assert got[0] >= 1 and (n == 1 or got[0] < n)
    # hand-made indices with -1 in them and arbitrary "distances"
    g = np.random.default_rng(n)
    index = torch.from_numpy(np.where(g.uniform(size=n) < 0.3, -1, g.integers(0, m, n))).to(DEV)
    sqdist = torch.from_numpy(g.uniform(0, 2, n)).to(DEV)
    check_sums(q, move, t, index, sqdist, anchor)
    none = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    assert np.array_equal(lib.icp_accumulate(torch.from_numpy(q).to(DEV), None, torch.from_numpy(t).to(DEV), none, sqdist, tuple(anchor)).cpu().numpy(),
                          np.zeros(17))


def test_accumulate_crosses_into_the_serial_joins():
    n, m = 4096 * 1024 + 5, 1000
    g = np.random.default_rng(9)
    q, t = g.uniform(-2, 2, (n, 3)), g.uniform(-2, 2, (m, 3))
    index = torch.arange(n, device=DEV) % m
    sqdist = torch.from_numpy(g.uniform(0, 1, n)).to(DEV)
    got = check_sums(q, None, t, index, sqdist, R.bounding_anchor(t))
    assert got[0] == n and lib.icp_sum_levels(n) == 23
    with pytest.raises(lib.VfnError, match="outside the targets"):
        lib.icp_accumulate(torch.from_numpy(q[:10]).to(DEV), None, torch.from_numpy(t).to(DEV), index[:10] + m, sqdist[:10], (0.0, 0.0, 0.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6 / 7: the loop
# ---------------------------------------------------------------------------------------------------------------------------------
_aligned = {}


def device_align(seed):
    if seed not in _aligned:
        src, tgt, radius = room_pair(seed)
        _aligned[seed] = icp.align(src, tgt, radius)
    return _aligned[seed]


@pytest.mark.parametrize("seed", [1, 2])
def test_loop_teacher_forced(seed):
    """Every recorded T_k goes to the restatement: its neighbours are the device's bit for bit, its count and fitness equal, its rmse
    within the sum bound ((L / 2 + 2) u relative: the sum of non-negative terms is within L u relative, the square root halves that,
    the division and the root round once each), and its T_{k+1} agrees with the device's within 16 x max(yardstick, 2^-50), the
    yardstick being the largest entrywise difference, over all steps, between the restatement's T_{k+1} from math.fsum sums and from
    numpy's sums — two legitimate float64 evaluations.  Measured on one MI355X: yardstick 1.77e-15 (seed 1, 12 searches) and
    1.91e-15 (seed 2, 21 searches); the device's largest difference 4.44e-16 and 7.77e-16; allowed 2.83e-14 and 3.06e-14."""
    src, tgt, radius = room_pair(seed)
    res = device_align(seed)
    anchor = R.bounding_anchor(tgt)
    L = lib.icp_sum_levels(len(src))
    hist = res.history
    assert len(hist) == res.iterations + 1 and np.array_equal(hist[0]["transformation"], np.eye(4))
    yardstick, device_gap = 0.0, 0.0
    for k, entry in enumerate(hist):
        t_k = entry["transformation"]
        index, sqdist, sums = R.step(src, t_k, tgt, radius, anchor, workers=W)
        assert_same(host(icp.nearest_within(src, tgt, radius, transform=t_k)), (index, sqdist), f"iteration {k}")
        count = int(sums[0])
        assert entry["count"] == count and entry["fitness"] == count / len(src)
        rmse = math.sqrt(sums[1] / count)
        assert abs(entry["inlier_rmse"] - rmse) <= (L / 2 + 2) * U * rmse, (k, entry["inlier_rmse"], rmse)
        if k + 1 < len(hist):
            exact = R.solve(sums, anchor) @ t_k
            plain = R.solve(R.sums_of(R.terms(src, t_k, tgt, index, sqdist, anchor), "numpy"), anchor) @ t_k
            yardstick = max(yardstick, float(np.abs(exact - plain).max()))
            device_gap = max(device_gap, float(np.abs(hist[k + 1]["transformation"] - exact).max()))
            assert not R.stop_rule(hist[:k + 1], icp.RELATIVE_FITNESS, icp.RELATIVE_RMSE)
    print(f"seed {seed}: {len(hist)} searches, yardstick {yardstick:.3g}, device's largest difference {device_gap:.3g}, "
          f"allowed {16 * max(yardstick, 2.0 ** -50):.3g}")
    assert device_gap <= 16 * max(yardstick, 2.0 ** -50)
    # the stop decision follows from the recorded numbers by the written rule
    assert res.converged == R.stop_rule(hist, icp.RELATIVE_FITNESS, icp.RELATIVE_RMSE)
    assert res.converged or res.iterations == icp.MAX_ITERATION
    assert np.array_equal(res.transformation, hist[-1]["transformation"])
    assert res.fitness == hist[-1]["fitness"] and res.inlier_rmse == hist[-1]["inlier_rmse"]


def test_align_recovers_the_motion():
    res = device_align(1)
    err = float(np.abs(res.transformation @ M - np.eye(4)).max())
    print(f"seed 1: {res.iterations} iterations, max|T M - I| = {err:.3g}, first count {res.history[0]['count']}")
    assert res.history[0]["count"] < N_ROOM
    assert res.converged and res.iterations <= 30
    assert err <= 1e-13
    assert res.transformation.dtype == np.float64 and res.transformation.shape == (4, 4)
    other = device_align(2)
    assert other.converged and other.iterations <= 30
    # a limit on the updates is honoured and reported
    src, tgt, radius = room_pair(1)
    short = icp.align(src, tgt, radius, max_iteration=2)
    assert short.iterations == 2 and not short.converged and len(short.history) == 3
    assert np.array_equal(short.history[2]["transformation"], res.history[2]["transformation"])
    started = icp.align(src, tgt, radius, init=res.history[3]["transformation"], max_iteration=1)
    assert np.array_equal(started.history[0]["transformation"], res.history[3]["transformation"])
    assert started.history[0]["count"] == res.history[3]["count"]


def test_align_refuses_what_determines_no_motion():
    g = np.random.default_rng(2)
    far = g.uniform(-1, 1, (50, 3))
    with pytest.raises(lib.VfnError, match="fewer than 3"):
        icp.align(far + 10.0, far, 0.1)
    line = np.outer(np.linspace(-1, 1, 50), [1.0, 2.0, -0.5])
    with pytest.raises(lib.VfnError, match="rank-deficient"):
        icp.align(line + 1e-3, line, 0.1)


# ---------------------------------------------------------------------------------------------------------------------------------
# 8: scoring
# ---------------------------------------------------------------------------------------------------------------------------------
def test_score_mesh_with_icp():
    from test_hip_metrics3d import extracted_mesh
    m = extracted_mesh()
    v = m.vertices_scaled
    moved = (torch.from_numpy(R.transform(v.cpu().numpy(), M)).to(DEV), m.faces)

    def gen():
        return torch.Generator(device=DEV).manual_seed(8)

    plain = metrics3d.score_mesh(moved, m, num_points=20000, distance_thresh=0.02, generator=gen())
    explicit = metrics3d.score_mesh(moved, m, num_points=20000, distance_thresh=0.02, generator=gen(), icp_align=False)
    assert plain == explicit and "icp" not in plain
    aligned = metrics3d.score_mesh(moved, m, num_points=20000, distance_thresh=0.02, generator=gen(), icp_align=True, icp_threshold=0.1)
    print({k: (round(e["chamfer distance"]["mean"], 6), round(e["precision"], 4), round(e["recall"], 4)) for k, e in (("plain", plain), ("icp", aligned))},
          aligned["icp"]["iterations"], aligned["icp"]["fitness"])
    assert aligned["chamfer distance"]["mean"] < plain["chamfer distance"]["mean"]
    assert aligned["precision"] >= plain["precision"] and aligned["recall"] >= plain["recall"]
    t = np.array(aligned["icp"]["transformation"])
    assert t.shape == (4, 4) and set(aligned["icp"]) == {"transformation", "fitness", "inlier_rmse", "iterations"}
    assert set(aligned) - {"icp"} == set(plain)


def test_metrics_3d_with_icp():
    s = TR.sphere_scene()
    hi = tuple(o + n * s.vl for o, n in zip(s.origin, s.dims))
    mesh = RR.merged(RR.icosphere(3, 0.5), RR.icosphere(1, 0.1))
    out = refuse.metrics_3d(mesh, RR.icosphere(3, 0.5), s.intrinsics_matrices(), s.poses, 48, 64, num_points=5000, distance_thresh=0.1,
                            generator=torch.Generator(device=DEV).manual_seed(3), icp_align=True, bounds=(s.origin, hi), voxel_length=s.vl,
                            sdf_trunc=s.trunc, device=DEV)
    assert list(out) == ["tsdf", "refused_tsdf", "tsdf_smoothed", "refused_tsdf_smoothed"]
    for entry in out.values():
        assert {"chamfer distance", "precision", "recall", "fscore", "icp"} <= set(entry)
        assert np.array(entry["icp"]["transformation"]).shape == (4, 4) and 0 < entry["icp"]["fitness"] <= 1.0
