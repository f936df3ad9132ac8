"""Mesh scoring on the MI355X (csrc/vfn_metrics.hip through vf_nerf_amd/metrics3d.py) against the CPU restatement
(tests/metrics3d_restatement.py) and scipy's cKDTree.  Distances, areas, samples, medians, minima, maxima and counts are compared bit
for bit; the two sums (cumulative areas, means) against math.fsum within the pairwise-summation bound of the tree the kernel builds,
and the statistics sum bit for bit against the restatement of that tree (tests/tree_restatement.py)."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, mesh, metrics3d  # noqa: E402
import metrics3d_restatement as R  # noqa: E402
from helpers import synthetic_field  # noqa: E402
from test_metrics3d_host import HAND_PRED, HAND_REF, NN_CASES, bits, nn_case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -53          # unit roundoff of float64


def dev_bits(t):
    return bits(t.cpu().numpy())


class FieldDecoder:
    """Serves a precomputed field [res^3,3] to mesh.extract_mesh in the order it asks for the lattice rows."""

    def __init__(self, field):
        self.field, self.row = field, 0

    def __call__(self, pts):
        out = self.field[self.row:self.row + pts.shape[0]]
        self.row += pts.shape[0]
        return out


_mesh_cache = {}


def extracted_mesh():
    if "m" not in _mesh_cache:
        res = 64
        field = synthetic_field(res, res).to(DEV)
        m = mesh.extract_mesh(FieldDecoder(field), res, scale=1.3, translation=torch.tensor([0.05, -0.02, 0.01]),
                              centroid=torch.tensor([0.0, 0.1, -0.05]))
        assert m.faces.shape[0] > 1000
        _mesh_cache["m"] = m
    return _mesh_cache["m"]


HAND_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [0, 0, 1], [2, 0, 1], [0, 2, 1], [0.1, 0.2, 0.3], [0.7, -0.4, 0.9], [-1.3, 0.6, 0.2]])
HAND_F = np.array([[0, 1, 2], [3, 3, 3], [4, 5, 6], [7, 8, 9], [1, 1, 2], [9, 7, 8], [0, 1, 1]])      # faces 1, 4, 6 are degenerate


# ---------------------------------------------------------------------------------------------------------------------------------
# 1 / 2: nearest distances
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NN_CASES)
def test_nearest_distances_equal_restatement_and_ckdtree(name):
    a, b = nn_case(name)
    for q, t in ((a, b), (b, a)):
        got = metrics3d.nearest_distances(q, t)
        assert got.is_cuda and got.dtype == torch.float64 and got.shape == (len(q),)
        want, tree = R.nearest_distances(q, t, workers=16), cKDTree(t).query(q)[0]
        assert np.array_equal(dev_bits(got), bits(want)), f"{name}: {int((dev_bits(got) != bits(want)).sum())} differ from the restatement"
        assert np.array_equal(dev_bits(got), bits(tree)), f"{name}: {int((dev_bits(got) != bits(tree)).sum())} differ from cKDTree"
        again = metrics3d.nearest_distances(torch.from_numpy(q).to(DEV), torch.from_numpy(t))
        assert torch.equal(again.view(torch.int64), got.view(torch.int64))


@pytest.mark.parametrize("n,m", [(1, 1), (1, 3000), (1037, 1805), (1024, 8), (3, 7), (2049, 100003)])
def test_nearest_distances_edge_shapes(n, m):
    """n = 1037 is not a multiple of the 1024 queries of a workgroup; with two query blocks m = 1805 is cut into 8 slices of 232 targets
    whose last holds 181 = 22 batches of 8 and a remainder of 5."""
    g = np.random.default_rng(1000 * n + m)
    q, t = g.uniform(-2, 2, (n, 3)), g.uniform(-2, 2, (m, 3))
    got = metrics3d.nearest_distances(q, t)
    assert np.array_equal(dev_bits(got), bits(R.nearest_distances(q, t)))
    assert np.array_equal(dev_bits(got), bits(cKDTree(t).query(q)[0]))
    assert torch.equal(metrics3d.nearest_distances(q, t).view(torch.int64), got.view(torch.int64))


def test_nearest_distances_2p17():
    g = np.random.default_rng(17)
    n = 1 << 17
    q, t = g.uniform(-1, 1, (n, 3)), g.uniform(-1, 1, (n, 3))
    t[:64] = q[:64]
    got = metrics3d.nearest_distances(q, t)
    first = dev_bits(got)
    assert np.array_equal(first, bits(cKDTree(t).query(q)[0]))
    assert np.array_equal(first, bits(R.nearest_distances(q, t, workers=16)))
    assert np.array_equal(dev_bits(metrics3d.nearest_distances(q, t)), first)
    assert int((got == 0).sum()) >= 64


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_coordinates_are_refused(bad):
    g = np.random.default_rng(3)
    q, t = g.uniform(-1, 1, (3000, 3)), g.uniform(-1, 1, (5000, 3))
    for which, row, col in ((0, 2999, 2), (1, 4100, 0), (0, 0, 1)):
        pair = [q.copy(), t.copy()]
        pair[which][row, col] = bad
        with pytest.raises(lib.VfnError, match="non-finite"):
            metrics3d.nearest_distances(*pair)
        with pytest.raises(lib.VfnError, match="non-finite"):
            metrics3d.chamfer_from_points(*pair)
        with pytest.raises(lib.VfnError, match="non-finite"):
            metrics3d.precision_recall_fscore(pair[0], pair[1], 0.1)
    assert metrics3d.nearest_distances(q, t).isfinite().all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: areas
# ---------------------------------------------------------------------------------------------------------------------------------
def test_triangle_areas_equal_restatement():
    m = extracted_mesh()
    for v, f in ((m.vertices_scaled, m.faces), (m.vertices, m.faces), (torch.from_numpy(HAND_V), torch.from_numpy(HAND_F))):
        got = metrics3d.face_areas(v, f)
        assert got.is_cuda and got.dtype == torch.float64
        assert np.array_equal(dev_bits(got), bits(R.tri_areas(v.cpu().numpy(), f.cpu().numpy())))
    hand = metrics3d.face_areas(HAND_V, HAND_F).cpu().numpy()
    assert hand[0] == 0.5 and hand[2] == 2.0 and hand[1] == hand[4] == hand[6] == 0.0 and hand[3] > 0 and hand[5] > 0


def test_out_of_range_face_index_is_refused():
    for bad in (len(HAND_V), -1, 1 << 40):
        f = HAND_F.copy()
        f[3, 1] = bad
        with pytest.raises(lib.VfnError, match="outside"):
            metrics3d.face_areas(HAND_V, f)
        with pytest.raises(lib.VfnError, match="outside"):
            metrics3d.sample_surface(HAND_V, f, 100)
    v = HAND_V.copy()
    v[8, 1] = float("nan")
    with pytest.raises(lib.VfnError, match="non-finite"):
        metrics3d.face_areas(v, HAND_F)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: the cumulative table and the samples
# ---------------------------------------------------------------------------------------------------------------------------------
def scan_bound_levels(n):
    """Additions on the longest path to a prefix of vfn_cumsum_f64 (csrc/vfn_metrics.hip): per scan level of 1024-value blocks a lane's
    3 serial additions, 8 Kogge-Stone levels over the 256 lane totals and 1 addition of the lane's own prefix = 12; a block total (3 + 8)
    plus the addition on the way down is 12 again.  Levels: 1 for n <= 1024, 2 for n <= 1024^2, 3 above."""
    levels = 1 if n <= 1024 else 2 if n <= 1024 ** 2 else 3
    assert levels == lib.cumsum_levels(n)
    return 12 * levels


def assert_prefixes_within_bound(x, cum, indices=None, table=False):
    """Every prefix (or the listed ones) within L x 2^-53 relative of the exact sum: the pairwise-summation bound for non-negative terms
    joined by a tree of depth L.  Exact rational arithmetic; math.fsum of a prefix is that sum rounded once."""
    L = scan_bound_levels(len(x))
    if table:         # the sampler's table (metrics3d.cumulative_areas): non-decreasing, and level across every zero-area face
        assert np.all(np.diff(cum) >= 0), "the cumulative table decreases"
        assert np.all(np.diff(cum)[x[1:] == 0] == 0) and (x[0] > 0 or cum[0] == 0), "the table rises across a zero-area face"
    worst = Fraction(0)
    if indices is None:
        run = Fraction(0)
        for i in range(len(x)):
            run += Fraction(float(x[i]))
            err = abs(Fraction(float(cum[i])) - run)
            assert err <= L * Fraction(U) * run, (i, float(err / run) / U if run else 0.0, L)
            if run:
                worst = max(worst, err / run)
    else:
        for i in indices:
            exact = Fraction(math.fsum(x[:i + 1]))
            err = abs(Fraction(float(cum[i])) - exact)
            # math.fsum itself is within half a unit of the exact sum
            assert err <= (L + Fraction(1, 2)) * Fraction(U) * exact, (i, float(err / exact) / U, L)
            worst = max(worst, err / exact)
    print(f"cumsum n={len(x)}: worst prefix error {float(worst) / U:.2f} x 2^-53, bound {L}")


@pytest.mark.parametrize("n", [1, 5, 1024, 1025, 4096, 100003])
def test_cumsum_is_a_fixed_tree_within_the_pairwise_bound(n):
    g = np.random.default_rng(n)
    x = g.uniform(0, 1, n) * 10.0 ** g.integers(-6, 3, n)
    x[g.integers(0, n, n // 10)] = 0.0
    cum = lib.cumsum_f64(torch.from_numpy(x).to(DEV))
    again = lib.cumsum_f64(torch.from_numpy(x).to(DEV))
    assert torch.equal(cum.view(torch.int64), again.view(torch.int64))
    assert_prefixes_within_bound(x, cum.cpu().numpy())


def test_cumsum_three_levels():
    n = 1024 * 1024 + 777
    g = np.random.default_rng(9)
    x = g.uniform(0, 1, n)
    cum = lib.cumsum_f64(torch.from_numpy(x).to(DEV)).cpu().numpy()
    idx = sorted({0, 1023, 1024, 1024 * 1024 - 1, 1024 * 1024, n - 1, *g.integers(0, n, 40).tolist()})
    assert_prefixes_within_bound(x, cum, idx)


def sampling_meshes():
    m = extracted_mesh()
    v, f = m.vertices_scaled.cpu().numpy(), m.faces.cpu().numpy()
    # degenerate faces spliced in at the front, in the middle and at the very end of the table
    deg = np.stack((f[:50, 0], f[:50, 0], f[:50, 1]), axis=1)
    f2 = np.concatenate((deg[:10], f[:777], deg[10:40], f[777:], deg[40:]))
    return [("extracted", v, f2), ("hand", HAND_V, HAND_F)]


@pytest.mark.parametrize("which", [0, 1])
def test_sample_surface_equals_restatement(which):
    name, v, f = sampling_meshes()[which]
    count = 200000 if which == 0 else 5000
    g = torch.Generator().manual_seed(40 + which)
    u = torch.rand(count, 3, dtype=torch.float64, generator=g)
    top = 1 - 2.0 ** -53
    u[:4] = torch.tensor([[0.0, 0.0, 0.0], [top, 0.5, 0.5], [0.5, top, top], [top, 0.0, top]], dtype=torch.float64)
    vd, fd = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    cum = metrics3d.cumulative_areas(vd, fd)
    areas = metrics3d.face_areas(vd, fd).cpu().numpy()
    assert np.array_equal(bits(areas), bits(R.tri_areas(v, f)))
    assert_prefixes_within_bound(areas, cum.cpu().numpy(), table=True)
    points, face = metrics3d.sample_surface(v, f, count, uniforms=u)
    assert points.is_cuda and face.is_cuda and points.dtype == torch.float64 and face.dtype == torch.int64
    want_p, want_f = R.sample_surface(v, f, cum.cpu().numpy(), u.numpy())
    face, points = face.cpu().numpy(), points.cpu().numpy()
    assert np.array_equal(face, want_f)
    assert np.array_equal(bits(points), bits(want_p))
    assert (areas == 0).sum() >= 3 and np.all(areas[face] > 0), "a degenerate face was chosen"
    # barycentric coordinates (1 - a - b, a, b) of the folded uniforms, in float64: all in [0, 1] ...
    a, b = u[:, 1].numpy().copy(), u[:, 2].numpy().copy()
    fold = a + b > 1.0
    a[fold], b[fold] = 1.0 - a[fold], 1.0 - b[fold]
    assert np.all((a >= 0) & (a <= 1) & (b >= 0) & (b <= 1) & (1.0 - a - b >= 0) & (1.0 - a - b <= 1))
    # ... so every point is a convex combination of its face's corners: inside their bounding box up to the rounding of two products
    # and two sums of values no larger than the box's largest coordinate
    tri = v[f[face]]
    slack = 8 * 2.0 ** -52 * np.abs(tri).max(axis=(1, 2))[:, None]
    assert np.all(points >= tri.min(axis=1) - slack) and np.all(points <= tri.max(axis=1) + slack)
    # every face with area is reachable and frequencies follow the areas: the largest face is drawn about count x share times
    big = int(np.argmax(areas))
    share = areas[big] / areas.sum()
    hits = int((face == big).sum())
    assert abs(hits - count * share) <= 6 * math.sqrt(count * share * (1 - share)) + 1


def test_sample_surface_generator_and_refusals():
    m = extracted_mesh()
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    p1, f1 = metrics3d.sample_surface(m.vertices_scaled, m.faces, 10000, generator=g)
    p2, f2 = metrics3d.sample_surface(m.vertices_scaled, m.faces, 10000, generator=g)
    assert not torch.equal(p1, p2)
    g.manual_seed(5)
    p3, f3 = metrics3d.sample_surface(m.vertices_scaled, m.faces, 10000, generator=g)
    assert torch.equal(p1.view(torch.int64), p3.view(torch.int64)) and torch.equal(f1, f3)
    with pytest.raises(ValueError, match="zero total area"):
        metrics3d.sample_surface(HAND_V, HAND_F[[1, 4, 6]], 10)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: statistics
# ---------------------------------------------------------------------------------------------------------------------------------
def sum_levels(n):
    """Addition levels of vfn_reduce_stats's sum (csrc/vfn_metrics.hip: 256 lanes x 16 values per first-level block, one second-level
    block of 1024 lanes): 4 (a lane's 16 values, balanced) + 8 (256 lanes, balanced) + ceil(P / 1024) - 1 (a second-level lane's serial
    run over its partials, P = ceil(n / 4096)) + 10 (1024 lanes, balanced)."""
    p = -(-n // 4096)
    levels = 4 + 8 + (-(-p // 1024) - 1) + 10
    assert levels == lib.reduce_sum_levels(n)
    return levels


@pytest.mark.parametrize("n", [1, 2, 255, 257, 4096, 4097, 1000003, 2500000, 4096 * 1024 + 5])
def test_statistics(n):
    g = np.random.default_rng(n)
    x = g.uniform(0, 1, n) ** 3 * 0.3
    if n > 10:
        x[g.integers(0, n, 5)] = 0.0
        x[n // 2] = x[n // 3]
    threshold = 0.05
    xd = torch.from_numpy(x).to(DEV)
    s = lib.reduce_stats(xd, threshold)
    s2 = lib.reduce_stats(xd, threshold)
    assert torch.equal(s.view(torch.int64), s2.view(torch.int64))
    total, mn, mx, cnt = s.cpu().tolist()
    assert bits(total) == bits(R.stats_sum(x))              # the fixed tree of include/vfn.h, lane order "far", bit for bit
    assert mn == x.min() and mx == x.max() and cnt == int((x < threshold).sum())
    assert lib.reduce_stats(xd, 0.0).cpu()[3] == 0 and lib.reduce_stats(xd, math.inf).cpu()[3] == n
    lo, hi = metrics3d._median_pair(xd).cpu().tolist()
    assert (lo + hi) / 2.0 == R.median(x) == float(np.median(x))
    L = sum_levels(n)
    exact = math.fsum(x) / n
    mean = total / n
    print(f"n={n}: mean error {abs(mean - exact) / exact / U:.2f} x 2^-53, bound {L}")
    assert abs(mean - exact) <= L * U * exact


def test_statistics_of_one_negative_zero():
    """The 4095 values past n join as +0.0: the sum of a lone -0.0 is +0.0; minimum and maximum keep the value itself."""
    x = np.array([-0.0])
    total, mn, mx, cnt = lib.reduce_stats(torch.from_numpy(x).to(DEV), 0.05).cpu().tolist()
    assert bits(total) == bits(R.stats_sum(x)) == bits(0.0)
    assert mn == 0.0 and mx == 0.0 and cnt == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# 6: end to end
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hand_case_on_the_device():
    assert metrics3d.nearest_distances(HAND_REF, HAND_PRED).cpu().tolist() == [0.0, 0.0, 3.0, 3.0]
    assert metrics3d.chamfer_from_points(HAND_PRED, HAND_REF) == (18.0 / 4.0 + 4.0 / 3.0, 4.5, 0.0, 9.0)
    assert metrics3d.chamfer_from_points(HAND_PRED, HAND_REF) == R.chamfer_from_points(HAND_PRED, HAND_REF)
    for thr in (0.0, 2.0, 2.5, 3.5):
        assert metrics3d.precision_recall_fscore(HAND_PRED, HAND_REF, thr) == R.precision_recall_fscore(HAND_PRED, HAND_REF, thr)


def test_score_mesh_against_itself_is_perfect():
    m = extracted_mesh()
    n = 50000
    u = torch.rand(n, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    out = metrics3d.score_mesh(m, m, num_points=n, distance_thresh=0.05, uniforms=u)
    assert out["chamfer distance"] == {"mean": 0.0, "median": 0.0, "min": 0.0, "max": 0.0}
    assert out["precision"] == out["recall"] == out["fscore"] == 1.0 and out["pred_within"] == out["ref_within"] == n
    assert set(out) == {"chamfer distance", "precision", "recall", "fscore", "pred_within", "ref_within"}
    p, _ = metrics3d.sample_surface(m.vertices_scaled, m.faces, n, uniforms=u)
    assert bool((metrics3d.nearest_distances(p, p) == 0).all())


def test_score_mesh_against_a_shifted_copy():
    """Vertices on the 2^-10 grid, barycentric uniforms on the 2^-10 grid and a dyadic shift make every sample exact, so sample i of the
    shifted mesh is sample i of the mesh plus t exactly and its nearest distance cannot exceed |t|; |t| = 7/32 is itself exact, so the
    squares of the rounded distances cannot exceed |t|^2 either."""
    m = extracted_mesh()
    v = torch.round(m.vertices_scaled * 1024.0) / 1024.0
    t = torch.tensor([2.0, -3.0, 6.0], dtype=torch.float64) / 32.0        # |t| = 7/32 and |t|^2 = 49/1024, both exact
    t2 = 49.0 / 1024.0
    n = 40000
    g = torch.Generator().manual_seed(8)
    u = torch.rand(n, 3, dtype=torch.float64, generator=g)
    u[:, 1:] = torch.randint(0, 1024, (n, 2), generator=g).double() / 1024.0
    shifted = (v + t.to(DEV), m.faces)
    p, fp = metrics3d.sample_surface(v, m.faces, n, uniforms=u)
    s, fs = metrics3d.sample_surface(*shifted, n, uniforms=u)
    assert torch.equal(fp, fs) and torch.equal(s, p + t.to(DEV))
    for a, b in ((p, s), (s, p)):
        d = metrics3d.nearest_distances(a, b)
        assert bool((d <= math.sqrt(t2)).all())
    out = metrics3d.score_mesh((v, m.faces), shifted, num_points=n, distance_thresh=0.05, uniforms=u)
    assert 0.0 < out["chamfer distance"]["max"] <= t2 and out["chamfer distance"]["min"] >= 0.0
    assert out["chamfer distance"]["mean"] <= 2 * t2 and out["chamfer distance"]["median"] <= 2 * t2
    assert 0.0 <= out["precision"] <= 1.0 and 0.0 <= out["recall"] <= 1.0
    far = metrics3d.score_mesh((v, m.faces), (v + 100.0, m.faces), num_points=2000, distance_thresh=0.05, uniforms=u[:2000])
    assert far["precision"] == far["recall"] == far["fscore"] == 0.0


def test_chamfer_distance_is_reproducible_and_equals_the_restatement():
    m = extracted_mesh()
    other = (m.vertices_scaled * 1.01 + 0.003, m.faces.flip(0))
    n = 20000
    g = torch.Generator(device=DEV)
    g.manual_seed(77)
    first = metrics3d.chamfer_distance(m, other, num_points=n, generator=g)
    g.manual_seed(77)
    second = metrics3d.chamfer_distance(m, other, num_points=n, generator=g)
    assert first == second and all(type(x) is float for x in first)
    # the device's own points: pred first, then ref, from the same generator
    g.manual_seed(77)
    pred, _ = metrics3d.sample_surface(m.vertices_scaled, m.faces, n, generator=g)
    ref, _ = metrics3d.sample_surface(*other, n, generator=g)
    pred, ref = pred.cpu().numpy(), ref.cpu().numpy()
    assert first == metrics3d.chamfer_from_points(pred, ref)
    mean, median, mn, mx = R.chamfer_from_points(pred, ref, workers=16)
    assert first[1:] == (median, mn, mx)
    one, two = np.square(R.nearest_distances(ref, pred, workers=16)), np.square(R.nearest_distances(pred, ref, workers=16))
    exact = math.fsum(one) / n + math.fsum(two) / n
    L = sum_levels(n) + 1               # each direction's mean as in test_statistics, and one more addition joins the two
    print(f"chamfer mean error {abs(first[0] - exact) / exact / U:.2f} x 2^-53 (numpy's mean: {abs(mean - exact) / exact / U:.2f}), bound {L}")
    assert abs(first[0] - exact) <= L * U * exact
    # score_mesh shares the sampling and the searches: the same chamfer numbers and the restatement's counts
    g.manual_seed(77)
    out = metrics3d.score_mesh(m, other, num_points=n, distance_thresh=0.01, generator=g)
    assert tuple(out["chamfer distance"][k] for k in ("mean", "median", "min", "max")) == first
    want = R.precision_recall_fscore(pred, ref, 0.01, workers=16)
    assert {k: out[k] for k in want} == want and 0 < want["pred_within"] < n
