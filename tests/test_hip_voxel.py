"""Voxel down-sampling on the MI355X (csrc/vfn_voxel.hip through vf_nerf_amd/voxel.py, metrics3d and icp.align_stages) against the CPU
restatement of its contract (tests/voxel_restatement.py).  Every comparison is bit for bit: points, normals, colours, counts,
voxel_of_point, origin and dims; the staged registration in every stage's transformation bits, counts and iterations."""
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
import voxel_restatement as V  # noqa: E402
from test_voxel_host import SMALL, assert_same_sample, bits, skewed_case, uniform  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
W = 16                  # threads of the brute-force restatement of the search


def host(s) -> dict:
    """A ``VoxelDownSample`` -> the restatement's dictionary of numpy arrays, the placement and dtypes checked on the way."""
    for t, dtype in ((s.points, torch.float64), (s.counts, torch.int64), (s.voxel_of_point, torch.int64)):
        assert t.is_cuda and t.dtype == dtype and t.is_contiguous()
    assert s.points.shape == (s.counts.shape[0], 3)
    assert isinstance(s.origin, tuple) and isinstance(s.dims, tuple) and all(isinstance(d, int) for d in s.dims)
    opt = {name: None if getattr(s, name) is None else getattr(s, name).cpu().numpy() for name in ("normals", "colours")}
    return dict(opt, points=s.points.cpu().numpy(), counts=s.counts.cpu().numpy(), voxel_of_point=s.voxel_of_point.cpu().numpy(),
                origin=s.origin, dims=s.dims)


def attributes(p):
    g = np.random.default_rng(len(p) + 1)
    return g.standard_normal(p.shape), g.uniform(0, 1, p.shape)


def check(p, h, what, normals=None, colours=None):
    got = host(metrics3d.voxel_down_sample(p, h, normals=normals, colours=colours))
    assert_same_sample(got, V.down_sample(p, h, normals, colours), what)
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: the down-sampling
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SMALL))
def test_small_cases_equal_the_restatement(name):
    """n = 1, 2 (one voxel, two voxels), the wave and block edges 63 / 64 / 65 and 255 / 256 / 257, 4097, negative coordinates,
    coordinates near 10^6, points exactly on voxel faces, a skewed set, a single -0.0 — with 3, 6 and 9 channels."""
    p, h = SMALL[name]
    normals, colours = attributes(p)
    check(p, h, name)                                                      # C = 3
    check(p, h, name + " + colours", colours=colours)                      # C = 6, the second block being the colours
    got = check(p, h, name + " + normals + colours", normals, colours)     # C = 9
    if name == "minus_zero":
        assert np.signbit(got["points"]).all(), "the sign bit of a lone -0.0 must survive"
    # torch tensors on the device and float32 inputs are the same points
    again = host(metrics3d.voxel_down_sample(torch.from_numpy(p).to(DEV), h, normals=torch.from_numpy(normals)))
    assert np.array_equal(bits(again["points"]), bits(got["points"])) and np.array_equal(bits(again["normals"]), bits(got["normals"]))
    p32 = p.astype(np.float32)
    assert_same_sample(host(metrics3d.voxel_down_sample(p32, h)), V.down_sample(p32.astype(np.float64), h), name + " float32")


_cloud = {}


def cloud():
    if "p" not in _cloud:
        _cloud["p"] = uniform(1 << 17, 17, 0.0, 1.0)
        _cloud["a"] = attributes(_cloud["p"])
    return _cloud["p"], _cloud["a"]


@pytest.mark.parametrize("h,kind", [(0.0358, "six"), (2e-5, "alone"), (4.0, "all")])
def test_random_cloud_at_three_voxel_sizes(h, kind):
    """2^17 uniform points: about 6 a voxel, every point alone (V = n), one voxel holding all (V = 1: the longest serial sum)."""
    p, (normals, colours) = cloud()
    got = check(p, h, kind, normals, colours)
    v = len(got["counts"])
    print(f"{kind}: h = {h}, V = {v}, largest voxel {got['counts'].max()}")
    if kind == "six":
        assert 5.0 < len(p) / v < 7.0
    elif kind == "alone":
        assert v == len(p) and np.array_equal(bits(got["points"][got["voxel_of_point"]]), bits(p))
    else:
        assert v == 1 and got["dims"] == (1, 1, 1)


def test_skewed_far_and_negative_clouds():
    p = skewed_case(1 << 15, 21)
    got = check(p, 0.05, "skewed", *attributes(p))
    assert got["counts"].max() == 1 << 14
    far = 1e6 + uniform(1 << 15, 22, 0.0, 0.05)
    got = check(far, 0.004, "far", *attributes(far))
    assert min(got["dims"]) >= 10
    neg = uniform(1 << 15, 23, -9.0, -1.0)
    check(neg, 0.3, "negative", *attributes(neg))


def test_a_permutation_of_the_rows():
    p, h = uniform(20000, 31), 0.1
    perm = np.random.default_rng(32).permutation(len(p))
    a, b = check(p, h, "as given"), check(p[perm], h, "permuted")
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["voxel_of_point"][perm], b["voxel_of_point"])
    assert a["origin"] == b["origin"] and a["dims"] == b["dims"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2: the statuses: the kernels' defined answers to bad input
# ---------------------------------------------------------------------------------------------------------------------------------
def test_non_finite_coordinates_are_refused_and_the_next_call_is_correct():
    p, h = SMALL["n257"]
    for value in (np.nan, np.inf, -np.inf):
        bad = p.copy()
        bad[100, 1] = value
        with pytest.raises(lib.VfnError, match="non-finite"):
            metrics3d.voxel_down_sample(bad, h)
        check(p, h, "after a refusal")
        # the kernel's own answer, without the box in front of it
        origin, _ = V.frame(p, h)
        info = torch.zeros(1, dtype=torch.int64, device=DEV)
        keys = lib.voxel_keys(torch.from_numpy(bad).to(DEV), origin, h, info=info).cpu().numpy()
        want, status = V.keys(bad, origin, h)
        assert int(info.cpu()) == status == lib.GEOM_STATUS_NONFINITE and keys[100] == -1 and np.array_equal(keys, want)
        with pytest.raises(lib.VfnError, match="non-finite"):
            lib.voxel_keys(torch.from_numpy(bad).to(DEV), origin, h)


def test_keys_with_an_origin_that_is_not_the_boxs():
    p, h = SMALL["n4097"]
    origin = (0.0, -1.5, -1.5)                        # every point with x < 0 has c_0 < 0
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    keys = lib.voxel_keys(torch.from_numpy(p).to(DEV), origin, h, info=info).cpu().numpy()
    want, status = V.keys(p, origin, h)
    assert int(info.cpu()) == status == lib.GEOM_STATUS_INDEX
    assert np.array_equal(keys, want) and np.array_equal(keys == -1, p[:, 0] < 0) and 1000 < (keys == -1).sum() < 3000
    far = (-3e6, -3e6, -3e6)                          # ... and beyond 2^21 voxels on the other side
    keys = lib.voxel_keys(torch.from_numpy(p).to(DEV), far, 1.0, info=info).cpu().numpy()
    assert (keys == -1).all() and np.array_equal(keys, V.keys(p, far, 1.0)[0])
    with pytest.raises(lib.VfnError, match="voxel index outside"):
        lib.voxel_keys(torch.from_numpy(p).to(DEV), origin, h)
    # the keys of the right frame are the restatement's
    origin, _ = V.frame(p, h)
    assert np.array_equal(lib.voxel_keys(torch.from_numpy(p).to(DEV), origin, h).cpu().numpy(), V.keys(p, origin, h)[0])


@pytest.mark.parametrize("channels", [1, 3, 9])
def test_means_do_not_trust_the_table(channels):
    n = 300
    x = np.random.default_rng(channels).standard_normal((n, channels))
    start = np.array([0, 2, 2, 70, 64, 64 + 130, n, n + 3, -4, 5, 5, n], dtype=np.int64)
    # segments: good, EMPTY, good (68 rows), DECREASING, good, good, BEYOND n, NEGATIVE bounds, from a negative bound, EMPTY, good
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    got = lib.voxel_means(torch.from_numpy(x).to(DEV), torch.from_numpy(start).to(DEV), info=info).cpu().numpy()
    want = V.serial_means(x, start)
    bad = np.isnan(want).all(axis=1)
    assert bad.tolist() == [False, True, False, True, False, False, True, True, True, True, False]
    assert int(info.cpu()) == lib.GEOM_STATUS_INDEX
    assert np.isnan(got[bad]).all() and np.array_equal(bits(got[~bad]), bits(want[~bad]))
    with pytest.raises(lib.VfnError, match="segment outside"):
        lib.voxel_means(torch.from_numpy(x).to(DEV), torch.from_numpy(start).to(DEV))
    good = np.array([0, 1, 64, 65, 129, n], dtype=np.int64)
    got = lib.voxel_means(torch.from_numpy(x).to(DEV), torch.from_numpy(good).to(DEV)).cpu().numpy()
    assert np.array_equal(bits(got), bits(V.serial_means(x, good)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: the purpose
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_occupied_voxel_votes_once():
    """A dyadic lattice, where every sum and mean is exact: the ref points k / 8 on a plane, the pred points 1 / 64 above a part of them
    (inside the threshold 1 / 32) and a part half a unit above (beyond it).  Replicating the far part four times changes the plain
    precision and leaves the voxel_size= precision, recall and F-score identical to the bit: at voxel 1 / 16 every lattice position
    is alone in its voxel, and the mean of four copies of x is x."""
    k = np.arange(16, dtype=np.float64) / 8.0
    ref = np.stack(np.meshgrid(k, k, [0.0], indexing="ij"), axis=-1).reshape(-1, 3)
    near = ref[:160] + np.array([0.0, 0.0, 1.0 / 64])
    far = ref[160:] + np.array([0.0, 0.0, 0.5])
    once, four = np.concatenate((near, far)), np.concatenate((near, far, far, far, far))
    t, h = 1.0 / 32, 1.0 / 16
    plain_once, plain_four = metrics3d.precision_recall_fscore(once, ref, t), metrics3d.precision_recall_fscore(four, ref, t)
    assert plain_once["precision"] == 160 / 256 and plain_four["precision"] == 160 / (160 + 4 * 96) and plain_once["recall"] == 160 / 256
    for search in metrics3d.SEARCHES:
        vox_once = metrics3d.precision_recall_fscore(once, ref, t, voxel_size=h, search=search)
        vox_four = metrics3d.precision_recall_fscore(four, ref, t, voxel_size=h, search=search)
        assert vox_once["voxel"] == vox_four["voxel"] == {"size": h, "pred_points": 256, "ref_points": 256}
        for key in ("precision", "recall", "fscore"):
            assert np.array_equal(bits(vox_once[key]), bits(vox_four[key])), key
        assert vox_once == vox_four
        assert vox_four["precision"] == plain_once["precision"] and vox_four["recall"] == plain_once["recall"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: scoring
# ---------------------------------------------------------------------------------------------------------------------------------
def gen(seed=8):
    return torch.Generator(device=DEV).manual_seed(seed)


PRED = RR.merged(RR.icosphere(3, 0.5), RR.icosphere(1, 0.1, centre=(0.9, 0.0, 0.0)))          # a sphere and a floater
REF = RR.icosphere(3, 0.52)
N_SAMPLES, THRESH, VOXEL = 20000, 0.05, 0.025


def test_score_mesh_without_voxel_size_is_unchanged():
    plain = metrics3d.score_mesh(PRED, REF, num_points=N_SAMPLES, distance_thresh=THRESH, generator=gen())
    explicit = metrics3d.score_mesh(PRED, REF, num_points=N_SAMPLES, distance_thresh=THRESH, generator=gen(), voxel_size=None)
    assert plain == explicit and "voxel" not in plain
    assert set(plain) == {"chamfer distance", "precision", "recall", "fscore", "pred_within", "ref_within"}


@pytest.mark.parametrize("search", metrics3d.SEARCHES)
def test_score_mesh_with_voxel_size_is_the_steps_by_hand(search):
    out = metrics3d.score_mesh(PRED, REF, num_points=N_SAMPLES, distance_thresh=THRESH, generator=gen(), voxel_size=VOXEL, search=search)
    g = gen()
    pred, _ = metrics3d.sample_surface(*PRED, N_SAMPLES, generator=g)
    ref, _ = metrics3d.sample_surface(*REF, N_SAMPLES, generator=g)
    p, r = metrics3d.voxel_down_sample(pred, VOXEL).points, metrics3d.voxel_down_sample(ref, VOXEL).points
    assert_same_sample(host(metrics3d.voxel_down_sample(pred, VOXEL)), V.down_sample(pred.cpu().numpy(), VOXEL), "the pred samples")
    mean, median, mn, mx = metrics3d.chamfer_from_points(p, r, search=search)
    assert out["chamfer distance"] == {"mean": mean, "median": median, "min": mn, "max": mx}
    prf = metrics3d.precision_recall_fscore(p, r, THRESH, search=search)
    assert {k: out[k] for k in prf} == prf
    assert out["voxel"] == {"size": VOXEL, "pred_points": p.shape[0], "ref_points": r.shape[0]} and 100 < p.shape[0] < N_SAMPLES
    assert set(out) == set(prf) | {"chamfer distance", "voxel"}
    # the keyword of precision_recall_fscore is the same two steps
    direct = metrics3d.precision_recall_fscore(pred, ref, THRESH, voxel_size=VOXEL, search=search)
    assert {k: direct[k] for k in prf} == prf and direct["voxel"] == out["voxel"]
    # the floater weighs by its samples without the keyword and by its voxels with it
    plain = metrics3d.score_mesh(PRED, REF, num_points=N_SAMPLES, distance_thresh=THRESH, generator=gen(), search=search)
    print(search, {k: (round(e["precision"], 4), round(e["recall"], 4)) for k, e in (("plain", plain), ("voxel", out))}, out["voxel"])
    assert plain["precision"] < 1.0 and out["precision"] < 1.0 and out["precision"] != plain["precision"]


def test_score_mesh_with_icp_and_voxel_size():
    moved = (R.transform(PRED[0], R.rigid((1.0, 2.0, 3.0), 1.0, (0.004, -0.002, 0.003))), PRED[1])
    kw = dict(num_points=N_SAMPLES, distance_thresh=THRESH, icp_align=True, icp_threshold=0.1)
    without = metrics3d.score_mesh(moved, REF, generator=gen(), **kw)
    with_voxel = metrics3d.score_mesh(moved, REF, generator=gen(), voxel_size=VOXEL, **kw)
    assert with_voxel["icp"] == without["icp"] and set(with_voxel) == set(without) | {"voxel"}
    g = gen()
    pred, _ = metrics3d.sample_surface(*moved, N_SAMPLES, generator=g)
    ref, _ = metrics3d.sample_surface(*REF, N_SAMPLES, generator=g)
    pred = icp.transform_points(pred, np.array(without["icp"]["transformation"]))
    prf = metrics3d.precision_recall_fscore(pred, ref, THRESH, voxel_size=VOXEL)
    assert {k: with_voxel[k] for k in prf} == prf
    with pytest.raises(ValueError, match="normal consistency is not defined"):
        metrics3d.score_mesh(moved, REF, num_points=100, voxel_size=VOXEL, normals=True)


def test_metrics_3d_with_and_without_voxel_size():
    s = TR.sphere_scene()
    hi = tuple(o + n * s.vl for o, n in zip(s.origin, s.dims))
    mesh = RR.merged(RR.icosphere(3, 0.5), RR.icosphere(1, 0.1))
    args = (mesh, RR.icosphere(3, 0.5), s.intrinsics_matrices(), s.poses, 48, 64)
    kw = dict(num_points=5000, distance_thresh=0.1, bounds=(s.origin, hi), voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    plain = refuse.metrics_3d(*args, generator=gen(3), **kw)
    explicit = refuse.metrics_3d(*args, generator=gen(3), voxel_size=None, **kw)
    assert plain == explicit and all("voxel" not in e for e in plain.values())
    out = refuse.metrics_3d(*args, generator=gen(3), voxel_size=0.05, search="grid", **kw)
    assert list(out) == list(plain)
    for entry in out.values():
        assert entry["voxel"]["size"] == 0.05 and 10 < entry["voxel"]["pred_points"] < 5000 and 10 < entry["voxel"]["ref_points"] < 5000
        assert 0.0 < entry["fscore"] <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: the staged registration
# ---------------------------------------------------------------------------------------------------------------------------------
OFFSET = R.rigid((1.0, 2.0, 3.0), 2.0, (0.012, -0.006, 0.009))
STAGES = [(0.04, 0.025, 6), (None, 0.02, 30)]          # the first stage rejects pairs and ends at its limit, the second converges


def test_align_stages_equals_the_restatement():
    src, tgt = R.transform(R.corner_room(4096, 1), OFFSET), R.corner_room(4096, 1)
    res = icp.align_stages(src, tgt, STAGES)
    want = V.align_stages(src, tgt, STAGES, workers=W)
    assert isinstance(res, icp.Result) and len(res.stages) == len(want["stages"]) == 2
    for k, (got, ref) in enumerate(zip(res.stages, want["stages"])):
        print(f"stage {k}: {got['source_points']} x {got['target_points']} points, {got['iterations']} iterations, fitness {got['fitness']:.4f}, "
              f"rmse {got['inlier_rmse']:.3g}")
        assert (got["source_points"], got["target_points"]) == (ref["source_points"], ref["target_points"]), k
        assert got["iterations"] == ref["iterations"] and got["converged"] == ref["converged"], k
        assert np.array_equal(bits(got["transformation"]), bits(ref["transformation"])), k
        mine = [e for e in res.history if e["stage"] == k]
        assert [e["count"] for e in mine] == [e["count"] for e in ref["history"]], k
        assert all(np.array_equal(bits(a["transformation"]), bits(b["transformation"])) for a, b in zip(mine, ref["history"])), k
        assert (got["voxel_size"], got["max_correspondence_distance"]) == STAGES[k][:2]
    assert res.stages[0]["source_points"] < 4096 and res.stages[1]["source_points"] == 4096
    assert not res.stages[0]["converged"] and res.stages[0]["iterations"] == 6 and len({e["count"] for e in res.history if e["stage"] == 0}) > 1
    assert np.array_equal(bits(res.transformation), bits(want["transformation"]))
    assert res.iterations == sum(s["iterations"] for s in res.stages) and res.converged == res.stages[-1]["converged"]
    assert res.fitness == res.stages[-1]["fitness"] and res.inlier_rmse == res.stages[-1]["inlier_rmse"]
    assert len(res.history) == sum(s["iterations"] + 1 for s in res.stages)
    err = float(np.abs(res.transformation @ OFFSET - np.eye(4)).max())
    print(f"max|T M - I| = {err:.3g}")
    assert res.converged and err <= 1e-12


def test_a_single_stage_without_voxel_is_align():
    src, tgt = R.transform(R.corner_room(4096, 1), OFFSET), R.corner_room(4096, 1)
    one = icp.align_stages(src, tgt, [(None, 0.03, 30)])
    ref = icp.align(src, tgt, 0.03)
    assert np.array_equal(bits(one.transformation), bits(ref.transformation))
    assert (one.iterations, one.converged, one.fitness, one.inlier_rmse) == (ref.iterations, ref.converged, ref.fitness, ref.inlier_rmse)
    assert [e["count"] for e in one.history] == [e["count"] for e in ref.history]
    assert all(np.array_equal(bits(a["transformation"]), bits(b["transformation"])) for a, b in zip(one.history, ref.history))
    # an initial transformation is where the first stage starts from
    started = icp.align_stages(src, tgt, [(None, 0.03, 0)], init=ref.transformation)
    assert np.array_equal(bits(started.transformation), bits(icp.compose(np.eye(4), ref.transformation))) and started.iterations == 0
    assert started.history[0]["count"] == ref.history[-1]["count"]
