"""K-means on the MI355X (csrc/vfn_kmeans.hip through vf_nerf_amd/cluster.py, meshops.dominant_bases and bases.get_dominant_bases)
against the CPU restatement of its contract (tests/kmeans_restatement.py).  Every comparison is bit for bit: the centres, the labels, the
counts, the squared distances, the inertia, the number of passes, the convergence flag and the winning restart."""
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import bases, cluster, dropin, lib, meshops, ply  # noqa: E402
import kmeans_restatement as K  # noqa: E402
import meshops_restatement as M  # noqa: E402
import simplify_restatement as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_want = {}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def golden_normals(tag):
    v, f = S.golden(tag)
    return np.ascontiguousarray(M.vertex_normals(v, f)[np.unique(f.reshape(-1))])


def duplicates():
    """Three distinct points, ten rows: with k = 5 two seeds repeat earlier ones and their clusters stay empty."""
    rows = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 0.6, 0.8]])
    return rows[[0, 1, 0, 2, 1, 1, 0, 2, 0, 1]]


def midway():
    """The third point lies exactly midway between the two given centres (both distances are 1.0): it belongs to cluster 0."""
    points = np.array([[-1.25, 0.0, 0.0], [1.5, 0.25, 0.0], [0.0, 0.0, 0.0], [-0.75, 0.5, 0.0], [1.0, -0.5, 0.25]])
    return points, np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])


# name -> () -> (points, k, keyword arguments of kmeans): built on first use, so that collecting this module costs nothing
CASES = {
    "one_point": lambda: (np.array([[0.3, -0.2, 0.9]]), 1, {}),
    "n4095": lambda: (K.blobs(4095, 1), 6, {}),
    "n4096": lambda: (K.blobs(4096, 2), 6, {}),
    "n4097": lambda: (K.blobs(4097, 3), 6, {}),
    "k1": lambda: (K.sphere(1000, 4), 1, {}),
    "k64": lambda: (K.sphere(1500, 5), 64, {}),
    "two_tiles_k16": lambda: (K.sphere(9000, 6), 16, {}),
    "duplicates": lambda: (duplicates(), 5, {}),
    "midway": lambda: (midway()[0], 2, {"init": midway()[1], "max_iter": 1}),
    "max_iter_1": lambda: (K.blobs(4097, 3), 6, {"max_iter": 1}),
    "max_iter_2": lambda: (K.blobs(4097, 3), 6, {"max_iter": 2}),
    "plusplus": lambda: (K.blobs(5000, 7), 6, {"init": "k-means++", "n_init": 3, "seed": 7}),
    "plusplus_duplicates": lambda: (duplicates(), 5, {"init": "k-means++", "n_init": 2, "seed": 1}),
    "golden_f16_k3": lambda: (golden_normals("f16"), 3, {}),
    "golden_f16_k6": lambda: (golden_normals("f16"), 6, {}),
    "golden_f32_k3": lambda: (golden_normals("f32"), 3, {}),
    "golden_f32_k6": lambda: (golden_normals("f32"), 6, {}),
}
_case = {}


def case(name):
    if name not in _case:
        _case[name] = CASES[name]()
    return _case[name]


def want(name):
    """The restatement of a case, computed once and shared."""
    if name not in _want:
        points, k, args = case(name)
        _want[name] = K.kmeans(points, k, **args)
    return _want[name]


def host(r) -> dict:
    assert isinstance(r, cluster.KMeans) and isinstance(r.n_iter, int) and isinstance(r.converged, bool) and isinstance(r.restart, int)
    for t, dtype in ((r.centres, torch.float64), (r.sqdist, torch.float64), (r.inertia, torch.float64), (r.labels, torch.int64), (r.counts, torch.int64)):
        assert t.is_cuda and t.dtype == dtype
    return dict(centres=r.centres.cpu().numpy(), labels=r.labels.cpu().numpy(), counts=r.counts.cpu().numpy(), sqdist=r.sqdist.cpu().numpy(),
                inertia=float(r.inertia.cpu()), n_iter=r.n_iter, converged=r.converged, restart=r.restart)


@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_the_restatement(name):
    points, k, args = case(name)
    r = cluster.kmeans(points, k, device=DEV, **args)
    got, ref = host(r), want(name)
    print(f"{name}: n {len(points)} k {k} passes {got['n_iter']} converged {got['converged']} restart {got['restart']} counts {got['counts'].tolist()}")
    assert got["n_iter"] == ref["n_iter"] and got["converged"] == ref["converged"] and got["restart"] == ref["restart"]
    assert np.array_equal(got["labels"], ref["labels"]) and np.array_equal(got["counts"], ref["counts"])
    assert same_bits(got["centres"], ref["centres"]) and same_bits(got["sqdist"], ref["sqdist"]) and same_bits(got["inertia"], ref["inertia"])
    # the invariants of the contract, on the device itself: the returned labels are the assignment against the returned centres ...
    p = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float64)).to(DEV)
    label = torch.empty(len(points), dtype=torch.int32, device=DEV)
    sqdist = torch.empty(len(points), dtype=torch.float64, device=DEV)
    changed = torch.zeros(1, dtype=torch.int64, device=DEV)
    lib.kmeans_assign(p, r.centres, r.labels.to(torch.int32), label, sqdist, changed)
    assert int(changed.cpu()) == 0 and torch.equal(label.to(torch.int64), r.labels) and same_bits(sqdist.cpu().numpy(), got["sqdist"])
    assert int(r.counts.sum()) == len(points) and torch.equal(torch.bincount(r.labels, minlength=k), r.counts)
    # ... and, converged, the centres are the update of the returned labels (an empty cluster keeps its centre)
    if r.converged:
        again = r.centres.clone()
        _, count = lib.kmeans_update(p, label, again)
        assert same_bits(again.cpu().numpy(), got["centres"]) and torch.equal(count, r.counts)


def test_what_the_cases_are_there_for():
    assert not want("max_iter_1")["converged"] and want("max_iter_1")["n_iter"] == 1
    assert not want("max_iter_2")["converged"] and want("max_iter_2")["n_iter"] == 2
    assert want("n4097")["converged"] and want("n4097")["n_iter"] > 2
    dup = want("duplicates")
    assert sorted(dup["counts"].tolist()) == [0, 0, 2, 4, 4] and dup["converged"]          # two empty clusters, reported and kept
    empty = np.flatnonzero(dup["counts"] == 0)
    assert all(any(np.array_equal(dup["centres"][j], row) for row in duplicates()) for j in empty)
    assert want("midway")["labels"][2] == 0 and want("midway")["sqdist"][2] == 1.0          # the tie went to the lower cluster
    assert want("plusplus")["restart"] in (0, 1, 2) and want("k64")["counts"].shape == (64,) and want("two_tiles_k16")["converged"]


def test_update_alone_across_the_serial_join():
    """n = 4096 x 1024 + 1: 1025 partials per cluster, so that lane 0 of the second level adds two of them serially."""
    n, k = lib.REDUCE_TILE * lib.REDUCE_TOP + 1, 2
    points, label = K.labelled_ramp(n, k)
    previous = np.array([[7.0, 8.0, 9.0], [-1.0, -2.0, -3.0]])
    sums, count, centres, status = K.update_arrays(points, label, previous)
    got_centres = torch.from_numpy(previous.copy()).to(DEV)
    got_sums, got_count = lib.kmeans_update(torch.from_numpy(points).to(DEV), torch.from_numpy(label).to(DEV), got_centres)
    assert status == 0 and count.tolist() == [n // 2 + 1, n // 2] and np.array_equal(got_count.cpu().numpy(), count)
    assert same_bits(got_sums.cpu().numpy(), sums) and same_bits(got_centres.cpu().numpy(), centres)


def test_update_keeps_an_empty_cluster_and_reports_a_bad_label():
    points = K.sphere(5000, 9)
    label = (np.arange(5000) % 3).astype(np.int32) * 2                  # clusters 0, 2 and 4 of 5: 1 and 3 stay empty
    label[[17, 4099]] = [5, -1]                                         # outside [0, 5): the status word, never memory
    previous = np.arange(15, dtype=np.float64).reshape(5, 3) + 0.5
    sums, count, centres, status = K.update_arrays(points, label, previous)
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    got_centres = torch.from_numpy(previous.copy()).to(DEV)
    got_sums, got_count = lib.kmeans_update(torch.from_numpy(points).to(DEV), torch.from_numpy(label).to(DEV), got_centres, info=info)
    assert status == 2 and int(info.cpu()) == 2 and int(count.sum()) == 4998 and count[1] == count[3] == 0
    assert np.array_equal(got_count.cpu().numpy(), count) and same_bits(got_sums.cpu().numpy(), sums) and same_bits(got_centres.cpu().numpy(), centres)
    assert same_bits(centres[[1, 3]], previous[[1, 3]])
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.kmeans_update(torch.from_numpy(points).to(DEV), torch.from_numpy(label).to(DEV), got_centres)


def test_seed_steps_and_a_bad_index():
    points = K.blobs(9001, 13)
    p = torch.from_numpy(points).to(DEV)
    mind2 = torch.empty(len(points), dtype=torch.float64, device=DEV)
    word = lambda x: torch.tensor([x], dtype=torch.int64, device=DEV)          # noqa: E731
    far = word(-7)
    ref, ref_far = None, 4100
    for t, newest in enumerate((4100, None, None)):
        newest = ref_far if newest is None else newest
        lib.kmeans_seed(p, word(newest), t == 0, mind2, far)
        ref, ref_far, _ = K.seed_arrays(points, newest, t == 0, ref)
        assert int(far.cpu()) == ref_far and same_bits(mind2.cpu().numpy(), ref)
    # an index outside [0, n): bit 2, mind2 untouched, -1 — nothing is read through it
    before = mind2.clone()
    for bad in (-1, len(points)):
        info = torch.zeros(1, dtype=torch.int64, device=DEV)
        lib.kmeans_seed(p, word(bad), False, mind2, far, info=info)
        assert int(info.cpu()) == 2 and int(far.cpu()) == -1 and torch.equal(mind2, before)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.kmeans_seed(p, word(len(points)), False, mind2, far)


def test_a_non_finite_point_raises():
    for bad in (float("nan"), float("inf")):
        points = K.blobs(5000, 3)
        points[4321, 1] = bad
        for init in ("farthest", "k-means++", points[:3].copy()):
            with pytest.raises(lib.VfnError, match="non-finite"):
                cluster.kmeans(points, 3, init=init, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
# dominant bases
# ---------------------------------------------------------------------------------------------------------------------------------
flat_cube = K.flat_cube


def test_the_flat_cube_has_the_six_axis_directions():
    v, f = flat_cube()
    d = meshops.dominant_bases((v, f), 6, device=DEV)
    assert isinstance(d, meshops.DominantBases) and d.n_vertices == 24 and d.n_faces == 12 and d.voxel_size is None and d.converged
    got = sorted(map(tuple, d.bases.cpu().numpy().tolist()))
    assert got == sorted(map(tuple, K.AXES.tolist())) and d.counts.cpu().tolist() == [4] * 6 and float(d.inertia.cpu()) == 0.0
    normals = meshops.vertex_normals((v, f), device=DEV)
    assert torch.equal(d.bases[d.labels], normals)
    three = meshops.dominant_bases((v, f), 3, device=DEV)
    counts = three.counts.cpu().tolist()
    assert sum(counts) == 24 and counts == sorted(counts, reverse=True) and torch.equal(torch.bincount(three.labels, minlength=3), three.counts)
    ref = K.dominant_bases(v, f, 3)
    assert same_bits(three.bases.cpu().numpy(), ref["bases"]) and np.array_equal(three.labels.cpu().numpy(), ref["labels"])
    assert np.array_equal(three.counts.cpu().numpy(), ref["counts"]) and three.n_iter == ref["n_iter"]
    unit = meshops.dominant_bases((v, f), 3, unit=True, device=DEV).bases.cpu().numpy()
    plain = three.bases.cpu().numpy()
    assert np.allclose((unit * unit).sum(axis=1), 1.0, rtol=0, atol=4e-16)
    assert np.allclose(unit * np.linalg.norm(plain, axis=1)[:, None], plain, rtol=0, atol=4e-16)
    # the second triangle of two squares wound the other way: with orient="first" the bases are those of the consistently wound cube
    g = f.copy()
    g[[1, 5]] = g[[1, 5]][:, [0, 2, 1]]
    assert meshops.dominant_bases((v, g), 6, device=DEV).counts.cpu().tolist() != [4] * 6          # (normals cancel along the shared diagonals)
    fixed = meshops.dominant_bases((v, g), 6, orient="first", device=DEV)
    assert sorted(map(tuple, fixed.bases.cpu().numpy().tolist())) == got and fixed.counts.cpu().tolist() == [4] * 6


def test_simplify_to_faces_equals_its_restatement():
    v, f, _ = S.cases()["cube_0.25"]
    for target in (400, 1):
        s, h = meshops.simplify_to_faces((v, f), target, device=DEV)
        ref, ref_h, tried = K.simplify_to_faces(v, f, target)
        print(f"target {target}: voxel edge {h!r}, {s.faces.shape[0]} faces; candidates {tried}")
        assert h == ref_h and len(tried) == 16 and (len(ref["faces"]) <= target or target == 1)
        assert same_bits(s.vertices.cpu().numpy(), ref["vertices"]) and np.array_equal(s.faces.cpu().numpy(), ref["faces"])
        assert np.array_equal(s.kept_faces.cpu().numpy(), ref["kept_faces"]) and np.array_equal(s.inverse.cpu().numpy(), ref["inverse"])


def test_get_dominant_bases_round_trips_through_a_ply_and_the_drop_in(tmp_path):
    v, f, _ = S.cases()["cube_0.25"]
    path = str(tmp_path / "room.ply")
    ply.write_ply(path, v, f, vertex_dtype="f8")
    rv, rf, _ = ply.read_ply(path)
    assert same_bits(rv, v) and np.array_equal(rf, f)
    ref = K.dominant_bases(v, f, 3, decimation=0.25)
    got = bases.get_dominant_bases(3, 0.25, path)
    assert isinstance(got, np.ndarray) and got.shape == (3, 3) and got.dtype == np.float64 and same_bits(got, ref["bases"])
    direct = meshops.dominant_bases((v, f), 3, decimation=0.25, device=DEV)
    assert direct.voxel_size == ref["voxel_size"] and direct.n_faces == ref["n_faces"] <= 768 and direct.n_vertices == ref["n_vertices"]
    assert np.array_equal(direct.counts.cpu().numpy(), ref["counts"]) and np.array_equal(direct.labels.cpu().numpy(), ref["labels"])
    by_voxel = meshops.dominant_bases((v, f), 3, voxel_size=0.25, device=DEV)
    assert same_bits(by_voxel.bases.cpu().numpy(), K.dominant_bases(v, f, 3, voxel_size=0.25)["bases"])
    # behind the reference's import path, only with the switch
    saved = {k: m for k, m in sys.modules.items() if k.split(".")[0] == "utils"}
    pkg, fake = types.ModuleType("utils"), types.ModuleType("utils.utils")
    pkg.__path__ = []
    reference = lambda num_bases, decimation, path_to_bases: "reference"          # noqa: E731
    fake.get_dominant_bases = reference
    try:
        sys.modules["utils"], sys.modules["utils.utils"] = pkg, fake
        dropin.install()
        assert fake.get_dominant_bases is reference
        dropin.install(patch_dominant_bases=True)
        assert same_bits(fake.get_dominant_bases(3, 0.25, path), ref["bases"]) and fake._reference_get_dominant_bases is reference
        dropin.install()
        assert fake.get_dominant_bases is reference
    finally:
        for key in [key for key in sys.modules if key.split(".")[0] == "utils"]:
            del sys.modules[key]
        sys.modules.update(saved)
        dropin.install()          # every switch as the import of the drop-in left it: the tests after this one train through it
