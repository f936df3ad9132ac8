"""K-means, host side: the C-ABI surface, the build recipe, the two CPU restatements of the contract (tests/kmeans_restatement.py) held
against each other bit for bit, the restatement held against scikit-learn's Lloyd iteration from the same seeds, what the contract
promises on small inputs, the argument checks that run before any device is asked for, and the drop-in's switch."""
import inspect
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import bases, cluster, dropin, geomargs, lib, meshops  # noqa: E402
import kmeans_restatement as K  # noqa: E402
import simplify_restatement as S  # noqa: E402
import tree_restatement as T  # noqa: E402

NEW_EXPORTS = ("vfn_kmeans_assign", "vfn_kmeans_update_workspace_bytes", "vfn_kmeans_update", "vfn_kmeans_seed_workspace_bytes", "vfn_kmeans_seed")

# Centres of the restatement against scikit-learn 1.7.2's KMeans(init=seeds, n_init=1, algorithm="lloyd", tol=0) on this project's
# development machine, over the 24 runs of ``test_restatement_agrees_with_scikit_learn`` (two data sets, n = 5 000 and 40 000, k = 3, 6, 16,
# farthest-point and D^2 seeds; 3 to 156 passes): every label and every n_iter_ equal, the largest centre difference 7.772e-16 (3.5 x 2^-52;
# scikit-learn centres the data on its mean first and adds in chunks per thread, hence not zero).  The bound is 8 x that, because the
# chunking reorders scikit-learn's sums from machine to machine.
SKLEARN_CENTRE_DIFF_MEASURED = 7.772e-16
SKLEARN_CENTRE_TOLERANCE = 8 * SKLEARN_CENTRE_DIFF_MEASURED


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_kmeans_assign"] == ("int", ["const double*", "int64_t", "const double*", "int32_t", "const int32_t*", "int32_t*", "double*",
                                                   "int64_t*", "int64_t*", "void*"])
    assert protos["vfn_kmeans_update"] == ("int", ["const double*", "int64_t", "const int32_t*", "int32_t", "double*", "int64_t*", "double*",
                                                   "int64_t*", "void*", "int64_t", "void*"])
    assert protos["vfn_kmeans_seed"] == ("int", ["const double*", "int64_t", "const int64_t*", "int32_t", "double*", "int64_t*", "int64_t*", "void*",
                                                 "int64_t", "void*"])
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    assert lib.kmeans_max_k() == lib.header_constant("VFN_KMEANS_MAX_K") == cluster.MAX_K == K.MAX_K == 64
    # the host-side checks of the exports answer without a device
    assign = lambda n, k: handle.vfn_kmeans_assign(None, n, None, k, None, None, None, None, None, None)          # noqa: E731
    assert assign(0, 3) != 0 and b"n 0 outside [1, 2^31)" in handle.vfn_last_error()
    assert assign(1 << 31, 3) != 0 and b"outside [1, 2^31)" in handle.vfn_last_error()
    assert assign(5, 0) != 0 and b"k 0 outside [1, 64]" in handle.vfn_last_error()
    assert assign(5, 65) != 0 and b"k 65 outside [1, 64]" in handle.vfn_last_error()
    assert assign(5, 3) != 0 and b"NULL" in handle.vfn_last_error()
    assert handle.vfn_kmeans_update(None, 5, None, 65, None, None, None, None, None, 0, None) != 0 and b"k 65 outside" in handle.vfn_last_error()
    assert handle.vfn_kmeans_update(None, 5, None, 3, None, None, None, None, None, 0, None) != 0 and b"NULL" in handle.vfn_last_error()
    assert handle.vfn_kmeans_seed(None, 0, None, 1, None, None, None, None, 0, None) != 0 and b"n 0 outside" in handle.vfn_last_error()
    assert handle.vfn_kmeans_seed(None, 5, None, 1, None, None, None, None, 0, None) != 0 and b"NULL" in handle.vfn_last_error()
    # the partials: a cluster's three sums and its count per tile of 4096 points; a (value, index) pair per tile
    assert handle.vfn_kmeans_update_workspace_bytes(4096, 3) == 3 * 4 * 8 and handle.vfn_kmeans_update_workspace_bytes(4097, 64) == 2 * 64 * 4 * 8
    assert handle.vfn_kmeans_update_workspace_bytes(0, 3) == -1 and handle.vfn_kmeans_update_workspace_bytes(5, 65) == -1
    assert handle.vfn_kmeans_seed_workspace_bytes(4097) == 2 * 16 and handle.vfn_kmeans_seed_workspace_bytes(1 << 31) == -1


def test_build_recipe_lists_the_unit_in_both_places():
    build = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "build.sh")).read()
    assert re.search(r'^UNITS=".*\bvfn_kmeans\b.*"', build, flags=re.M)
    assert re.search(r"\|vfn_simplify\|vfn_kmeans\).*-ffp-contract=off", build)
    unit = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "vfn_kmeans.hip")).read()
    # no floating-point atomics: the two atomic additions of the unit count changed labels, in integers
    adds = [line for line in unit.splitlines() if "atomicAdd(" in line and not line.lstrip().startswith("//")]
    assert len(adds) == 2 and all("(unsigned" in line and "double" not in line for line in adds)
    assert "atomicAdd_system" not in unit and "unsafeAtomicAdd" not in unit and "atomicMax" not in unit and "atomicMin" not in unit
    for phrase in ("tree_lane<", "tree_block<TREE_LANES>", "tree_block<TREE_TOP>", "tree_top_lane(", "vfn_pair_sqdist("):
        assert phrase in unit, phrase
    header = open(os.path.join(REPO, "include", "vfn.h")).read()
    for phrase in ("vfn_kmeans_assign", "vfn_kmeans_update", "vfn_kmeans_seed", "#define VFN_KMEANS_MAX_K 64", "a tie going to the LOWEST j",
                   'lane order "near", P = ceil(n / 4096) partials per cluster', "a cluster with count 0 KEEPS its centre",
                   "NOT verified: scikit-learn's own seeding"):
        assert phrase in header, phrase


def test_signatures_and_defaults():
    assert list(inspect.signature(cluster.kmeans).parameters) == ["points", "k", "init", "n_init", "max_iter", "seed", "device"]
    defaults = {k: p.default for k, p in inspect.signature(cluster.kmeans).parameters.items()}
    assert defaults == {"points": inspect.Parameter.empty, "k": inspect.Parameter.empty, "init": "farthest", "n_init": 1, "max_iter": 300,
                        "seed": None, "device": None}
    assert cluster.KMeans._fields == K.FIELDS and cluster.INITS == ("farthest", "k-means++")
    assert list(inspect.signature(meshops.dominant_bases).parameters) == ["mesh", "num_bases", "voxel_size", "decimation", "orient", "unit", "init",
                                                                         "n_init", "seed", "max_iter", "device"]
    defaults = {k: p.default for k, p in inspect.signature(meshops.dominant_bases).parameters.items()}
    assert defaults["voxel_size"] is None and defaults["decimation"] is None and defaults["orient"] is None and defaults["unit"] is False
    assert defaults["init"] == "farthest" and defaults["n_init"] == 1 and defaults["seed"] is None and defaults["max_iter"] == 300
    assert meshops.DominantBases._fields == ("bases", "counts", "labels", "inertia", "n_iter", "converged", "n_vertices", "n_faces", "voxel_size")
    to_faces = inspect.signature(meshops.simplify_to_faces).parameters
    assert list(to_faces)[:4] == ["mesh", "target_faces", "contraction", "steps"] and to_faces["contraction"].default == "quadric"
    assert to_faces["steps"].default == 16
    assert list(inspect.signature(bases.get_dominant_bases).parameters) == ["num_bases", "decimation", "path_to_bases"]
    install = inspect.signature(dropin.install).parameters
    assert install["patch_dominant_bases"].default is False
    assert list(install)[-2:] == ["patch_dominant_bases", "mesh_orient"]
    for doc in (cluster.kmeans.__doc__, cluster.__doc__):
        assert "NOT scikit-learn's greedy k-means++" in doc or "its greedy\nk-means++ and its random stream" in doc
    assert "AS SPECIFIED BY US" in meshops.simplify_to_faces.__doc__ and "AS SPECIFIED BY US" in meshops.dominant_bases.__doc__
    assert "dominant_bases" in meshops.__doc__ and "csrc/vfn_kmeans.hip" in meshops.__doc__


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 4095, 4096, 4097, 9000])
def test_the_tree_in_loops_is_the_tree_in_arrays(n):
    x = np.random.default_rng(n).normal(size=n) * 10.0 ** np.random.default_rng(n + 1).integers(-3, 4, n)
    assert same(K.tree_sum_loops(x.tolist()), T.two_level(x[:, None], "near")[0])


@pytest.mark.parametrize("n", [1, 4, 1023, 1024, 1025, 5000])
def test_the_scan_in_loops_is_the_scan_in_arrays(n):
    x = np.random.default_rng(n).uniform(0.0, 4.0, n)
    loops, arrays = K.cumsum_loops(x), K.cumsum_arrays(x)
    assert same(loops, arrays) and np.allclose(arrays, np.cumsum(x), rtol=1e-14, atol=0)


def test_the_scan_over_three_levels_stays_near_the_serial_sum():
    x = np.random.default_rng(5).uniform(0.0, 1.0, 1024 * 1024 + 7)
    assert np.allclose(K.cumsum_arrays(x), np.cumsum(x), rtol=1e-12, atol=0)


RESTATED = {
    "one_point": (np.array([[0.3, -0.2, 0.9]]), 1, {}),
    "blobs_farthest": (K.blobs(700, 1), 4, {}),
    "sphere_k7": (K.sphere(300, 2), 7, {}),
    "two_tiles": (K.blobs(4097, 3), 3, {"max_iter": 3}),
    "plusplus": (K.blobs(1500, 4), 5, {"init": "k-means++", "n_init": 2, "seed": 3}),
    "plusplus_duplicates": (np.repeat(np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]), 3, axis=0), 4, {"init": "k-means++", "n_init": 2, "seed": 0}),
    "given_centres": (K.sphere(200, 5), 3, {"init": K.sphere(3, 6), "max_iter": 2}),
}


@pytest.mark.parametrize("name", list(RESTATED))
def test_two_restatements_agree(name):
    points, k, args = RESTATED[name]
    one, two = K.kmeans(points, k, impl=K.LOOPS, **args), K.kmeans(points, k, impl=K.ARRAYS, **args)
    assert set(one) == set(two) == set(K.FIELDS)
    for key in one:
        assert same(one[key], two[key]), (name, key)
    # under both stops the labels are the assignment against the centres; converged, the centres are the update of the labels
    label, sqdist = K.assign_arrays(points, two["centres"])
    assert np.array_equal(label, two["labels"]) and same(sqdist, two["sqdist"]) and np.array_equal(np.bincount(label, minlength=k), two["counts"])
    if two["converged"]:
        assert same(K.update_arrays(points, label, two["centres"])[2], two["centres"])


def test_restated_properties():
    # a tie goes to the lowest cluster; a point midway keeps distance 1 to both
    label, sqdist = K.assign_arrays(np.array([[0.0, 0.0, 0.0]]), np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
    assert label.tolist() == [0] and sqdist.tolist() == [1.0] and same(K.assign_loops(np.zeros((1, 3)), np.eye(3))[0], np.zeros(1, np.int32))
    # an empty cluster keeps its centre's bits and shows in the counts; a bad label joins nothing
    previous = np.array([[1.0, 2.0, 3.0], [-0.0, 5e-324, np.pi]])
    for update in (K.update_loops, K.update_arrays):
        sums, count, centres, status = update(np.array([[2.0, 4.0, 6.0], [4.0, 4.0, 0.0], [9.0, 9.0, 9.0]]), np.array([0, 0, 2]), previous)
        assert status == 2 and count.tolist() == [2, 0] and same(centres, np.array([[3.0, 4.0, 3.0], previous[1]])) and same(sums[1], np.zeros(3))
    # seeding: the maximum's ties go to the lowest index, a bad index reads nothing
    points = np.array([[0.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0], [1.0, 0, 0]])
    for seed in (K.seed_loops, K.seed_arrays):
        mind2, far, status = seed(points, 0, True, None)
        assert mind2.tolist() == [0.0, 1.0, 1.0, 1.0] and far == 1 and status == 0
        mind2, far, status = seed(points, 1, False, mind2)
        assert mind2.tolist() == [0.0, 0.0, 1.0, 0.0] and far == 2
        assert seed(points, 4, False, mind2)[1:] == (-1, 2) and seed(points, -1, False, mind2)[1:] == (-1, 2)
    assert K.seeds_farthest(points, 3) == [2, 1, 0] and K.seeds_farthest(points, 3, K.LOOPS) == [2, 1, 0]          # the mean is (0.25, 0, 0)
    # D^2 sampling never draws a point that is a seed already while another is left, and falls back to the uniform draw when none is
    two = np.repeat(np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]), 3, axis=0)
    for u in np.random.default_rng(1).random((20, 3)):
        index = K.seeds_d2(two, 3, u)
        assert (index[0] < 3) != (index[1] < 3) and index[2] == K.first_index(u[2], 6)
    assert K.first_index(0.999999999999, 5) == 4 and K.first_index(0.0, 5) == 0 and cluster.first_index(0.37, 1000) == K.first_index(0.37, 1000) == 370
    # the flat cube: six separate squares, so every vertex normal is an axis direction and six bases are exactly those
    v, f = K.flat_cube()
    d = K.dominant_bases(v, f, 6)
    assert sorted(map(tuple, d["bases"].tolist())) == sorted(map(tuple, K.AXES.tolist())) and d["counts"].tolist() == [4] * 6 and d["inertia"] == 0.0
    d = K.dominant_bases(v, f, 3)
    assert int(d["counts"].sum()) == 24 == d["n_vertices"] and d["counts"].tolist() == sorted(d["counts"].tolist(), reverse=True)
    # the bisection: 16 candidates, geometric, the result the evaluated candidate with the most faces that fit
    v, f, _ = S.cases()["cube_0.25"]
    s, h, tried = K.simplify_to_faces(v, f, 400)
    fits = [(count, -i) for i, (_, count) in enumerate(tried) if count <= 400]
    assert len(tried) == 16 and tried[0][0] == 2.0 ** -10 and len(s["faces"]) == max(fits)[0] and h == tried[-max(fits)[1]][0]
    assert all(lo < hi for lo, hi in zip(sorted(e for e, _ in tried), sorted(e for e, _ in tried)[1:]))


# ---------------------------------------------------------------------------------------------------------------------------------
# against scikit-learn
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["blobs", "sphere"])
@pytest.mark.parametrize("n", [5000, 40000])
@pytest.mark.parametrize("k", [3, 6, 16])
def test_restatement_agrees_with_scikit_learn(data, n, k):
    sk = pytest.importorskip("sklearn.cluster")
    x = K.blobs(n, 11) if data == "blobs" else K.sphere(n, 12)
    for seeding in ("farthest", "k-means++"):
        seeds = x[K.seeds_farthest(x, k)] if seeding == "farthest" else x[K.seeds_d2(x, k, np.random.default_rng(5).random(k))]
        ref = K.kmeans(x, k, init=seeds, max_iter=1000)
        fit = sk.KMeans(n_clusters=k, init=seeds, n_init=1, algorithm="lloyd", tol=0, max_iter=1000).fit(x)
        diff = float(np.abs(fit.cluster_centers_ - ref["centres"]).max())
        print(f"{data} n {n} k {k} {seeding}: passes {ref['n_iter']}, scikit-learn n_iter_ {fit.n_iter_}, largest centre difference {diff:.3e}")
        assert ref["converged"] and np.array_equal(fit.labels_, ref["labels"]) and fit.n_iter_ == ref["n_iter"]
        assert diff <= SKLEARN_CENTRE_TOLERANCE


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals before a device is asked for
# ---------------------------------------------------------------------------------------------------------------------------------
PTS = np.array([[0.0, 0, 1], [1.0, 0, 0], [0, 1.0, 0], [0.5, 0.5, 0]])
TRI = (np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]]))


@pytest.mark.parametrize("call", [
    lambda: cluster.kmeans(PTS, 0),
    lambda: cluster.kmeans(PTS, 65),
    lambda: cluster.kmeans(PTS, 2.0),
    lambda: cluster.kmeans(PTS, True),
    lambda: cluster.kmeans(PTS[:, :2], 2),
    lambda: cluster.kmeans(PTS[:0], 1),
    lambda: cluster.kmeans(PTS.astype(np.int64), 2),
    lambda: cluster.kmeans(PTS, 2, init="random"),
    lambda: cluster.kmeans(PTS, 2, init=np.zeros((3, 3))),
    lambda: cluster.kmeans(PTS, 2, init=np.array([[0.0, 0, 1], [np.nan, 0, 0]])),
    lambda: cluster.kmeans(PTS, 2, init=np.zeros((2, 3), dtype=np.int64)),
    lambda: cluster.kmeans(PTS, 2, n_init=0),
    lambda: cluster.kmeans(PTS, 2, n_init=2),
    lambda: cluster.kmeans(PTS, 2, init=PTS[:2], n_init=2),
    lambda: cluster.kmeans(PTS, 2, max_iter=0),
    lambda: cluster.kmeans(PTS, 2, max_iter=2.5),
    lambda: cluster.kmeans(PTS, 2, init="k-means++", seed=-1),
    lambda: cluster.kmeans(PTS, 2, init="k-means++", seed=1.5),
    lambda: meshops.dominant_bases(TRI, 0),
    lambda: meshops.dominant_bases(TRI, 2, voxel_size=0.0),
    lambda: meshops.dominant_bases(TRI, 2, voxel_size=0.1, decimation=0.5),
    lambda: meshops.dominant_bases(TRI, 2, decimation=0.0),
    lambda: meshops.dominant_bases(TRI, 2, decimation=1.5),
    lambda: meshops.dominant_bases(TRI, 2, decimation="0.5"),
    lambda: meshops.dominant_bases(TRI, 2, orient="viewpoints"),
    lambda: meshops.dominant_bases(TRI, 2, unit=1),
    lambda: meshops.dominant_bases(TRI, 2, init="random"),
    lambda: meshops.dominant_bases((TRI[0], TRI[1][:0]), 2),
    lambda: meshops.dominant_bases((TRI[0], np.array([[0, 1, 3]])), 2),
    lambda: meshops.simplify_to_faces(TRI, 0),
    lambda: meshops.simplify_to_faces(TRI, 4, contraction="median"),
    lambda: meshops.simplify_to_faces(TRI, 4, steps=0),
    lambda: meshops.simplify_to_faces((TRI[0], TRI[1][:0]), 4),
])
def test_bad_arguments_raise_before_any_device_call(call, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(geomargs, "device", no_device)
    monkeypatch.setattr(cluster, "_device", no_device)
    with pytest.raises(ValueError):
        call()


def test_wrong_container_types_raise_type_error():
    with pytest.raises(TypeError):
        cluster.kmeans([[0.0, 0.0, 1.0]], 1)
    with pytest.raises(TypeError):
        meshops.dominant_bases("mesh.ply", 3)


def test_binding_refuses_shapes_before_the_device():
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)          # noqa: E731
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)            # noqa: E731
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64)            # noqa: E731
    with pytest.raises(lib.VfnError, match=r"points must be \[n,3\] with n >= 1"):
        lib.kmeans_assign(f64(0, 3), f64(2, 3), None, i32(0), f64(0), i64(1))
    with pytest.raises(lib.VfnError, match=r"centres must be \[k,3\] with 1 <= k <= 64"):
        lib.kmeans_assign(f64(5, 3), f64(65, 3), None, i32(5), f64(5), i64(1))
    with pytest.raises(lib.VfnError, match="the points' 5 rows"):
        lib.kmeans_assign(f64(5, 3), f64(2, 3), i32(4), i32(5), f64(5), i64(1))
    with pytest.raises(lib.VfnError, match=r"centres must be \[k,3\]"):
        lib.kmeans_update(f64(5, 3), i32(5), f64(0, 3))
    with pytest.raises(lib.VfnError, match="label must have the points' 5 rows"):
        lib.kmeans_update(f64(5, 3), i32(6), f64(2, 3))
    with pytest.raises(lib.VfnError, match="one of them may be None"):
        lib.kmeans_seed(f64(5, 3), None, True, f64(5), None)
    with pytest.raises(lib.VfnError, match="mind2 must have the points' 5 rows"):
        lib.kmeans_seed(f64(5, 3), i64(1), True, f64(4), i64(1))
    # host tensors never reach the library: there is no CPU path
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.kmeans_assign(f64(5, 3), f64(2, 3), None, i32(5), f64(5), i64(1), info=i64(1))
    lib.kmeans_check(0)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.kmeans_check(2)
    with pytest.raises(lib.VfnError, match="non-finite"):
        lib.kmeans_check(3)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is visible: the call would run")
def test_no_cpu_fallback():
    with pytest.raises(lib.VfnError, match="no GPU"):
        cluster.kmeans(PTS, 2)
    with pytest.raises(lib.VfnError, match="no GPU"):
        meshops.dominant_bases(TRI, 1)
    with pytest.raises(lib.VfnError, match="no GPU"):
        meshops.simplify_to_faces(TRI, 1)
    with pytest.raises(lib.VfnError, match="no CPU fallback"):
        cluster.kmeans(PTS, 2, device="cpu")


# ---------------------------------------------------------------------------------------------------------------------------------
# the drop-in, the device stood in for
# ---------------------------------------------------------------------------------------------------------------------------------
def test_install_patches_get_dominant_bases_only_with_the_switch(monkeypatch, tmp_path):
    from vf_nerf_amd import ply
    saved = {k: m for k, m in sys.modules.items() if k.split(".")[0] == "utils"}
    pkg, fake = types.ModuleType("utils"), types.ModuleType("utils.utils")
    pkg.__path__ = []
    reference = lambda num_bases, decimation, path_to_bases: "reference"          # noqa: E731
    fake.get_dominant_bases = reference
    asked = []

    def dominant_bases(mesh, num_bases, **kw):
        asked.append((tuple(mesh[0].shape), tuple(mesh[1].shape), num_bases, kw))
        return types.SimpleNamespace(bases=torch.arange(3.0 * num_bases, dtype=torch.float64).reshape(num_bases, 3))

    monkeypatch.setattr(meshops, "dominant_bases", dominant_bases)
    path = str(tmp_path / "mesh.ply")
    ply.write_ply(path, *TRI)
    try:
        sys.modules["utils"], sys.modules["utils.utils"] = pkg, fake
        dropin.install()
        assert fake.get_dominant_bases is reference and not hasattr(fake, "_reference_get_dominant_bases")          # off by default
        dropin.install(patch_dominant_bases=True)
        assert fake.get_dominant_bases is bases.get_dominant_bases and fake._reference_get_dominant_bases is reference
        dropin.install(patch_dominant_bases=True)                                                       # twice: the reference's is kept
        assert fake._reference_get_dominant_bases is reference
        out = fake.get_dominant_bases(2, 0.5, path)
        assert isinstance(out, np.ndarray) and out.dtype == np.float64 and np.array_equal(out, np.arange(6.0).reshape(2, 3))
        assert asked == [((3, 3), (1, 3), 2, {"decimation": 0.5})]
        dropin.install()
        assert fake.get_dominant_bases is reference
    finally:
        dropin.uninstall_clip_grad_norm()
        for key in [key for key in sys.modules if key.split(".")[0] == "utils"]:
            del sys.modules[key]
        sys.modules.update(saved)
