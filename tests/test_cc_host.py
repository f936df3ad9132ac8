"""Connected components, host side: the C-ABI surface, the build recipe, the two CPU restatements of the partition
(tests/cc_restatement.py) held against each other — and against scipy where it imports — on every shape, the union-find of
csrc/vfn_forest_core.h run on 16 host threads by the stand-alone program tests/c_abi/forest_core_host.cpp (under the sanitizers where
their runtimes exist), the argument checks that run before any device is asked for, and the unchanged call path of ``score_mesh`` / ``metrics_3d`` without the culling keywords."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import dropin, evaluator, lib, meshops, metrics3d, refuse  # noqa: E402
import cc_restatement as CC  # noqa: E402

NEW_EXPORTS = ("vfn_cc_union_runs", "vfn_cc_flatten", "vfn_cc_segment_sums")
SHAPES = CC.shapes()
CASES = [(name, c) for name in SHAPES for c in CC.CONNECTIVITIES]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_cc_union_runs"] == ("int", ["const int64_t*", "const int64_t*", "int64_t", "int32_t*", "int64_t", "int64_t*", "void*"])
    assert protos["vfn_cc_flatten"] == ("int", ["const int32_t*", "int64_t", "int64_t*", "int64_t*", "void*"])
    assert protos["vfn_cc_segment_sums"] == ("int", ["const double*", "int64_t", "const int64_t*", "int64_t", "double*", "int64_t*", "void*"])
    assert lib.header_abi_version() == 5
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    for name in NEW_EXPORTS:
        assert getattr(handle, name).argtypes is not None
    # the host-side checks of the exports answer without a device
    assert handle.vfn_cc_union_runs(None, None, 5, None, 0, None, None) != 0 and b"n_nodes 0 outside [1, 2^31)" in handle.vfn_last_error()
    assert handle.vfn_cc_union_runs(None, None, 5, None, 1 << 31, None, None) != 0 and b"n_nodes" in handle.vfn_last_error()
    assert handle.vfn_cc_union_runs(None, None, 0, None, 4, None, None) != 0 and b"n_items 0 outside" in handle.vfn_last_error()
    assert handle.vfn_cc_union_runs(None, None, 3 << 31, None, 4, None, None) != 0 and b"n_items" in handle.vfn_last_error()
    assert handle.vfn_cc_union_runs(None, None, 5, None, 4, None, None) != 0 and b"NULL" in handle.vfn_last_error()
    assert handle.vfn_cc_flatten(None, 0, None, None, None) != 0 and b"n_nodes 0 outside" in handle.vfn_last_error()
    assert handle.vfn_cc_flatten(None, 4, None, None, None) != 0 and b"NULL" in handle.vfn_last_error()
    assert handle.vfn_cc_segment_sums(None, 0, None, 1, None, None, None) != 0 and b"n 0 outside" in handle.vfn_last_error()
    assert handle.vfn_cc_segment_sums(None, 5, None, 6, None, None, None) != 0 and b"n_segments 6 outside [1, n = 5]" in handle.vfn_last_error()
    assert handle.vfn_cc_segment_sums(None, 5, None, 0, None, None, None) != 0 and b"n_segments" in handle.vfn_last_error()
    assert handle.vfn_cc_segment_sums(None, 5, None, 2, None, None, None) != 0 and b"NULL" in handle.vfn_last_error()


def test_build_recipe_lists_the_unit_in_both_places():
    build = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "build.sh")).read()
    assert re.search(r'^UNITS=".*\bvfn_cc\b.*"', build, flags=re.M)
    assert re.search(r"\|vfn_cc[|)].*-ffp-contract=off", build)
    csrc = os.path.join(REPO, "vf_nerf_amd", "csrc")
    for name in ("vfn_cc.hip", "vfn_forest_core.h", "vfn_geom.h"):
        assert os.path.exists(os.path.join(csrc, name))
    # the forest is re-read through the atomic load only (the shared header's, which the core includes), and the device and the host
    # program compile ONE text of the loops
    unit, core, geom = (open(os.path.join(csrc, name)).read() for name in ("vfn_cc.hip", "vfn_forest_core.h", "vfn_geom.h"))
    assert "__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)" in geom and "__hip_atomic_load" not in unit + core
    assert '#include "vfn_forest_core.h"' in unit and '#include "vfn_geom.h"' in core and "DeviceMem" in unit
    assert "vfn_forest_core.h" in open(os.path.join(REPO, "tests", "c_abi", "forest_core_host.cpp")).read()


def test_signatures_and_defaults():
    assert list(inspect.signature(meshops.connected_components).parameters) == ["mesh", "connectivity", "areas", "device"]
    assert list(inspect.signature(meshops.filter_components).parameters) == ["mesh", "min_faces", "min_area", "keep_largest", "by",
                                                                            "connectivity", "device"]
    assert meshops.Components._fields == ("face_label", "vertex_label", "n_components", "face_count", "area", "first_face")
    defaults = {k: p.default for k, p in inspect.signature(meshops.filter_components).parameters.items()}
    assert defaults == {"mesh": inspect.Parameter.empty, "min_faces": None, "min_area": None, "keep_largest": None, "by": "faces",
                        "connectivity": "edge", "device": None}
    for fn in (metrics3d.score_mesh, refuse.metrics_3d):
        for name in ("min_component_faces", "keep_largest"):
            assert inspect.signature(fn).parameters[name].default is None, (fn.__name__, name)
    assert evaluator.TSDF_MIN_COMPONENT_FACES is None
    assert inspect.signature(dropin.install).parameters["tsdf_min_component_faces"].default is None
    assert inspect.signature(meshops.remove_degenerate_faces).parameters["zero_area"].default is False
    doc = meshops.__doc__
    assert "connected_components" in doc and "AS REMEMBERED" in doc and "removing degenerate or duplicate faces" not in doc


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,connectivity", CASES)
def test_two_restatements_agree(name, connectivity):
    v, f = SHAPES[name]
    a, b = CC.roots_serial(f, len(v), connectivity), CC.roots_propagate(f, len(v), connectivity)
    assert a.dtype == b.dtype == np.int64 and np.array_equal(a, b), name
    if len(f):
        assert (a <= np.arange(len(f))).all() and (a[a] == a).all()          # a root is its class's lowest face, and its own root
    one, two = CC.components(v, f, connectivity, CC.roots_serial), CC.components(v, f, connectivity, CC.roots_propagate)
    for key in ("face_label", "vertex_label", "face_count", "first_face"):
        assert np.array_equal(one[key], two[key]), (name, key)
    assert np.array_equal(bits(one["area"]), bits(two["area"])) and one["n_components"] == two["n_components"]
    assert one["face_count"].sum() == len(f) and np.array_equal(one["first_face"], np.unique(a))
    assert np.array_equal(CC.renumber_by_lowest(a), one["face_label"])


@pytest.mark.parametrize("name,connectivity", CASES)
def test_restatements_agree_with_scipy(name, connectivity):
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    v, f = SHAPES[name]
    m = len(f)
    if m == 0:
        return
    u, w = CC.pairs(f, len(v), connectivity)
    graph = sparse.coo_matrix((np.ones(len(u)), (u, w)), shape=(m, m)).tocsr()
    k, labels = csgraph.connected_components(graph, directed=False)
    want = CC.components(v, f, connectivity)
    assert k == want["n_components"] and np.array_equal(CC.renumber_by_lowest(labels), want["face_label"]), name


def test_restated_properties():
    counts = {name: tuple(CC.components(*SHAPES[name], c)["n_components"] for c in CC.CONNECTIVITIES) for name in SHAPES}
    assert counts["nothing"] == counts["no_faces"] == (0, 0) and counts["one_face"] == (1, 1) and counts["shared_edge"] == (1, 1)
    assert counts["bow_tie"] == (2, 1) and counts["disjoint"] == (2, 2) and counts["three_on_an_edge"] == (1, 1)
    assert counts["repeated_vertex"] == (2, 2) and counts["duplicate_face"] == (2, 2) and counts["unreferenced_vertex"] == (2, 2)
    assert all(counts[f"count_{k}"] == (k, k) for k in (255, 256, 257)) and counts["tetrahedra_300"] == (300, 300)
    assert all(counts[f"strip_4097_{o}"] == (1, 1) for o in ("ascending", "descending", "shuffled"))
    assert counts["floaters"] == (201, 201)
    # (0, 1, 1) holds the edge {0, 1} once — its pair (1, 1) is none — and so joins (0, 1, 2); (3, 3, 3) has no edge at all
    assert CC.components(*SHAPES["repeated_vertex"], "edge")["face_label"].tolist() == [0, 0, 1]
    keys, nodes = CC.items(SHAPES["repeated_vertex"][1], 4, "edge")
    assert (keys == -1).sum() == 4 and (np.diff(keys) >= 0).all()
    # labels of vertices: the lowest among the faces, -1 where no face names the vertex
    bow = CC.components(*SHAPES["bow_tie"], "edge")
    assert bow["vertex_label"].tolist() == [0, 0, 0, 1, 1] and bow["first_face"].tolist() == [0, 1]
    assert CC.components(*SHAPES["unreferenced_vertex"], "edge")["vertex_label"].tolist() == [0, 0, 0, 0, -1, 1, 1, 1, -1]
    assert CC.components(*SHAPES["no_faces"], "edge")["vertex_label"].tolist() == [-1, -1, -1]
    # the order of the area rule: not the serial sum, not numpy's pairwise sum, and a lone -0.0 comes out +0.0
    x = np.random.default_rng(0).uniform(0, 1, 129)
    assert CC.wave_sum(x[:1]) == x[0] and CC.wave_sum(x[:2]) == x[0] + x[1]
    lanes = [x[t] + x[t + 64] if t + 64 < 129 else x[t] for t in range(64)]
    lanes[0] = lanes[0] + x[128]
    for o in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[t] + lanes[t + o] for t in range(o)]
    assert CC.wave_sum(x) == lanes[0] and abs(CC.wave_sum(x) - x.sum()) <= 129 * 2.0 ** -53 * x.sum()
    assert not np.signbit(CC.wave_sum(np.array([-0.0])))
    # a permutation of the face list moves labels, not the partition
    v, f, big = CC.floater_scene()
    perm = np.random.default_rng(9).permutation(len(f))
    a, b = CC.components(v, f, "edge"), CC.components(v, f[perm], "edge")
    assert np.array_equal(CC.renumber_by_lowest(a["face_label"][perm]), b["face_label"])
    assert sorted(a["face_count"].tolist()) == sorted(b["face_count"].tolist()) == sorted([20000] + 4 * list(range(1, 51)))
    # the filter: 51 faces keep the torus alone, in the faces' order, with its own vertices' bits
    fv, ff, kept, inverse, labels = CC.filter_components(v, f, min_faces=51)
    assert np.array_equal(kept, np.nonzero(big)[0]) and len(labels) == 1 and len(fv) == 10000
    assert np.array_equal(bits(fv), bits(v[:10000])) and np.array_equal(ff, f[big]) and (inverse[10000:] == -1).all()
    assert len(CC.filter_components(v, f, keep_largest=1)[2]) == 20000 and len(CC.filter_components(v, f, keep_largest=5)[2]) == 20200
    assert len(CC.filter_components(v, f, keep_largest=3, by="area")[4]) == 3
    assert len(CC.filter_components(v, f)[2]) == len(f)
    none = CC.filter_components(*SHAPES["unreferenced_vertex"])
    assert len(none[0]) == 7 and none[3].tolist() == [0, 1, 2, 3, -1, 4, 5, 6, -1]
    # ties in keep_largest go to the lower label
    assert CC.filter_components(*SHAPES["disjoint"], keep_largest=1)[2].tolist() == [0]
    # the two cleaning functions
    assert CC.remove_degenerate_faces(*SHAPES["repeated_vertex"])[1].tolist() == [1]
    flat = (np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2], [0, 1, 3]]))
    assert CC.remove_degenerate_faces(*flat)[1].tolist() == [0, 1] and CC.remove_degenerate_faces(*flat, zero_area=True)[1].tolist() == [1]
    assert CC.remove_duplicate_faces(SHAPES["duplicate_face"][1])[1].tolist() == [0, 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the loops of csrc/vfn_forest_core.h (the plain forest) on 16 host threads, before any card sees them
# ---------------------------------------------------------------------------------------------------------------------------------
def _build_host_program(tmp_path, sanitizer):
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    source = os.path.join(REPO, "tests", "c_abi", "forest_core_host.cpp")
    exe = str(tmp_path / "forest_core_host")
    base = [compiler, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", source, "-o", exe]
    build = subprocess.run(base + sanitizer, capture_output=True, text=True)
    if build.returncode != 0:          # a machine without the sanitizer's runtime: the plain program (an error in the text fails it too)
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


@pytest.mark.parametrize("sanitizer", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["-fsanitize=thread"]],
                         ids=["address_undefined", "thread"])
def test_union_find_core_on_sixteen_host_threads(tmp_path, sanitizer):
    exe = _build_host_program(tmp_path, sanitizer)
    text, want = [], []
    for name, connectivity in CASES:
        v, f = SHAPES[name]
        if len(f) == 0:
            continue
        keys, nodes = CC.items(f, len(v), connectivity)
        text.append(f"{len(f)} {len(keys)}\n" + "".join(f"{k} {n}\n" for k, n in zip(keys.tolist(), nodes.tolist())))
        want.append((name, connectivity, CC.roots_serial(f, len(v), connectivity)))
    # negative keys unite nothing; a node outside [0, n) is not followed (neither of the two pairs it stands in) and the status says so
    text.append("4 5\n-1 0\n-1 1\n7 2\n7 9\n7 3\n")
    want.append(("bad node", None, None))
    # (the program holds its four 16-thread runs of every case to its own serial run, and exits with 4 where one differs)
    run = subprocess.run([exe, "plain", "16"], input="".join(text) + "0 0\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    lines = run.stdout.strip().split("\n")
    assert len(lines) == len(want)
    for line, (name, connectivity, roots) in zip(lines, want):
        got = np.array(line.split(), dtype=np.int64)
        if roots is None:
            assert got.tolist() == [2, 0, 1, 2, 3], line
        else:
            assert got[0] == 0 and np.array_equal(got[1:], roots), (name, connectivity)


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals before a device is asked for
# ---------------------------------------------------------------------------------------------------------------------------------
TRI_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.array([[0, 1, 2]])
TRI = (TRI_V, TRI_F)


@pytest.mark.parametrize("call", [
    lambda: meshops.connected_components(TRI, connectivity="face"),
    lambda: meshops.connected_components(TRI, connectivity=None),
    lambda: meshops.connected_components(TRI, areas=1),
    lambda: meshops.connected_components((TRI_V, np.array([[0, 1, 3]]))),
    lambda: meshops.connected_components((TRI_V, np.array([[0, -1, 2]]))),
    lambda: meshops.connected_components((TRI_V, np.array([[0.0, 1.0, 2.0]]))),
    lambda: meshops.connected_components((TRI_V[:, :2], TRI_F)),
    lambda: meshops.filter_components(TRI, min_faces=-1),
    lambda: meshops.filter_components(TRI, min_faces=2.0),
    lambda: meshops.filter_components(TRI, min_faces=True),
    lambda: meshops.filter_components(TRI, min_area=-0.5),
    lambda: meshops.filter_components(TRI, min_area=float("nan")),
    lambda: meshops.filter_components(TRI, min_area="1"),
    lambda: meshops.filter_components(TRI, keep_largest=0),
    lambda: meshops.filter_components(TRI, keep_largest=1.5),
    lambda: meshops.filter_components(TRI, keep_largest=1, by="volume"),
    lambda: meshops.filter_components(TRI, connectivity="corner"),
    lambda: meshops.filter_components((TRI_V, np.array([[0, 1, 3]])), min_faces=1),
    lambda: meshops.remove_degenerate_faces(TRI, zero_area="yes"),
    lambda: meshops.remove_degenerate_faces((TRI_V, np.array([[0, 1, 3]]))),
    lambda: meshops.remove_duplicate_faces((TRI_V, np.array([[0, 1, 3]]))),
    lambda: meshops.clean(TRI, weld_digits=16),
    lambda: meshops.clean(TRI, degenerate=None),
    lambda: meshops.clean(TRI, duplicates=0),
    lambda: meshops.clean(TRI, min_faces=-2),
    lambda: meshops.clean(TRI, smallest=3),
    lambda: metrics3d.score_mesh(TRI, TRI, num_points=10, min_component_faces=-1),
    lambda: metrics3d.score_mesh(TRI, TRI, num_points=10, min_component_faces=2.5),
    lambda: metrics3d.score_mesh(TRI, TRI, num_points=10, keep_largest=0),
    lambda: metrics3d.score_mesh(TRI, TRI, num_points=10, keep_largest=True),
    lambda: refuse.metrics_3d(None, None, None, None, 4, 4, min_component_faces=-1),
    lambda: refuse.metrics_3d(None, None, None, None, 4, 4, keep_largest=0),
    lambda: dropin.install(tsdf_min_component_faces=-1),
    lambda: dropin.install(tsdf_min_component_faces=2.5),
])
def test_bad_arguments_raise_before_any_device_call(call, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(meshops.geomargs, "device", no_device)
    monkeypatch.setattr(metrics3d, "_device", no_device)
    monkeypatch.setattr(refuse, "reconstruction_meshes", no_device)
    with pytest.raises(ValueError):
        call()
    assert evaluator.TSDF_MIN_COMPONENT_FACES is None


def test_wrong_container_types_raise_type_error():
    with pytest.raises(TypeError):
        meshops.connected_components("mesh.ply")
    with pytest.raises(TypeError):
        meshops.filter_components(([[0.0, 0, 0]], TRI_F), min_faces=1)


def test_binding_refuses_shapes_before_the_device():
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64)          # noqa: E731
    with pytest.raises(lib.VfnError, match=r"keys and nodes must be \[k\]"):
        lib.cc_union_runs(i64(5), i64(4), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(lib.VfnError, match="at least 1"):
        lib.cc_union_runs(i64(0), i64(0), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(lib.VfnError, match="at least 1"):
        lib.cc_union_runs(i64(5), i64(5), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(lib.VfnError, match=r"parent must be \[n\]"):
        lib.cc_flatten(torch.zeros(0, dtype=torch.int32))
    with pytest.raises(lib.VfnError, match="entries"):
        lib.cc_segment_sums(torch.zeros(5, dtype=torch.float64), i64(7))
    with pytest.raises(lib.VfnError, match="entries"):
        lib.cc_segment_sums(torch.zeros(5, dtype=torch.float64), i64(1))
    with pytest.raises(lib.VfnError, match=r"\[S\+1\]"):
        lib.cc_segment_sums(torch.zeros(5, 1, dtype=torch.float64), i64(2))
    # host tensors never reach the library: there is no CPU path
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.cc_union_runs(i64(5), i64(5), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.cc_flatten(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.cc_segment_sums(torch.zeros(5, dtype=torch.float64), i64(2))
    lib.cc_check(0)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.cc_check(2)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is visible: the calls would run")
def test_no_cpu_fallback():
    for call in (lambda: meshops.connected_components(TRI), lambda: meshops.filter_components(TRI, min_faces=1),
                 lambda: meshops.remove_duplicate_faces(TRI), lambda: meshops.remove_degenerate_faces(TRI), lambda: meshops.clean(TRI),
                 lambda: metrics3d.score_mesh(TRI, TRI, num_points=10, min_component_faces=1)):
        with pytest.raises(lib.VfnError, match="no GPU"):
            call()


# ---------------------------------------------------------------------------------------------------------------------------------
# the call paths, the device stood in for
# ---------------------------------------------------------------------------------------------------------------------------------
def test_score_mesh_without_the_keywords_takes_todays_path(monkeypatch):
    calls = []

    def sample(v, f, count, generator=None, uniforms=None, device=None):
        calls.append(("sample", tuple(v.shape), tuple(f.shape), count, generator, uniforms))
        return torch.full((count, 3), float(len(calls))), None

    def both(pred, ref, threshold, device=None, **kw):
        calls.append(("both", float(pred[0, 0]), float(ref[0, 0]), threshold, tuple(pred.shape), kw))
        return np.array([[4.0, 0.0, 2.0, 1.0, 1.0, 4.0, 3.0], [3.0, 0.5, 1.0, 1.0, 1.0, 3.0, 2.0]])

    def no_cull(*a, **k):
        raise AssertionError("the culling was reached")

    monkeypatch.setattr(metrics3d, "sample_surface", sample)
    monkeypatch.setattr(metrics3d, "_both_directions", both)
    monkeypatch.setattr(metrics3d, "_cull_components", no_cull)
    monkeypatch.setattr(meshops, "_components", no_cull)
    plain = metrics3d.score_mesh(TRI, TRI, num_points=10, distance_thresh=0.25, generator="g")
    first = list(calls)
    del calls[:]
    explicit = metrics3d.score_mesh(TRI, TRI, num_points=10, distance_thresh=0.25, generator="g", min_component_faces=None, keep_largest=None)
    assert plain == explicit and calls == first and "components" not in plain
    assert first == [("sample", (3, 3), (1, 3), 10, "g", None), ("sample", (3, 3), (1, 3), 10, "g", None),
                     ("both", 1.0, 2.0, 0.25, (10, 3), {})]

    # with a value: pred_mesh alone goes through the culling, before the sampling
    def cull(v, f, min_faces, keep_largest, device=None):
        calls.append(("cull", tuple(v.shape), min_faces, keep_largest))
        return torch.zeros(7, 3), torch.zeros(5, 3, dtype=torch.int64), {"found": 3}

    monkeypatch.setattr(metrics3d, "_cull_components", cull)
    del calls[:]
    out = metrics3d.score_mesh(TRI, TRI, num_points=10, distance_thresh=0.25, generator="g", min_component_faces=51)
    assert calls == [("cull", (3, 3), 51, None), ("sample", (7, 3), (5, 3), 10, "g", None), ("sample", (3, 3), (1, 3), 10, "g", None),
                     ("both", 2.0, 3.0, 0.25, (10, 3), {})]
    assert out["components"] == {"found": 3} and {k: v for k, v in out.items() if k != "components"} == plain
    del calls[:]
    metrics3d.score_mesh(TRI, TRI, num_points=10, keep_largest=2)
    assert calls[0] == ("cull", (3, 3), None, 2)


def test_metrics_3d_passes_the_keywords_through(monkeypatch):
    got = []
    monkeypatch.setattr(refuse, "reconstruction_meshes", lambda *a, **k: {name: (torch.zeros(1, 3), name) for name in refuse.MESH_NAMES})
    monkeypatch.setattr(metrics3d, "score_mesh", lambda mesh, gt, **k: got.append(k) or {"mesh": mesh[1]})
    refuse.metrics_3d("tsdf", "gt", None, None, 4, 4, num_points=7)
    assert len(got) == 4 and all("min_component_faces" not in k and "keep_largest" not in k for k in got)
    del got[:]
    refuse.metrics_3d("tsdf", "gt", None, None, 4, 4, num_points=7, min_component_faces=51)
    assert len(got) == 4 and all(k["min_component_faces"] == 51 and k["keep_largest"] is None and k["num_points"] == 7 for k in got)
    del got[:]
    refuse.metrics_3d("tsdf", "gt", None, None, 4, 4, keep_largest=1, voxel_size=0.025)
    assert len(got) == 4 and all(k["keep_largest"] == 1 and k["voxel_size"] == 0.025 for k in got)


def test_evaluator_filters_only_with_the_switch(tmp_path, monkeypatch):
    """evaluator.tsdf_mesh with the reference's modules stood in for and the device calls stubbed: with the switch set the file holds the
    filtered mesh, and colours and normals of the vertices that stay; with it clear the filter is not reached."""
    import types
    from PIL import Image
    from vf_nerf_amd import ply, tsdf
    os.makedirs(tmp_path / "rendered_images")
    np.save(tmp_path / "rendered_images" / "depth-0.npy", np.ones((4, 5, 1)))
    Image.fromarray(np.zeros((4, 5, 3), dtype=np.uint8)).save(tmp_path / "rendered_images" / "image-0.png")

    class Dataset:
        def __init__(self, config):
            self.intrinsics, self.poses = torch.eye(4), torch.eye(4)[None]

    v, f = CC.shapes()["disjoint"]
    colours = np.round(np.linspace(0, 1, 18).reshape(6, 3) * 255) / 255
    nrm = np.linspace(-1, 1, 18).reshape(6, 3)
    asked = []

    def keep_second(mesh, min_faces=None, **kw):
        asked.append(min_faces)
        return (mesh[0][3:], torch.tensor([[0, 1, 2]]), torch.tensor([1]), torch.tensor([-1, -1, -1, 0, 1, 2]))

    monkeypatch.setattr(tsdf, "fuse_rgbd_maps", lambda *a, **k: (torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(colours)))
    monkeypatch.setattr(meshops, "vertex_normals", lambda mesh, device=None: torch.from_numpy(nrm))
    monkeypatch.setattr(meshops, "filter_components", keep_second)
    names = ("datasets", "datasets.normal_datasets")
    saved = {key: sys.modules[key] for key in names if key in sys.modules}
    fakes = {key: types.ModuleType(key) for key in names}
    fakes["datasets"].__path__ = []
    fakes["datasets.normal_datasets"].dataset_dict = {"fake": Dataset}
    files = {}
    try:
        sys.modules.update(fakes)
        for switch, with_normals in ((None, False), (7, False), (7, True)):
            monkeypatch.setattr(evaluator, "TSDF_MIN_COMPONENT_FACES", switch)
            monkeypatch.setattr(evaluator, "TSDF_VERTEX_NORMALS", with_normals)
            evaluator.tsdf_mesh(str(tmp_path), types.SimpleNamespace(dataset_name="fake"))
            files[switch, with_normals] = ply.read_ply(str(tmp_path / "tsdf-mesh" / "tsdf.ply"), normals=True)
    finally:
        for key in names:
            del sys.modules[key]
        sys.modules.update(saved)
    assert asked == [7, 7]
    whole, culled, culled_n = files[None, False], files[7, False], files[7, True]
    assert len(whole[0]) == 6 and len(whole[1]) == 2 and whole[3] is None
    assert np.array_equal(culled[0], whole[0][3:]) and np.array_equal(culled[1], [[0, 1, 2]]) and np.array_equal(culled[2], whole[2][3:])
    assert culled[3] is None and np.array_equal(culled_n[3], nrm[3:].astype(np.float32).astype(np.float64))
    assert all(np.array_equal(a, b) for a, b in zip(culled[:3], culled_n[:3]))


def test_install_sets_the_switch(monkeypatch):
    monkeypatch.setattr(evaluator, "TSDF_MIN_COMPONENT_FACES", None)
    sig = inspect.signature(dropin.install)
    assert sig.parameters["tsdf_min_component_faces"].default is None
    source = inspect.getsource(dropin.install)
    assert "evaluator.TSDF_MIN_COMPONENT_FACES = tsdf_min_component_faces" in source
    assert "TSDF_MIN_COMPONENT_FACES is not None" in inspect.getsource(evaluator.tsdf_mesh)
