"""Orientation, host side: the C-ABI surface, the build recipe, the two CPU restatements of the parities (tests/orient_restatement.py)
held against each other on every shape and every reference, the properties an oriented mesh must have, the parity union-find of
csrc/vfn_forest_core.h run on 16 host threads by the stand-alone program tests/c_abi/forest_core_host.cpp (under the sanitizers where
their runtimes exist), the argument checks that run before any device is asked for, and the unchanged call path of the drop-in's
``contrastive_marching_cubes`` without the switch."""
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

from vf_nerf_amd import dropin, lib, mesh, meshops  # noqa: E402
import orient_restatement as R  # noqa: E402

NEW_EXPORTS = ("vfn_orient_union_runs", "vfn_orient_flatten", "vfn_orient_votes")
SHAPES = R.shapes()
CASES = [(name, reference) for name in SHAPES for reference in meshops.REFERENCES]          # the package's own list: every case is one it offers
_done = {}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def restated(name, reference, parities=R.parity_serial):
    """A shape's restatement, computed once and shared."""
    key = (name, reference, parities.__name__)
    if key not in _done:
        _done[key] = R.orientation(*SHAPES[name], reference, R.VIEWPOINTS if reference == "viewpoints" else None, parities)
    return _done[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_orient_union_runs"] == ("int", ["const int64_t*", "const int64_t*", "const uint8_t*", "int64_t", "int32_t*", "int64_t",
                                                       "int64_t*", "void*"])
    assert protos["vfn_orient_flatten"] == ("int", ["const int32_t*", "int64_t", "int64_t*", "uint8_t*", "int64_t*", "void*"])
    assert protos["vfn_orient_votes"] == ("int", ["const double*", "int64_t", "const int64_t*", "int64_t", "const uint8_t*", "int32_t",
                                                  "const double*", "int64_t", "double*", "int64_t*", "void*"])
    assert lib.header_abi_version() == 5
    assert (lib.header_constant("VFN_ORIENT_VOLUME"), lib.header_constant("VFN_ORIENT_VIEWPOINTS")) == (lib.ORIENT_VOLUME, lib.ORIENT_VIEWPOINTS)
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    for name in NEW_EXPORTS:
        assert getattr(handle, name).argtypes is not None
    # the host-side checks of the exports answer without a device
    union, flatten, votes, err = handle.vfn_orient_union_runs, handle.vfn_orient_flatten, handle.vfn_orient_votes, handle.vfn_last_error
    assert union(None, None, None, 5, None, 0, None, None) != 0 and b"n_nodes 0 outside [1, 2^30)" in err()
    assert union(None, None, None, 5, None, 1 << 30, None, None) != 0 and b"n_nodes 1073741824 outside [1, 2^30)" in err()
    assert union(None, None, None, 0, None, 4, None, None) != 0 and b"n_items 0 outside" in err()
    assert union(None, None, None, 3 << 30, None, 4, None, None) != 0 and b"n_items" in err()
    assert union(None, None, None, 5, None, 4, None, None) != 0 and b"NULL" in err()
    assert flatten(None, 0, None, None, None, None) != 0 and b"n_nodes 0 outside" in err()
    assert flatten(None, 1 << 30, None, None, None, None) != 0 and b"n_nodes" in err()
    assert flatten(None, 4, None, None, None, None) != 0 and b"NULL" in err()
    assert votes(None, -1, None, 4, None, 0, None, 0, None, None, None) != 0 and b"n -1 outside" in err()
    assert votes(None, 3, None, 0, None, 0, None, 0, None, None, None) != 0 and b"m 0 outside" in err()
    assert votes(None, 3, None, 4, None, 2, None, 0, None, None, None) != 0 and b"mode 2" in err()
    assert votes(None, 3, None, 4, None, 1, None, 0, None, None, None) != 0 and b"n_views 0 outside [1, 2^31)" in err()
    assert votes(None, 3, None, 4, None, 1, None, 2, None, None, None) != 0 and b"NULL viewpoints" in err()
    assert votes(None, 3, None, 4, None, 0, None, 2, None, None, None) != 0 and b"VFN_ORIENT_VOLUME" in err()
    assert votes(None, 3, None, 4, None, 0, None, 0, None, None, None) != 0 and b"NULL argument" in err()


def test_build_recipe_lists_the_unit_in_both_places():
    build = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "build.sh")).read()
    assert re.search(r'^UNITS=".*\bvfn_orient\b.*"', build, flags=re.M)
    assert re.search(r"\|vfn_orient[|)].*-ffp-contract=off", build)
    # the VFN_ONLY shortcut refuses objects older than the core: than every header beside the units, the core among them
    assert re.search(r'for src in "\$u\.hip" \*\.h \.\./\.\./include/vfn\.h; do\n +\[ "\$OBJDIR/\$u\.o" -nt "\$src" \] \|\| fresh=0\n', build)
    csrc = os.path.join(REPO, "vf_nerf_amd", "csrc")
    for name in ("vfn_orient.hip", "vfn_forest_core.h", "vfn_geom.h"):
        assert os.path.exists(os.path.join(csrc, name))
    # the forest is re-read through the atomic load only (the shared header's, which the core includes), and the device and the host
    # program compile ONE text of the loops
    unit, core, geom = (open(os.path.join(csrc, name)).read() for name in ("vfn_orient.hip", "vfn_forest_core.h", "vfn_geom.h"))
    assert "__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)" in geom and "__hip_atomic_load" not in unit + core
    assert '#include "vfn_forest_core.h"' in unit and '#include "vfn_geom.h"' in core and "DeviceMem" in unit
    assert "vfn_forest_core.h" in open(os.path.join(REPO, "tests", "c_abi", "forest_core_host.cpp")).read()


def test_signatures_and_defaults():
    assert list(inspect.signature(meshops.orientation).parameters) == ["mesh", "reference", "viewpoints", "device"]
    assert list(inspect.signature(meshops.orient).parameters) == ["mesh", "reference", "viewpoints", "device"]
    assert list(inspect.signature(meshops.inconsistent_edges).parameters) == ["mesh", "device"]
    assert inspect.signature(meshops.orientation).parameters["reference"].default == "first"
    assert meshops.Orientation._fields[:8] == ("flip", "face_label", "n_components", "first_face", "face_count", "orientable", "flipped_count",
                                               "inconsistent_edges")
    assert meshops.REFERENCES == R.REFERENCES and mesh.ORIENT_REFERENCES == ("first", "majority", "volume")
    params = list(inspect.signature(mesh.extract_mesh).parameters)
    assert params[-1] == "orient" and inspect.signature(mesh.extract_mesh).parameters["orient"].default is None
    assert list(inspect.signature(dropin.install).parameters)[-1] == "mesh_orient"
    assert inspect.signature(dropin.install).parameters["mesh_orient"].default is None
    assert mesh.ORIENT is None and mesh.Mesh._fields == ("vertices", "faces", "vertices_scaled")
    doc = meshops.__doc__
    assert "orienting a mesh" not in doc and "fix_normals" in doc and "orient_triangles" in doc
    assert "signed normal consistency" in doc and "filling\nholes" in doc and "simplification" in doc


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,reference", CASES)
def test_two_restatements_agree(name, reference):
    one, two = restated(name, reference, R.parity_serial), restated(name, reference, R.parity_colouring)
    for key in ("flip", "face_label", "first_face", "face_count", "orientable", "flipped_count", "faces"):
        assert one[key].dtype == two[key].dtype and np.array_equal(one[key], two[key]), (name, key)
    assert one["n_components"] == two["n_components"] and one["inconsistent_edges"] == two["inconsistent_edges"]
    if reference in ("volume", "viewpoints"):
        assert np.array_equal(bits(one["votes"]), bits(two["votes"])), name
    else:
        assert one["votes"] is None and two["votes"] is None
    m = len(SHAPES[name][1])
    assert one["face_count"].sum() == m and (one["first_face"] == np.unique(one["first_face"])).all()
    assert (one["first_face"][one["face_label"]] <= np.arange(m)).all()          # a root is its component's lowest face


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_two_parity_walks_agree_before_anything_is_zeroed(name):
    v, f = SHAPES[name]
    (ra, pa, ca), (rb, pb, cb) = R.parity_serial(f, len(v)), R.parity_colouring(f, len(v))
    assert np.array_equal(ra, rb)
    bad_a, bad_b = np.unique(ra[ca]), np.unique(rb[cb])
    assert np.array_equal(bad_a, bad_b)                                           # the same components are found contradictory
    ok = ~np.isin(ra, bad_a)
    assert np.array_equal(pa[ok], pb[ok]) and (pa[ra == np.arange(len(f))] == 0).all()


@pytest.mark.parametrize("name,reference", CASES)
def test_an_oriented_mesh_is_consistent_and_stays_so(name, reference):
    v, f = SHAPES[name]
    o = restated(name, reference)
    views = R.VIEWPOINTS if reference == "viewpoints" else None
    if R.ORIENTABLE(name):
        assert o["orientable"].all()
        assert R.count_inconsistent(o["faces"], len(v)) == 0
    again = R.orientation(v, o["faces"], reference, views)
    assert not again["flip"].any() and np.array_equal(again["faces"], o["faces"]), "orientation is not idempotent"
    assert np.array_equal(again["face_label"], o["face_label"]) and np.array_equal(again["orientable"], o["orientable"])
    assert np.array_equal(o["faces"][:, 0], f[:, 0]) and np.array_equal(np.sort(o["faces"], axis=1), np.sort(f, axis=1))
    if reference == "first":
        assert not o["flip"][o["first_face"]].any()                               # every root keeps its winding
    if reference == "majority":
        assert (2 * o["flipped_count"] <= o["face_count"]).all()
        tie = 2 * o["flipped_count"] == o["face_count"]
        assert not o["flip"][o["first_face"][tie]].any()                          # on a tie the root keeps its winding
    if reference in ("volume", "viewpoints"):
        assert (again["votes"][again["orientable"]] >= 0).all()
        # a component's sign is all that the reference decides: against "first" a component is flipped whole or not at all
        first = restated(name, "first")
        differs = o["flip"] ^ first["flip"]
        per = np.bincount(o["face_label"], weights=differs, minlength=o["n_components"]).astype(np.int64)
        assert ((per == 0) | (per == o["face_count"])).all()


def test_restated_properties():
    o = restated("moebius_4097", "first")
    v, f = SHAPES["moebius_4097"]
    assert o["n_components"] == 1 and o["orientable"].tolist() == [False] and not o["flip"].any() and np.array_equal(o["faces"], f)
    assert o["flipped_count"].tolist() == [0]
    for reference in R.REFERENCES:
        assert np.array_equal(restated("moebius_4097", reference)["faces"], f), reference
    # the closed surfaces enclose a positive volume after "volume", whatever was flipped before
    for name in ("sphere", "torus", "inside_out_sphere"):
        v, f = SHAPES[name]
        o = restated(name, "volume")
        assert o["n_components"] == 1 and R.signed_volume6(v, o["faces"]) > 0, name
    # (the vote is taken after the parities and before the sign: the inside-out sphere's is negative, and every face is flipped for it)
    assert R.signed_volume6(*SHAPES["inside_out_sphere"]) < 0 and restated("inside_out_sphere", "volume")["flip"].all()
    assert restated("inside_out_sphere", "volume")["votes"][0] < 0
    assert abs(R.signed_volume6(SHAPES["sphere"][0], restated("sphere", "volume")["faces"]) / 6 - 4.18) < 0.2          # (a unit sphere's 4.19, inscribed)
    assert restated("inside_out_sphere", "first")["inconsistent_edges"] == 0 and not restated("inside_out_sphere", "first")["flip"].any()
    # the viewpoints surround the unit sphere: every face looks at the nearest one from outside
    o = restated("sphere", "viewpoints")
    assert np.array_equal(o["faces"], restated("sphere", "volume")["faces"])
    # what connects and what does not
    assert restated("one_face", "first")["n_components"] == 1 and restated("two_sheets", "first")["n_components"] == 2
    fin = restated("fin", "first")                                                # the run of three is ignored: three separate sheets
    assert fin["n_components"] == 3 and fin["face_label"].tolist() == [0, 1, 2, 0, 1, 2] and fin["inconsistent_edges"] == 2
    assert fin["flip"].tolist() == [False, False, False, False, True, True]          # (2, 1, 5) runs 2 -> 1 against (0, 1, 2)'s 1 -> 2
    dup = restated("duplicate_pair", "first")
    assert dup["face_label"].tolist() == [0, 1, 0, 1] and dup["flip"].tolist() == [False, False, True, False] and dup["inconsistent_edges"] == 3
    rep = restated("repeated_vertex", "first")
    assert rep["face_label"].tolist() == [0, 1, 1, 2] and rep["flip"].tolist() == [False, False, True, False]
    assert restated("repeated_vertex_run_of_three", "first")["n_components"] == 3
    keys, nodes, dirs = R.items(SHAPES["repeated_vertex"][1], 7)
    assert (keys == -1).sum() == 4 and (np.diff(keys) >= 0).all() and dirs.dtype == np.uint8
    # the strip: one deep chain, alternate parities
    strip = restated("strip_4096", "first")
    assert strip["n_components"] == 1 and strip["flip"].tolist() == [bool(j % 2) for j in range(4096)] and strip["inconsistent_edges"] == 4095
    assert not restated("strip_4096", "majority")["flip"][0] and restated("strip_4096", "majority")["flipped_count"].tolist() == [2048]
    # a permutation of the face list moves labels and roots, not the constraint graph: the rewound sheets are the same up to ONE sign
    a, b = restated("sheet_64", "majority"), restated("sheet_64_permuted", "majority")
    perm = np.random.default_rng(9).permutation(8192)
    assert np.array_equal(SHAPES["sheet_64"][1][perm], SHAPES["sheet_64_permuted"][1])
    assert a["inconsistent_edges"] == b["inconsistent_edges"] and a["n_components"] == b["n_components"] == 1
    assert np.array_equal(a["faces"][perm], b["faces"]) or np.array_equal(R.rewind(a["faces"], np.ones(8192, dtype=bool))[perm], b["faces"])
    # the vote of a face: a flipped face votes the opposite way, exactly
    v, f = SHAPES["sphere"]
    none, every = np.zeros(len(f), dtype=np.uint8), np.ones(len(f), dtype=np.uint8)
    assert np.array_equal(bits(R.votes_volume(v, f, every)), bits(R.votes_volume(v, R.rewind(f, every.astype(bool)), none)))
    assert np.array_equal(bits(R.votes_viewpoints(v, f, every, R.VIEWPOINTS)), bits(R.votes_viewpoints(v, R.rewind(f, every.astype(bool)), none, R.VIEWPOINTS)))
    on_it = R.votes_viewpoints(np.array([[0.0, 0, 0], [3, 0, 0], [0, 3, 0]]), np.array([[0, 1, 2]]), [0], np.array([[1.0, 1.0, 0.0]]))
    assert on_it.tolist() == [0.0]                                                # the viewpoint at the centroid: s == 0, t = 0


def test_golden_meshes_are_orientable_and_how_inconsistent_they_are():
    """The reference's own recorded contrastive marching-cubes meshes: what the restatement finds on them, recorded here as found."""
    found = {}
    for tag in R.GOLDEN:
        v, f = SHAPES[tag]
        o = restated(tag, "first")
        assert o["orientable"].all(), tag
        assert R.count_inconsistent(o["faces"], len(v)) == 0
        found[tag] = (len(f), len(R.manifold_edges(f, len(v))[0]), o["inconsistent_edges"], o["n_components"], int((~o["orientable"]).sum()))
    print(found)
    # faces, two-face edges, wound the same way, pieces over two-face edges, non-orientable
    assert found == {"f16": (2673, 2509, 225, 382, 0), "f16.after": (4070, 3296, 126, 775, 0), "f16.all": (4034, 3322, 158, 714, 0),
                     "f24": (3593, 3568, 376, 528, 0), "f32": (4543, 4806, 586, 657, 0)}
    assert all(4 < 100.0 * n_same / n_edges < 13 for _, n_edges, n_same, _, _ in (found[t] for t in ("f16", "f24", "f32")))


# ---------------------------------------------------------------------------------------------------------------------------------
# the loops of csrc/vfn_forest_core.h (the parity forest) on 16 host threads, before any card sees them
# ---------------------------------------------------------------------------------------------------------------------------------
def _build_host_program(tmp_path, sanitizer, name):
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    source = os.path.join(REPO, "tests", "c_abi", "forest_core_host.cpp")
    exe = str(tmp_path / name)
    base = [compiler, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", source, "-o", exe]
    build = subprocess.run(base + sanitizer, capture_output=True, text=True)
    if build.returncode != 0:          # a machine without the sanitizer's runtime: the plain program (an error in the text fails it too)
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


HOST_SHAPES = ("sheet_64", "strip_4096", "moebius_4097", "two_sheets", "fin", "duplicate_pair", "repeated_vertex", "f32")


@pytest.mark.parametrize("sanitizer", [["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], ["-fsanitize=thread"]],
                         ids=["address_undefined", "thread"])
def test_parity_union_find_core_on_sixteen_host_threads(tmp_path, sanitizer):
    exe = _build_host_program(tmp_path, sanitizer, "forest_core_host")
    text = []
    for name in HOST_SHAPES:
        v, f = SHAPES[name]
        keys, nodes, dirs = R.items(f, len(v))
        text.append(f"{len(f)} {len(keys)}\n" + "".join(f"{k} {n} {d}\n" for k, n, d in zip(keys.tolist(), nodes.tolist(), dirs.tolist())))
    # negative keys unite nothing; a node outside [0, n) is not followed and the status says so; {5: 0, 1} is a good pair wound the same way
    text.append("4 7\n-1 0 1\n-1 1 1\n5 0 1\n5 1 1\n7 2 0\n7 9 1\n8 3 0\n")
    run = subprocess.run([exe, "parity", "16"], input="".join(text) + "0 0\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    lines = run.stdout.strip().split("\n")
    assert len(lines) == 3 * (len(HOST_SHAPES) + 1)
    for at, name in enumerate(HOST_SHAPES):
        v, f = SHAPES[name]
        status, mismatches, broken = (int(x) for x in lines[3 * at].split())
        root, parity, conflict = R.parity_serial(f, len(v))
        o = restated(name, "first")
        fine = o["orientable"][o["face_label"]]
        assert status == 0 and mismatches == 0, (name, lines[3 * at])              # every threaded run equalled the program's serial one
        assert (broken > 0) == (not o["orientable"].all()) == conflict.any(), name
        assert np.array_equal(np.array(lines[3 * at + 1].split(), dtype=np.int64), root), name
        assert np.array_equal(np.array(lines[3 * at + 2].split(), dtype=np.uint8)[fine], parity[fine]), name
    assert lines[-3].split() == ["2", "0", "0"] and lines[-2].split() == ["0", "0", "2", "3"] and lines[-1].split() == ["0", "1", "0", "0"]


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals before a device is asked for
# ---------------------------------------------------------------------------------------------------------------------------------
TRI_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.array([[0, 1, 2]])
TRI = (TRI_V, TRI_F)
EYE = np.array([[0.0, 0.0, 5.0]])


@pytest.mark.parametrize("call", [
    lambda: meshops.orientation(TRI, reference="last"),
    lambda: meshops.orientation(TRI, reference=None),
    lambda: meshops.orientation(TRI, reference="viewpoints"),
    lambda: meshops.orientation(TRI, reference="first", viewpoints=EYE),
    lambda: meshops.orientation(TRI, reference="volume", viewpoints=EYE),
    lambda: meshops.orientation(TRI, reference="viewpoints", viewpoints=np.zeros((0, 3))),
    lambda: meshops.orientation(TRI, reference="viewpoints", viewpoints=np.zeros((2, 2))),
    lambda: meshops.orientation(TRI, reference="viewpoints", viewpoints=np.zeros(3)),
    lambda: meshops.orientation(TRI, reference="viewpoints", viewpoints=np.array([[0, 0, 5]])),
    lambda: meshops.orientation(TRI, reference="viewpoints", viewpoints=np.array([[0.0, np.nan, 5.0]])),
    lambda: meshops.orientation((TRI_V, np.array([[0, 1, 3]]))),
    lambda: meshops.orientation((TRI_V, np.array([[0, -1, 2]]))),
    lambda: meshops.orientation((TRI_V[:, :2], TRI_F)),
    lambda: meshops.orient(TRI, reference="area"),
    lambda: meshops.orient(TRI, reference="viewpoints"),
    lambda: meshops.orient(TRI, viewpoints=EYE),
    lambda: meshops.orient((TRI_V, np.array([[0, 1, 3]]))),
    lambda: meshops.inconsistent_edges((TRI_V, np.array([[0, 1, 3]]))),
    lambda: mesh.extract_mesh(None, 4, orient="viewpoints"),
    lambda: mesh.extract_mesh(None, 4, orient="last"),
    lambda: mesh.extract_mesh(None, 4, orient=True),
    lambda: dropin.install(mesh_orient="viewpoints"),
    lambda: dropin.install(mesh_orient=1),
])
def test_bad_arguments_raise_before_any_device_call(call, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(meshops.geomargs, "device", no_device)
    with pytest.raises(ValueError):
        call()
    assert mesh.ORIENT is None


def test_binding_refuses_shapes_before_the_device():
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64)          # noqa: E731
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)           # noqa: E731
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)          # noqa: E731
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)        # noqa: E731
    with pytest.raises(lib.VfnError, match=r"keys, nodes and dirs must be \[k\]"):
        lib.orient_union_runs(i64(5), i64(5), u8(4), i32(3))
    with pytest.raises(lib.VfnError, match="at least 1 item"):
        lib.orient_union_runs(i64(0), i64(0), u8(0), i32(3))
    with pytest.raises(lib.VfnError, match=r"nodes in \[1, 2\^30\)"):
        lib.orient_union_runs(i64(5), i64(5), u8(5), i32(0))
    with pytest.raises(lib.VfnError, match=r"nodes in \[1, 2\^30\)"):
        lib.orient_union_runs(i64(5), i64(5), u8(5), i32(1).expand(1 << 30))          # (a view: no memory)
    with pytest.raises(lib.VfnError, match=r"forest must be \[n\]"):
        lib.orient_flatten(i32(0))
    with pytest.raises(lib.VfnError, match=r"forest must be \[n\]"):
        lib.orient_flatten(i32(1).expand(1 << 30))
    with pytest.raises(lib.VfnError, match="m >= 1"):
        lib.orient_votes(f64(3, 3), i64(0, 3), None, lib.ORIENT_VOLUME)
    with pytest.raises(lib.VfnError, match=r"parity must be \[2\]"):
        lib.orient_votes(f64(3, 3), i64(2, 3), u8(3), lib.ORIENT_VOLUME)
    with pytest.raises(lib.VfnError, match="mode must be"):
        lib.orient_votes(f64(3, 3), i64(2, 3), None, 2)
    with pytest.raises(lib.VfnError, match=r"C >= 1"):
        lib.orient_votes(f64(3, 3), i64(2, 3), None, lib.ORIENT_VIEWPOINTS)
    with pytest.raises(lib.VfnError, match=r"C >= 1"):
        lib.orient_votes(f64(3, 3), i64(2, 3), None, lib.ORIENT_VIEWPOINTS, f64(0, 3))
    with pytest.raises(lib.VfnError, match="takes no viewpoints"):
        lib.orient_votes(f64(3, 3), i64(2, 3), None, lib.ORIENT_VOLUME, f64(1, 3))
    # host tensors never reach the library: there is no CPU path
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.orient_union_runs(i64(5), i64(5), u8(5), i32(3))
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.orient_flatten(i32(3))
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.orient_votes(f64(3, 3), i64(2, 3), None, lib.ORIENT_VOLUME)
    lib.orient_check(0)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.orient_check(2)
    with pytest.raises(lib.VfnError, match="non-finite"):
        lib.orient_check(1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is visible: the calls would run")
def test_no_cpu_fallback():
    for call in (lambda: meshops.orientation(TRI), lambda: meshops.orient(TRI, reference="majority"), lambda: meshops.inconsistent_edges(TRI),
                 lambda: meshops.orientation(TRI, reference="viewpoints", viewpoints=EYE)):
        with pytest.raises(lib.VfnError, match="no GPU"):
            call()


# ---------------------------------------------------------------------------------------------------------------------------------
# the call paths, the device stood in for
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_drop_in_without_the_switch_takes_todays_path(monkeypatch):
    calls = []
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]], dtype=torch.float64)
    f = torch.tensor([[0, 1, 2], [1, 2, 3]])

    def triangulate(comb, **kw):
        calls.append(("triangulate", comb, kw))
        return v, f

    def no_orient(*a, **k):
        raise AssertionError("the orientation was reached")

    def orient(m, reference="first", viewpoints=None, device=None):
        calls.append(("orient", m[0] is v, m[1] is f, reference, viewpoints))
        return m[0], torch.tensor([[0, 1, 2], [1, 3, 2]]), None

    monkeypatch.setattr(mesh, "triangulate", triangulate)
    monkeypatch.setattr(meshops, "orient", no_orient)
    monkeypatch.setattr(meshops, "_orientation", no_orient)
    monkeypatch.setattr(mesh, "ORIENT", None)
    saved = {k: m for k, m in sys.modules.items() if k.split(".")[0] in ("models", "evaluation")}
    try:
        dropin.install()                                                          # without the keyword: the switch stays as it is
        assert mesh.ORIENT is None
        vs, fs = mesh.contrastive_marching_cubes("comb", isovalue=0.5, res=4, size=3.0, udf="udf", selected_indices="cells")
        assert calls == [("triangulate", "comb", dict(isovalue=0.5, res=4, size=3.0, udf="udf", selected_indices="cells"))]
        assert (vs, fs) == mesh.to_reference(v, f) and fs == [[1, 2, 3], [2, 3, 4]]
        # with the switch: the triangulation's mesh goes through meshops.orient, the rewound faces are listed, the vertices keep their ids
        monkeypatch.setattr(meshops, "orient", orient)
        dropin.install(mesh_orient="majority")
        assert mesh.ORIENT == "majority"
        del calls[:]
        vs2, fs2 = mesh.contrastive_marching_cubes("comb")
        assert [c[0] for c in calls] == ["triangulate", "orient"] and calls[1] == ("orient", True, True, "majority", None)
        assert vs2 == vs and fs2 == [[1, 2, 3], [2, 4, 3]]
        dropin.install()                                                          # None leaves the switch as it is
        assert mesh.ORIENT == "majority"
    finally:
        mesh.ORIENT = None
        dropin.uninstall_clip_grad_norm()
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "evaluation")]:
            del sys.modules[k]
        sys.modules.update(saved)
    from vf_nerf_amd import evaluator
    assert "mesh.ORIENT = mesh_orient" in inspect.getsource(dropin.install)
    assert "orient" not in inspect.getsource(evaluator.tsdf_mesh)                 # the TSDF meshes are wound consistently by construction


def test_a_refused_install_sets_no_switch(monkeypatch):
    from vf_nerf_amd import evaluator
    monkeypatch.setattr(mesh, "ORIENT", None)
    monkeypatch.setattr(evaluator, "TSDF_MIN_COMPONENT_FACES", None)
    with pytest.raises(ValueError, match="tsdf_min_component_faces"):
        dropin.install(mesh_orient="first", tsdf_min_component_faces=-1)
    assert mesh.ORIENT is None and evaluator.TSDF_MIN_COMPONENT_FACES is None
    with pytest.raises(ValueError, match="mesh_orient"):
        dropin.install(mesh_orient="last", tsdf_min_component_faces=5)
    assert mesh.ORIENT is None and evaluator.TSDF_MIN_COMPONENT_FACES is None
