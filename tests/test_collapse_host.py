"""Quadric edge-collapse decimation, host side: the two CPU restatements of the contract (tests/collapse_restatement.py) held against each
other bit for bit, round by round and over whole calls; the properties that follow from the contract, on the restatement; the C-ABI
surface and the build recipe; the per-edge routine of csrc/vfn_collapse_core.h run by the stand-alone program
tests/c_abi/collapse_core_host.cpp under a sanitizer; the argument checks that answer before any device is asked for; the switches."""
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

from vf_nerf_amd import bases, decimate, dropin, evaluator, lib, meshops  # noqa: E402
from vf_nerf_amd.meshops import simplify_edge_collapse  # noqa: E402
import cc_restatement as CC  # noqa: E402
import collapse_restatement as R  # noqa: E402
import simplify_restatement as SR  # noqa: E402

NEW_EXPORTS = ("vfn_boundary_planes", "vfn_vertex_quadrics", "vfn_edge_collapse_candidates", "vfn_collapse_select")
SHAPES = R.cases()
_whole = {}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    return np.array_equal(bits(a), bits(b)) if b.dtype.kind == "f" else np.array_equal(a, b)


def whole(name):
    """A case through the array text, with every round; computed once and shared."""
    if name not in _whole:
        v, f, kw = SHAPES[name]
        history = []
        _whole[name] = (R.collapse(v, f, history=history, **kw), history)
    return _whole[name]


# ---------------------------------------------------------------------------------------------------------------------------------
# the two texts
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_two_restatements_agree(name):
    """Every round's every field and the whole call's every field, bit for bit.  (On the flat squares about one edge collapses a round —
    every cost ties at 0 —, so the loops, at 50 ms a round, follow the arrays through the first 24 rounds there.)"""
    v, f, kw = SHAPES[name]
    if name.startswith("square"):
        kw = dict(kw, max_rounds=24)
    col, nrm = R.attributes(len(v))
    ha, hl = [], []
    a = R.collapse(v, f, colours=col, normals=nrm, text="arrays", history=ha, **kw)
    b = R.collapse(v, f, colours=col, normals=nrm, text="loops", history=hl, **kw)
    assert len(ha) == len(hl) == a["rounds"] == b["rounds"]
    for i, (x, y) in enumerate(zip(ha, hl)):
        for key in R.ROUND_FIELDS:
            assert x[key].dtype == y[key].dtype and same(x[key], y[key]), (name, i, key)
        assert x["n_taken"] == y["n_taken"]
    for key in R.FIELDS:
        assert same(a[key], b[key]), (name, key)
    plain = whole(name)[0] if not name.startswith("square") else R.collapse(v, f, **kw)
    assert same(plain["vertices"], a["vertices"]) and same(plain["faces"], a["faces"])          # the attributes move no bit of the mesh


# ---------------------------------------------------------------------------------------------------------------------------------
# what follows from the contract
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_output_invariants(name):
    v, f, kw = SHAPES[name]
    out, history = whole(name)
    faces = out["faces"]
    assert not ((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 2] == faces[:, 0])).any()
    assert len(np.unique(np.sort(faces, axis=1), axis=0)) == len(faces)
    if out["reached"]:
        assert len(faces) <= kw["target_faces"]
    assert out["reached"] == ("target_faces" in kw and len(faces) <= kw["target_faces"])
    # inverse composed with the output reproduces the kept faces' corners; every output vertex is named
    assert np.array_equal(out["inverse"][f[out["kept_faces"]]], faces) and (np.diff(out["kept_faces"]) > 0).all()
    assert np.array_equal(np.unique(faces), np.arange(len(out["vertices"]))) and out["inverse"].max(initial=-1) == len(out["vertices"]) - 1
    assert (out["cost"] >= 0).all() and not np.signbit(out["cost"]).any() and out["rounds"] == len(history) <= kw.get("max_rounds", 256)
    assert out["collapsed"] == sum(r["n_taken"] for r in history)
    for r in history:
        taken, stays = r["taken"], r["proposed"] & ~r["withdrawn"]
        assert not (taken & ~stays).any() and not (r["proposed"] & ((r["flags"] & R.CANDIDATE) == 0)).any()
        assert not np.signbit(r["cost"]).any() and (r["cost"] >= 0).all() and ((r["s"] >= 0) & (r["s"] <= 1)).all()
        live = np.nonzero(r["flags"] & R.CANDIDATE)[0]
        if len(live):                                                   # the globally cheapest candidate always stays: a round is never idle
            cheapest = live[np.lexsort((live, r["cost"][live]))[0]]
            assert stays[cheapest] and r["n_taken"] >= 1
        else:
            assert r["n_taken"] == 0
        # what stays shares no vertex, and no face sees two of them: their 1-rings share no moving vertex
        ends = np.concatenate((r["edge_a"][stays], r["edge_b"][stays]))
        assert len(np.unique(ends)) == len(ends)
        moving = np.full(len(v), -1)
        moving[r["edge_a"][stays]] = moving[r["edge_b"][stays]] = np.nonzero(stays)[0]
        seen = moving[r["inputs"][1]]
        for c in range(3):
            d = (c + 1) % 3
            assert not ((seen[:, c] >= 0) & (seen[:, d] >= 0) & (seen[:, c] != seen[:, d])).any()


def test_the_flat_square_keeps_its_outline():
    """16 x 16 cells, coordinates multiples of 1/16, max_error = 1e-12, target 1.  A zero-cost collapse moves a vertex within every plane it
    lies on, the boundary planes included; the smallest non-zero cost on this grid is of the order area x distance^2 >= (1/512) (1/32)^2,
    about 2e-6, so 1e-12 separates them: every z stays exactly 0, the four corners stay with their bits, the area stays 1."""
    v, f, kw = SHAPES["square_outline"]
    assert len(f) == 512 and kw == {"max_error": 1e-12, "target_faces": 1} and np.array_equal(v * 16, np.round(v * 16))
    out = whole("square_outline")[0]
    assert (out["vertices"][:, 2] == 0).all() and not out["reached"] and len(out["faces"]) < 512
    for corner in ((0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0)):
        assert ((out["vertices"][:, 0] == corner[0]) & (out["vertices"][:, 1] == corner[1])).sum() == 1
    assert abs(CC.tri_areas(out["vertices"], out["faces"]).sum() - 1.0) <= 1e-12
    assert (out["cost"] <= 1e-12).all()
    # run to the end: the outline still holds when nothing more may collapse
    end = R.collapse(v, f, max_rounds=4096, **kw)
    assert end["rounds"] < 4096 and not end["reached"] and len(end["faces"]) >= 2 and abs(CC.tri_areas(end["vertices"], end["faces"]).sum() - 1.0) <= 1e-12


def test_without_the_boundary_term_the_square_shrinks():
    v, f, kw = SHAPES["square_free"]
    assert kw["boundary_weight"] == 0.0 and kw["target_faces"] == 2 and "max_error" not in kw
    assert whole("square_free")[0]["reached"] and len(whole("square_free")[0]["faces"]) <= 2


def test_no_face_of_the_cube_turns_over():
    """The closed, consistently wound cube of 4 x 4 cells a side at 96 faces: no output face's normal opposes the outward normal of the
    side that all three of its vertices lie on (the flip test)."""
    v, f, kw = SHAPES["cube_96"]
    assert len(f) == 192 and kw == {"target_faces": 96}
    out = whole("cube_96")[0]
    p = out["vertices"][out["faces"]]
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    checked = 0
    for axis in range(3):
        for side, sign in ((0.0, -1.0), (1.0, 1.0)):
            on = (p[:, :, axis] == side).all(axis=1)
            checked += int(on.sum())
            assert (sign * normal[on, axis] >= 0).all(), (axis, side)
    assert checked >= 48 and out["reached"]


def test_a_non_manifold_edge_never_collapses_but_its_neighbours_do():
    out, history = whole("book")
    for r in history:
        assert not (r["taken"] & (r["run"] > 2)).any()
    assert history[0]["run"].max() == 3 and out["collapsed"] > 0 and out["reached"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_boundary_planes"] == ("int", ["const double*", "int64_t", "const double*", "int64_t", "const int64_t*", "const int64_t*",
                                                     "const int64_t*", "int64_t", "const double*", "double", "double*", "int64_t*", "void*"])
    assert protos["vfn_vertex_quadrics"] == ("int", ["const double*", "int64_t", "const int64_t*", "int64_t", "const int64_t*", "int64_t", "double*",
                                                     "int64_t*", "void*"])
    assert protos["vfn_edge_collapse_candidates"][1][-6:] == ["double*", "double*", "double*", "uint8_t*", "int64_t*", "void*"]
    assert protos["vfn_collapse_select"][1][-3:] == ["uint8_t*", "int64_t*", "void*"]
    assert lib.header_abi_version() == 5
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    for name in NEW_EXPORTS:
        assert getattr(handle, name).argtypes is not None
    # the host-side checks of the exports answer without a device
    origin = (lib.C.c_double * 3)(0.0, 0.0, 0.0)
    bad_origin = (lib.C.c_double * 3)(0.0, float("nan"), 0.0)
    err = handle.vfn_last_error
    assert handle.vfn_boundary_planes(None, 0, None, 4, None, None, None, 1, origin, 1.0, None, None, None) != 0 and b"n 0 outside [1, 2^31)" in err()
    assert handle.vfn_boundary_planes(None, 4, None, 1 << 31, None, None, None, 1, origin, 1.0, None, None, None) != 0 and b"m " in err()
    assert handle.vfn_boundary_planes(None, 4, None, 4, None, None, None, 13, origin, 1.0, None, None, None) != 0 and b"count 13 outside [1, 3 m = 12]" in err()
    assert handle.vfn_boundary_planes(None, 4, None, 4, None, None, None, 1, origin, 1.0, None, None, None) != 0 and b"NULL" in err()
    assert handle.vfn_vertex_quadrics(None, 0, None, 5, None, 4, None, None, None) != 0 and b"rows 0 outside" in err()
    assert handle.vfn_vertex_quadrics(None, 4, None, 0, None, 4, None, None, None) != 0 and b"n_items 0 outside" in err()
    assert handle.vfn_vertex_quadrics(None, 4, None, 5, None, 1 << 31, None, None, None) != 0 and b"n " in err()
    assert handle.vfn_vertex_quadrics(None, 4, None, 5, None, 4, None, None, None) != 0 and b"NULL" in err()
    candidates = lambda *, n=4, m=4, items=12, rows=6, edges=9, o=origin, rcond=1e-9, reach=2.0, limit=1.0: handle.vfn_edge_collapse_candidates(  # noqa: E731
        None, n, None, m, None, None, items, None, rows, None, None, None, edges, o, rcond, reach, limit, None, None, None, None, None, None)
    assert candidates(n=0) != 0 and b"n 0 outside" in err()
    assert candidates(m=0) != 0 and b"m 0 outside" in err()
    assert candidates(rows=3) != 0 and b"rows 3 outside [m = 4, 4 m]" in err()
    assert candidates(rows=17) != 0 and b"rows 17 outside" in err()
    assert candidates(edges=13) != 0 and b"n_edges 13 outside [1, 3 m = 12]" in err()
    assert candidates(edges=0) != 0 and b"n_edges 0 outside" in err()
    assert candidates() != 0 and b"NULL" in err()
    v = torch.zeros(1)          # any non-NULL host address: the checks below answer before anything is read
    p = lib.C.c_void_p(v.data_ptr())
    full = lambda o=origin, rcond=1e-9, reach=2.0, limit=1.0: handle.vfn_edge_collapse_candidates(  # noqa: E731
        p, 4, p, 4, p, p, 12, p, 6, p, p, p, 9, o, rcond, reach, limit, p, p, p, p, p, None)
    assert full(o=bad_origin) != 0 and b"non-finite origin" in err()
    assert full(rcond=2.0) != 0 and b"rcond 2 outside [0, 1]" in err()
    assert full(reach=-1.0) != 0 and b"reach -1" in err()
    assert full(reach=float("inf")) != 0 and b"reach inf" in err()
    assert full(limit=-1.0) != 0 and b"max_error -1" in err()
    assert full(limit=float("nan")) != 0 and b"max_error" in err()
    assert handle.vfn_collapse_select(None, None, None, None, 9, None, 4, 0, None, None, None, None, None, None) != 0 and b"n 0 outside" in err()
    assert handle.vfn_collapse_select(None, None, None, None, 13, None, 4, 4, None, None, None, None, None, None) != 0 and b"n_edges 13" in err()
    assert handle.vfn_collapse_select(None, None, None, None, 9, None, 4, 4, None, None, None, None, None, None) != 0 and b"NULL" in err()


def test_build_recipe_lists_the_unit_in_both_places():
    build = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "build.sh")).read()
    assert re.search(r'^UNITS=".*\bvfn_collapse\b.*"', build, flags=re.M)
    assert re.search(r"\|vfn_collapse[|)].*-ffp-contract=off", build)
    # the VFN_ONLY shortcut refuses objects older than the core: than every header beside the units, the core among them
    assert re.search(r'for src in "\$u\.hip" \*\.h \.\./\.\./include/vfn\.h; do\n +\[ "\$OBJDIR/\$u\.o" -nt "\$src" \] \|\| fresh=0\n', build)
    for name in ("vfn_collapse.hip", "vfn_collapse_core.h"):
        assert os.path.exists(os.path.join(REPO, "vf_nerf_amd", "csrc", name))
    # the device and the host program compile ONE text of the per-edge routine; the unit has no floating-point atomic
    unit = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "vfn_collapse.hip")).read()
    assert '#include "vfn_collapse_core.h"' in unit and "atomicAdd" not in unit and "__shared__" not in unit
    assert "vfn_collapse_core.h" in open(os.path.join(REPO, "tests", "c_abi", "collapse_core_host.cpp")).read()


def test_signatures_switches_and_words():
    assert list(inspect.signature(simplify_edge_collapse).parameters) == ["mesh", "target_faces", "max_error", "boundary_weight", "rcond", "reach",
                                                                          "colours", "normals", "max_rounds", "device"]
    defaults = {k: p.default for k, p in inspect.signature(simplify_edge_collapse).parameters.items()}
    assert defaults == {"mesh": inspect.Parameter.empty, "target_faces": None, "max_error": None, "boundary_weight": 1.0, "rcond": 1e-9, "reach": 2.0,
                        "colours": None, "normals": None, "max_rounds": 256, "device": None}
    assert meshops.simplify_edge_collapse is decimate.simplify_edge_collapse and meshops.collapse_round is decimate.collapse_round
    assert decimate.Collapsed._fields == ("vertices", "faces", "kept_faces", "inverse", "colours", "normals", "cost", "rounds", "collapsed", "reached")
    assert set(R.ROUND_FIELDS) | {"n_taken"} == set(decimate.Round._fields)
    # the switches are off
    assert meshops.DECIMATION == "clustering" and evaluator.TSDF_SIMPLIFY_FACES is None and evaluator.TSDF_SIMPLIFY_VOXEL is None
    install = inspect.signature(dropin.install).parameters
    assert install["dominant_bases_decimation"].default is None and install["tsdf_simplify_faces"].default is None
    assert list(install)[-2:] == ["patch_dominant_bases", "mesh_orient"]
    assert "decimation" in inspect.signature(meshops.dominant_bases).parameters and "decimation" in inspect.signature(bases.get_dominant_bases).parameters
    source = inspect.getsource(dropin.install)
    assert "evaluator.TSDF_SIMPLIFY_FACES = tsdf_simplify_faces" in source and "meshops.DECIMATION = dominant_bases_decimation" in source
    assert "TSDF_SIMPLIFY_FACES is not None" in inspect.getsource(evaluator.tsdf_mesh)
    for doc in (decimate.__doc__, simplify_edge_collapse.__doc__, R.__doc__):
        assert "AS SPECIFIED BY US" in doc and "not verified against trimesh / Open3D" in doc
    assert "link condition" in decimate.__doc__ and "link condition" in simplify_edge_collapse.__doc__
    assert "simplify_edge_collapse" in meshops.__doc__ and "AS SPECIFIED BY US" in meshops.simplify_to_faces.__doc__
    header = open(lib.HEADER_PATH).read()
    assert "AS SPECIFIED\n * BY US" in header and "link condition" in header


# ---------------------------------------------------------------------------------------------------------------------------------
# the per-edge routine of csrc/vfn_collapse_core.h on the host, under a sanitizer, before any card sees it
# ---------------------------------------------------------------------------------------------------------------------------------
def _build_host_program(tmp_path):
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    source = os.path.join(REPO, "tests", "c_abi", "collapse_core_host.cpp")
    exe = str(tmp_path / "collapse_core_host")
    base = [compiler, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", source, "-o", exe]
    build = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if build.returncode != 0:          # a machine without the sanitizers' runtime: the plain program (an error in the text fails it too)
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def _case_text(position, f, origin, r, kw, item_row=None):
    numbers = lambda a: " ".join(float(x).hex() for x in np.asarray(a, dtype=np.float64).reshape(-1))          # noqa: E731
    ints = lambda a: " ".join(str(int(x)) for x in np.asarray(a).reshape(-1))          # noqa: E731
    limit = "inf" if kw.get("max_error") is None else float(kw["max_error"]).hex()
    rows = r["item_row"] if item_row is None else item_row
    head = f"{len(position)} {len(f)} {len(rows)} {len(r['planes'])} {len(r['edge_a'])}\n"
    head += f"{numbers(origin)} {float(kw.get('rcond', 1e-9)).hex()} {float(kw.get('reach', 2.0)).hex()} {limit}\n"
    edges = "\n".join(f"{a} {b} {c}" for a, b, c in zip(r["edge_a"].tolist(), r["edge_b"].tolist(), r["run"].tolist()))
    return head + "\n".join((numbers(position), ints(f), numbers(r["quadrics"]), ints(rows), ints(r["start"]), edges)) + "\n"


def test_edge_routine_on_the_host_equals_the_restatement(tmp_path):
    """The first and the last round of the small cases through the stand-alone program: flags, costs, parameters and points equal the
    restatement's bits.  Then a table that lies (a row outside its range, a face that is not the vertex's): the status says so, the
    edges that walk it are no candidates, and the sanitizer sees no read outside an array."""
    exe = _build_host_program(tmp_path)
    names = ("bow_tie", "three_on_an_edge", "square_outline", "ribbon_40", "cube_12", "cube_error_only", "moebius", "book", "fan_65", "edges_256")
    text, wanted = [], []
    for name in names:
        history = whole(name)[1]
        for r in (history[0], history[-1]):
            text.append(_case_text(*r["inputs"], r, SHAPES[name][2]))
            wanted.append((name, r, 0, True))
    r = whole("cube_12")[1][0]
    for bad in (len(r["planes"]), -1, int(r["item_row"][-1])):
        lying = r["item_row"].copy()
        lying[0] = bad
        text.append(_case_text(*r["inputs"], r, SHAPES["cube_12"][2], item_row=lying))
        wanted.append(("cube_12 with a lying table", r, 2, bad != int(r["item_row"][-1])))
    run = subprocess.run([exe], input="".join(text) + "0 0 0 0 0\n", capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    lines = iter(run.stdout.strip().split("\n"))
    for name, r, status, strict in wanted:
        head = next(lines).split()
        assert [int(x) for x in head] == [status, len(r["edge_a"])], (name, head)
        got = np.array([[int(x, 16) if i else int(x) for i, x in enumerate(next(lines).split())] for _ in range(len(r["edge_a"]))], dtype=np.uint64)
        if status:
            walks = (r["edge_a"] == 0) | (r["edge_b"] == 0)          # the edges of vertex 0 walk the item that lies
            # (an edge whose other end the substituted face names skips that face before it can notice: only the first two are strict)
            assert not (strict and (got[walks, 0] & R.CANDIDATE).any()) and np.array_equal(got[~walks, 0], r["flags"][~walks])
        else:
            assert np.array_equal(got[:, 0], r["flags"]), name
        assert np.array_equal(got[:, 1], bits(r["cost"])) and np.array_equal(got[:, 2], bits(r["s"])), name
        assert np.array_equal(got[:, 3:], bits(r["point"])), name
    assert next(lines, None) is None


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals before a device is asked for
# ---------------------------------------------------------------------------------------------------------------------------------
TRI_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.array([[0, 1, 2]])
TRI = (TRI_V, TRI_F)


@pytest.mark.parametrize("call", [
    lambda: simplify_edge_collapse(TRI),
    lambda: simplify_edge_collapse(TRI, target_faces=0),
    lambda: simplify_edge_collapse(TRI, target_faces=1.5),
    lambda: simplify_edge_collapse(TRI, target_faces=True),
    lambda: simplify_edge_collapse(TRI, max_error=-1.0),
    lambda: simplify_edge_collapse(TRI, max_error=float("nan")),
    lambda: simplify_edge_collapse(TRI, max_error=float("inf")),
    lambda: simplify_edge_collapse(TRI, max_error="1"),
    lambda: simplify_edge_collapse(TRI, target_faces=1, boundary_weight=-1.0),
    lambda: simplify_edge_collapse(TRI, target_faces=1, boundary_weight=None),
    lambda: simplify_edge_collapse(TRI, target_faces=1, rcond=2.0),
    lambda: simplify_edge_collapse(TRI, target_faces=1, reach=-0.5),
    lambda: simplify_edge_collapse(TRI, target_faces=1, reach=1e200),
    lambda: simplify_edge_collapse(TRI, target_faces=1, max_rounds=0),
    lambda: simplify_edge_collapse(TRI, target_faces=1, max_rounds=2.0),
    lambda: simplify_edge_collapse(TRI, target_faces=1, colours=np.zeros((4, 3))),
    lambda: simplify_edge_collapse(TRI, target_faces=1, normals=np.zeros((3, 2))),
    lambda: simplify_edge_collapse((TRI_V, np.array([[0, 1, 3]])), target_faces=1),
    lambda: simplify_edge_collapse((TRI_V, np.array([[0, -1, 2]])), target_faces=1),
    lambda: simplify_edge_collapse((TRI_V[:, :2], TRI_F), target_faces=1),
    lambda: decimate.collapse_round(torch.zeros(3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int64), (0.0, 0.0, 0.0)),
    lambda: dropin.install(dominant_bases_decimation="quadric"),
    lambda: dropin.install(tsdf_simplify_faces=0),
    lambda: dropin.install(tsdf_simplify_faces=2.5),
    lambda: dropin.install(tsdf_simplify_faces=True),
    lambda: dropin.install(tsdf_simplify_faces=100, tsdf_simplify_voxel=0.1),
])
def test_bad_arguments_raise_before_any_device_call(call, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(meshops.geomargs, "device", no_device)
    with pytest.raises(ValueError):
        call()
    assert evaluator.TSDF_SIMPLIFY_FACES is None and evaluator.TSDF_SIMPLIFY_VOXEL is None and meshops.DECIMATION == "clustering"


def test_binding_refuses_shapes_before_the_device():
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)          # noqa: E731
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64)          # noqa: E731
    with pytest.raises(lib.VfnError, match="boundary_planes: vertices must be"):
        lib.boundary_planes(f64(3, 3), f64(1, 5), i64(0), i64(0), i64(0), (0, 0, 0), 1.0)
    with pytest.raises(lib.VfnError, match="vertex_quadrics: planes must be"):
        lib.vertex_quadrics(f64(1, 4), i64(3), i64(4))
    with pytest.raises(lib.VfnError, match="edge_collapse_candidates: vertices must be"):
        lib.edge_collapse_candidates(f64(3, 3), i64(1, 3), f64(3, 9), i64(3), i64(4), 1, i64(3), i64(3), i64(3), (0, 0, 0), 1e-9, 2.0, 1.0)
    with pytest.raises(lib.VfnError, match="collapse_select: cost"):
        lib.collapse_select(f64(3), torch.zeros(2, dtype=torch.uint8), i64(3), i64(3), i64(1, 3), 3)
    # host tensors never reach the library: there is no CPU path
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.vertex_quadrics(f64(1, 5), i64(3), i64(4))
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.collapse_select(f64(3), torch.zeros(3, dtype=torch.uint8), i64(3), i64(3), i64(1, 3), 3)
    lib.collapse_check(0)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.collapse_check(2)
    with pytest.raises(lib.VfnError, match="non-finite"):
        lib.collapse_check(1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is visible: the calls would run")
def test_no_cpu_fallback(monkeypatch):
    with pytest.raises(lib.VfnError, match="no GPU"):
        simplify_edge_collapse(TRI, target_faces=1)
    monkeypatch.setattr(meshops, "DECIMATION", "collapse")
    with pytest.raises(lib.VfnError, match="no GPU"):
        meshops.dominant_bases(SR.cube(4), 3, decimation=0.5)
