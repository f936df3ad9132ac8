"""The closest point on a triangle mesh without a device: the two restatements of tests/proximity_restatement.py against each other, the
properties P1-P5 of include/vfn.h, the flaw of the four-candidate form, the accuracy against an exact rational oracle, the grid model
(no bit changes, whatever the grid), the pair routine of csrc/vfn_proximity_core.h through the stand-alone program of
tests/c_abi/proximity_core_host.cpp under a sanitizer, and the argument checks that answer before any device is asked for."""
from __future__ import annotations

import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import proximity_restatement as R
from vf_nerf_amd import lib, metrics3d, refuse

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("vfn_tri_cell_ranges", "vfn_tri_cell_pairs", "vfn_tri_nearest", "vfn_tri_nearest_list")

# The largest errors of d2 against the exact value, measured on the families of R.accuracy_pairs(): relative where the exact
# d2 is positive, d2 / (longest edge)^2 where it is 0.  "on" (dyadic, every intermediate exact) and "vertex" (a vertex of a needle or a
# tiny triangle in its own bits: candidates 5-7) give exactly 0.  "near" is where rounding is live: rounded midpoints and inner points
# of needles and tiny triangles; 14 of its 80 pairs have an exact d2 of 0, the others one at the level of a squared ulp, where a
# relative error says nothing (it is measured and printed, not bounded) and |d2 - exact| / edge^2 over all 80 is the figure.
# The test allows 8 times each.
MEASURED_RELATIVE = {"random": 2.14e-15, "needle": 2.27e-16, "tiny": 1.11e-10, "far": 2.66e-16, "on": 0.0, "vertex": 0.0, "near": None}
MEASURED_ZERO = {"random": 0.0, "needle": 0.0, "tiny": 0.0, "far": 0.0, "on": 0.0, "vertex": 0.0, "near": 3.18e-23}
MEASURED_NEAR_ABSOLUTE = 2.71e-21
EXACT_ZEROS = {"on": 60, "vertex": 80, "near": 14}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.cases()))
def test_two_restatements_agree(name):
    v, f, q = R.cases()[name]
    assert same(R.brute_scalar(q, v, f), R.brute(q, v, f))


def test_a_face_that_is_none_and_a_nan_query():
    v, f, q = R.cases()["soup"]
    f = f.copy()
    f[3, 1], f[7, 0] = len(v), -1
    q = q[:20].copy()
    q[5, 1] = np.nan
    a, b = R.brute_scalar(q, v, f), R.brute(q, v, f)
    assert same(a, b)
    assert a[0][5] == -1 and np.isinf(a[2][5]) and np.isinf(a[1][5]).all()
    assert not np.isin(a[0], (3, 7)).any() and (np.delete(a[0], 5) >= 0).all()


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_the_grid_changes_no_bit(name):
    """For every grid setting the ring path alone — large faces, rings 0..the ring at which the rule stops — gives the definition's bits;
    the model's pair, large and leftover counts are what they must be at the ends of each setting's range."""
    v, f, q = R.cases()[name]
    want = R.brute(q, v, f)
    n_valid = int(R.valid_faces(v, f).sum())
    for setting in R.GRID_SETTINGS:
        box, dims = R.host_grid(v, f, setting.get("cells"))
        big = setting.get("big_face_cells", metrics3d.BIG_FACE_CELLS)
        ring, *got = R.ring_search(q, v, f, box, dims, big)
        assert same(got, want), setting
        ncells = R.cell_ranges(v, f, box, dims)[2]
        n_pairs, n_large = R.grid_counts(ncells, big)
        assert n_pairs + int(ncells[ncells > big].sum()) == int(ncells.sum()) and (ncells >= 1).sum() == n_valid
        if big == 0:
            assert (n_pairs, n_large) == (0, n_valid)
        if big == 10 ** 9:
            assert n_large == 0
        if setting.get("cells") == 1:
            assert dims == (1, 1, 1) and n_pairs == n_valid and R.leftovers(ring, 0) == 0          # ring 0 covers a 1 x 1 x 1 grid
        assert R.leftovers(ring, max(dims)) == 0 and R.leftovers(ring, 0) >= R.leftovers(ring, 1) >= R.leftovers(ring, 8)


# ---------------------------------------------------------------------------------------------------------------------------------
# P1 - P5
# ---------------------------------------------------------------------------------------------------------------------------------
def _property_pairs():
    g = np.random.default_rng(31)
    pairs = [p for family in R.accuracy_pairs().values() for p in family]
    for _ in range(60):                                                       # degenerate: A = B, collinear, A = B = C, each in every rotation
        A, B = g.uniform(-1, 1, (2, 3))
        q = g.uniform(-2, 2, 3)
        t = g.uniform(-1, 2)
        pairs += [(q, A, A, B), (q, A, B, A), (q, B, A, A), (q, A, B, A + t * (B - A)), (q, A + t * (B - A), A, B), (q, A, A, A)]
    for scale in (1e-160, 1e-300, 1e150, 1e300):                              # products that underflow or overflow
        for _ in range(10):
            q, A, B, C = g.uniform(-1, 1, (4, 3)) * scale
            pairs += [(q, A, B, C), (q * 1e-5, A, B, C), (q, A, A, B)]
    return pairs


def test_p1_to_p4():
    for q, A, B, C in _property_pairs():
        c, d2, number = R.pair_scalar(q, A, B, C)
        lo, hi = np.minimum(np.minimum(A, B), C), np.maximum(np.maximum(A, B), C)
        assert all(math.isfinite(x) for x in c) and not math.isnan(d2), (q, A, B, C)                    # P1
        if max(np.abs(np.concatenate((q, A, B, C)))) < 1e153:
            assert math.isfinite(d2)
        assert all(lo[k] <= c[k] <= hi[k] for k in range(3))                                             # P2
        assert bits(d2) == bits(R._sqdist([float(x) for x in q], c))                                     # P3
        assert all(d2 <= R._sqdist([float(x) for x in q], [float(x) for x in P]) for P in (A, B, C))    # P4
        assert 1 <= number <= 7


def test_p4_against_the_vertices_of_a_mesh():
    """The search's sqdist is at most the least point-to-point expression over the named vertices, computed directly."""
    for name in ("soup", "degenerate", "far_queries", "spanning"):
        v, f, q = R.cases()[name]
        d = q[:, None, :] - v[np.unique(f)][None]
        vertex = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).min(axis=1)
        assert (R.brute(q, v, f)[2] <= vertex).all(), name


# a query far above a corner of a small triangle, its foot just inside: q, A, B, C
FLAW = [float.fromhex(x) for x in (
    "-0x1.c9abac27d76f0p+8", "0x1.a47256bc473f8p+9", "-0x1.1f4315ceaf79bp+8", "-0x1.8bd08b0ec9360p-4", "-0x1.9c5e852439dc0p-1", "-0x1.385159b582758p-1",
    "-0x1.8c86f15ec4e11p-4", "-0x1.9c8c137bc316fp-1", "-0x1.38b2b8d8a3ed6p-1", "-0x1.8fb4e02af34a6p-4", "-0x1.9cc40bfd62087p-1", "-0x1.38b4a98dc9376p-1")]


def test_four_candidates_alone_break_p4():
    """The flaw include/vfn.h records: without the vertices as candidates the routine can answer with a d2 ABOVE a vertex's."""
    q, A, B, C = (FLAW[3 * k:3 * k + 3] for k in range(4))
    assert R.pair_scalar(q, A, B, C, candidates=4)[1] > R._sqdist(q, A)
    c, d2, number = R.pair_scalar(q, A, B, C)
    assert d2 == R._sqdist(q, A) and number == 5 and list(c) == A
    g = np.random.default_rng(1)
    found = 0
    for _ in range(400):
        A, d, e = g.uniform(-1, 1, 3), g.uniform(-1, 1, 3) * 1e-3, g.uniform(-1, 1, 3) * 1e-3
        up = np.cross(d, e) / np.linalg.norm(np.cross(d, e))
        t = 10 ** g.uniform(-9, -2)
        q = A + float(10 ** g.integers(0, 5)) * up + t * d + t * e
        four, seven = R.pair_scalar(q, A, A + d, A + e, candidates=4)[1], R.pair_scalar(q, A, A + d, A + e)[1]
        least = min(R._sqdist(q, P) for P in (A, A + d, A + e))
        found += four > least
        assert seven <= least and seven <= four
    assert found > 0


def test_p5_the_unit_cube_on_a_dyadic_lattice():
    q = R.lattice_queries()
    assert len(q) == 13 ** 3 and len(R.CUBE_F) == 12
    face, closest, sqdist = R.brute(q, R.CUBE_V, R.CUBE_F)
    assert np.array_equal(bits(sqdist), bits(R.cube_surface_sqdist(q)))
    d = q - closest
    assert np.array_equal(bits((d * d).sum(axis=1)), bits(sqdist))                       # exact arithmetic: any association
    on_surface = ((closest == 0) | (closest == 1)).any(axis=1) & (closest >= 0).all(axis=1) & (closest <= 1).all(axis=1)
    assert on_surface.all() and (face >= 0).all()


@pytest.mark.parametrize("family", sorted(MEASURED_RELATIVE))
def test_accuracy_against_the_exact_oracle(family):
    relative, absolute = R.accuracy_errors(R.accuracy_pairs()[family])
    print(f"{family}: relative {relative!r}, absolute / edge^2 {absolute!r}")
    assert absolute <= 8 * MEASURED_ZERO[family]
    if MEASURED_RELATIVE[family] is not None:
        assert relative <= 8 * MEASURED_RELATIVE[family]
    else:
        overall = R.absolute_error(R.accuracy_pairs()[family])
        print(f"{family}: |d2 - exact| / edge^2 over all pairs {overall!r}")
        assert overall <= 8 * MEASURED_NEAR_ABSOLUTE
    exact_zero = sum(R.exact_sqdist(*p) == 0 for p in R.accuracy_pairs()[family])
    assert exact_zero == EXACT_ZEROS.get(family, 0)


def test_the_exact_oracle_knows_every_region():
    A, B, C = [0.0, 0, 0], [4.0, 0, 0], [0.0, 4, 0]
    for q, want in (([-1, -1, 0], 2), ([5, -1, 0], 2), ([-1, 5, 0], 2), ([2, -3, 0], 9), ([-3, 2, 0], 9), ([4, 4, 0], 8), ([1, 1, 5], 25),
                    ([1, 1, 0], 0), ([2, 2, 3], 9)):
        assert R.exact_sqdist([float(x) for x in q], A, B, C) == want, q


# ---------------------------------------------------------------------------------------------------------------------------------
# the pair routine of csrc/vfn_proximity_core.h on the host, under a sanitizer, before any card sees it
# ---------------------------------------------------------------------------------------------------------------------------------
def _build_host_program(tmp_path):
    compiler = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    source = os.path.join(REPO, "tests", "c_abi", "proximity_core_host.cpp")
    exe = str(tmp_path / "proximity_core_host")
    base = [compiler, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", source, "-o", exe]
    build = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if build.returncode != 0:          # a machine without the sanitizers' runtime: the plain program (an error in the text fails it too)
        build = subprocess.run(base, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def test_pair_routine_on_the_host_equals_the_restatement(tmp_path):
    exe = _build_host_program(tmp_path)
    pairs = _property_pairs() + [tuple(FLAW[3 * k:3 * k + 3] for k in range(4))]
    v, f, q = R.cases()["special_positions"]
    pairs += [(p, v[t[0]], v[t[1]], v[t[2]]) for p in q for t in f]
    pairs += [(p, R.CUBE_V[t[0]], R.CUBE_V[t[1]], R.CUBE_V[t[2]]) for p in R.lattice_queries()[::11] for t in R.CUBE_F]
    nan = np.array([0.5, np.nan, 0.25])
    pairs.append((nan, v[0], v[1], v[2]))
    text = f"{len(pairs)}\n" + "".join(" ".join(float(x).hex() for p in pair for x in p) + "\n" for pair in pairs)
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stderr[-2000:])
    got = np.array([[int(x, 16) for x in line.split()] for line in run.stdout.strip().split("\n")], dtype=np.uint64)
    want = np.array([list(bits(c)) + [int(bits(d2)[0])] for c, d2, _ in (R.pair_scalar(*pair) for pair in pairs)], dtype=np.uint64)
    assert got.shape == want.shape == (len(pairs), 4)
    assert np.array_equal(got[:-1], want[:-1])
    assert np.isnan(got[-1:, 3].view(np.float64)).all() and np.isnan(want[-1:, 3].view(np.float64)).all()          # a NaN query: d2 is NaN, never below a best


# ---------------------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_tri_nearest_list"] == ("int", ["const double*", "int64_t", "const double*", "const int32_t*", "int64_t", "const int64_t*", "int64_t",
                                                      "int64_t*", "double*", "double*", "int64_t*", "void*"])
    assert protos["vfn_tri_nearest"][1][-7:] == ["int64_t*", "double*", "double*", "int64_t*", "int64_t*", "int64_t*", "void*"]
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    err = handle.vfn_last_error
    box = (lib.C.c_double * 7)(0, 0, 0, 1, 1, 1, 0.5)
    assert handle.vfn_tri_cell_ranges(None, 0, None, 4, box, 2, 2, 2, None, None, None, None, None, None) != 0 and b"n_vertices 0" in err()
    assert handle.vfn_tri_cell_ranges(None, 4, None, 1 << 31, box, 2, 2, 2, None, None, None, None, None, None) != 0 and b"outside [1, 2^31)" in err()
    assert handle.vfn_tri_cell_ranges(None, 4, None, 4, box, 2, 129, 2, None, None, None, None, None, None) != 0 and b"grid 2 x 129 x 2" in err()
    assert handle.vfn_tri_cell_ranges(None, 4, None, 4, box, 2, 2, 2, None, None, None, None, None, None) != 0 and b"NULL" in err()
    bad_box = (lib.C.c_double * 7)(0, 0, 0, 1, 1, 1, 1e-3)
    assert handle.vfn_tri_cell_ranges(None, 4, None, 4, bad_box, 2, 2, 2, None, None, None, None, None, None) != 0 and b"the box" in err()
    assert handle.vfn_tri_cell_pairs(None, None, None, None, 4, 8, 2, 2, 2, 1 << 31, None, None, None, None) != 0 and b"n_pairs" in err()
    assert handle.vfn_tri_cell_pairs(None, None, None, None, 4, -1, 2, 2, 2, 8, None, None, None, None) != 0 and b"big_face_cells -1" in err()
    assert handle.vfn_tri_cell_pairs(None, None, None, None, 4, 8, 2, 2, 2, 8, None, None, None, None) != 0 and b"NULL" in err()
    nearest = lambda *, n=4, nf=4, n_pairs=8, n_large=0, rings=8: handle.vfn_tri_nearest(  # noqa: E731
        None, n, None, nf, None, n_pairs, None, None, n_large, box, 2, 2, 2, rings, None, None, None, None, None, None, None, None)
    assert nearest(n=0) != 0 and b"n 0 / n_faces 4" in err()
    assert nearest(nf=1 << 31) != 0 and b"outside [1, 2^31)" in err()
    assert nearest(n_pairs=1 << 31) != 0 and b"n_pairs" in err()
    assert nearest(n_large=5) != 0 and b"n_large 5" in err()
    assert nearest(rings=-1) != 0 and b"max_rings -1" in err()
    assert nearest() != 0 and b"NULL" in err()
    assert handle.vfn_tri_nearest_list(None, 4, None, None, 4, None, 5, None, None, None, None, None) != 0 and b"count 5 outside [1, n = 4]" in err()
    assert handle.vfn_tri_nearest_list(None, 4, None, None, 4, None, 4, None, None, None, None, None) != 0 and b"NULL" in err()


def test_build_recipe_and_texts():
    build = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "build.sh")).read()
    assert re.search(r'^UNITS=".*\bvfn_proximity\b.*"', build, flags=re.M)
    assert re.search(r"\|vfn_proximity[|)].*-ffp-contract=off", build)
    unit = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "vfn_proximity.hip")).read()
    # ONE text of the pair routine for the device and the host program; the only atomicAdd is the integer one on the leftover count
    assert '#include "vfn_proximity_core.h"' in unit and unit.count("atomicAdd(") == 1 and "atomicAdd(leftover_count, 1ull)" in unit
    assert "__shared__" not in unit and "WHY THE GRID CANNOT CHANGE A BIT" in unit and "(a)-(e)" in unit
    assert "vfn_proximity_core.h" in open(os.path.join(REPO, "tests", "c_abi", "proximity_core_host.cpp")).read()
    core = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "vfn_proximity_core.h")).read()
    assert "fmin" not in core.split("#pragma once")[1] and "fmax" not in core.split("#pragma once")[1]
    header = open(lib.HEADER_PATH).read()
    for word in ("vfn_closest_on_triangle", "P1 ", "P2 ", "P3 ", "P4 ", "P5 ", "verified against neither"):
        assert word in header, word
    for doc in (metrics3d.closest_point.__doc__, open(os.path.join(REPO, "README.md")).read()):
        assert "as remembered" in doc and "verified against neither" in doc
    readme = open(os.path.join(REPO, "README.md")).read()
    for word in ("barycentric", "signed distance", "ray queries", "hole filling"):
        assert word in readme, word


def test_signatures_and_defaults():
    assert list(inspect.signature(metrics3d.closest_point).parameters) == ["mesh", "points", "search", "max_rings", "cells", "big_face_cells", "device"]
    defaults = {k: p.default for k, p in inspect.signature(metrics3d.closest_point).parameters.items()}
    assert defaults["search"] == "grid" and defaults["max_rings"] == metrics3d.MAX_RINGS and defaults["cells"] is None and defaults["big_face_cells"] is None
    assert metrics3d.ClosestPoint._fields == ("points", "sqdist", "distance", "face")
    assert list(inspect.signature(metrics3d.triangle_grid).parameters)[:3] == ["mesh", "cells", "big_face_cells"]
    assert list(inspect.signature(metrics3d.surface_distances).parameters)[:3] == ["points", "mesh", "search"]
    deviation = inspect.signature(metrics3d.surface_deviation).parameters
    assert list(deviation)[:6] == ["mesh_a", "mesh_b", "num_points", "generator", "uniforms", "vertices"] and deviation["vertices"].default is False
    for fn in (metrics3d.chamfer_distance, metrics3d.score_mesh, metrics3d.normal_consistency, refuse.metrics_3d):
        assert inspect.signature(fn).parameters["surface"].default == "samples", fn.__name__
    assert metrics3d.SURFACES == ("samples", "mesh")


TRI_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.array([[0, 1, 2]])
TRI = (TRI_V, TRI_F)
PTS = np.zeros((2, 3))


@pytest.mark.parametrize("call", [
    lambda: metrics3d.closest_point(TRI, PTS, search="kd"),
    lambda: metrics3d.closest_point(TRI, PTS, max_rings=-1),
    lambda: metrics3d.closest_point(TRI, PTS, max_rings=1.5),
    lambda: metrics3d.closest_point(TRI, PTS, cells=0),
    lambda: metrics3d.closest_point(TRI, PTS, cells=129),
    lambda: metrics3d.closest_point(TRI, PTS, big_face_cells=-1),
    lambda: metrics3d.closest_point(TRI, PTS, big_face_cells=True),
    lambda: metrics3d.closest_point(TRI, np.zeros((0, 3))),
    lambda: metrics3d.closest_point(TRI, np.zeros((2, 2))),
    lambda: metrics3d.closest_point((TRI_V, np.zeros((0, 3), dtype=np.int64)), PTS),
    lambda: metrics3d.closest_point((TRI_V[:, :2], TRI_F), PTS),
    lambda: metrics3d.triangle_grid(TRI, cells=200),
    lambda: metrics3d.triangle_grid(TRI, big_face_cells=2.5),
    lambda: metrics3d.triangle_grid((np.zeros((0, 3)), TRI_F)),
    lambda: metrics3d.surface_distances(PTS, TRI, search=None),
    lambda: metrics3d.surface_deviation(TRI, TRI, num_points=0),
    lambda: metrics3d.surface_deviation(TRI, TRI, vertices=1),
    lambda: metrics3d.surface_deviation(TRI, TRI, search="octree"),
    lambda: metrics3d.score_mesh(TRI, TRI, num_points=4, surface="faces"),
    lambda: metrics3d.chamfer_distance(TRI, TRI, num_points=4, surface=None),
    lambda: metrics3d.normal_consistency(TRI, TRI, num_points=4, surface="Mesh"),
    lambda: refuse.metrics_3d(TRI, TRI, np.eye(3), np.eye(4)[None], 4, 4, surface="both"),
    lambda: metrics3d._check_pair_count(1 << 31, (128, 128, 128), 64),
])
def test_bad_arguments_raise_before_any_device_call(call, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(metrics3d, "_device", no_device)
    monkeypatch.setattr(metrics3d.geomargs, "device", no_device)
    with pytest.raises(ValueError):
        call()


def test_the_pair_count_refusal_names_cells():
    with pytest.raises(ValueError, match="`cells`"):
        metrics3d._check_pair_count(1 << 31, (128, 128, 128), 64)
    assert metrics3d._check_pair_count((1 << 31) - 1, (128, 128, 128), 64) == (1 << 31) - 1


def test_binding_refuses_shapes_before_the_device():
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)          # noqa: E731
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64)          # noqa: E731
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)          # noqa: E731
    box, dims = (0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0), (1, 1, 1)
    with pytest.raises(lib.VfnError, match="tri_cell_ranges: vertices must be"):
        lib.tri_cell_ranges(f64(3, 2), i64(1, 3), box, dims, i64(1))
    with pytest.raises(lib.VfnError, match="tri_cell_pairs: cell_lo"):
        lib.tri_cell_pairs(i32(2, 3), i32(1, 3), i32(1), i64(1), 8, dims, 1, i64(1))
    grid = (f64(1, 9), i32(1), i32(1), i32(2), i64(0), box, dims)
    with pytest.raises(lib.VfnError, match="tri_nearest: max_rings"):
        lib.tri_nearest(f64(2, 3), grid, -1, 3)
    with pytest.raises(lib.VfnError, match="tri_nearest: queries must be"):
        lib.tri_nearest(f64(2, 2), grid, 8, 3)
    with pytest.raises(lib.VfnError, match="tri_nearest: cell_start"):
        lib.tri_nearest(f64(2, 3), (f64(1, 9), i32(1), i32(1), i32(3), i64(0), box, dims), 8, 3)
    with pytest.raises(lib.VfnError, match="tri_nearest_list: tri must be"):
        lib.tri_nearest_list(f64(2, 3), f64(1, 9), i32(2), i64(2), 2, i64(2), f64(2, 3), f64(2), i64(1))
    # host tensors never reach the library: there is no CPU path
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.tri_cell_ranges(f64(3, 3), i64(1, 3), box, dims, i64(1))
    lib.proximity_check(0, 3)
    with pytest.raises(lib.VfnError, match=r"outside \[0, 3\)"):
        lib.proximity_check(2, 3)
    with pytest.raises(lib.VfnError, match="non-finite"):
        lib.proximity_check(1, 3)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is visible: the calls would run")
def test_no_cpu_fallback():
    with pytest.raises(lib.VfnError, match="no GPU"):
        metrics3d.closest_point(TRI, PTS)
    with pytest.raises(lib.VfnError, match="no GPU"):
        metrics3d.surface_deviation(TRI, TRI, vertices=True)
    with pytest.raises(lib.VfnError, match="no GPU"):
        metrics3d.triangle_grid(TRI)
