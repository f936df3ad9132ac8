"""Depth rasteriser and Laplacian smoothing, host side: the new entry points are declared, bound and linked; their argument checks answer
before any launch; the Python surface refuses before it asks for a device; the NumPy restatement (tests/raster_restatement.py) on
hand-set cases whose answers are known without it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, raster, refuse  # noqa: E402
import raster_restatement as R  # noqa: E402

NEW_EXPORTS = ("vfn_raster_depth", "vfn_smooth_laplacian_step")
EYE = R.extrinsic(np.eye(4))
K = np.array([8.0, 8.0, 4.0, 4.0], dtype=np.float32)            # fx fy cx cy: with pixel_centre 0 the ray of pixel (u, v) is ((u - 4) / 8, (v - 4) / 8, 1)


def one_view(v, f, h=9, w=9, c=0.0, k4=K, e12=EYE, **kw):
    return R.rasterize_view(np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64).reshape(-1, 3), k4, e12, h, w, c=c, **kw)


def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_raster_depth"] == ("int", ["const double*", "int64_t", "const int64_t*", "int64_t", "const float*", "const float*", "int32_t",
                                                  "int32_t", "int32_t", "float", "float", "float", "float*", "int64_t*", "void*"])
    assert protos["vfn_smooth_laplacian_step"] == ("int", ["const double*", "double*", "int64_t", "const int64_t*", "const int64_t*", "int64_t",
                                                           "double", "int64_t*", "void*"])
    assert lib.header_abi_version() == 5
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    assert handle.vfn_abi_version() == 5
    for name in NEW_EXPORTS:
        assert getattr(handle, name).argtypes is not None


def test_export_argument_checks_answer_before_any_launch():
    """No device is needed to be refused: every call below returns from the checks that precede the first launch."""
    handle = lib.load()

    def call(n=3, m=1, views=1, h=4, w=4, near=0.05, far=100.0, c=0.5):
        return handle.vfn_raster_depth(None, n, None, m, None, None, views, h, w, near, far, c, None, None, None)

    for kw, word in (({"h": 0}, b"bad views"), ({"w": 0}, b"bad views"), ({"views": -1}, b"bad views"), ({"far": 0.05}, b"near"),
                     ({"far": 0.01}, b"near"), ({"near": 0.0}, b"near"), ({"far": float("inf")}, b"near"), ({"near": float("nan")}, b"near"),
                     ({"c": float("nan")}, b"pixel_centre"), ({"c": float("inf")}, b"pixel_centre"),
                     ({"views": 1024, "h": 1024, "w": 2048}, b"2^31"), ({"views": 1, "h": 65536, "w": 32768}, b"2^31"),
                     ({"m": 1 << 31}, b"2^31"), ({"n": -1}, b"2^31"), ({}, b"NULL")):
        assert call(**kw) == -1, kw
        assert word in handle.vfn_last_error(), (kw, handle.vfn_last_error())
    assert call(views=0) == 0                                         # no view: nothing to do, nothing launched
    assert handle.vfn_smooth_laplacian_step(None, None, 1 << 31, None, None, 0, 0.5, None, None) == -1
    assert handle.vfn_smooth_laplacian_step(None, None, 4, None, None, 0, float("nan"), None, None) == -1
    assert b"lam" in handle.vfn_last_error()
    assert handle.vfn_smooth_laplacian_step(None, None, 4, None, None, 0, 0.5, None, None) == -1
    assert b"NULL" in handle.vfn_last_error()
    assert handle.vfn_smooth_laplacian_step(None, None, 0, None, None, 0, 0.5, None, None) == 0


def test_python_checks_raise_before_a_device_is_asked_for():
    v = np.array([[0.0, 0, 2], [1, 0, 2], [0, 1, 2]])
    f = np.array([[0, 1, 2]])
    k = np.array([[8.0, 0, 4], [0, 8, 4], [0, 0, 1]], dtype=np.float32)
    pose = np.eye(4)[None]
    ok = dict(intrinsics=k, poses=pose, height=9, width=9)
    for bad in ({"height": 0}, {"width": -3}, {"height": 2.5}, {"near": 1.0, "far": 1.0}, {"near": 2.0, "far": 1.0}, {"near": 0.0},
                {"far": float("inf")}, {"pixel_centre": float("nan")}, {"pixel_centre": float("inf")}, {"height": 1 << 16, "width": 1 << 15},
                {"poses": np.eye(4)[None].repeat(2, 0)[:, :3]}, {"intrinsics": k[:2]}, {"poses": np.zeros((1, 4, 4))}):
        with pytest.raises(ValueError):
            raster.rasterize_depth(v, f, **{**ok, **bad})
    for bad_v, bad_f in ((v[:, :2], f), (v.astype(np.int64), f), (v, f.astype(np.float64)), (v, f[:, :2])):
        with pytest.raises(ValueError):
            raster.rasterize_depth(bad_v, bad_f, **ok)
    with pytest.raises(TypeError):
        raster.rasterize_depth("mesh", None, **ok)
    with pytest.raises(ValueError):
        refuse.refuse((v, f), k, pose, 9, 9, depth_trunc=0.0)
    with pytest.raises(ValueError):
        refuse.refuse((v, f), k, pose, 9, 9, bounds=((1, 1, 1), (0, 2, 2)), voxel_length=-1.0)
    for bad in ({"iterations": -1}, {"iterations": 2.5}, {"lam": float("nan")}):
        with pytest.raises(ValueError):
            refuse.smooth_laplacian((v, f), **bad)
    if not torch.cuda.is_available():                                   # no device: no fallback
        with pytest.raises(lib.VfnError):
            raster.rasterize_depth(v, f, **ok)
        with pytest.raises(lib.VfnError):
            raster.rasterize_depth(v, np.zeros((0, 3), dtype=np.int64), **ok)
        with pytest.raises(lib.VfnError):
            refuse.smooth_laplacian((v, f))
        with pytest.raises(lib.VfnError):
            refuse.refuse((v, f), k, pose, 9, 9)
        with pytest.raises(lib.VfnError):
            lib.raster_depth(torch.zeros(3, 3, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int64), torch.ones(1, 4), torch.ones(1, 12), 4, 4,
                             0.05, 100.0, 0.5)


def test_one_dyadic_triangle_covers_exactly_the_expected_pixels():
    """The triangle (-1,-1,2) (1,-1,2) (-1,1,2): rays x = (u - 4) / 8, y = (v - 4) / 8 hit it at (2x, 2y, 2); inside iff 2x >= -1,
    2y >= -1 and 2x + 2y <= 0 — edges inclusive — i.e. u >= 0, v >= 0, u + v <= 8.  Every number is dyadic: no rounding anywhere."""
    tri = [[-1.0, -1, 2], [1, -1, 2], [-1, 1, 2]]
    d = one_view(tri, [0, 1, 2])
    vv, uu = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    want = np.where(uu + vv <= 8, np.float32(2.0), np.float32(0.0))
    assert d.dtype == np.float32 and np.array_equal(d, want)
    assert np.array_equal(one_view(tri, [0, 2, 1]), want)               # the other winding: no face is culled


def test_centres_on_a_shared_edge_and_on_a_vertex_are_covered():
    """Two faces sharing the edge x = 0 (pixel column u = 4), four sharing the vertex (0, 0, 2) (pixel (4, 4)): each alone covers the
    edge (inclusive), together no pixel is lost; a centre on the shared vertex is covered by all four."""
    v = [[0.0, -1, 2], [0, 1, 2], [-1, 0, 2], [1, 0, 2], [0, 0, 2]]
    left, right = one_view(v, [0, 1, 2]), one_view(v, [1, 0, 3])
    assert (left[:, 4] == 2).sum() == 9 and (right[:, 4] == 2).sum() == 9       # y from -0.5 to 0.5 on the edge: inside both
    both = one_view(v, [[0, 1, 2], [1, 0, 3]])
    assert np.array_equal(both, np.maximum(left, right)) and both[4, 4] == 2
    fan = [[4, 0, 3], [4, 3, 1], [4, 1, 2], [4, 2, 0]]
    for f in fan:
        assert one_view(v, f)[4, 4] == 2, f
    assert np.array_equal(one_view(v, fan), both)


def test_faces_that_give_nothing():
    behind = [[-1.0, -1, -2], [1, -1, -2], [-1, 1, -2]]
    assert not one_view(behind, [0, 1, 2]).any()
    edge_on = [[0.0, 0, 1], [0, 0, 3], [0, 0, 2]]                         # through the optical axis: D = 0
    assert not one_view(edge_on, [0, 1, 2]).any()
    assert not one_view(behind, [0, 0, 0]).any() and not one_view(behind, [0, 1, 1]).any()
    between = [[0.03, 0.03, 2], [0.2, 0.03, 2], [0.03, 0.2, 2]]          # x, y in (0, 0.25) at depth 2: between the centres 4 and 5
    counts = {}
    assert not one_view(between, [0, 1, 2], counts=counts).any() and counts["off_screen"] == 0 and counts["fragments"] == 0
    too_near, too_far = [[-1.0, -1, 0.04], [1, -1, 0.04], [-1, 1, 0.04]], [[-1.0, -1, 101], [1, -1, 101], [-1, 1, 101]]
    assert not one_view(too_near, [0, 1, 2]).any() and not one_view(too_far, [0, 1, 2]).any()
    assert not one_view(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)).any()


def test_a_face_through_the_camera_plane_gives_the_ray_plane_depth():
    """The plane z = 1 + x through (-3,-4,-2) (3,-4,4) (0,6,1): it crosses z = 0 and the near plane.  The ray (dx, dy, 1) meets it at
    z = 1 / (1 - dx); inside the triangle for every pixel of the view whose z is at least ``near``."""
    tri = [[-3.0, -4, -2], [3, -4, 4], [0, 6, 1]]
    counts = {}
    d = one_view(tri, [0, 1, 2], counts=counts)
    assert counts["straddling"] == 1
    dx = (np.arange(9) - 4.0) / 8.0
    want = np.broadcast_to((1.0 / (1.0 - dx)).astype(np.float32), (9, 9))
    assert np.array_equal(d, want), (d, want)
    assert np.array_equal(one_view(tri, [0, 1, 2], candidates=False), d)


def test_tessellated_plane_is_exactly_two():
    v, f = R.plane()
    h, w = 48, 64
    for c in (0.0, 0.5):
        d = R.rasterize_view(v, f, R.pinhole(h, w), EYE, h, w, c=c)
        assert np.array_equal(d, np.full((h, w), 2.0, dtype=np.float32)), c


def test_sphere_is_closed_and_the_candidate_rules_change_no_bit():
    v, f = R.icosphere(2)
    assert f.shape == (320, 3)
    h, w = 48, 64
    k4, e12 = R.pinhole(h, w), R.extrinsic(R.look_at((1.3, 1.2, 1.1)))
    d = R.rasterize_view(v, f, k4, e12, h, w)
    hit = d > 0
    assert hit.any() and not hit.all()
    rows = np.flatnonzero(hit.any(axis=1))
    for r in rows:                                                       # no interior hole: every row's hits are one run
        cols = np.flatnonzero(hit[r])
        assert cols[-1] - cols[0] + 1 == len(cols), r
    assert rows[-1] - rows[0] + 1 == len(rows)
    assert np.array_equal(R.rasterize_view(v, f, k4, e12, h, w, candidates=False).view(np.uint32), d.view(np.uint32))


def test_face_permutation_and_rotation_change_no_bit():
    v, f = R.soup(600, seed=3)
    h, w = 30, 40
    k4 = R.pinhole(h, w, 0.6 * w)
    counts = {}
    d = R.rasterize_view(v, f, k4, EYE, h, w, counts=counts)
    print(counts)
    assert counts["z_culled"] > 0 and counts["off_screen"] > 0 and counts["straddling"] > 0 and (d > 0).any()
    g = np.random.default_rng(0)
    shuffled = np.roll(f[g.permutation(len(f))], 1, axis=1)
    assert np.array_equal(R.rasterize_view(v, shuffled, k4, EYE, h, w).view(np.uint32), d.view(np.uint32))
    assert np.array_equal(R.rasterize_view(v, f, k4, EYE, h, w, candidates=False).view(np.uint32), d.view(np.uint32))


def test_camera_inside_a_box_hits_a_wall_in_every_pixel():
    import tsdf_restatement as T
    v, f = R.box(0.6)
    h, w = 30, 40
    k4 = R.pinhole(h, w, 0.6 * w)
    for eye, target in T.ROOM_VIEWS:
        pose = R.look_at(eye, target)
        d = R.rasterize_view(v, f, k4, R.extrinsic(pose), h, w, c=0.0)
        want = T.room_depth(pose, k4, h, w, 0.6)
        assert (d > 0).all() and np.abs(d - want).max() < 1e-6           # (float32 poses against the float64 analytic rays)


def test_smoothing_statement():
    tet = np.array([[0.0, 0, 0], [6, 0, 0], [0, 6, 0], [0, 0, 6]])
    faces = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])
    one = R.smooth_laplacian(tet, faces, iterations=1, lam=0.5)
    assert np.array_equal(one[0], [1.0, 1.0, 1.0])                       # (0,0,0) + 0.5 ((6,6,6) / 3 - (0,0,0))
    assert np.array_equal(R.smooth_laplacian(tet, faces, iterations=0), tet)
    # an isolated vertex stays; duplicate and degenerate faces change no neighbour set
    more_v = np.concatenate([tet, [[9.0, 9, 9]]])
    more_f = np.concatenate([faces, [[0, 1, 2], [2, 1, 0], [3, 3, 3], [1, 1, 2]]])
    assert R.neighbours(more_f, 5) == R.neighbours(faces, 5) == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], []]
    out = R.smooth_laplacian(more_v, more_f, iterations=3)
    assert np.array_equal(out[4], [9.0, 9, 9]) and np.array_equal(out[:4], R.smooth_laplacian(tet, faces, iterations=3))
    # the package's adjacency (torch; runs on any device) builds the same rows
    row_start, nb = refuse.vertex_adjacency(torch.from_numpy(more_f), 5)
    assert row_start.tolist() == [0, 3, 6, 9, 12, 12] and nb.tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]
