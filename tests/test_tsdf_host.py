"""TSDF fusion, host side: the new entry points are declared, bound and linked; the NumPy restatement (tests/tsdf_restatement.py) on a
hand-set volume and on an analytic sphere; the argument checks that run before any launch."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, tsdf  # noqa: E402
import tsdf_restatement as R  # noqa: E402

NEW_EXPORTS = ("vfn_tsdf_integrate", "vfn_tsdf_count", "vfn_tsdf_emit")


def tables():
    _, edge_vertex, tri = lib.mesh_tables()
    return tri, edge_vertex


def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_tsdf_integrate"] == ("int", ["float*", "float*", "int32_t", "int32_t", "int32_t", "float", "float", "float", "float", "float",
                                                    "const float*", "int32_t", "int32_t", "const float*", "const float*", "int32_t", "void*"])
    assert lib.header_abi_version() == 5
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    for name in NEW_EXPORTS:
        assert getattr(handle, name).argtypes is not None
    # the argument checks of the exports answer before any launch: no device is needed to be refused
    assert handle.vfn_tsdf_integrate(None, None, 0, 1, 1, 0.0, 0.0, 0.0, 1.0, 1.0, None, 1, 1, None, None, 1, None) != 0
    assert b"dims" in handle.vfn_last_error()
    assert handle.vfn_tsdf_emit(None, None, 2, 2, 2, 0.0, 0.0, 0.0, -1.0, None, None, None, None) != 0
    assert b"voxel_length" in handle.vfn_last_error()


def test_hand_set_cell_gives_one_triangle():
    """A 2x2x2 volume, corner 0 inside (tsdf -0.25), the others outside (+0.75): case 1, the table's single triangle on edges 0, 8, 3 —
    towards corners 1 = (0,1,0), 4 = (0,0,1), 3 = (1,0,0) — each vertex a quarter of a voxel from corner 0's centre."""
    t = np.full((2, 2, 2), 0.75, dtype=np.float32)
    t[0, 0, 0] = -0.25
    w = np.ones((2, 2, 2), dtype=np.float32)
    origin, vl = (1.0, 2.0, 3.0), 0.5
    v, f = R.extract(t, w, origin, vl, tables())
    c = np.array(origin) + 0.25                       # the centre of voxel (0,0,0)
    assert np.array_equal(f, [[0, 1, 2]])
    assert np.array_equal(v, [c + [0, 0.125, 0], c + [0, 0, 0.125], c + [0.125, 0, 0]])
    # one unobserved corner voids the cell
    w[1, 0, 1] = 0
    v, f = R.extract(t, w, origin, vl, tables())
    assert v.shape == (0, 3) and f.shape == (0, 3)
    # exactly 0 counts as outside: no crossing at all when the only negative corner becomes 0
    t[0, 0, 0] = 0
    v, f = R.extract(t, np.ones_like(w), origin, vl, tables())
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_vertices_merge_at_a_zero_corner_and_faces_stay():
    """Voxel (0,1,0) exactly 0 (outside) between two negative voxels: the cut edges that end at it from either side put their vertex
    ON its centre, from two different cells — one vertex after the merge, used by both triangles."""
    t = np.full((2, 3, 2), 0.5, dtype=np.float32)
    t[0, 0, 0] = t[0, 2, 0] = -0.5
    t[0, 1, 0] = 0.0
    w = np.ones_like(t)
    v, f = R.extract(t, w, (0.0, 0.0, 0.0), 1.0, tables())
    assert f.shape == (2, 3) and v.shape == (5, 3)              # six slots, one shared
    assert len(np.unique(v, axis=0)) == len(v)
    on_corner = np.flatnonzero(np.all(v == [0.5, 1.5, 0.5], axis=1))
    assert len(on_corner) == 1 and (f == on_corner[0]).any(axis=1).all()


def test_restatement_keeps_float32_and_rounds_per_view():
    s = R.sphere_scene()
    one, w1 = s.fused(slice(0, 1))
    assert one.dtype == np.float32 and w1.dtype == np.float32
    allv, wall = s.fused()
    # V single-view calls are the definition of one V-view call
    t, w = np.zeros(s.dims, dtype=np.float32), np.zeros(s.dims, dtype=np.float32)
    for i in range(len(s.depths)):
        R.integrate_view(t, w, s.origin, s.vl, s.trunc, s.depths[i], s.k4s[i], s.e12s[i])
    assert np.array_equal(t.view(np.uint32), allv.view(np.uint32)) and np.array_equal(w, wall)
    assert wall.max() >= 3 and set(np.unique(wall)) <= set(float(i) for i in range(8))
    with pytest.raises(AssertionError):
        R.f32(np.float32(1.0) * 2.5 * np.ones(2))               # the widening check is alive


def test_restatement_describes_the_sphere():
    """The analytic scene of the contract: a sphere of radius 0.5, 7 look-at cameras, 48 x 64 maps, dims (32,32,29) over [-0.7, 0.7],
    truncation three voxels.  Every vertex of the extracted surface lies near the sphere: median <= 0.25 voxel, max <= 1.5 voxel — a
    check that the restatement describes a surface (the prototype gave 0.10 / 0.88), not a device tolerance."""
    s = R.sphere_scene()
    t, w = s.fused()
    observed = int((w > 0).sum())
    v, f = R.extract(t, w, s.origin, s.vl, tables())
    err = np.abs(np.linalg.norm(v, axis=1) - 0.5) / s.vl
    print(f"observed voxels {observed} of {t.size}, vertices {len(v)}, faces {len(f)}, |r - 0.5| median {np.median(err):.3f} max {err.max():.3f} voxel")
    assert observed > t.size // 4 and len(v) > 1000
    assert (f < len(v)).all() and f.min() == 0
    assert np.median(err) <= 0.25 and err.max() <= 1.5


def test_room_scene_takes_every_branch():
    s = R.room_scene()
    t, w = s.fused()
    x = R.centres(s.origin[0], s.dims[0], s.vl)[:, None, None]
    y = R.centres(s.origin[1], s.dims[1], s.vl)[None, :, None]
    z = R.centres(s.origin[2], s.dims[2], s.vl)[None, None, :]
    e = s.e12s[0].astype(np.float64)
    zc = e[8] * x + e[9] * y + e[10] * z + e[11]
    assert (zc <= 0).any() and (zc > 0).any()                   # voxels behind the first camera
    assert (w == 0).any() and (w >= 2).any() and (t == 1).any() and (t < 0).any()
    v, f = R.extract(t, w, s.origin, s.vl, tables())
    # every vertex lies near a wall of the box
    wall = np.abs(np.abs(v).max(axis=1) - 0.6) / s.vl
    assert len(f) > 500 and np.median(wall) <= 0.25


def test_reference_depth_statement_and_refusals():
    d = np.array([[0.0, 0.0004, 1.2345678, 9.9994], [9.9996, 10.0, 12.5, 65.535]], dtype=np.float32)
    got = tsdf.reference_depth(d)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), R.reference_depth(d))
    assert np.array_equal(got.numpy(), np.array([[0, 0, 1.234, 9.999], [9.999, 0, 0, 0]], dtype=np.float32))
    assert np.array_equal(tsdf.reference_depth(torch.from_numpy(d)).numpy(), got.numpy())
    for bad in (np.nan, np.inf, -0.5, 65.536, 70.0):
        with pytest.raises(ValueError):
            tsdf.reference_depth(np.array([[1.0, bad]], dtype=np.float32))


def test_arguments_are_refused_before_any_launch():
    depth = np.ones((2, 4, 5), dtype=np.float32)
    k = np.array([[4.0, 0, 2], [0, 4, 1.5], [0, 0, 1]], dtype=np.float32)
    poses = np.tile(np.eye(4), (2, 1, 1))
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            tsdf.TSDFVolume((0, 0, 0), (4, 4, 4), voxel_length=bad)
        with pytest.raises(ValueError):
            tsdf.TSDFVolume((0, 0, 0), (4, 4, 4), sdf_trunc=bad)
    for dims in ((0, 4, 4), (4, 4), (4, 4, -1), (2.5, 4, 4), (2048, 1024, 1024)):
        with pytest.raises(ValueError):
            tsdf.TSDFVolume((0, 0, 0), dims)
    with pytest.raises(ValueError):
        tsdf.TSDFVolume((0, 0), (4, 4, 4))
    bounds = ((-1, -1, -1), (1, 1, 1))
    with pytest.raises(ValueError):
        tsdf.fuse_depth_maps(depth, k, poses[:1], bounds=bounds)                        # one pose for two maps
    with pytest.raises(ValueError):
        tsdf.fuse_depth_maps(depth, np.tile(k, (3, 1, 1)), poses, bounds=bounds)         # three intrinsics for two maps
    with pytest.raises(ValueError):
        tsdf.fuse_depth_maps(depth, k[:2], poses, bounds=bounds)                        # intrinsics not square
    with pytest.raises(ValueError):
        tsdf.fuse_depth_maps(depth.reshape(-1), k, poses, bounds=bounds)                # depth not a map
    singular = poses.copy()
    singular[1, :3, :3] = 0
    with pytest.raises(ValueError):
        tsdf.fuse_depth_maps(depth, k, singular, bounds=bounds)
    for bad in (np.nan, np.inf, -1.0):
        d = depth.copy()
        d[1, 2, 3] = bad
        with pytest.raises(ValueError):
            tsdf.fuse_depth_maps(d, k, poses, bounds=bounds)
    with pytest.raises(ValueError):
        tsdf.fuse_depth_maps(depth, k, poses, bounds=((1, 1, 1), (0, 2, 2)))
    with pytest.raises(ValueError):
        tsdf.fuse_depth_maps(depth, k, poses, bounds=bounds, voxel_length=1e-4)         # 8e12 voxels
    e = tsdf.extrinsics_from_poses(poses, 2)
    assert e.dtype == torch.float32 and tuple(e.shape) == (2, 12)
    assert np.array_equal(tsdf.split_intrinsics(k, 2).numpy(), [[4, 4, 2, 1.5]] * 2)
    if not torch.cuda.is_available():
        with pytest.raises(lib.VfnError):
            tsdf.TSDFVolume((0, 0, 0), (4, 4, 4))                                       # no device: no fallback
        with pytest.raises(lib.VfnError):
            tsdf.fuse_depth_maps(depth, k, poses, bounds=bounds)
        with pytest.raises(lib.VfnError):
            lib.tsdf_integrate(torch.zeros(2, 2, 2), torch.zeros(2, 2, 2), (0, 0, 0), 1.0, 1.0, torch.zeros(1, 2, 2), torch.zeros(1, 4),
                               torch.zeros(1, 12))
