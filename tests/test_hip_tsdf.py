"""TSDF fusion on the device (csrc/vfn_tsdf.hip, vf_nerf_amd/tsdf.py) against the NumPy restatement of its contract
(tests/tsdf_restatement.py): tsdf / weight bit for bit with no tolerance and no excluded voxel, vertices bit for bit, faces equal."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import evaluator, lib, metrics3d, synthetic, tsdf  # noqa: E402
import tsdf_restatement as R  # noqa: E402
from helpers import build_model, load_fixture  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

_CACHE = {}


def tables():
    if "tables" not in _CACHE:
        _, edge_vertex, tri = lib.mesh_tables()
        _CACHE["tables"] = (tri, edge_vertex)
    return _CACHE["tables"]


def scene(name):
    """The scene, its restated volume (all views) and the restated mesh: computed once, never written to."""
    if name not in _CACHE:
        s = {"sphere": R.sphere_scene, "room": R.room_scene}[name]()
        t, w = s.fused()
        _CACHE[name] = (s, t, w, R.extract(t, w, s.origin, s.vl, tables()))
    return _CACHE[name]


def device_volume(s, views=slice(None), batched=True):
    vol = tsdf.TSDFVolume(s.origin, s.dims, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    assert vol.origin == s.origin and vol.voxel_length == s.vl and vol.sdf_trunc == s.trunc
    depths, k, poses = s.depths[views], s.intrinsics_matrices()[views], s.poses[views]
    if batched:
        vol.integrate(depths, k, poses)
    else:
        for i in range(len(depths)):
            vol.integrate(depths[i], k[i], poses[i])
    return vol


def assert_volume_bits(vol, t, w, what=""):
    got_t, got_w = vol.tsdf.cpu(), vol.weight.cpu()
    bad = int((got_t.view(torch.int32) != torch.from_numpy(t).view(torch.int32)).sum())
    print(f"{what}: {bad} of {t.size} tsdf words differ, weights equal: {torch.equal(got_w, torch.from_numpy(w))}, observed {int((w > 0).sum())}")
    assert torch.equal(got_t.view(torch.int32), torch.from_numpy(t).view(torch.int32)), what
    assert torch.equal(got_w.view(torch.int32), torch.from_numpy(w).view(torch.int32)), what


def assert_mesh_bits(mesh_dev, mesh_ref, what=""):
    v, f = mesh_dev
    ev, ef = mesh_ref
    assert v.dtype == torch.float64 and f.dtype == torch.int64 and v.is_cuda and f.is_cuda
    assert tuple(v.shape) == ev.shape and tuple(f.shape) == ef.shape, (what, tuple(v.shape), ev.shape, tuple(f.shape), ef.shape)
    assert np.array_equal(v.cpu().numpy().view(np.uint64), ev.view(np.uint64)), what
    assert np.array_equal(f.cpu().numpy(), ef), what
    assert f.numel() == 0 or int(f.max()) < v.shape[0]


@pytest.mark.parametrize("name", ["sphere", "room"])
def test_all_views_equal_the_restatement_bit_for_bit(name):
    s, t, w, ref_mesh = scene(name)
    vol = device_volume(s)
    assert_volume_bits(vol, t, w, f"{name}, {len(s.depths)} views")
    assert (w > 0).sum() > t.size // 4 and (w == 0).any()
    assert_mesh_bits(vol.extract_mesh(), ref_mesh, name)
    assert ref_mesh[1].shape[0] > 500


def test_one_view_equals_the_restatement_bit_for_bit():
    s = scene("sphere")[0]
    t, w = s.fused(slice(0, 1))
    vol = device_volume(s, slice(0, 1))
    assert_volume_bits(vol, t, w, "sphere, 1 view")
    assert_mesh_bits(vol.extract_mesh(), R.extract(t, w, s.origin, s.vl, tables()), "sphere, 1 view")


def test_room_scene_exercises_the_branches():
    s, t, w, _ = scene("room")
    x = R.centres(s.origin[0], s.dims[0], s.vl)[:, None, None].astype(np.float64)
    y = R.centres(s.origin[1], s.dims[1], s.vl)[None, :, None].astype(np.float64)
    z = R.centres(s.origin[2], s.dims[2], s.vl)[None, None, :].astype(np.float64)
    for e, k in zip(s.e12s.astype(np.float64), s.k4s.astype(np.float64)):
        zc = e[8] * x + e[9] * y + e[10] * z + e[11]
        xc = e[0] * x + e[1] * y + e[2] * z + e[3]
        front = zc > 1e-3
        u = np.where(front, xc * k[0] / np.where(front, zc, 1.0) + k[2], 0.0)
        assert (zc <= 0).any() and front.any()                                    # voxels behind the camera
        assert (front & ((u < -1) | (u > s.depths.shape[2]))).any()               # projections outside the image


def test_one_call_of_v_views_equals_v_calls():
    s = scene("sphere")[0]
    one, many = device_volume(s, batched=True), device_volume(s, batched=False)
    assert len(s.depths) == 7
    assert torch.equal(one.tsdf.view(torch.int32), many.tsdf.view(torch.int32)) and torch.equal(one.weight, many.weight)
    one.reset()
    assert not bool(one.tsdf.any()) and not bool(one.weight.any())


EXTRA_EYES = ((-1.2, 1.4, -1.0), (0.3, -1.9, 0.6))


@pytest.mark.parametrize("dims,h,w,n_views", [((1, 1, 1), 1, 1, 1), ((5, 3, 2), 7, 5, 2), ((33, 17, 70), 48, 64, 9), ((32, 32, 29), 5, 7, 9),
                                              ((33, 17, 70), 1, 1, 2), ((5, 3, 2), 48, 64, 1), ((1, 1, 1), 7, 5, 9), ((32, 32, 29), 48, 64, 2)])
def test_shapes_where_indexing_can_go_wrong(dims, h, w, n_views):
    """Volumes of one voxel, of rows shorter than a lane's run, of rows that are no multiple of it (70, 29: the scalar form) and of
    several bricks per axis; maps of one pixel and of odd sizes; 1, 2 and 9 views — with, among nine, a map that is all zero and a
    camera that looks away from the volume."""
    s = R.sphere_scene(dims=dims, h=h, w=w, eyes=(R.SPHERE_EYES + EXTRA_EYES)[:n_views])
    if n_views == 9:
        s.depths[1] = 0.0                                                           # no measurement anywhere
        away = R.look_at((2.0, 0.5, 0.0), (4.0, 0.5, 0.0))                           # the volume is behind this camera
        s.poses[3], s.e12s[3] = away, R.extrinsic(away)
        s.depths[3] = 1.0
    t, wt = s.fused()
    vol = device_volume(s)
    assert_volume_bits(vol, t, wt, f"dims {dims}, maps {h} x {w}, {n_views} views")
    assert_mesh_bits(vol.extract_mesh(), R.extract(t, wt, s.origin, s.vl, tables()), f"dims {dims}")
    if n_views == 9:
        for i in (1, 3):                                                            # those two views alone leave the volume untouched
            only = device_volume(s, slice(i, i + 1))
            assert not bool(only.weight.any()) and not bool(only.tsdf.any())


def test_boundary_decisions():
    """Hand-built voxels on the decisions of the contract.  An identity camera with a 1 x 1 map (fx = fy = 1, cx = cy = 0) of depth 1 and a
    column of voxels on the optical axis (m = 1): zc = 0.25, 0.5, 0.75 (sdf / trunc above and exactly 1: clamped, 1), 1.0 (0), 1.25 (-0.5),
    1.5 (sdf exactly -sdf_trunc: skipped), beyond (skipped)."""
    eye = np.eye(4)
    vol = tsdf.TSDFVolume((-0.125, -0.125, 0.125), (1, 1, 8), voxel_length=0.25, sdf_trunc=0.5, device=DEV)
    depth = np.ones((1, 1), dtype=np.float32)
    k = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]], dtype=np.float32)
    vol.integrate(depth, k, eye)
    assert vol.tsdf.reshape(-1).tolist() == [1.0, 1.0, 0.5, 0.0, -0.5, 0.0, 0.0, 0.0]
    assert vol.weight.reshape(-1).tolist() == [1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    t, w = R.fused((1, 1, 8), vol.origin, 0.25, 0.5, depth[None], [[1, 1, 0, 0]], [R.extrinsic(eye)])
    assert_volume_bits(vol, t, w, "axis column")
    # u + 0.5 exactly on W: a 1 x 2 map, cx = 0.5; the voxel at x = z = 1 projects to (1 + 0.5) + 0.5 = 2 = W (outside), its neighbour at
    # x = 0.75 to 1.75 -> pixel 1 (inside, sdf = 0)
    vol = tsdf.TSDFVolume((0.625, -0.125, 0.875), (2, 1, 1), voxel_length=0.25, sdf_trunc=0.5, device=DEV)
    depth = np.ones((1, 2), dtype=np.float32)
    k = np.array([[1.0, 0, 0.5], [0, 1.0, 0], [0, 0, 1]], dtype=np.float32)
    vol.integrate(depth, k, eye)
    assert vol.weight.reshape(-1).tolist() == [1.0, 0.0] and vol.tsdf.reshape(-1).tolist() == [0.0, 0.0]
    t, w = R.fused((2, 1, 1), vol.origin, 0.25, 0.5, depth[None], [[1, 1, 0.5, 0]], [R.extrinsic(eye)])
    assert_volume_bits(vol, t, w, "u + 0.5 on W")
    # the running mean: a second observation one quarter further gives (1 x 0 + 0.5) / 2 at the voxel the first put on the surface
    vol = tsdf.TSDFVolume((-0.125, -0.125, 0.125), (1, 1, 8), voxel_length=0.25, sdf_trunc=0.5, device=DEV)
    k = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]], dtype=np.float32)
    vol.integrate(np.array([[[1.0]], [[1.25]]], dtype=np.float32), k, np.stack([eye, eye]))
    assert vol.tsdf.reshape(-1).tolist() == [1.0, 1.0, 0.75, 0.25, -0.25, -0.5, 0.0, 0.0]
    assert vol.weight.reshape(-1).tolist() == [2.0, 2.0, 2.0, 2.0, 2.0, 1.0, 0.0, 0.0]


def test_extraction_of_hand_set_volumes():
    vol = tsdf.TSDFVolume((1.0, 2.0, 3.0), (2, 2, 2), voxel_length=0.5, sdf_trunc=1.0, device=DEV)
    vol.tsdf.fill_(0.75)
    vol.tsdf[0, 0, 0] = -0.25
    vol.weight.fill_(1.0)
    v, f = vol.extract_mesh()
    c = np.array([1.25, 2.25, 3.25])
    assert f.tolist() == [[0, 1, 2]] and np.array_equal(v.cpu().numpy(), [c + [0, 0.125, 0], c + [0, 0, 0.125], c + [0.125, 0, 0]])
    vol.weight[1, 0, 1] = 0                                                       # one unobserved corner voids the cell
    v, f = vol.extract_mesh()
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and v.dtype == torch.float64 and f.dtype == torch.int64 and v.is_cuda
    # no crossing: all outside, all inside, and an empty (never integrated) volume
    for value, weight in ((0.5, 1.0), (-0.5, 1.0), (0.0, 0.0)):
        vol.tsdf.fill_(value)
        vol.weight.fill_(weight)
        v, f = vol.extract_mesh()
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
    # a zero between two negative voxels: the two cells' vertices on it merge (tests/test_tsdf_host.py states the expected mesh)
    t = np.full((2, 3, 2), 0.5, dtype=np.float32)
    t[0, 0, 0] = t[0, 2, 0] = -0.5
    t[0, 1, 0] = 0.0
    vol = tsdf.TSDFVolume((0.0, 0.0, 0.0), (2, 3, 2), voxel_length=1.0, sdf_trunc=1.0, device=DEV)
    vol.tsdf.copy_(torch.from_numpy(t))
    vol.weight.fill_(1.0)
    assert_mesh_bits(vol.extract_mesh(), R.extract(t, np.ones_like(t), (0.0, 0.0, 0.0), 1.0, tables()), "zero corner")
    assert vol.extract_mesh()[0].shape[0] == 5


def test_reference_depth_on_the_device():
    g = np.random.default_rng(3)
    d = (g.random((9, 11)) * 12.0).astype(np.float32)
    d[0, :4] = [0.0, 0.0004, 9.9996, 65.535]
    got = tsdf.reference_depth(torch.from_numpy(d).to(DEV))
    assert got.is_cuda and got.dtype == torch.float32 and np.array_equal(got.cpu().numpy(), R.reference_depth(d))
    assert (got == 0).any() and (got > 0).any()
    for bad in (np.nan, -0.5, 65.536):
        x = torch.from_numpy(d).to(DEV).clone()
        x[3, 3] = bad
        with pytest.raises(ValueError):
            tsdf.reference_depth(x)


def test_fuse_depth_maps_finds_its_box():
    s, t, w, ref_mesh = scene("sphere")
    hi = tuple(o + n * s.vl for o, n in zip(s.origin, s.dims))
    v, f = tsdf.fuse_depth_maps(s.depths, s.intrinsics_matrices(), s.poses, bounds=(s.origin, hi), voxel_length=s.vl, sdf_trunc=s.trunc)
    assert tuple(f.shape) == ref_mesh[1].shape                                    # the same box (ceil may add a plane of free space)
    v, f = tsdf.fuse_depth_maps(s.depths, s.intrinsics_matrices(), s.poses, voxel_length=s.vl, sdf_trunc=s.trunc)
    err = (v.norm(dim=1) - 0.5).abs() / s.vl
    assert f.shape[0] > 1000 and float(err.median()) <= 0.25 and float(err.max()) <= 3.0      # (every crossing lies inside the 3-voxel band)
    v, f = tsdf.fuse_depth_maps(np.zeros_like(s.depths), s.intrinsics_matrices(), s.poses)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)


def test_fuse_rendered_views_is_render_then_fuse():
    """Plumbing on the synthetic model (random weights: the geometry means nothing): two views of 16 x 12 pixels rendered and fused in one
    call give the mesh of fuse_depth_maps on the depth maps evaluator.render_view returns for the same views; the result goes straight
    into metrics3d.score_mesh."""
    fx, d = load_fixture("c1_perturb")
    model = build_model(fx, d, device=DEV)
    w, h = 16, 12
    poses = torch.stack([synthetic.orbit_pose(20.0, 8.0, 0.9), synthetic.orbit_pose(-35.0, 15.0, 1.0)])
    k4 = torch.eye(4)
    k4[0, 0] = k4[1, 1] = 15.0
    k4[0, 2], k4[1, 2] = (w - 1) / 2, (h - 1) / 2
    maps = []
    model.rng_seed, model._rng_offset = 5, 0
    for p in poses:
        uv, pose, k = synthetic.pinhole_image(w, h, 15.0, pose=p)
        assert torch.equal(k[0], k4)
        _, depth = evaluator.render_view(model, pose, uv, k, 0)
        maps.append(depth.reshape(h, w))
    maps = np.stack(maps)
    print(f"rendered depth in [{maps.min():.4g}, {maps.max():.4g}], {int((maps < 0).sum())} of {maps.size} below zero")
    assert np.isfinite(maps).all() and maps.max() > 0.05
    maps = np.maximum(maps, np.float32(0))                     # a negative rendered depth is no measurement (fuse_rendered_views)
    want = tsdf.fuse_depth_maps(tsdf.reference_depth(maps), k4, poses, voxel_length=0.05, sdf_trunc=0.15)
    model.rng_seed, model._rng_offset = 5, 0
    got = tsdf.fuse_rendered_views(model, poses, k4, h, w, 0, voxel_length=0.05, sdf_trunc=0.15)
    assert got[1].shape[0] > 0 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    model.rng_seed, model._rng_offset = 5, 0
    raw = tsdf.fuse_rendered_views(model, poses, k4[:3, :3], h, w, 0, voxel_length=0.05, sdf_trunc=0.15, as_reference=False)
    want_raw = tsdf.fuse_depth_maps(maps, k4, poses, voxel_length=0.05, sdf_trunc=0.15)
    assert torch.equal(raw[0], want_raw[0]) and torch.equal(raw[1], want_raw[1])
    n = 20000
    u = torch.rand(n, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    out = metrics3d.score_mesh(got, got, num_points=n, distance_thresh=0.05, uniforms=u)
    assert out["fscore"] == 1.0 and out["precision"] == out["recall"] == 1.0


def test_refusals_on_the_device():
    s = scene("sphere")[0]
    k, poses = s.intrinsics_matrices(), s.poses
    vol = tsdf.TSDFVolume(s.origin, s.dims, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    for bad in (np.nan, np.inf, -1.0):
        d = s.depths[:2].copy()
        d[1, 5, 5] = bad
        with pytest.raises(ValueError):
            vol.integrate(d, k[:2], poses[:2])
        with pytest.raises(ValueError):
            vol.integrate(torch.from_numpy(d).to(DEV), k[:2], poses[:2])
    with pytest.raises(ValueError):
        vol.integrate(s.depths[:2], k[:2], poses[:3])
    with pytest.raises(ValueError):
        vol.integrate(s.depths[:2], k[:3], poses[:2])
    singular = poses[:1].copy()
    singular[0, 2] = singular[0, 1]
    with pytest.raises(ValueError):
        vol.integrate(s.depths[:1], k[:1], singular)
    assert not bool(vol.weight.any())                                             # nothing was launched
    with pytest.raises(ValueError):
        tsdf.TSDFVolume(s.origin, (2048, 1024, 1024), device=DEV)
    with pytest.raises(lib.VfnError):
        tsdf.TSDFVolume(s.origin, s.dims, device="cpu")
    with pytest.raises(lib.VfnError):
        lib.tsdf_integrate(vol.tsdf, vol.weight.cpu(), vol.origin, vol.voxel_length, vol.sdf_trunc, torch.zeros(1, 2, 2, device=DEV),
                           torch.zeros(1, 4, device=DEV), torch.zeros(1, 12, device=DEV))
