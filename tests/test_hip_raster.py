"""Depth rasteriser, Laplacian smoothing and refuse on the device (csrc/vfn_raster.hip, vf_nerf_amd/raster.py, vf_nerf_amd/refuse.py)
against the NumPy restatement of their contract (tests/raster_restatement.py): depth maps bit for bit with no tolerance and no
excluded pixel, smoothed vertices bit for bit, the refused mesh bit for bit against the restated chain."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, metrics3d, raster, refuse, tsdf  # noqa: E402
import raster_restatement as R  # noqa: E402
import tsdf_restatement as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CENTRES = (0.0, 0.5)

_CACHE = {}


def matrices(k4s):
    k = np.tile(np.eye(3, dtype=np.float32), (len(k4s), 1, 1))
    k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2] = np.asarray(k4s, dtype=np.float32).T
    return k


def views(name):
    """(vertices, faces, poses, k4s, h, w) of the three scenes of the contract."""
    if name == "sphere":
        h, w = 48, 64
        poses = [T.look_at(e) for e in T.SPHERE_EYES]
        return R.icosphere(3, 0.5) + (poses, [T.pinhole(h, w)] * len(poses), h, w)
    if name == "box":
        h, w = 30, 40
        poses = [T.look_at(e, t) for e, t in T.ROOM_VIEWS]
        return R.box(0.6) + (poses, [T.pinhole(h, w, 0.6 * w)] * len(poses), h, w)
    h, w = 48, 64
    poses = [T.look_at((0.05, -0.02, 0.03), (0.4, 0.1, 1.0))]
    return R.soup(3000) + (poses, [T.pinhole(h, w, 0.6 * w)], h, w)


def scene(name, c):
    """The scene and its restated depth maps at pixel centre c: computed once, never written to."""
    if (name, c) not in _CACHE:
        v, f, poses, k4s, h, w = views(name)
        counts = {}
        want = R.rasterize(v, f, k4s, [T.extrinsic(p) for p in poses], h, w, c=c, counts=counts)
        want.setflags(write=False)
        _CACHE[(name, c)] = (v, f, np.asarray(poses), matrices(k4s), h, w, want, counts)
    return _CACHE[(name, c)]


def same_bits(got: torch.Tensor, want: np.ndarray, what=""):
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    g = got.cpu().numpy().view(np.uint32)
    bad = int((g != want.view(np.uint32)).sum())
    print(f"{what}: {bad} of {want.size} depth words differ, {int((want > 0).sum())} pixels hit")
    assert bad == 0, what


@pytest.mark.parametrize("c", CENTRES)
@pytest.mark.parametrize("name", ["sphere", "box", "soup"])
def test_depth_equals_the_restatement_bit_for_bit(name, c):
    v, f, poses, k, h, w, want, counts = scene(name, c)
    got, dev_counts = raster.rasterize_depth_counted((v, f), k, poses, h, w, pixel_centre=c, device=DEV)
    print(name, c, counts, dev_counts)
    same_bits(got, want, f"{name}, pixel centre {c}")
    assert dev_counts["fragments"] == counts["fragments"] and 0 < dev_counts["atomics"] <= dev_counts["fragments"]
    hit = int((want > 0).sum())
    if name == "sphere":
        assert len(f) == 1280 and want.shape == (7, 48, 64) and 0 < hit < want.size
        assert counts["z_culled"] == counts["off_screen"] == counts["straddling"] == 0
    if name == "box":
        # 12 large faces seen from inside: faces behind the camera, faces through the near plane, and the wave-cooperative form
        assert want.shape == (5, 30, 40) and hit == want.size
        assert counts["z_culled"] > 0 and counts["straddling"] > 0 and dev_counts["cooperative"] >= counts["straddling"]
    if name == "soup":
        assert len(f) == 3000 and counts["z_culled"] > 0 and counts["off_screen"] > 0 and counts["straddling"] > 0 and 0 < hit < want.size


def test_compared_pixels_are_hit_and_missed():
    """Over the three scenes and both pixel centres at least a quarter of the compared pixels are hit, and some are not.  (Taken over
    the scenes together: the camera inside the closed box sees a wall in every pixel, and the sphere of radius 0.5 from a distance of
    2 with a focal length of 0.9 W covers 23 % of a 48 x 64 map — neither scene alone can give both.)"""
    hit = total = 0
    for name in ("sphere", "box", "soup"):
        for c in CENTRES:
            want = scene(name, c)[6]
            hit, total = hit + int((want > 0).sum()), total + want.size
            print(name, c, int((want > 0).sum()), want.size)
    assert 4 * hit >= total and hit < total


def camera_set(n_views, h, w):
    """n look-at cameras around the sphere; among nine, camera 3 looks away and camera 5 stands so close that one face fills its image."""
    eyes = (T.SPHERE_EYES + ((-1.2, 1.4, -1.0), (0.3, -1.9, 0.6)))[:n_views]
    poses = [T.look_at(e) for e in eyes]
    if n_views == 9:
        poses[3] = T.look_at((2.0, 0.5, 0.0), (4.0, 0.5, 0.0))
    return np.asarray(poses), [T.pinhole(h, w)] * n_views


@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, 4097])
def test_face_counts_where_indexing_can_go_wrong(n_faces):
    """One face, a wave short of one, a full wave, one over, and more than sixteen workgroups — the first n faces of icosphere(4)
    (5 120) behind one degenerate face, which draws nothing."""
    v, f = R.icosphere(4, 0.5)
    f = np.concatenate([[[0, 0, 0]], f[:n_faces - 1]]) if n_faces > 1 else np.array([[0, 0, 0]])
    h, w = 48, 64
    poses, k4s = camera_set(2, h, w)
    want = R.rasterize(v, f, k4s, [T.extrinsic(p) for p in poses], h, w)
    got = raster.rasterize_depth(v, f, matrices(k4s), poses, h, w, device=DEV)
    same_bits(got, want, f"{n_faces} faces")
    assert (want > 0).any() == (n_faces > 1)


@pytest.mark.parametrize("h,w,n_views", [(1, 1, 1), (7, 5, 2), (48, 64, 9), (65, 130, 1), (1, 1, 9), (7, 5, 9), (65, 130, 2)])
def test_image_and_view_counts_where_indexing_can_go_wrong(h, w, n_views):
    v, f = R.icosphere(2, 0.5)
    big = np.array([[-1.0, -1, 0.3], [1, -1, 0.3], [0, 1.5, 0.3]])                          # fills the image of a camera at the origin that looks along +z
    v, f = np.concatenate([v, big]), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]])
    poses, k4s = camera_set(n_views, h, w)
    if n_views >= 2:
        poses[1] = np.eye(4)                                                                # at the origin, inside the sphere, looking at the big face
    want = R.rasterize(v, f, k4s, [T.extrinsic(p) for p in poses], h, w)
    got = raster.rasterize_depth(v, f, matrices(k4s), poses, h, w, device=DEV)
    same_bits(got, want, f"{n_views} views of {h} x {w}")
    if n_views >= 2:
        assert (want[1] == np.float32(0.3)).all()                                           # one face fills the whole image
    if n_views == 9:
        assert not want[3].any() and not bool(got[3].any())                                 # the camera that looks away


def test_an_empty_mesh_gives_all_zeros():
    poses, k4s = camera_set(2, 7, 5)
    got = raster.rasterize_depth(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), matrices(k4s), poses, 7, 5, device=DEV)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (2, 7, 5) and not bool(got.any())
    got = raster.rasterize_depth(R.icosphere(0)[0], np.zeros((0, 3), dtype=np.int64), matrices(k4s), poses, 7, 5, device=DEV)
    assert tuple(got.shape) == (2, 7, 5) and not bool(got.any())
    # a mesh whose only face is degenerate goes through the kernel and gives the same
    got = raster.rasterize_depth(R.icosphere(0)[0], np.array([[0, 0, 0]]), matrices(k4s), poses, 7, 5, device=DEV)
    assert not bool(got.any())


def test_one_call_of_v_views_equals_v_calls_and_face_order_changes_no_bit():
    v, f, poses, k, h, w, want, _ = scene("sphere", 0.5)
    one = raster.rasterize_depth(v, f, k, poses, h, w, device=DEV)
    many = torch.stack([raster.rasterize_depth(v, f, k[i], poses[i], h, w, device=DEV)[0] for i in range(len(poses))])
    assert torch.equal(one.view(torch.int32), many.view(torch.int32))
    g = np.random.default_rng(1)
    shuffled = np.roll(f[g.permutation(len(f))], 1, axis=1)
    again = raster.rasterize_depth(v, shuffled, k, poses, h, w, device=DEV)
    assert torch.equal(one.view(torch.int32), again.view(torch.int32))
    v, f, poses, k, h, w, want, _ = scene("soup", 0.5)
    again = raster.rasterize_depth(v, np.roll(f[g.permutation(len(f))], 2, axis=1), k, poses, h, w, device=DEV)
    same_bits(again, want, "soup, permuted")


def test_bad_meshes_raise_without_a_fault():
    v, f, poses, k, h, w, _, _ = scene("sphere", 0.5)
    for bad in (len(v), -1, 1 << 40):
        g = f.copy()
        g[700, 1] = bad
        with pytest.raises(lib.VfnError):
            raster.rasterize_depth(v, g, k, poses, h, w, device=DEV)
    for bad in (np.nan, np.inf):
        x = v.copy()
        x[300, 2] = bad
        with pytest.raises(lib.VfnError):
            raster.rasterize_depth(x, f, k, poses, h, w, device=DEV)
    with pytest.raises(lib.VfnError):
        raster.rasterize_depth(np.zeros((0, 3)), f, k, poses, h, w, device=DEV)            # faces without vertices
    with pytest.raises(lib.VfnError):
        refuse.smooth_laplacian((v, np.array([[0, 1, len(v)]])), device=DEV)
    with pytest.raises(lib.VfnError):
        raster.rasterize_depth(v, f, k, poses, h, w, device="cpu")
    same_bits(raster.rasterize_depth(v, f, k, poses, h, w, device=DEV), scene("sphere", 0.5)[6], "after the refusals")


@pytest.mark.parametrize("iterations", [0, 1, 10])
def test_smooth_laplacian_equals_the_restatement_bit_for_bit(iterations):
    v, f = R.icosphere(2, 0.5)
    g = np.random.default_rng(5)
    v = np.concatenate([v + g.normal(0, 0.01, v.shape), [[0.9, 0.8, 0.7]]])                 # noise to smooth, and an isolated vertex
    f = np.concatenate([f, f[17:18], [[4, 4, 4]], [[7, 7, 9]]])                             # a duplicated face, two degenerate ones
    want = R.smooth_laplacian(v, f, iterations=iterations, lam=0.5)
    got_v, got_f = refuse.smooth_laplacian((v, f), iterations=iterations, device=DEV)
    assert got_v.dtype == torch.float64 and got_v.is_cuda and got_f.dtype == torch.int64 and np.array_equal(got_f.cpu().numpy(), f)
    assert np.array_equal(got_v.cpu().numpy().view(np.uint64), want.view(np.uint64))
    assert np.array_equal(got_v[-1].cpu().numpy(), [0.9, 0.8, 0.7])
    assert (iterations == 0) == np.array_equal(want, v)


def refuse_scene():
    """sphere_scene()'s cameras and volume; the mesh is icosphere(3) of radius 0.5 with a closed blob (icosphere(1), radius 0.1) hidden at
    its centre."""
    if "refuse" not in _CACHE:
        s = T.sphere_scene()
        hi = tuple(o + n * s.vl for o, n in zip(s.origin, s.dims))
        origin, dims = tsdf._box((s.origin, hi), s.vl)                                      # the box fuse_depth_maps makes of these bounds
        assert tuple(np.float32(origin).tolist()) == s.origin
        mesh = R.merged(R.icosphere(3, 0.5), R.icosphere(1, 0.1))
        _, edge_vertex, tri = lib.mesh_tables()
        tables = (tri, edge_vertex)
        out = {}
        for c in CENTRES:
            d = R.rasterize(mesh[0], mesh[1], s.k4s, s.e12s, 48, 64, c=c)
            d[d >= np.float32(5.0)] = 0
            t, w = T.fused(dims, s.origin, s.vl, s.trunc, d, s.k4s, s.e12s)
            out[c] = T.extract(t, w, s.origin, s.vl, tables)
        _CACHE["refuse"] = (s, (s.origin, hi), mesh, out)
    return _CACHE["refuse"]


@pytest.mark.parametrize("c", CENTRES)
def test_refuse_end_to_end(c):
    s, bounds, mesh, restated = refuse_scene()
    ev, ef = restated[c]
    v, f = refuse.refuse(mesh, s.intrinsics_matrices(), s.poses, 48, 64, bounds=bounds, voxel_length=s.vl, sdf_trunc=s.trunc, pixel_centre=c,
                         device=DEV)
    assert v.dtype == torch.float64 and f.dtype == torch.int64 and v.is_cuda and f.is_cuda
    assert tuple(v.shape) == ev.shape and tuple(f.shape) == ef.shape and len(ef) > 1000
    assert np.array_equal(v.cpu().numpy().view(np.uint64), ev.view(np.uint64)) and np.array_equal(f.cpu().numpy(), ef)
    r = v.norm(dim=1)
    err_dev, err_restated = float((r - 0.5).abs().max()), float(np.abs(np.linalg.norm(ev, axis=1) - 0.5).max())
    print(f"pixel centre {c}: max | |v| - 0.5 | = {err_dev:.4f} (restated chain {err_restated:.4f}), voxel {s.vl:.5f}, {len(ef)} faces")
    assert float(r.min()) > 0.3                                                            # the hidden blob is gone
    assert (np.linalg.norm(mesh[0], axis=1) < 0.3).any()                                    # (it was there)
    if c == 0.0:
        assert err_dev <= s.vl                                                              # a cap, not a measurement


def test_metrics_3d_returns_the_four_entries():
    s, bounds, mesh, _ = refuse_scene()
    gt = R.icosphere(3, 0.5)
    args = dict(bounds=bounds, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    out = refuse.metrics_3d(mesh, gt, s.intrinsics_matrices(), s.poses, 48, 64, num_points=20000, distance_thresh=0.1,
                            generator=torch.Generator(device=DEV).manual_seed(3), **args)
    assert list(out) == ["tsdf", "refused_tsdf", "tsdf_smoothed", "refused_tsdf_smoothed"]
    for entry in out.values():
        assert set(entry["chamfer distance"]) == {"mean", "median", "min", "max"} and {"precision", "recall", "fscore"} <= set(entry)
    direct = metrics3d.score_mesh(mesh, gt, num_points=20000, distance_thresh=0.1, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)
    assert out["tsdf"] == direct
    # the blob inside (0.4 from the surface) costs precision; refusing removes it (a refused vertex lies within a voxel, 0.044, of the sphere)
    print({k: (round(e["precision"], 4), round(e["recall"], 4)) for k, e in out.items()})
    assert out["tsdf"]["precision"] < 1.0 and out["refused_tsdf"]["precision"] == 1.0
    meshes = refuse.reconstruction_meshes(mesh, s.intrinsics_matrices(), s.poses, 48, 64, **args)
    assert set(meshes) == set(out) and all(m[0].is_cuda and m[1].shape[0] > 0 for m in meshes.values())
