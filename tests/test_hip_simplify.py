"""Vertex-clustering simplification on the MI355X (csrc/vfn_simplify.hip through vf_nerf_amd/meshops.py and evaluator.tsdf_mesh) against
the CPU restatements of its contract (tests/simplify_restatement.py).  Every comparison is bit for bit: the vertices, the faces, the
face and vertex maps, the attribute means, the placed flags and the quadric errors, for both contractions."""
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import evaluator, lib, meshops, metrics3d, ply, tsdf  # noqa: E402
import simplify_restatement as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = S.cases()
CASES = [(name, c) for name in SHAPES for c in S.CONTRACTIONS]
WITH_FACES = [name for name in SHAPES if len(SHAPES[name][1])]
_want, _got = {}, {}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_numbers(a, b):
    """float64 arrays equal bit for bit, every NaN standing for every other NaN (``error`` of "average" is NaN by contract)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a[~np.isnan(a)]), bits(b[~np.isnan(b)]))


def attributes(name):
    return S.attributes(len(SHAPES[name][0]))


def want(name, contraction):
    """The restatement of a case with colours and normals, computed once and shared."""
    if (name, contraction) not in _want:
        v, f, h = SHAPES[name]
        _want[name, contraction] = S.simplify_arrays(v, f, h, contraction, *attributes(name))
    return _want[name, contraction]


def got(name, contraction):
    """The device's answer for a case with colours and normals, computed once and shared (never changed by a test)."""
    if (name, contraction) not in _got:
        v, f, h = SHAPES[name]
        col, nrm = attributes(name)
        _got[name, contraction] = meshops.simplify_vertex_clustering((v, f), h, contraction=contraction, colours=col, normals=nrm)
    return _got[name, contraction]


def host(s) -> dict:
    """A ``Simplified`` -> the restatement's dictionary of numpy arrays, the placement and dtypes checked on the way."""
    assert isinstance(s, meshops.Simplified) and isinstance(s.n_clusters, int)
    for t in (s.vertices, s.error):
        assert t.is_cuda and t.dtype == torch.float64
    for t in (s.faces, s.kept_faces, s.inverse):
        assert t.is_cuda and t.dtype == torch.int64
    assert s.placed.is_cuda and s.placed.dtype == torch.bool
    assert s.vertices.shape[0] == s.placed.shape[0] == s.error.shape[0] and s.faces.shape[0] == s.kept_faces.shape[0]
    out = {"n_clusters": s.n_clusters}
    for key in ("vertices", "faces", "kept_faces", "inverse", "colours", "normals", "placed", "error"):
        t = getattr(s, key)
        out[key] = None if t is None else t.cpu().numpy()
    return out


def assert_same(one: dict, ref: dict, what):
    assert one["n_clusters"] == ref["n_clusters"], (what, one["n_clusters"], ref["n_clusters"])
    for key in ("faces", "kept_faces", "inverse", "placed"):
        assert one[key].shape == ref[key].shape and np.array_equal(one[key], ref[key]), (what, key)
    for key in ("vertices", "colours", "normals", "error"):
        assert (one[key] is None) == (ref[key] is None), (what, key)
        if ref[key] is not None:
            assert same_numbers(one[key], ref[key]), (what, key, one[key].shape, ref[key].shape)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: the device equals the restatement, field by field
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,contraction", CASES)
def test_device_equals_the_restatement(name, contraction):
    """The cube at four voxel edges (one of them a single cluster of 9 216 items), the recorded reference meshes f16 and f32 at two, the
    small shapes (no faces, one face, a bow tie, an unreferenced vertex, a repeated vertex), fans whose centre cluster holds exactly
    1 / 63 / 64 / 65 / 128 / 129 items — both contractions, with colours and normals."""
    assert_same(host(got(name, contraction)), want(name, contraction), (name, contraction))
    v, f, h = SHAPES[name]
    plain = meshops.simplify_vertex_clustering((torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)), h, contraction=contraction)
    assert plain.colours is None and plain.normals is None
    assert same_numbers(plain.vertices.cpu().numpy(), want(name, contraction)["vertices"])          # the attributes move no bit of the mesh
    assert np.array_equal(plain.faces.cpu().numpy(), want(name, contraction)["faces"])


@pytest.mark.parametrize("k", S.FAN_SIZES)
def test_the_fans_sit_on_the_lane_boundaries(k):
    ref = want(f"fan_{k}", "quadric")
    centre = ref["cluster_of_vertex"][0]
    assert ref["items_per_cluster"][centre] == k and ref["items_per_cluster"].max() == (max(k, 2) if k > 1 else 1)   # a rim vertex has one or two faces
    s = host(got(f"fan_{k}", "quadric"))
    assert s["inverse"][0] >= 0 and bool(s["placed"][s["inverse"][0]]) == (k > 2)          # all planes meet in the centre: it is its own minimiser


def test_one_cluster_holds_every_incidence():
    """A voxel of 4 on the cube: all 9 216 incidences fall into one segment and no face survives.  (At a voxel of 2 the frame's origin
    is -1, so the coordinate 1 falls into cell 1: eight clusters, the largest of 4 323 items, twelve faces left — that case runs above.)"""
    ref = want("cube_4.0", "quadric")
    assert ref["n_clusters"] == 1 and ref["items_per_cluster"].tolist() == [9216]
    for contraction in S.CONTRACTIONS:
        s = got("cube_4.0", contraction)
        assert s.n_clusters == 1 and s.vertices.shape == (0, 3) and s.faces.shape == (0, 3) and (s.inverse == -1).all()
    assert want("cube_2.0", "quadric")["items_per_cluster"].max() == 4323


# ---------------------------------------------------------------------------------------------------------------------------------
# 2: "average" is voxel_down_sample on the referenced vertices: an independent path through existing code
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WITH_FACES)
def test_average_equals_voxel_down_sample(name):
    v, f, h = SHAPES[name]
    referenced = np.unique(f)
    down = metrics3d.voxel_down_sample(v[referenced], h)
    s = host(got(name, "average"))
    assert s["n_clusters"] == down.points.shape[0]
    out = s["inverse"][referenced]
    cluster = down.voxel_of_point.cpu().numpy()
    stays = out >= 0
    assert np.array_equal(bits(s["vertices"][out[stays]]), bits(down.points.cpu().numpy()[cluster[stays]]))
    assert len(np.unique(out[stays])) == len(s["vertices"]) and (s["inverse"][np.setdiff1d(np.arange(len(v)), referenced)] == -1).all()
    assert np.isnan(s["error"]).all() and not s["placed"].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: the cube holds exactly
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,clusters,faces", [(0.25, 98, 192), (0.1875, 152, None)])
def test_the_cube_keeps_its_corners_exactly(h, clusters, faces):
    name = f"cube_{h}"
    v, f, _ = SHAPES[name]
    assert v.shape == (1538, 3) and f.shape == (3072, 3)
    q, a = host(got(name, "quadric")), host(got(name, "average"))
    assert q["n_clusters"] == a["n_clusters"] == clusters and len(q["vertices"]) == clusters
    assert faces is None or len(q["faces"]) == len(a["faces"]) == faces
    assert int(q["placed"].sum()) == 8
    corners = sorted(map(tuple, q["vertices"][q["placed"]].tolist()))
    assert np.array_equal(np.array(corners), np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)]))
    assert np.array_equal(q["error"][q["placed"]], np.zeros(8))
    # every other cluster equals its mean, which is what "average" returns; "average" pulls the corners inwards
    assert np.array_equal(bits(q["vertices"][~q["placed"]]), bits(a["vertices"][~q["placed"]]))
    inside = a["vertices"][q["placed"]]
    assert ((inside > 0.0) & (inside < 1.0)).all()
    assert np.array_equal(q["faces"], a["faces"]) and np.array_equal(q["inverse"], a["inverse"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: both branches on the recorded meshes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f16_0.1", "f32_0.25"])
def test_both_branches_are_taken_on_the_golden_meshes(name):
    ref, s = want(name, "quadric"), host(got(name, "quadric"))
    placed, kept = int(ref["placed"].sum()), int((~ref["placed"]).sum())
    assert placed > 0 and kept > 0, (placed, kept)
    assert ref["n_clusters"] == {"f16_0.1": 2033, "f32_0.25": 200}[name]
    assert int(s["placed"].sum()) == placed and int((~s["placed"]).sum()) == kept
    # an accepted minimiser moves the vertex off the mean (not always: a cluster of ONE vertex whose planes all pass through it keeps
    # it); every other cluster has the mean's bits
    mean = host(got(name, "average"))["vertices"]
    assert (s["vertices"][s["placed"]] != mean[s["placed"]]).any(axis=1).sum() > placed // 2
    assert np.array_equal(bits(s["vertices"][~s["placed"]]), bits(mean[~s["placed"]]))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: what holds of every output
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,contraction", [(n, c) for n, c in CASES if len(SHAPES[n][1])])
def test_output_invariants(name, contraction):
    v, f, h = SHAPES[name]
    ref, s = want(name, contraction), host(got(name, contraction))
    faces = s["faces"]
    assert ((faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])).all()
    assert len(np.unique(np.sort(faces, axis=1), axis=0)) == len(faces)
    assert np.array_equal(np.unique(faces), np.arange(len(s["vertices"])))                      # every output vertex is named
    # the closed cell: an accepted minimiser is fl(g + x) with |x| <= h / 2; a mean is a serial sum of at most `most` coordinates of the
    # cell, each within a rounding of the cell's bounds, over their count: every step rounds once, relative to the coordinates' size
    most = np.bincount(ref["cluster_of_vertex"][ref["cluster_of_vertex"] >= 0]).max()
    slack = (most + 8) * 2.0 ** -53 * (np.abs(v).max() + h)
    assert (np.abs(s["vertices"] - ref["centres"]) <= 0.5 * h + slack).all()
    # inverse and kept_faces against the input
    assert ((s["inverse"] >= 0) <= np.isin(np.arange(len(v)), f)).all() and s["inverse"].max(initial=-1) == len(s["vertices"]) - 1
    assert (np.diff(s["kept_faces"]) > 0).all() and np.array_equal(s["inverse"][f[s["kept_faces"]]], faces)
    dropped = np.setdiff1d(np.arange(len(f)), s["kept_faces"])
    mapped = s["inverse"][f[dropped]]
    kept_triples = {tuple(t) for t in np.sort(faces, axis=1).tolist()}
    for tri in mapped.tolist():                                                                 # a dropped face collapsed, or repeats a kept one
        assert len(set(tri)) < 3 or -1 in tri or tuple(sorted(tri)) in kept_triples
    col, nrm = attributes(name)
    again = meshops.simplify_vertex_clustering((v, f), h, contraction=contraction, colours=col, normals=nrm)
    assert_same(host(again), s, (name, contraction, "second run"))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6: values that must never reach an address
# ---------------------------------------------------------------------------------------------------------------------------------
def dev(x, dtype):
    return torch.tensor(x, dtype=dtype, device=DEV)


def _tables():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0.25]])
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 4, 2]])
    origin, h = (-0.5, -0.5, -0.5), 1.0
    planes = lib.face_planes(dev(v, torch.float64), dev(f, torch.int64), origin)
    assert np.array_equal(bits(planes.cpu().numpy()), bits(S.planes_arrays(v, f, origin)))
    centres = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    means = centres + np.array([[0.1, 0.2, -0.1], [0.0, 0.1, 0.1], [-0.2, 0.0, 0.3]])
    return planes, centres, means, origin, h


@pytest.mark.parametrize("start", [[0, 3, 2, 5], [0, 2, 2, 5], [-1, 2, 4, 5], [0, 2, 4, 6], [0, 2, 1 << 40, 5], [2, -(1 << 62), 4, 5]])
def test_a_segment_outside_its_range_sets_the_status(start):
    planes, centres, means, origin, h = _tables()
    items = [0, 1, 2, 3, 1]
    args = (planes, dev(items, torch.int64), dev(start, torch.int64), dev(centres, torch.float64), dev(means, torch.float64), origin, h, 1e-9)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.cluster_quadrics(*args)
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    position, placed, error = (t.cpu().numpy() for t in lib.cluster_quadrics(*args, info=info))
    ok = np.array([0 <= b < e <= 5 for b, e in zip(start[:-1], start[1:])])
    assert int(info.cpu()) == 2 and np.array_equal(np.isnan(position).all(axis=1), ~ok) and np.array_equal(np.isnan(error), ~ok)
    assert not placed[~ok].any()
    ref = S.quadrics_arrays(planes.cpu().numpy(), items, start, centres, means, origin, h, 1e-9)
    assert ref[3] == 2 and same_numbers(position, ref[0]) and np.array_equal(placed != 0, ref[1]) and same_numbers(error, ref[2])


@pytest.mark.parametrize("bad", [4, -1, 1 << 40, -(1 << 62)])
def test_a_face_outside_its_range_sets_the_status(bad):
    planes, centres, means, origin, h = _tables()
    items, start = [0, 1, 2, bad, 3], [0, 2, 4, 5]
    args = (planes, dev(items, torch.int64), dev(start, torch.int64), dev(centres, torch.float64), dev(means, torch.float64), origin, h, 1e-9)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.cluster_quadrics(*args)
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    position, placed, error = (t.cpu().numpy() for t in lib.cluster_quadrics(*args, info=info))
    assert int(info.cpu()) == 2 and np.isnan(position[1]).all() and np.isnan(error[1]) and placed[1] == 0
    ref = S.quadrics_arrays(planes.cpu().numpy(), items, start, centres, means, origin, h, 1e-9)
    assert ref[3] == 2 and same_numbers(position, ref[0]) and np.array_equal(placed != 0, ref[1]) and same_numbers(error, ref[2])
    assert not np.isnan(position[[0, 2]]).any()
    # the planes refuse a vertex outside [0, n) the same way: five +0.0, nothing read through it
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    v, f = dev([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]], torch.float64), dev([[0, 1, 2], [0, bad, 2]], torch.int64)
    out = lib.face_planes(v, f, origin, info=info).cpu().numpy()
    assert int(info.cpu()) == 2 and np.array_equal(bits(out[1]), np.zeros(5, dtype=np.uint64)) and out[0].tolist() == [0.0, 0.0, 1.0, 0.5, 0.5]


def test_a_non_finite_coordinate_raises():
    v, f, h = SHAPES["cube_0.25"]
    for value in (np.nan, np.inf):
        broken = v.copy()
        broken[7, 1] = value
        with pytest.raises(lib.VfnError, match="non-finite"):
            meshops.simplify_vertex_clustering((broken, f), h, contraction="quadric")
    spread = v.copy()
    spread[0, 0] = 1.0e7                                                     # a frame wider than 2^21 cells is refused, as voxel.frame does
    with pytest.raises(ValueError, match="voxels"):
        meshops.simplify_vertex_clustering((spread, f), 1.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7: the evaluator's switch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_evaluator_simplifies_only_with_the_switch(tmp_path, monkeypatch):
    """evaluator.tsdf_mesh with the reference's dataset module stood in for and the fusion handing over the cube: with the switch unset
    the file's bytes are those of the fused mesh as before; with it set the file holds the simplified mesh with its mean colours, and
    the normals of the simplified mesh when they are asked for."""
    from PIL import Image
    os.makedirs(tmp_path / "rendered_images")
    np.save(tmp_path / "rendered_images" / "depth-0.npy", np.ones((4, 5, 1)))
    Image.fromarray(np.zeros((4, 5, 3), dtype=np.uint8)).save(tmp_path / "rendered_images" / "image-0.png")

    class Dataset:
        def __init__(self, config):
            self.intrinsics, self.poses = torch.eye(4), torch.eye(4)[None]

    v, f, _ = SHAPES["cube_0.25"]
    colours = np.round(S.attributes(len(v))[0] * 255) / 255
    fused = (torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(colours).to(DEV))
    monkeypatch.setattr(tsdf, "fuse_rgbd_maps", lambda *a, **k: fused)
    names = ("datasets", "datasets.normal_datasets")
    saved = {key: sys.modules[key] for key in names if key in sys.modules}
    fakes = {key: types.ModuleType(key) for key in names}
    fakes["datasets"].__path__ = []
    fakes["datasets.normal_datasets"].dataset_dict = {"fake": Dataset}
    path = str(tmp_path / "tsdf-mesh" / "tsdf.ply")
    files, raw = {}, {}
    assert evaluator.TSDF_SIMPLIFY_VOXEL is None
    try:
        sys.modules.update(fakes)
        for switch, with_normals in ((None, False), (0.25, False), (0.25, True)):
            monkeypatch.setattr(evaluator, "TSDF_SIMPLIFY_VOXEL", switch)
            monkeypatch.setattr(evaluator, "TSDF_VERTEX_NORMALS", with_normals)
            evaluator.tsdf_mesh(str(tmp_path), types.SimpleNamespace(dataset_name="fake"))
            files[switch, with_normals] = ply.read_ply(path, normals=True)
            raw[switch, with_normals] = open(path, "rb").read()
    finally:
        for key in names:
            del sys.modules[key]
        sys.modules.update(saved)
    ply.write_ply(str(tmp_path / "as_fused.ply"), *fused)
    assert raw[None, False] == open(tmp_path / "as_fused.ply", "rb").read()
    ref = S.simplify_arrays(v, f, 0.25, "quadric", colours)
    for key in ((0.25, False), (0.25, True)):
        vs, fs, cs, ns = files[key]
        assert np.array_equal(vs, ref["vertices"].astype(np.float32).astype(np.float64)) and np.array_equal(fs, ref["faces"])
        assert np.array_equal(cs, ply.colour_bytes(ref["colours"])) and len(vs) == 98 and len(fs) == 192
    assert files[0.25, False][3] is None
    normals = meshops.vertex_normals((ref["vertices"], ref["faces"])).cpu().numpy()
    assert np.array_equal(files[0.25, True][3], normals.astype(np.float32).astype(np.float64))
