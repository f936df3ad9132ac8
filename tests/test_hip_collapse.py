"""Quadric edge-collapse decimation on the MI355X (csrc/vfn_collapse.hip through vf_nerf_amd/decimate.py, meshops.dominant_bases and
evaluator.tsdf_mesh) against the CPU restatement of its contract (tests/collapse_restatement.py).  Every comparison is bit for bit: every
field of ``Collapsed``, and of single rounds the planes, the quadrics, the edges' points, costs, parameters and flags, every vertex's
choice, and the proposed / withdrawn / taken flags."""
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import decimate, evaluator, lib, meshops, ply, tsdf  # noqa: E402
from vf_nerf_amd.meshops import simplify_edge_collapse  # noqa: E402  (absent before this unit: nothing here passes without it)
import collapse_restatement as R  # noqa: E402
import simplify_restatement as SR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = R.cases()
_want, _got = {}, {}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(a, b):
    """equal shapes and equal values; float64 bit for bit"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    return np.array_equal(bits(a), bits(b)) if b.dtype.kind == "f" else np.array_equal(a, b)


def want(name):
    """The restatement of a case (with every round's dictionary), computed once and shared."""
    if name not in _want:
        v, f, kw = SHAPES[name]
        history = []
        _want[name] = (R.collapse(v, f, history=history, **kw), history)
    return _want[name]


def got(name):
    """The device's answer for a case, computed once and shared (never changed by a test)."""
    if name not in _got:
        v, f, kw = SHAPES[name]
        _got[name] = simplify_edge_collapse((v, f), **kw)
    return _got[name]


def host(c) -> dict:
    """A ``Collapsed`` -> the restatement's dictionary of numpy arrays, the placement and dtypes checked on the way."""
    assert isinstance(c, decimate.Collapsed) and isinstance(c.rounds, int) and isinstance(c.collapsed, int) and isinstance(c.reached, bool)
    for t in (c.vertices, c.cost):
        assert t.is_cuda and t.dtype == torch.float64
    for t in (c.faces, c.kept_faces, c.inverse):
        assert t.is_cuda and t.dtype == torch.int64
    out = {key: getattr(c, key) for key in ("rounds", "collapsed", "reached")}
    for key in ("vertices", "faces", "kept_faces", "inverse", "colours", "normals", "cost"):
        t = getattr(c, key)
        out[key] = None if t is None else t.cpu().numpy()
    return out


def assert_same(one: dict, ref: dict, what):
    for key in R.FIELDS:
        assert (one[key] is None) == (ref[key] is None), (what, key)
        if ref[key] is not None:
            assert same(one[key], ref[key]), (what, key, one[key], ref[key])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: the whole call
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_the_restatement(name):
    """The degenerate inputs (no faces, one face, a bow tie, an unreferenced vertex, a face naming a vertex twice, a duplicated face, three
    faces on one edge), the flat squares (every cost ties at 0: every tie-break to the lowest index), a ribbon of boundary vertices only,
    the 192-face cube at 96 and 12 faces, after one and two rounds and by the error alone, a Möbius strip, a book of three pages on one
    spine, fans whose centre has 63 / 64 / 65 / 300 faces, meshes of exactly 255 / 256 / 257 edges and vertices, the recorded reference
    meshes at half and a tenth of their faces."""
    assert_same(host(got(name)), want(name)[0], name)


@pytest.mark.parametrize("name", ["cube_12", "book", "fan_65", "f16_tenth"])
def test_colours_and_normals_follow(name):
    v, f, kw = SHAPES[name]
    col, nrm = R.attributes(len(v))
    ref = R.collapse(v, f, colours=col, normals=nrm, **kw)
    one = host(simplify_edge_collapse((torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)), colours=col, normals=torch.from_numpy(nrm), **kw))
    assert_same(one, ref, name)
    assert ref["colours"].shape == ref["vertices"].shape and same(one["vertices"], want(name)[0]["vertices"])          # they move no bit of the mesh


# ---------------------------------------------------------------------------------------------------------------------------------
# 2: single rounds, stage by stage
# ---------------------------------------------------------------------------------------------------------------------------------
def device_round(inputs, kw):
    position, f, origin = inputs
    args = {k: kw[k] for k in ("target_faces", "max_error", "boundary_weight", "rcond", "reach") if k in kw}
    r = decimate.collapse_round(torch.from_numpy(position).to(DEV), torch.from_numpy(f).to(DEV), origin.tolist(), **args)
    assert isinstance(r.n_taken, int)
    return {key: getattr(r, key).cpu().numpy() for key in R.ROUND_FIELDS}, r.n_taken


@pytest.mark.parametrize("name", [n for n in SHAPES if n not in ("no_faces", "one_face", "repeated_vertex")])
def test_rounds_equal_the_restatement(name):
    """The first two rounds, a middle one and the last of every case that runs any, from the restatement's own inputs of that round: the
    planes (the boundary rows after the faces'), the items, the quadrics, every edge's point, cost, parameter and flags, every vertex's
    choice, the proposed, withdrawn and taken edges."""
    history = want(name)[1]
    assert history
    for i in sorted({0, min(1, len(history) - 1), len(history) // 2, len(history) - 1}):
        ref = history[i]
        one, n_taken = device_round(ref["inputs"], SHAPES[name][2])
        for key in R.ROUND_FIELDS:
            assert same(one[key], ref[key]), (name, i, key)
        assert n_taken == ref["n_taken"]
        assert one["flags"].dtype == np.uint8 and one["proposed"].dtype == bool


def test_every_kind_of_edge_occurs():
    """What the cases are there for: accepted minimisers and fallbacks, non-manifold edges, edges over the bound, flipped faces, withdrawn
    proposals, costs that tie at +0.0 — each is there in some first round of the restatement, to which the tests above hold the device."""
    first = {name: want(name)[1][0] for name in ("square_outline", "cube_12", "book", "fan_300", "f32_tenth")}
    flags = {name: r["flags"] for name, r in first.items()}
    assert (flags["book"] & R.NONMANIFOLD).any() and (flags["book"] & R.CANDIDATE).any()
    assert (first["square_outline"]["cost"] == 0).all() and (flags["square_outline"] & R.CANDIDATE).all()          # 800 edges tie
    last = want("cube_error_only")[1][-1]
    assert (last["flags"] & R.OVER).any() and last["n_taken"] == 0 and not (last["flags"] & R.CANDIDATE).any()
    assert (flags["f32_tenth"] & R.FLIP).any() and (flags["f32_tenth"] & R.ACCEPTED).any() and ((flags["f32_tenth"] & R.ACCEPTED) == 0).any()
    assert first["f32_tenth"]["withdrawn"].any() and (first["f32_tenth"]["proposed"] & ~first["f32_tenth"]["withdrawn"]).any()
    assert not np.signbit(first["f32_tenth"]["cost"]).any()
    three = want("three_on_an_edge")[1][0]
    assert three["run"].max() == 3 and not (three["flags"][three["run"] == 3] & R.CANDIDATE).any()


def test_a_round_takes_only_what_the_budget_needs():
    v, f, _ = SHAPES["cube_12"]
    origin = v.min(axis=0)
    for target in (191, 190, 150, 12, 192, 500, None):
        ref = R.round_arrays(v, f, origin, target_faces=target)
        one, n_taken = device_round((v, f, origin), {"target_faces": target} if target else {"max_error": 1.0})
        assert same(one["taken"], ref["taken"]) and n_taken == ref["n_taken"], target
    assert R.round_arrays(v, f, origin, target_faces=191)["n_taken"] == 1 and R.round_arrays(v, f, origin, target_faces=192)["n_taken"] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: tables that lie, coordinates that are not numbers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_table_outside_its_range_sets_the_status():
    v, f, _ = SHAPES["cube_12"]
    r = R.round_arrays(v, f, v.min(axis=0))
    dev = lambda x, dtype=None: torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)          # noqa: E731
    tv, tf, planes, quadrics = dev(v), dev(f), dev(r["planes"]), dev(r["quadrics"])
    item_row, start, edge_a, edge_b, run = (dev(r[k]) for k in ("item_row", "start", "edge_a", "edge_b", "run"))
    origin = v.min(axis=0).tolist()
    for bad in (len(r["planes"]), -1, 1 << 40):
        rows = item_row.clone()
        rows[0] = bad
        info = torch.zeros(1, dtype=torch.int64, device=DEV)
        q = lib.vertex_quadrics(planes, rows, start, info=info).cpu().numpy()
        assert int(info.cpu()) == 2 and np.isnan(q[0]).all() and same(q[1:], r["quadrics"][1:])
        info.zero_()
        flags = lib.edge_collapse_candidates(tv, tf, quadrics, rows, start, len(r["planes"]), edge_a, edge_b, run, origin, 1e-9, 2.0, np.inf, info=info)[3]
        assert int(info.cpu()) & 2 and not (flags.cpu().numpy()[(r["edge_a"] == 0) | (r["edge_b"] == 0)] & R.CANDIDATE).any()
    for bad in ([0, 5, 3], [0, -1, 9], [0, 1 << 40, 1 << 41]):
        lying = start.clone()
        lying[:3] = torch.tensor(bad)
        info = torch.zeros(1, dtype=torch.int64, device=DEV)
        lib.vertex_quadrics(planes, item_row, lying, info=info)
        assert int(info.cpu()) == 2
    for bad in (len(v), -1, 1 << 40):
        ends = edge_b.clone()
        ends[0] = bad
        info = torch.zeros(1, dtype=torch.int64, device=DEV)
        point, cost, s, flags = lib.edge_collapse_candidates(tv, tf, quadrics, item_row, start, len(r["planes"]), edge_a, ends, run, origin, 1e-9, 2.0,
                                                             np.inf, info=info)
        assert int(info.cpu()) == 2 and int(flags[0]) == 0 and bool(torch.isnan(cost[0])) and same(cost[1:].cpu().numpy(), r["cost"][1:])
        info.zero_()
        as_candidate = dev(r["flags"] | R.CANDIDATE)
        best, proposed, withdrawn = lib.collapse_select(cost, as_candidate, edge_a, ends, tf, len(v), info=info)
        assert int(info.cpu()) == 2 and not bool(proposed[0])
        info.zero_()
        out = lib.boundary_planes(tv, planes[:len(f)].contiguous(), dev([0]), dev([bad]), dev([1]), origin, 1.0, info=info)
        assert int(info.cpu()) == 2 and not out.cpu().numpy().any()


def test_a_non_finite_coordinate_raises():
    v, f, _ = SHAPES["cube_12"]
    for value in (np.nan, np.inf):
        broken = v.copy()
        broken[7, 1] = value
        with pytest.raises(lib.VfnError, match="non-finite"):
            simplify_edge_collapse((broken, f), target_faces=12)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: the wiring
# ---------------------------------------------------------------------------------------------------------------------------------
def test_dominant_bases_by_collapse_equals_the_pieces(monkeypatch):
    v, f = SR.cube(4)
    assert meshops.DECIMATION == "clustering"
    before = meshops.dominant_bases((v, f), 3, decimation=0.5)
    monkeypatch.setattr(meshops, "DECIMATION", "collapse")
    one = meshops.dominant_bases((v, f), 3, decimation=0.5)
    c = simplify_edge_collapse((v, f), target_faces=96)
    by_hand = meshops.dominant_bases((c.vertices, c.faces), 3)
    assert one.voxel_size is None and one.n_faces == int(c.faces.shape[0]) <= 96 and one.n_vertices == by_hand.n_vertices
    for key in ("bases", "counts", "labels", "inertia"):
        assert same(getattr(one, key).cpu().numpy(), getattr(by_hand, key).cpu().numpy()), key
    assert same(c.faces.cpu().numpy(), want("cube_96")[0]["faces"])
    monkeypatch.setattr(meshops, "DECIMATION", "clustering")
    after = meshops.dominant_bases((v, f), 3, decimation=0.5)
    assert before.voxel_size == after.voxel_size and before.voxel_size is not None          # the default is the bisection, bit for bit
    for key in ("bases", "counts", "labels", "inertia"):
        assert same(getattr(before, key).cpu().numpy(), getattr(after, key).cpu().numpy()), key
    monkeypatch.setattr(meshops, "DECIMATION", "quadric")
    with pytest.raises(ValueError, match="DECIMATION"):
        meshops.dominant_bases((v, f), 3, decimation=0.5)


def test_evaluator_decimates_only_with_the_switch(tmp_path, monkeypatch):
    """evaluator.tsdf_mesh with the reference's dataset module stood in for and the fusion handing over the cube: with the switch unset
    the file's bytes are those of the fused mesh as before; with it set the file holds at most that many faces, the restatement's, with
    the interpolated colours, and the normals of the decimated mesh when they are asked for; both simplifications at once are refused."""
    from PIL import Image
    os.makedirs(tmp_path / "rendered_images")
    np.save(tmp_path / "rendered_images" / "depth-0.npy", np.ones((4, 5, 1)))
    Image.fromarray(np.zeros((4, 5, 3), dtype=np.uint8)).save(tmp_path / "rendered_images" / "image-0.png")

    class Dataset:
        def __init__(self, config):
            self.intrinsics, self.poses = torch.eye(4), torch.eye(4)[None]

    v, f = SR.cube(4)
    colours = np.round(R.attributes(len(v))[0] * 255) / 255
    fused = (torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(colours).to(DEV))
    monkeypatch.setattr(tsdf, "fuse_rgbd_maps", lambda *a, **k: fused)
    names = ("datasets", "datasets.normal_datasets")
    saved = {key: sys.modules[key] for key in names if key in sys.modules}
    fakes = {key: types.ModuleType(key) for key in names}
    fakes["datasets"].__path__ = []
    fakes["datasets.normal_datasets"].dataset_dict = {"fake": Dataset}
    path = str(tmp_path / "tsdf-mesh" / "tsdf.ply")
    files, raw = {}, {}
    assert evaluator.TSDF_SIMPLIFY_FACES is None and evaluator.TSDF_SIMPLIFY_VOXEL is None
    try:
        sys.modules.update(fakes)
        for switch, with_normals in ((None, False), (96, False), (96, True)):
            monkeypatch.setattr(evaluator, "TSDF_SIMPLIFY_FACES", switch)
            monkeypatch.setattr(evaluator, "TSDF_VERTEX_NORMALS", with_normals)
            evaluator.tsdf_mesh(str(tmp_path), types.SimpleNamespace(dataset_name="fake"))
            files[switch, with_normals] = ply.read_ply(path, normals=True)
            raw[switch, with_normals] = open(path, "rb").read()
        monkeypatch.setattr(evaluator, "TSDF_SIMPLIFY_VOXEL", 0.25)
        with pytest.raises(ValueError, match="cannot both"):
            evaluator.tsdf_mesh(str(tmp_path), types.SimpleNamespace(dataset_name="fake"))
    finally:
        for key in names:
            del sys.modules[key]
        sys.modules.update(saved)
    ply.write_ply(str(tmp_path / "as_fused.ply"), *fused)
    assert raw[None, False] == open(tmp_path / "as_fused.ply", "rb").read()
    ref = R.collapse(v, f, target_faces=96, colours=colours)
    for key in ((96, False), (96, True)):
        vs, fs, cs, ns = files[key]
        assert len(fs) <= 96 and np.array_equal(vs, ref["vertices"].astype(np.float32).astype(np.float64)) and np.array_equal(fs, ref["faces"])
        assert cs is not None and np.array_equal(cs, ply.colour_bytes(ref["colours"]))
    assert files[96, False][3] is None
    normals = meshops.vertex_normals((ref["vertices"], ref["faces"])).cpu().numpy()
    assert np.array_equal(files[96, True][3], normals.astype(np.float32).astype(np.float64))
