"""Vertex-clustering simplification, host side: the C-ABI surface, the build recipe, the two CPU restatements of the contract
(tests/simplify_restatement.py) held against each other bit for bit on every case the device is held to, what the contract promises on
the cube, the argument checks that run before any device is asked for, and the evaluator's switch with the device stood in for."""
import inspect
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import dropin, evaluator, lib, meshops, voxel  # noqa: E402
import simplify_restatement as S  # noqa: E402

NEW_EXPORTS = ("vfn_face_planes", "vfn_cluster_quadrics")
SHAPES = S.cases()
CASES = [(name, c) for name in SHAPES for c in S.CONTRACTIONS]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a[~np.isnan(a)]), bits(b[~np.isnan(b)]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_face_planes"] == ("int", ["const double*", "int64_t", "const int64_t*", "int64_t", "const double*", "double*", "int64_t*",
                                                 "void*"])
    assert protos["vfn_cluster_quadrics"] == ("int", ["const double*", "int64_t", "const int64_t*", "int64_t", "const int64_t*", "int64_t",
                                                      "const double*", "const double*", "const double*", "double", "double", "double*",
                                                      "uint8_t*", "double*", "int64_t*", "void*"])
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    # the host-side checks of the exports answer without a device
    assert handle.vfn_face_planes(None, 3, None, 0, None, None, None, None) != 0 and b"m 0 outside [1, 2^31)" in handle.vfn_last_error()
    assert handle.vfn_face_planes(None, -1, None, 2, None, None, None, None) != 0 and b"n -1 outside" in handle.vfn_last_error()
    assert handle.vfn_face_planes(None, 3, None, 2, None, None, None, None) != 0 and b"NULL" in handle.vfn_last_error()
    quadrics = lambda m, items, k, h=1.0, rcond=1e-9: handle.vfn_cluster_quadrics(None, m, None, items, None, k, None, None, None, h, rcond,   # noqa: E731
                                                                                  None, None, None, None, None)
    assert quadrics(0, 5, 2) != 0 and b"m 0 outside" in handle.vfn_last_error()
    assert quadrics(4, 0, 1) != 0 and b"n_items 0 outside" in handle.vfn_last_error()
    assert quadrics(4, 5, 6) != 0 and b"n_clusters 6 outside" in handle.vfn_last_error()
    assert quadrics(4, 5, 0) != 0 and b"n_clusters 0 outside" in handle.vfn_last_error()
    assert quadrics(4, 5, 2) != 0 and b"NULL" in handle.vfn_last_error()


def test_build_recipe_lists_the_unit_in_both_places():
    build = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "build.sh")).read()
    assert re.search(r'^UNITS=".*\bvfn_simplify\b.*"', build, flags=re.M)
    assert re.search(r"\|vfn_simplify[|)].*-ffp-contract=off", build)
    unit = open(os.path.join(REPO, "vf_nerf_amd", "csrc", "vfn_simplify.hip")).read()
    assert "atomicAdd" not in unit and "__shared__" not in unit                     # no floating-point atomics, no LDS: the order is the header's
    header = open(os.path.join(REPO, "include", "vfn.h")).read()
    for phrase in ("vfn_face_planes", "vfn_cluster_quadrics", "det = (a00 m00 + a01 m01) + a02 m02", "AS REMEMBERED: neither Open3D nor trimesh"):
        assert phrase in header, phrase


def test_signatures_and_defaults():
    assert list(inspect.signature(meshops.simplify_vertex_clustering).parameters) == ["mesh", "voxel_size", "contraction", "colours", "normals",
                                                                                     "rcond", "device"]
    defaults = {k: p.default for k, p in inspect.signature(meshops.simplify_vertex_clustering).parameters.items()}
    assert defaults["rcond"] == 1e-9 and defaults["colours"] is None and defaults["normals"] is None and defaults["device"] is None
    assert defaults["contraction"] in meshops.CONTRACTIONS == S.CONTRACTIONS
    assert meshops.Simplified._fields == S.FIELDS
    assert evaluator.TSDF_SIMPLIFY_VOXEL is None
    assert inspect.signature(dropin.install).parameters["tsdf_simplify_voxel"].default is None
    doc = meshops.__doc__
    assert "simplify_vertex_clustering" in doc and "Average / Quadric) AS REMEMBERED" in doc
    scope = doc[doc.index("Out of scope:"):]
    assert "simplification" not in scope and "edge-collapse" in scope and "k-means" in scope and "filling\nholes" in scope and "scale in ICP" in scope
    assert "AS REMEMBERED" in meshops.simplify_vertex_clustering.__doc__ and "Three host reads" in meshops.simplify_vertex_clustering.__doc__


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,contraction", CASES)
def test_two_restatements_agree(name, contraction):
    v, f, h = SHAPES[name]
    col, nrm = S.attributes(len(v))
    one, two = S.simplify_loops(v, f, h, contraction, col, nrm), S.simplify_arrays(v, f, h, contraction, col, nrm)
    assert set(one) == set(two) and set(S.FIELDS) <= set(one)
    for key in one:
        assert same(one[key], two[key]), (name, contraction, key)
    plain = S.simplify_arrays(v, f, h, contraction)
    assert plain["colours"] is None and plain["normals"] is None and same(plain["vertices"], one["vertices"]) and same(plain["faces"], one["faces"])


def test_restated_properties():
    # the cube: 98 clusters at 1/4 and 152 at 3/16, the 8 corner clusters placed — exactly on the corners —, every other one at its mean
    for h, clusters, faces in ((0.25, 98, 192), (0.1875, 152, None)):
        q, a = (S.simplify_loops(*SHAPES[f"cube_{h}"], c) for c in ("quadric", "average"))
        assert q["n_clusters"] == clusters and int(q["placed"].sum()) == 8 and (faces is None or len(q["faces"]) == faces)
        corners = np.array(sorted(map(tuple, q["vertices"][q["placed"]].tolist())))
        assert np.array_equal(corners, np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)]))
        assert np.array_equal(q["error"][q["placed"]], np.zeros(8)) and np.isnan(a["error"]).all() and not a["placed"].any()
        assert same(q["vertices"][~q["placed"]], a["vertices"][~q["placed"]])
        assert ((a["vertices"][q["placed"]] > 0) & (a["vertices"][q["placed"]] < 1)).all()
    off = S.simplify_loops(*SHAPES["cube_0.1875"], "quadric")
    assert np.abs(off["vertices"] - off["centres"]).max() == 0.0625          # at 3/16 the corners at coordinate 1 sit off the cell centre by 1/16
    v, f, _ = SHAPES["cube_0.25"]
    assert v.shape == (1538, 3) and f.shape == (3072, 3)
    # one cluster: every incidence in one segment, and no face survives
    one = S.simplify_arrays(*SHAPES["cube_4.0"], "quadric")
    assert one["n_clusters"] == 1 and one["items_per_cluster"].tolist() == [9216] and len(one["faces"]) == 0 and (one["inverse"] == -1).all()
    # the recorded meshes take both branches
    for name, clusters in (("f16_0.1", 2033), ("f32_0.25", 200)):
        ref = S.simplify_arrays(*SHAPES[name], "quadric")
        assert ref["n_clusters"] == clusters and 0 < int(ref["placed"].sum()) < len(ref["placed"])
    # the fans: the centre's cluster holds exactly k items
    for k in S.FAN_SIZES:
        ref = S.simplify_arrays(*SHAPES[f"fan_{k}"], "quadric")
        assert ref["items_per_cluster"][ref["cluster_of_vertex"][0]] == k
    # the adjugate solves A x = -b: against numpy's solver on a well-conditioned cluster, to rounding
    g = np.random.default_rng(3)
    nrm = g.normal(size=(40, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    planes = np.concatenate((nrm, g.uniform(-0.05, 0.05, (40, 1)), g.uniform(0.1, 1.0, (40, 1))), axis=1)
    centre, mean = np.zeros((1, 3)), np.full((1, 3), 0.01)
    position, placed, error, status = S.quadrics_arrays(planes, np.arange(40), [0, 40], centre, mean, (0.0, 0.0, 0.0), 1.0, 1e-9)
    a = np.einsum("i,ij,ik->jk", planes[:, 4], nrm, nrm)
    b = np.einsum("i,i,ij->j", planes[:, 4], -planes[:, 3], nrm)
    assert status == 0 and placed[0] and np.allclose(position[0], np.linalg.solve(a, -b), rtol=0, atol=1e-13)
    at = lambda x: float(np.sum(planes[:, 4] * (nrm @ x - planes[:, 3]) ** 2))          # noqa: E731
    assert abs(error[0] - at(position[0])) <= 1e-13 and error[0] <= at(mean[0])
    # the in-cell test: the same cluster in a cell too small for its minimiser keeps the mean, and the error is the quadric's there
    position, placed, error, _ = S.quadrics_arrays(planes, np.arange(40), [0, 40], centre, mean, (0.0, 0.0, 0.0), 1e-3, 1e-9)
    assert not placed[0] and np.array_equal(bits(position[0]), bits(mean[0])) and abs(error[0] - at(mean[0])) <= 1e-13
    # rcond = 1 accepts nothing that is not a perfect cube of a diagonal
    assert not S.quadrics_arrays(planes, np.arange(40), [0, 40], centre, mean, (0.0, 0.0, 0.0), 1.0, 1.0)[1][0]


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals before a device is asked for
# ---------------------------------------------------------------------------------------------------------------------------------
TRI_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.array([[0, 1, 2]])
TRI = (TRI_V, TRI_F)


@pytest.mark.parametrize("call", [
    lambda: meshops.simplify_vertex_clustering(TRI, 0.0),
    lambda: meshops.simplify_vertex_clustering(TRI, -1.0),
    lambda: meshops.simplify_vertex_clustering(TRI, float("nan")),
    lambda: meshops.simplify_vertex_clustering(TRI, float("inf")),
    lambda: meshops.simplify_vertex_clustering(TRI, 1e-200),
    lambda: meshops.simplify_vertex_clustering(TRI, True),
    lambda: meshops.simplify_vertex_clustering(TRI, "0.1"),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, contraction="median"),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, contraction=None),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, contraction="Quadric"),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, rcond=-1e-9),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, rcond=1.5),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, rcond=float("nan")),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, rcond="1e-9"),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, rcond=True),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, colours=np.zeros((2, 3))),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, colours=np.zeros((3, 4))),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, normals=np.zeros((4, 3))),
    lambda: meshops.simplify_vertex_clustering(TRI, 0.5, normals=np.zeros(3)),
    lambda: meshops.simplify_vertex_clustering((TRI_V, np.array([[0, 1, 3]])), 0.5),
    lambda: meshops.simplify_vertex_clustering((TRI_V, np.array([[0, -1, 2]])), 0.5),
    lambda: meshops.simplify_vertex_clustering((TRI_V[:, :2], TRI_F), 0.5),
    lambda: dropin.install(tsdf_simplify_voxel=0.0),
    lambda: dropin.install(tsdf_simplify_voxel=-0.1),
    lambda: dropin.install(tsdf_simplify_voxel="0.02"),
    lambda: dropin.install(tsdf_simplify_voxel=0.02, tsdf_min_component_faces=-1),
    lambda: dropin.install(tsdf_simplify_voxel=0.02, mesh_orient="last"),
])
def test_bad_arguments_raise_before_any_device_call(call, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was reached")
    monkeypatch.setattr(meshops.geomargs, "device", no_device)
    with pytest.raises(ValueError):
        call()
    assert evaluator.TSDF_SIMPLIFY_VOXEL is None and evaluator.TSDF_MIN_COMPONENT_FACES is None


def test_a_frame_wider_than_the_key_is_refused():
    with pytest.raises(ValueError, match="voxels"):
        voxel.frame((0.0, 0.0, 0.0), (1.0e7, 1.0, 1.0), 1.0)


def test_wrong_container_types_raise_type_error():
    with pytest.raises(TypeError):
        meshops.simplify_vertex_clustering("mesh.ply", 0.5)


def test_binding_refuses_shapes_before_the_device():
    f64 = lambda *shape: torch.zeros(*shape, dtype=torch.float64)          # noqa: E731
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64)            # noqa: E731
    origin = (0.0, 0.0, 0.0)
    with pytest.raises(lib.VfnError, match=r"faces \[m,3\] with m >= 1"):
        lib.face_planes(f64(3, 3), i64(0, 3), origin)
    with pytest.raises(lib.VfnError, match="origin three values"):
        lib.face_planes(f64(3, 3), i64(1, 3), (0.0, 0.0))
    with pytest.raises(lib.VfnError, match=r"planes must be \[m,5\]"):
        lib.cluster_quadrics(f64(4, 3), i64(5), i64(3), f64(2, 3), f64(2, 3), origin, 1.0, 1e-9)
    with pytest.raises(lib.VfnError, match="entries"):
        lib.cluster_quadrics(f64(4, 5), i64(5), i64(7), f64(6, 3), f64(6, 3), origin, 1.0, 1e-9)
    with pytest.raises(lib.VfnError, match="entries"):
        lib.cluster_quadrics(f64(4, 5), i64(5), i64(1), f64(0, 3), f64(0, 3), origin, 1.0, 1e-9)
    with pytest.raises(lib.VfnError, match=r"centres and means must be \[2,3\]"):
        lib.cluster_quadrics(f64(4, 5), i64(5), i64(3), f64(3, 3), f64(2, 3), origin, 1.0, 1e-9)
    # host tensors never reach the library: there is no CPU path
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.face_planes(f64(3, 3), i64(1, 3), origin)
    with pytest.raises(lib.VfnError, match="CUDA/HIP tensor"):
        lib.cluster_quadrics(f64(4, 5), i64(5), i64(3), f64(2, 3), f64(2, 3), origin, 1.0, 1e-9)
    lib.simplify_check(0)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.simplify_check(2)
    with pytest.raises(lib.VfnError, match="non-finite"):
        lib.simplify_check(1)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is visible: the call would run")
def test_no_cpu_fallback():
    for contraction in S.CONTRACTIONS:
        with pytest.raises(lib.VfnError, match="no GPU"):
            meshops.simplify_vertex_clustering(TRI, 0.5, contraction=contraction)


# ---------------------------------------------------------------------------------------------------------------------------------
# the call paths, the device stood in for
# ---------------------------------------------------------------------------------------------------------------------------------
def test_evaluator_simplifies_only_with_the_switch(tmp_path, monkeypatch):
    """evaluator.tsdf_mesh with the reference's modules stood in for and the device calls stubbed: with the switch clear neither the
    simplification nor anything new is reached and the file is the fused mesh; with it set the culling (if asked for) comes first, the
    simplification is asked for "quadric" with the colours, and the normals are those of the simplified mesh."""
    from PIL import Image
    from vf_nerf_amd import ply, tsdf
    os.makedirs(tmp_path / "rendered_images")
    np.save(tmp_path / "rendered_images" / "depth-0.npy", np.ones((4, 5, 1)))
    Image.fromarray(np.zeros((4, 5, 3), dtype=np.uint8)).save(tmp_path / "rendered_images" / "image-0.png")

    class Dataset:
        def __init__(self, config):
            self.intrinsics, self.poses = torch.eye(4), torch.eye(4)[None]

    v = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0.5, 0], [2, 1.5, 1]])
    f = np.array([[0, 1, 2], [3, 4, 5]])
    colours = np.round(np.linspace(0, 1, 18).reshape(6, 3) * 255) / 255
    calls = []

    def simplify(mesh, voxel_size, contraction="average", colours=None, normals=None, rcond=1e-9, device=None):
        calls.append(("simplify", tuple(mesh[0].shape), voxel_size, contraction, None if colours is None else tuple(colours.shape), normals))
        none = torch.zeros(0)
        return meshops.Simplified(mesh[0][:3] + 0.5, torch.tensor([[0, 1, 2]]), none, none, colours[:3] * 0.5, None, none, none, 3)

    def cull(mesh, min_faces=None, **kw):
        calls.append(("cull", min_faces))
        return mesh[0][3:], torch.tensor([[0, 1, 2]]), torch.tensor([1]), torch.tensor([-1, -1, -1, 0, 1, 2])

    def vertex_normals(mesh, device=None):
        calls.append(("normals", tuple(mesh[0].shape)))
        return torch.ones(mesh[0].shape[0], 3, dtype=torch.float64) * torch.tensor([0.0, 0.6, 0.8], dtype=torch.float64)

    monkeypatch.setattr(tsdf, "fuse_rgbd_maps", lambda *a, **k: (torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(colours)))
    monkeypatch.setattr(meshops, "simplify_vertex_clustering", simplify)
    monkeypatch.setattr(meshops, "filter_components", cull)
    monkeypatch.setattr(meshops, "vertex_normals", vertex_normals)
    names = ("datasets", "datasets.normal_datasets")
    saved = {key: sys.modules[key] for key in names if key in sys.modules}
    fakes = {key: types.ModuleType(key) for key in names}
    fakes["datasets"].__path__ = []
    fakes["datasets.normal_datasets"].dataset_dict = {"fake": Dataset}
    path = str(tmp_path / "tsdf-mesh" / "tsdf.ply")
    files, raw, asked = {}, {}, {}
    try:
        sys.modules.update(fakes)
        for switch, min_faces, with_normals in ((None, None, False), (0.5, None, False), (0.5, 7, True)):
            monkeypatch.setattr(evaluator, "TSDF_SIMPLIFY_VOXEL", switch)
            monkeypatch.setattr(evaluator, "TSDF_MIN_COMPONENT_FACES", min_faces)
            monkeypatch.setattr(evaluator, "TSDF_VERTEX_NORMALS", with_normals)
            del calls[:]
            evaluator.tsdf_mesh(str(tmp_path), types.SimpleNamespace(dataset_name="fake"))
            files[switch, min_faces] = ply.read_ply(path, normals=True)
            raw[switch, min_faces] = open(path, "rb").read()
            asked[switch, min_faces] = list(calls)
    finally:
        for key in names:
            del sys.modules[key]
        sys.modules.update(saved)
    ply.write_ply(str(tmp_path / "as_fused.ply"), v, f, colours)
    assert asked[None, None] == [] and raw[None, None] == open(tmp_path / "as_fused.ply", "rb").read()
    assert asked[0.5, None] == [("simplify", (6, 3), 0.5, "quadric", (6, 3), None)]
    vs, fs, cs, ns = files[0.5, None]
    assert np.array_equal(vs, v[:3] + 0.5) and np.array_equal(fs, [[0, 1, 2]]) and np.array_equal(cs, ply.colour_bytes(colours[:3] * 0.5)) and ns is None
    assert asked[0.5, 7] == [("cull", 7), ("simplify", (3, 3), 0.5, "quadric", (3, 3), None), ("normals", (3, 3))]
    vs, fs, cs, ns = files[0.5, 7]
    assert np.array_equal(vs, v[3:] + 0.5) and np.array_equal(cs, ply.colour_bytes(colours[3:] * 0.5))
    assert np.array_equal(ns, np.tile(np.array([0.0, 0.6, 0.8], dtype=np.float32).astype(np.float64), (3, 1)))


def test_install_sets_the_switch(monkeypatch):
    monkeypatch.setattr(evaluator, "TSDF_SIMPLIFY_VOXEL", None)
    source = inspect.getsource(dropin.install)
    assert "evaluator.TSDF_SIMPLIFY_VOXEL = tsdf_simplify_voxel" in source
    assert "TSDF_SIMPLIFY_VOXEL is not None" in inspect.getsource(evaluator.tsdf_mesh)
    assert '"quadric"' in inspect.getsource(evaluator.tsdf_mesh)
