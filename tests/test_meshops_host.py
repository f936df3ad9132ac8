"""Mesh normals, welding, PLY normals and the evaluator's switch without a device: the contract in the header and the library's exports,
the NumPy restatement (tests/meshops_restatement.py) on closed-form cases and against an independent formulation, every refusal that
answers before a launch, and the PLY writer and reader byte for byte."""
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, meshops, metrics3d, ply, refuse  # noqa: E402
import meshops_restatement as M  # noqa: E402

NEW_EXPORTS = ("vfn_face_normals", "vfn_vertex_normals", "vfn_normal_dots")

OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
# the eight faces wound outwards: (a x b) . centroid > 0
OCTA_F = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int64)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


# ---- the contract ------------------------------------------------------------------------------------------------------
def test_header_declares_the_three_entry_points_and_abi_stays_5():
    protos = lib.header_prototypes()
    assert lib.header_abi_version() == 5
    assert protos["vfn_face_normals"] == ("int", ["const double*", "int64_t", "const int64_t*", "int64_t", "int32_t", "double*", "int64_t*", "void*"])
    assert protos["vfn_vertex_normals"] == ("int", ["const double*", "int64_t", "const int64_t*", "const int64_t*", "int64_t", "double*", "int64_t*",
                                                    "void*"])
    assert protos["vfn_normal_dots"] == ("int", ["const double*", "int64_t", "const double*", "int64_t", "const int64_t*", "double*", "int64_t*",
                                                 "void*"])


def test_library_exports_the_symbols_and_checks_arguments_before_any_launch():
    handle = lib.load()
    assert handle.vfn_abi_version() == 5
    for name in NEW_EXPORTS:
        assert name in lib.EXPORTS and hasattr(handle, name)
    # (no device here: every one of these answers from the argument checks)
    assert handle.vfn_face_normals(None, 1 << 31, None, 1, 0, None, None, None) == -1
    assert handle.vfn_face_normals(None, 3, None, 1, 2, None, None, None) == -1            # normalise is 0 or 1
    assert handle.vfn_face_normals(None, 3, None, 1, 1, None, None, None) == -1            # NULL info
    assert handle.vfn_vertex_normals(None, 1, None, None, 1 << 31, None, None, None) == -1
    assert handle.vfn_vertex_normals(None, -1, None, None, 1, None, None, None) == -1
    assert handle.vfn_normal_dots(None, 1, None, 1 << 31, None, None, None, None) == -1
    assert handle.vfn_normal_dots(None, 1, None, 1, None, None, None, None) == -1
    assert b"vfn_normal_dots" in handle.vfn_last_error()
    word = (lib.C.c_int64 * 1)(0)
    assert handle.vfn_face_normals(None, 3, None, 1, 1, None, word, None) == -1            # NULL faces with m = 1
    assert handle.vfn_face_normals(None, 0, None, 0, 1, None, word, None) == 0             # nothing to do: no launch
    assert handle.vfn_vertex_normals(None, 0, None, None, 0, None, word, None) == 0
    assert handle.vfn_normal_dots(None, 0, None, 0, None, None, word, None) == 0
    assert word[0] == 0


# ---- the restatement on closed forms -----------------------------------------------------------------------------------
def test_octahedron_is_wound_outwards():
    c = M.face_normals(OCTA_V, OCTA_F, False)
    assert (np.einsum("ij,ij->i", c, OCTA_V[OCTA_F].mean(axis=1)) > 0).all() and (np.abs(c) == 1.0).all()


def test_restated_octahedron_normals():
    vn = M.vertex_normals(OCTA_V, OCTA_F)
    assert np.array_equal(bits(vn), bits(OCTA_V))                                          # exactly +-e_i
    fn = M.face_normals(OCTA_V, OCTA_F, True)
    want = np.sign(M.face_normals(OCTA_V, OCTA_F, False)) / np.sqrt(3.0)
    assert np.abs(fn - want).max() <= 2 * np.spacing(1.0 / np.sqrt(3.0))
    raw = M.face_normals(OCTA_V, OCTA_F, False)
    assert np.array_equal(np.sqrt((raw * raw).sum(axis=1)) / 2, np.full(8, np.sqrt(3.0) / 2))          # |c| is twice the area


def test_restated_fallbacks():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [5, 5, 5]])
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 3, 1]])                    # a face without area, then two opposite faces
    assert np.array_equal(M.face_normals(v, f, True), [[0, 0, 0], [0, 0, 1], [0, 0, -1]])
    vn = M.vertex_normals(v, f)
    assert np.array_equal(vn[4], [0, 0, 1])                            # no face
    assert np.array_equal(vn[0], [0, 0, 1]) and np.array_equal(vn[2], [0, 0, 1])          # a sum without length: the fallback
    out, overflow = M.unit(np.array([[1e200, 0, 0], [0.0, 0, 0], [3, 4, 0]]), (0.0, 0.0, 1.0))
    assert overflow.tolist() == [True, False, False] and np.array_equal(out, [[0, 0, 1], [0, 0, 1], [0.6, 0.8, 0]])


def test_vertex_faces_on_host_tensors_equals_the_restated_rows():
    g = np.random.default_rng(3)
    n, m = 40, 300
    f = g.integers(0, n - 1, (m, 3))                                   # vertex n - 1 has no face; repeated indices occur
    f[7] = (5, 5, 9)
    row_start, incident = meshops.vertex_faces(torch.from_numpy(f), n)
    want_start, want_incident = M.csr(M.vertex_faces(f, n))
    assert row_start.dtype == torch.int64 and incident.dtype == torch.int64
    assert np.array_equal(row_start.numpy(), want_start) and np.array_equal(incident.numpy(), want_incident)
    assert want_start[-1] == want_start[-2] and (np.asarray(M.vertex_faces(f, n)[5]) == 7).sum() == 1
    row_start, incident = meshops.vertex_faces(np.zeros((0, 3), dtype=np.int64), 4)
    assert row_start.tolist() == [0] * 5 and incident.numel() == 0


# ---- weld: the restatement against an independent formulation ----------------------------------------------------------
def weld_by_unique(vertices, faces, digits):
    """np.unique over the key rows of the referenced vertices, its classes reordered by first index."""
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    used = np.unique(f)
    vr = v[used]
    keys = (vr if digits is None else np.rint(vr * 10.0 ** digits)) + 0.0
    _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    inverse = np.full(v.shape[0], -1, dtype=np.int64)
    inverse[used] = rank[inv.reshape(-1)]
    return vr[first[order]], inverse[f], inverse


def soup(seed=5, n=30, m=50):
    """A mesh with every vertex duplicated per face: 3 m vertices, face j = (3 j, 3 j + 1, 3 j + 2)."""
    g = np.random.default_rng(seed)
    v = g.integers(-3, 4, (n, 3)).astype(np.float64) / 4
    f = g.integers(0, n, (m, 3))
    return v[f.reshape(-1)], np.arange(3 * m, dtype=np.int64).reshape(m, 3), v, f


def weld_cases():
    sv, sf, _, _ = soup()
    zeros = np.array([[0.0, 1, 2], [-0.0, 1, 2], [0, -0.0, 2], [1, 1, 1], [0, 0, 2.0]])
    close = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1 + 3e-9, 0, 0], [0, 1, 3e-9], [7, 7, 7]])
    return {
        "soup": (sv, sf),
        "signed zeros": (zeros, np.array([[0, 3, 2], [1, 4, 3]])),
        "unreferenced": (np.arange(30, dtype=np.float64).reshape(10, 3), np.array([[7, 2, 4], [4, 2, 9]])),
        "3e-9 apart": (close, np.array([[0, 1, 2], [0, 3, 4]])),
        "degenerate after the merge": (close, np.array([[1, 3, 2], [0, 1, 2], [2, 4, 4]])),
    }


@pytest.mark.parametrize("name", list(weld_cases()))
@pytest.mark.parametrize("digits", [None, 8, 0])
def test_restated_weld_equals_unique_formulation(name, digits):
    v, f = weld_cases()[name]
    got, want = M.weld(v, f, digits), weld_by_unique(v, f, digits)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[1].shape == f.shape and got[0].shape[0] == got[2].max() + 1
    assert (got[2] >= 0).sum() == np.unique(f).shape[0]


def test_restated_weld_properties():
    sv, sf, v, f = soup()
    wv, wf, inverse = M.weld(sv, sf, None)
    assert wv.shape[0] == np.unique(v[np.unique(f)], axis=0).shape[0] and np.array_equal(wv[wf], v[f])          # the mesh is the indexed one again
    assert (np.diff([np.nonzero(inverse == k)[0][0] for k in range(wv.shape[0])]) > 0).all()                    # ascending representatives
    zv, zf = weld_cases()["signed zeros"]
    wv, wf, inverse = M.weld(zv, zf, None)
    assert inverse.tolist() == [0, 0, 1, 2, 1] and np.signbit(wv[0, 0]) == np.signbit(zv[0, 0]) and wv.shape[0] == 3
    assert np.array_equal(bits(wv[1]), bits(zv[2]))                                                            # the lowest index's bits: -0.0 kept
    uv, uf = weld_cases()["unreferenced"]
    wv, wf, inverse = M.weld(uv, uf, 8)
    assert inverse.tolist() == [-1, -1, 0, -1, 1, -1, -1, 2, -1, 3] and np.array_equal(wv, uv[[2, 4, 7, 9]]) and np.array_equal(wf, [[2, 0, 1], [1, 0, 3]])
    cv, cf = weld_cases()["3e-9 apart"]
    assert M.weld(cv, cf, None)[0].shape[0] == 5 and M.weld(cv, cf, 8)[0].shape[0] == 3                        # they merge only when rounded
    assert np.array_equal(M.weld(cv, cf, 8)[0], cv[:3])                                                        # original bits, not rounded ones
    dv, df = weld_cases()["degenerate after the merge"]
    wv, wf, _ = M.weld(dv, df, 8)
    assert wf.tolist() == [[1, 1, 2], [0, 1, 2], [2, 2, 2]]                                                    # kept, in place


# ---- refusals that need no device --------------------------------------------------------------------------------------
def test_refusals_answer_before_any_device_is_asked_for(tmp_path):
    tri = (OCTA_V, OCTA_F)
    for bad in (-1, 16, 2.0, True, "8"):
        with pytest.raises(ValueError, match="digits"):
            meshops.weld(tri, digits=bad)
    out_of_range = (OCTA_V, np.array([[0, 1, 6]]))
    negative = (OCTA_V, np.array([[0, -1, 2]]))
    for bad in (out_of_range, negative):
        for call in (meshops.face_normals, meshops.vertex_normals, meshops.weld):
            with pytest.raises(ValueError, match="face index"):
                call(bad)
        with pytest.raises(ValueError, match="face index"):
            meshops.vertex_faces(bad[1], 6)
    with pytest.raises(ValueError):
        meshops.face_normals(tri, normalise=1)
    with pytest.raises(ValueError):
        meshops.face_normals((OCTA_V.astype(np.int64), OCTA_F))
    with pytest.raises(TypeError):
        meshops.vertex_normals(OCTA_V)
    with pytest.raises(ValueError):
        meshops.vertex_faces(OCTA_F.astype(np.float64), 6)
    with pytest.raises(ValueError):
        meshops.vertex_faces(OCTA_F, -1)
    # normals= of the wrong shape or type
    path = str(tmp_path / "bad.ply")
    for bad in (np.zeros((5, 3)), np.zeros((6, 2)), np.zeros(18), np.zeros((6, 3), dtype=np.int32)):
        with pytest.raises(ValueError, match="normals"):
            ply.write_ply(path, OCTA_V, OCTA_F, normals=bad)
    # normals=True with an empty mesh, or with something that is not a bool
    empty = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
    with pytest.raises(ValueError, match="no faces"):
        metrics3d.score_mesh(empty, tri, num_points=10, normals=True)
    with pytest.raises(ValueError, match="no faces"):
        metrics3d.score_mesh(tri, empty, num_points=10, normals=True)
    with pytest.raises(ValueError, match="no faces"):
        metrics3d.normal_consistency(empty, tri, num_points=10)
    with pytest.raises(ValueError, match="normals"):
        metrics3d.score_mesh(tri, tri, num_points=10, normals="yes")
    with pytest.raises(ValueError):
        metrics3d.normal_consistency(tri, tri, num_points=0)


def test_metrics_3d_passes_normals_only_when_asked(monkeypatch):
    seen = []
    monkeypatch.setattr(refuse, "reconstruction_meshes", lambda *a, **k: {name: (torch.zeros(1, 3), None) for name in refuse.MESH_NAMES})
    monkeypatch.setattr(metrics3d, "score_mesh", lambda *a, **k: seen.append(k) or {})
    refuse.metrics_3d(None, None, None, None, 4, 4)
    assert len(seen) == 4 and all("normals" not in k for k in seen)
    refuse.metrics_3d(None, None, None, None, 4, 4, normals=True)
    assert len(seen) == 8 and all(k["normals"] is True for k in seen[4:])


# ---- PLY ---------------------------------------------------------------------------------------------------------------
TRI_V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
TRI_F = np.array([[0, 1, 2]])
TRI_BYTES = (b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
             b"element face 1\nproperty list uchar int vertex_indices\nend_header\n"
             b"\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00\x00"
             b"\x00\x00\x80\x3f\x00\x00\x00\x00\x00\x00\x00\x00"
             b"\x00\x00\x00\x00\x00\x00\x80\x3f\x00\x00\x00\x00"
             b"\x03\x00\x00\x00\x00\x01\x00\x00\x00\x02\x00\x00\x00")


def test_a_file_without_normals_is_what_it_was(tmp_path):
    path = str(tmp_path / "tri.ply")
    ply.write_ply(path, TRI_V, TRI_F)
    with open(path, "rb") as fh:
        assert fh.read() == TRI_BYTES
    ply.write_ply(path, TRI_V, TRI_F, normals=None)
    with open(path, "rb") as fh:
        assert fh.read() == TRI_BYTES
    assert len(ply.read_ply(path)) == 3
    v, f, c, nrm = ply.read_ply(path, normals=True)
    assert nrm is None and c is None and np.array_equal(v, TRI_V) and np.array_equal(f, TRI_F)


def test_normals_sit_between_position_and_colour(tmp_path):
    path = str(tmp_path / "tri.ply")
    nrm = np.array([[0.0, 0, 1], [0, 0, 1], [0.6, 0, 0.8]])
    ply.write_ply(path, TRI_V, TRI_F, np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], dtype=np.uint8), normals=nrm)
    with open(path, "rb") as fh:
        raw = fh.read()
    head, body = raw.split(b"end_header\n")
    names = [line.split()[-1] for line in head.decode().splitlines() if line.startswith("property") and "list" not in line]
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert [line.split()[1] for line in head.decode().splitlines() if line.startswith("property") and "list" not in line] == ["float"] * 6 + ["uchar"] * 3
    record = 6 * 4 + 3
    assert len(body) == 3 * record + 13
    third = body[2 * record:3 * record]
    assert np.array_equal(np.frombuffer(third[:24], dtype="<f4"), np.array([0, 1, 0, 0.6, 0, 0.8], dtype=np.float32)) and third[24:] == bytes([7, 8, 9])


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("vertex_dtype", ["f4", "f8"])
@pytest.mark.parametrize("coloured", [True, False])
def test_normals_make_the_round_trip(tmp_path, binary, vertex_dtype, coloured):
    g = np.random.default_rng(11)
    n, m = 57, 90
    v, f = g.standard_normal((n, 3)) * 3, g.integers(0, n, (m, 3))
    nrm = M.vertex_normals(v, f)
    nrm[3] = (-0.0, 1e-30, -1.0)
    col = g.integers(0, 256, (n, 3), dtype=np.uint8) if coloured else None
    path = str(tmp_path / "mesh.ply")
    ply.write_ply(path, v, f, col, binary=binary, vertex_dtype=vertex_dtype, normals=torch.from_numpy(nrm))
    rv, rf, rc, rn = ply.read_ply(path, normals=True)
    at = np.float32 if vertex_dtype == "f4" else np.float64                      # bit for bit at the file's precision (an ASCII float is
    assert rn.dtype == np.float64 and rn.shape == (n, 3)                         # read as the double nearest to its shortest text)
    assert np.array_equal(bits(rn.astype(at)), bits(nrm.astype(at))) and np.array_equal(bits(rv.astype(at)), bits(v.astype(at))) and np.array_equal(rf, f)
    if binary:
        assert np.array_equal(bits(rn), bits(nrm.astype(at)))
    assert (rc is None) if col is None else np.array_equal(rc, col)
    three = ply.read_ply(path)                                                   # the default return stays the 3-tuple
    assert len(three) == 3 and np.array_equal(bits(three[0]), bits(rv)) and np.array_equal(three[1], rf)
    # the same mesh without normals: the same vertices, faces and colours
    ply.write_ply(path, v, f, col, binary=binary, vertex_dtype=vertex_dtype)
    pv, pf, pc, pn = ply.read_ply(path, normals=True)
    assert pn is None and np.array_equal(bits(pv), bits(rv)) and np.array_equal(pf, rf) and ((pc is None) if col is None else np.array_equal(pc, col))


def test_normals_of_an_odd_type_are_refused_by_the_reader(tmp_path):
    path = str(tmp_path / "odd.ply")
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nproperty int nx\nproperty int ny\n"
                 b"property int nz\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n0 0 0 1 0 0\n")
    with pytest.raises(ply.PlyError):
        ply.read_ply(path, normals=True)


# ---- the evaluator's switch and the drop-in ----------------------------------------------------------------------------
def test_switch_is_off_after_import_and_install_sets_it():
    from vf_nerf_amd import evaluator
    assert evaluator.TSDF_VERTEX_NORMALS is False
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in ("models", "evaluation")}
    fake_pkg, fake = types.ModuleType("evaluation"), types.ModuleType("evaluation.methods")
    fake_pkg.__path__ = []
    fake.render_images, fake.metrics, fake.tsdf_mesh = (lambda *a, **k: "r"), (lambda *a, **k: "m"), (lambda *a, **k: "t")
    try:
        sys.modules["evaluation"], sys.modules["evaluation.methods"] = fake_pkg, fake
        dropin = importlib.import_module("vf_nerf_amd.dropin")
        dropin.install()
        assert evaluator.TSDF_VERTEX_NORMALS is False                             # None leaves it as it is
        dropin.install(tsdf_vertex_normals=True)
        assert evaluator.TSDF_VERTEX_NORMALS is True
        dropin.install()
        assert evaluator.TSDF_VERTEX_NORMALS is True
        dropin.install(tsdf_vertex_normals=False)
        assert evaluator.TSDF_VERTEX_NORMALS is False
    finally:
        evaluator.TSDF_VERTEX_NORMALS = False
        import vf_nerf_amd.dropin as dropin
        dropin.uninstall_clip_grad_norm()
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "evaluation")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_evaluator_writes_normals_only_with_the_switch(tmp_path, monkeypatch):
    """evaluator.tsdf_mesh with the reference's modules stood in for and the two device calls stubbed: with the switch set the file holds
    what meshops.vertex_normals returned, after x y z; with it clear the file is the one without normals."""
    from PIL import Image
    from vf_nerf_amd import evaluator, tsdf
    os.makedirs(tmp_path / "rendered_images")
    np.save(tmp_path / "rendered_images" / "depth-0.npy", np.ones((4, 5, 1)))
    Image.fromarray(np.zeros((4, 5, 3), dtype=np.uint8)).save(tmp_path / "rendered_images" / "image-0.png")

    class Dataset:
        def __init__(self, config):
            self.intrinsics, self.poses = torch.eye(4), torch.eye(4)[None]

    nrm = M.vertex_normals(OCTA_V, OCTA_F) * 0.5
    colours = np.linspace(0, 1, 18).reshape(6, 3)
    asked = []
    monkeypatch.setattr(tsdf, "fuse_rgbd_maps", lambda *a, **k: (torch.from_numpy(OCTA_V), torch.from_numpy(OCTA_F), torch.from_numpy(colours)))
    monkeypatch.setattr(meshops, "vertex_normals", lambda mesh, device=None: asked.append(mesh) or torch.from_numpy(nrm))
    names = ("datasets", "datasets.normal_datasets")
    saved = {key: sys.modules[key] for key in names if key in sys.modules}
    fakes = {key: types.ModuleType(key) for key in names}
    fakes["datasets"].__path__ = []
    fakes["datasets.normal_datasets"].dataset_dict = {"fake": Dataset}
    files = {}
    try:
        sys.modules.update(fakes)
        for switch in (False, True):
            monkeypatch.setattr(evaluator, "TSDF_VERTEX_NORMALS", switch)
            evaluator.tsdf_mesh(str(tmp_path), types.SimpleNamespace(dataset_name="fake"))
            files[switch] = ply.read_ply(str(tmp_path / "tsdf-mesh" / "tsdf.ply"), normals=True)
            assert len(asked) == int(switch)
    finally:
        for key in names:
            del sys.modules[key]
        sys.modules.update(saved)
    assert files[False][3] is None and np.array_equal(files[True][3], nrm.astype(np.float32).astype(np.float64))
    assert all(np.array_equal(a, b) for a, b in zip(files[False][:3], files[True][:3]))
    assert torch.equal(asked[0][0], torch.from_numpy(OCTA_V)) and torch.equal(asked[0][1], torch.from_numpy(OCTA_F))
