"""Orientation on the MI355X (csrc/vfn_orient.hip through vf_nerf_amd/meshops.py and mesh.extract_mesh) against the CPU restatement of its
contract (tests/orient_restatement.py).  Every comparison is bit for bit: flip, face_label, first_face, face_count, orientable,
flipped_count, the vote sums and the rewound faces."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, mesh, meshops  # noqa: E402
import meshops_restatement as M  # noqa: E402
import orient_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = R.shapes()
CASES = [(name, reference) for name in SHAPES for reference in meshops.REFERENCES]          # the package's own list: every case is one it offers
_want = {}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def want(name, reference):
    """The restatement of a shape, computed once and shared."""
    if (name, reference) not in _want:
        _want[name, reference] = R.orientation(*SHAPES[name], reference, R.VIEWPOINTS if reference == "viewpoints" else None)
    return _want[name, reference]


def host(o, faces) -> dict:
    """An ``Orientation`` and the rewound faces -> the restatement's dictionary of numpy arrays, placement and dtypes checked on the way."""
    for t in (o.face_label, o.first_face, o.face_count, o.flipped_count):
        assert t.is_cuda and t.dtype == torch.int64
    for t in (o.flip, o.orientable):
        assert t.is_cuda and t.dtype == torch.bool
    assert isinstance(o.n_components, int) and isinstance(o.inconsistent_edges, int)
    assert o.first_face.shape == o.face_count.shape == o.orientable.shape == o.flipped_count.shape == (o.n_components,)
    assert o.votes is None or (o.votes.is_cuda and o.votes.dtype == torch.float64 and o.votes.shape == (o.n_components,))
    assert faces.is_cuda and faces.dtype == torch.int64 and faces.is_contiguous()
    return {"flip": o.flip.cpu().numpy(), "face_label": o.face_label.cpu().numpy(), "n_components": o.n_components,
            "first_face": o.first_face.cpu().numpy(), "face_count": o.face_count.cpu().numpy(), "orientable": o.orientable.cpu().numpy(),
            "flipped_count": o.flipped_count.cpu().numpy(), "inconsistent_edges": o.inconsistent_edges,
            "votes": None if o.votes is None else o.votes.cpu().numpy(), "faces": faces.cpu().numpy()}


def assert_same(got: dict, ref: dict, what):
    assert got["n_components"] == ref["n_components"], (what, got["n_components"], ref["n_components"])
    assert got["inconsistent_edges"] == ref["inconsistent_edges"], (what, got["inconsistent_edges"], ref["inconsistent_edges"])
    for key in ("flip", "face_label", "first_face", "face_count", "orientable", "flipped_count", "faces"):
        assert got[key].shape == ref[key].shape and got[key].dtype == ref[key].dtype and np.array_equal(got[key], ref[key]), (what, key)
    if ref["votes"] is None:
        assert got["votes"] is None, what
    else:
        assert np.array_equal(bits(got["votes"]), bits(ref["votes"])), f"{what}: vote sums differ in {int((bits(got['votes']) != bits(ref['votes'])).sum())} values"


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: every shape, every reference
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,reference", CASES)
def test_orientation_equals_the_restatement(name, reference):
    """One face; the 64 x 64 sheet with a random half flipped (8192 lanes on one root, 96 blocks) and a face-permuted copy; the strip of
    4096 alternately flipped triangles (one deep chain); the Möbius strip (reported, untouched); a closed sphere and a torus with random
    flips, and a sphere inside out; two sheets; a fin of three faces on an edge; duplicated faces; faces naming a vertex twice; the
    five recorded contrastive marching-cubes meshes — by first face, majority, volume and viewpoints."""
    v, f = SHAPES[name]
    views = R.VIEWPOINTS if reference == "viewpoints" else None
    vertices, faces, o = meshops.orient((v, f), reference=reference, viewpoints=views)
    assert np.array_equal(bits(vertices.cpu().numpy()), bits(v))
    got = host(o, faces)
    assert_same(got, want(name, reference), (name, reference))
    if R.ORIENTABLE(name):
        assert meshops.inconsistent_edges((vertices, faces)) == 0
    else:
        assert got["orientable"].tolist() == [False] and np.array_equal(got["faces"], f)


def test_orientation_alone_and_the_edge_count():
    v, f = SHAPES["f32"]
    o = meshops.orientation((torch.from_numpy(v).to(DEV), torch.from_numpy(f.astype(np.int32)).to(DEV)), reference="majority")
    ref = want("f32", "majority")
    assert np.array_equal(o.flip.cpu().numpy(), ref["flip"]) and o.inconsistent_edges == ref["inconsistent_edges"] > 0
    assert meshops.inconsistent_edges((v, f)) == ref["inconsistent_edges"]
    assert meshops.inconsistent_edges((v, np.zeros((0, 3), dtype=np.int64))) == 0
    none = meshops.orient((v, np.zeros((0, 3), dtype=np.int64)), reference="volume")
    assert none[1].shape == (0, 3) and none[2].n_components == 0 and none[2].flip.shape == (0,) and none[2].votes.shape == (0,)


def test_vertex_normals_of_the_oriented_mesh():
    """What the orientation is for: on the rewound f32 mesh the vertex normals are those of the restatement on the restated faces — and
    no longer those of the mesh as extracted, whose opposite faces cancel."""
    v, f = SHAPES["f32"]
    _, faces, _ = meshops.orient((v, f), reference="volume")
    ref_faces = want("f32", "volume")["faces"]
    assert np.array_equal(faces.cpu().numpy(), ref_faces)
    got = meshops.vertex_normals((v, faces)).cpu().numpy()
    assert np.array_equal(bits(got), bits(M.vertex_normals(v, ref_faces)))
    assert not np.array_equal(bits(got), bits(M.vertex_normals(v, f)))


class FieldDecoder:
    """Serves a precomputed field [res^3,3] to mesh.extract_mesh in the order it asks for the lattice rows."""

    def __init__(self, field):
        self.field, self.row = field, 0

    def __call__(self, pts):
        out = self.field[self.row:self.row + pts.shape[0]]
        self.row += pts.shape[0]
        return out


def test_extract_mesh_orients_what_it_would_have_returned():
    fix = np.load(os.path.join(REPO, "tests", "golden", "mesh_stages.npz"))
    field = torch.from_numpy(fix["f24.pred"]).to(DEV)
    kw = dict(scale=1.3, translation=torch.tensor([0.05, -0.02, 0.01]), centroid=torch.tensor([0.0, 0.1, -0.05]))
    plain = mesh.extract_mesh(FieldDecoder(field), 24, **kw)
    assert np.array_equal(plain.faces.cpu().numpy(), fix["f24.fs"] - 1)                       # the default: the reference's faces, every bit
    for reference in mesh.ORIENT_REFERENCES:
        got = mesh.extract_mesh(FieldDecoder(field), 24, orient=reference, **kw)
        _, by_hand, o = meshops.orient(plain, reference=reference)
        assert torch.equal(got.faces, by_hand) and torch.equal(got.vertices, plain.vertices) and torch.equal(got.vertices_scaled, plain.vertices_scaled)
        assert o.inconsistent_edges > 0 and meshops.inconsistent_edges(got) == 0
        ref = R.orientation(plain.vertices_scaled.cpu().numpy(), plain.faces.cpu().numpy(), reference)
        assert np.array_equal(got.faces.cpu().numpy(), ref["faces"])


def test_the_drop_in_with_the_switch_lists_the_oriented_faces(monkeypatch):
    """mesh.contrastive_marching_cubes on the recorded f16 cells: with mesh.ORIENT set its 1-based faces are the restatement's rewinding of
    the reference's recorded faces, over the same vertex dictionary; with None every bit is the reference's."""
    fix = np.load(os.path.join(REPO, "tests", "golden", "mesh_stages.npz"))
    kw = dict(comb_values=fix["f16.comb"].reshape(-1), udf=fix["f16.udf"].reshape(-1, 2), selected_indices=fix["f16.cells"], res=16)
    monkeypatch.setattr(mesh, "ORIENT", None)
    vs, fs = mesh.contrastive_marching_cubes(**kw)
    assert fs == fix["f16.fs"].tolist() and np.array_equal(bits(np.array(list(vs.keys()))), bits(fix["f16.vs"]))
    for reference in mesh.ORIENT_REFERENCES:
        monkeypatch.setattr(mesh, "ORIENT", reference)
        vs2, fs2 = mesh.contrastive_marching_cubes(**kw)
        ref = want("f16", reference)
        assert vs2 == vs and list(vs2.values()) == list(range(1, len(vs) + 1))
        assert isinstance(fs2, list) and all(type(q) is int for q in fs2[0]) and fs2 == (ref["faces"] + 1).tolist() and fs2 != fs
        assert R.count_inconsistent(np.array(fs2) - 1, len(vs2)) == 0


@pytest.mark.parametrize("reference", meshops.REFERENCES)
def test_the_plumbing_reads_the_host_twice(reference):
    """At most two host reads per call, as ``_components`` is meant to: K inside ``torch.unique``, and the status words with the count of
    inconsistent edges.  Counted by torch's synchronisation debug mode (which sees ``nonzero``, boolean-mask indexing, ``bincount``,
    ``.item()`` and ``.cpu()``), on a mesh already on the device."""
    import warnings
    v, f = (torch.from_numpy(x).to(DEV) for x in SHAPES["f32"])
    views = torch.from_numpy(R.VIEWPOINTS).to(DEV) if reference == "viewpoints" else None
    meshops._orientation(v, f, reference, views)                                   # (first use of anything is not what is counted)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            o = meshops._orientation(v, f, reference, views)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    reads = [w for w in seen if "called a synchronizing" in str(w.message)]          # (not the mode's own once-only notice that it is a prototype)
    assert len(reads) <= 2, [str(w.message) for w in reads]
    assert np.array_equal(o.flip.cpu().numpy(), want("f32", reference)["flip"])


def test_device_viewpoints_are_checked_by_the_kernel():
    """Viewpoints already on the device are not read back to be checked: a non-finite one is the vote kernel's status bit."""
    v, f = SHAPES["two_sheets"]
    views = torch.from_numpy(R.VIEWPOINTS).to(DEV)
    got = meshops.orientation((v, f), reference="viewpoints", viewpoints=views)
    assert np.array_equal(got.flip.cpu().numpy(), want("two_sheets", "viewpoints")["flip"])
    views[2, 1] = float("nan")
    with pytest.raises(lib.VfnError, match="non-finite"):
        meshops.orientation((v, f), reference="viewpoints", viewpoints=views)
    with pytest.raises(ValueError, match="non-finite"):
        meshops.orientation((v, f), reference="viewpoints", viewpoints=views.cpu())


# ---------------------------------------------------------------------------------------------------------------------------------
# 2: the kernels on their own
# ---------------------------------------------------------------------------------------------------------------------------------
def dev(x, dtype):
    return torch.tensor(x, dtype=dtype, device=DEV)


def test_forest_roots_and_parities_equal_the_serial_walk():
    for name in ("sheet_64", "strip_4096", "f32"):
        v, f = SHAPES[name]
        keys, nodes, dirs = (torch.from_numpy(x).to(DEV) for x in R.items(f, len(v)))
        mine = meshops.orient_items(torch.from_numpy(f).to(DEV), len(v))
        assert all(torch.equal(a, b) for a, b in zip(mine, (keys, nodes, dirs)))              # the items are the restatement's
        assert all(torch.equal(a, b) for a, b in zip(mine[:2], meshops.component_items(torch.from_numpy(f).to(DEV), len(v), "edge")))
        forest = lib.orient_union_runs(keys, nodes, dirs, torch.arange(0, 2 * len(f), 2, dtype=torch.int32, device=DEV))
        root, parity = lib.orient_flatten(forest)
        ref_root, ref_parity, conflict = R.parity_serial(f, len(v))
        assert not conflict.any() and parity.dtype == torch.uint8
        assert np.array_equal(root.cpu().numpy(), ref_root) and np.array_equal(parity.cpu().numpy(), ref_parity), name
        words = forest.cpu().numpy()
        assert ((words >> 1) <= np.arange(len(f))).all() and (words[ref_root == np.arange(len(f))] & 1 == 0).all()


def test_votes_equal_the_formulas_face_by_face():
    v, f = SHAPES["torus"]
    parity = (np.arange(len(f)) % 3 == 0).astype(np.uint8)
    vd, fd, pd = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(parity).to(DEV)
    assert np.array_equal(bits(lib.orient_votes(vd, fd, pd, lib.ORIENT_VOLUME).cpu().numpy()), bits(R.votes_volume(v, f, parity)))
    assert np.array_equal(bits(lib.orient_votes(vd, fd, None, lib.ORIENT_VOLUME).cpu().numpy()), bits(R.votes_volume(v, f, 0 * parity)))
    for views in (R.VIEWPOINTS, R.VIEWPOINTS[:1], np.concatenate((R.VIEWPOINTS, v[f[7]].mean(axis=0, keepdims=True), v[:3]))):
        got = lib.orient_votes(vd, fd, pd, lib.ORIENT_VIEWPOINTS, torch.from_numpy(views).to(DEV)).cpu().numpy()
        assert np.array_equal(bits(got), bits(R.votes_viewpoints(v, f, parity, views)))
    # a viewpoint exactly at a face's centroid: s == 0, t = 0
    tri = np.array([[0.0, 0, 0], [3, 0, 0], [0, 3, 0]])
    got = lib.orient_votes(dev(tri, torch.float64), dev([[0, 1, 2]], torch.int64), None, lib.ORIENT_VIEWPOINTS, dev([[1.0, 1.0, 0.0]], torch.float64))
    assert got.cpu().tolist() == [0.0]


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: values that must never reach an address
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [4, -1, 1 << 40, -(1 << 62)])
def test_a_node_outside_its_range_sets_the_status(bad):
    keys, dirs = dev([3, 3, 5, 5, 6], torch.int64), dev([1, 1, 0, 1, 1], torch.uint8)
    forest = torch.arange(0, 8, 2, dtype=torch.int32, device=DEV)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.orient_union_runs(keys, dev([0, 1, 2, bad, 3], torch.int64), dirs, forest.clone())
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = lib.orient_union_runs(keys, dev([0, 1, 2, bad, 3], torch.int64), dirs, forest.clone(), info=info)
    assert int(info.cpu()) == 2 and out.cpu().tolist() == [0, 1, 4, 6]              # the good pair is united (parity 1), the bad one not followed
    # negative keys are no keys, a run of three connects nothing, two items of one face connect nothing: nothing is wrong, nothing is written
    out = lib.orient_union_runs(dev([-1, -1, 7, 7, 7, 9, 9], torch.int64), dev([0, 1, 0, 1, 2, 3, 3], torch.int64),
                                dev([1, 1, 1, 1, 1, 0, 1], torch.uint8), forest.clone())
    assert out.cpu().tolist() == [0, 2, 4, 6]


@pytest.mark.parametrize("words", [[0, 0, 3 << 1, 4], [0, 0, 9 << 1, 4], [0, 0, -2, 4], [0, 0, -(1 << 31), 4], [0, 0, (1 << 31) - 1, 4],
                                   [0, 0, (2 << 1) | 1, 4], [1, 0, 0, 4], [0x55555555, 0x2AAAAAAA, -1, 0x7FFFFFFE]])
def test_a_forest_that_is_not_ours_is_reported(words):
    """Words whose parent leaves [0, its node], or a root word with its parity bit set: the range guard of csrc/vfn_forest_core.h ends the
    walk before the word indexes anything.  Neither the flatten nor the unions follow it."""
    forest = dev(words, torch.int32)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.orient_flatten(forest)
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    root, parity = lib.orient_flatten(forest, info=info)
    assert int(info.cpu()) == 2 and (root.cpu().numpy() == -1).any() and parity.cpu().numpy()[root.cpu().numpy() == -1].tolist() == [0] * int((root == -1).sum())
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.orient_union_runs(dev([1, 1, 2, 2], torch.int64), dev([0, 2, 1, 3], torch.int64), dev([1, 1, 1, 1], torch.uint8), forest.clone())
    good = lib.orient_flatten(dev([0, 0 | 1, (1 << 1) | 1, (2 << 1) | 0], torch.int32))
    assert good[0].cpu().tolist() == [0, 0, 0, 0] and good[1].cpu().tolist() == [0, 1, 0, 0]


@pytest.mark.parametrize("face", [[0, 1, 3], [0, -1, 2], [1 << 40, 1, 2], [0, 1, -(1 << 62)]])
def test_a_face_index_outside_its_range_sets_the_status(face):
    v = dev([[0.0, 0, 1], [1, 0, 1], [0, 1, 1]], torch.float64)
    f = dev([[0, 1, 2], face], torch.int64)
    for mode, views in ((lib.ORIENT_VOLUME, None), (lib.ORIENT_VIEWPOINTS, dev([[0.0, 0.0, 5.0]], torch.float64))):
        with pytest.raises(lib.VfnError, match="outside its range"):
            lib.orient_votes(v, f, None, mode, views)
        info = torch.zeros(1, dtype=torch.int64, device=DEV)
        out = lib.orient_votes(v, f, None, mode, views, info=info).cpu().numpy()
        assert int(info.cpu()) == 2 and out[1] == 0.0 and out[0] > 0


def test_a_non_finite_coordinate_sets_the_status():
    v = dev([[0.0, 0, 1], [1, float("nan"), 1], [0, 1, 1], [0, 0, 2], [1, 0, 2], [0, 1, 2]], torch.float64)
    f = dev([[3, 4, 5], [0, 1, 2]], torch.int64)
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    lib.orient_votes(v, f, None, lib.ORIENT_VOLUME, info=info)
    assert int(info.cpu()) == 1
    info.zero_()
    lib.orient_votes(v, f[:1].contiguous(), None, lib.ORIENT_VIEWPOINTS, dev([[0.0, float("inf"), 5.0]], torch.float64), info=info)
    assert int(info.cpu()) == 1
    with pytest.raises(lib.VfnError, match="non-finite"):
        meshops.orientation((v, f), reference="volume")
    assert meshops.orientation((v, f), reference="first").n_components == 2          # (no coordinate is read without a vote)
