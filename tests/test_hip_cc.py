"""Connected components on the MI355X (csrc/vfn_cc.hip through vf_nerf_amd/meshops.py and metrics3d.score_mesh) against the CPU
restatement of their contract (tests/cc_restatement.py).  Every comparison is bit for bit: face_label, vertex_label, face_count,
first_face, area, the filtered meshes and the scores."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, mesh, meshops, metrics3d  # noqa: E402
import cc_restatement as CC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = CC.shapes()
CASES = [(name, c) for name in SHAPES for c in CC.CONNECTIVITIES]
_want = {}


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def want(name, connectivity):
    """The restatement of a shape, computed once and shared."""
    if (name, connectivity) not in _want:
        _want[name, connectivity] = CC.components(*SHAPES[name], connectivity)
    return _want[name, connectivity]


def host(c) -> dict:
    """A ``Components`` -> the restatement's dictionary of numpy arrays, the placement and dtypes checked on the way."""
    for t in (c.face_label, c.vertex_label, c.face_count, c.first_face):
        assert t.is_cuda and t.dtype == torch.int64
    assert isinstance(c.n_components, int) and c.face_count.shape == c.first_face.shape == (c.n_components,)
    assert c.area is None or (c.area.is_cuda and c.area.dtype == torch.float64 and c.area.shape == (c.n_components,))
    return {"face_label": c.face_label.cpu().numpy(), "vertex_label": c.vertex_label.cpu().numpy(), "n_components": c.n_components,
            "face_count": c.face_count.cpu().numpy(), "area": None if c.area is None else c.area.cpu().numpy(),
            "first_face": c.first_face.cpu().numpy()}


def assert_same_components(got: dict, ref: dict, what):
    assert got["n_components"] == ref["n_components"], (what, got["n_components"], ref["n_components"])
    for key in ("face_label", "vertex_label", "face_count", "first_face"):
        assert got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), (what, key)
    assert np.array_equal(bits(got["area"]), bits(ref["area"])), f"{what}: areas differ in {int((bits(got['area']) != bits(ref['area'])).sum())} values"


def assert_same_filter(got, ref, what):
    v, f, kept, inverse = (t.cpu().numpy() for t in got)
    assert v.shape == ref[0].shape and np.array_equal(bits(v), bits(ref[0])), what
    assert f.shape == ref[1].shape and np.array_equal(f, ref[1]) and np.array_equal(kept, ref[2]) and np.array_equal(inverse, ref[3]), what
    assert all(t.is_cuda for t in got) and got[0].dtype == torch.float64 and all(t.dtype == torch.int64 for t in got[1:])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: the components
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,connectivity", CASES)
def test_components_equal_the_restatement(name, connectivity):
    """No faces, one face, a shared edge, a bow-tie, disjoint faces, a face naming a vertex twice, three faces on an edge, a duplicate
    face, an unreferenced vertex; sums over 1 / 63 / 64 / 65 / 129 faces; 255 / 256 / 257 components; the strip of 4097 triangles
    numbered three ways; 300 interleaved tetrahedra; the floater scene — by edge and by vertex."""
    v, f = SHAPES[name]
    got = host(meshops.connected_components((v, f), connectivity=connectivity))
    assert_same_components(got, want(name, connectivity), (name, connectivity))
    without = meshops.connected_components((torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)), connectivity=connectivity, areas=False)
    assert without.area is None and np.array_equal(without.face_label.cpu().numpy(), got["face_label"])
    f32 = f.astype(np.int32)                                                       # any integer dtype names the same faces
    assert np.array_equal(meshops.connected_components((v, f32), connectivity=connectivity, areas=False).face_label.cpu().numpy(), got["face_label"])


@pytest.mark.parametrize("connectivity", CC.CONNECTIVITIES)
def test_a_permutation_of_the_faces_gives_the_same_partition(connectivity):
    v, f, _ = CC.floater_scene()
    perm = np.random.default_rng(9).permutation(len(f))
    a = meshops.connected_components((v, f), connectivity=connectivity).face_label.cpu().numpy()
    b = host(meshops.connected_components((v, f[perm]), connectivity=connectivity))
    assert np.array_equal(CC.renumber_by_lowest(a[perm]), b["face_label"])
    assert_same_components(b, CC.components(v, f[perm], connectivity), "permuted")


def test_golden_extracted_mesh():
    """The f24 field of tests/golden/mesh_stages.npz through the extraction's own device path: a marching-cubes mesh with its real pieces."""
    fix = np.load(os.path.join(REPO, "tests", "golden", "mesh_stages.npz"))
    v, f = mesh.field_to_mesh(torch.from_numpy(fix["f24.pred"]).to(DEV), 24)
    assert f.shape[0] > 1000
    for connectivity in CC.CONNECTIVITIES:
        got = host(meshops.connected_components((v, f), connectivity=connectivity))
        assert_same_components(got, CC.components(v.cpu().numpy(), f.cpu().numpy(), connectivity), ("f24", connectivity))


def test_segment_sums_equal_the_rule():
    x = np.random.default_rng(5).uniform(-1.0, 1.0, 6000)
    sizes = [1, 63, 64, 65, 129, 1, 2, 127, 128, 4097, 1, 31, 33]
    start = np.concatenate(([0], np.cumsum(sizes), [len(x)])).astype(np.int64)          # (and a last segment of what is left)
    assert start[5] == 322 and start[6] == 323
    x[322] = -0.0                                                                     # a segment that is one -0.0
    got = lib.cc_segment_sums(torch.from_numpy(x).to(DEV), torch.from_numpy(start).to(DEV)).cpu().numpy()
    ref = np.array([CC.wave_sum(x[b:e]) for b, e in zip(start[:-1], start[1:])])
    assert np.array_equal(bits(got), bits(ref))
    assert got[5] == 0.0 and not np.signbit(got[5])                                   # lane 0 adds lane 32's +0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2: the filter and the cleaning functions
# ---------------------------------------------------------------------------------------------------------------------------------
def test_filter_returns_exactly_the_big_surface():
    v, f, big = CC.floater_scene()
    got = meshops.filter_components((v, f), min_faces=51)
    assert_same_filter(got, CC.filter_components(v, f, min_faces=51)[:4], "min_faces=51")
    assert np.array_equal(got[2].cpu().numpy(), np.nonzero(big)[0]) and got[0].shape[0] == 10000
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(v[:10000]))


@pytest.mark.parametrize("kw", [dict(), dict(min_faces=1), dict(min_faces=50), dict(min_faces=20001), dict(keep_largest=1), dict(keep_largest=5),
                                dict(keep_largest=3, by="area"), dict(min_area=0.01), dict(min_faces=10, keep_largest=2, connectivity="vertex"),
                                dict(min_area=1e9)])
def test_filter_equals_the_restatement(kw):
    v, f, _ = CC.floater_scene()
    assert_same_filter(meshops.filter_components((v, f), **kw), CC.filter_components(v, f, **kw)[:4], kw)


@pytest.mark.parametrize("name", ["nothing", "no_faces", "one_face", "bow_tie", "disjoint", "unreferenced_vertex", "repeated_vertex"])
def test_filter_on_the_small_shapes(name):
    v, f = SHAPES[name]
    for kw in (dict(), dict(keep_largest=1), dict(min_faces=2)):
        assert_same_filter(meshops.filter_components((v, f), **kw), CC.filter_components(v, f, **kw)[:4], (name, kw))


def test_cleaning_functions_equal_the_restatement():
    flat = (np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2], [0, 1, 3]]))
    for v, f in list(SHAPES[n] for n in ("repeated_vertex", "duplicate_face", "one_face", "no_faces", "tetrahedra_300")) + [flat]:
        for zero_area in (False, True):
            got, ref = meshops.remove_degenerate_faces((v, f), zero_area=zero_area), CC.remove_degenerate_faces(v, f, zero_area)
            assert np.array_equal(got[0].cpu().numpy(), ref[0]) and np.array_equal(got[1].cpu().numpy(), ref[1])
        got, ref = meshops.remove_duplicate_faces((v, f)), CC.remove_duplicate_faces(f)
        assert np.array_equal(got[0].cpu().numpy(), ref[0]) and np.array_equal(got[1].cpu().numpy(), ref[1])
    # every face of the floater scene twice, the copies wound the other way, plus faces without area: clean() gives the big surface back
    v, f, big = CC.floater_scene()
    doubled = np.concatenate((f, f[:, ::-1], np.stack((f[:50, 0], f[:50, 0], f[:50, 1]), axis=1)))
    got = meshops.clean((v, doubled), min_faces=51)
    assert_same_filter(got, CC.filter_components(v, f, min_faces=51)[:4], "clean")
    welded = meshops.clean((np.concatenate((v, v)), np.concatenate((f, f + len(v)))), weld_digits=8, keep_largest=1)
    assert np.array_equal(welded[1].cpu().numpy(), got[1].cpu().numpy()) and np.array_equal(welded[2].cpu().numpy(), np.nonzero(big)[0])
    inverse = welded[3].cpu().numpy()
    assert np.array_equal(inverse[:len(v)], inverse[len(v):]) and np.array_equal(inverse[:len(v)], got[3].cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: score_mesh
# ---------------------------------------------------------------------------------------------------------------------------------
def test_score_mesh_culls_before_it_samples():
    v, f, big = CC.floater_scene()
    ref_mesh = CC.torus(40, 40)
    uniforms = np.random.default_rng(1).uniform(0, 1, (3000, 3))
    kw = dict(num_points=3000, distance_thresh=0.05, uniforms=uniforms)
    # without the keyword: the entry the existing path gives, built here from its own pieces
    pred_points, _ = metrics3d.sample_surface(v, f, 3000, uniforms=uniforms)
    ref_points, _ = metrics3d.sample_surface(*ref_mesh, 3000, uniforms=uniforms)
    rows = metrics3d._both_directions(pred_points, ref_points, 0.05, None)
    mean, median, mn, mx = metrics3d._chamfer(rows[0], rows[1])
    expected = {"chamfer distance": {"mean": mean, "median": median, "min": mn, "max": mx}}
    expected.update(metrics3d._prf(rows[1], rows[0]))
    plain = metrics3d.score_mesh((v, f), ref_mesh, **kw)
    assert plain == expected and "components" not in plain
    # with it: the scores of the hand-filtered mesh, bit for bit
    hand = CC.filter_components(v, f, min_faces=51)
    by_hand = metrics3d.score_mesh((hand[0], hand[1]), ref_mesh, **kw)
    culled = metrics3d.score_mesh((v, f), ref_mesh, min_component_faces=51, **kw)
    entry = culled.pop("components")
    assert culled == by_hand and culled != plain
    c = CC.components(v, f, "edge")
    removed = c["area"][c["face_count"] < 51]
    assert entry == {"connectivity": "edge", "found": 201, "kept": 1, "faces_removed": int((~big).sum()),
                     "area_removed": __import__("math").fsum(removed.tolist())}
    largest = metrics3d.score_mesh((v, f), ref_mesh, keep_largest=1, **kw)
    assert largest.pop("components") == entry and largest == by_hand
    with pytest.raises(ValueError, match="none of its 201 components"):
        metrics3d.score_mesh((v, f), ref_mesh, min_component_faces=20001, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: values that must never reach an address
# ---------------------------------------------------------------------------------------------------------------------------------
def dev(x, dtype):
    return torch.tensor(x, dtype=dtype, device=DEV)


@pytest.mark.parametrize("bad", [4, -1, 1 << 40, -(1 << 62)])
def test_a_node_outside_its_range_sets_the_status(bad):
    keys, parent = dev([3, 3, 5, 5, 5], torch.int64), torch.arange(4, dtype=torch.int32, device=DEV)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.cc_union_runs(keys, dev([0, 1, 2, bad, 3], torch.int64), parent.clone())
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = lib.cc_union_runs(keys, dev([0, 1, 2, bad, 3], torch.int64), parent.clone(), info=info)
    assert int(info.cpu()) == 2 and out.cpu().tolist() == [0, 0, 2, 3]            # the good pair is united, the bad ones are not followed
    # negative keys are no keys: nothing is united and nothing is wrong
    out = lib.cc_union_runs(dev([-1, -1, -1, 7, 7], torch.int64), dev([0, 1, 2, 2, 3], torch.int64), parent.clone())
    assert out.cpu().tolist() == [0, 1, 2, 2]


@pytest.mark.parametrize("bad", [3, 4, -1, (1 << 31) - 1, -(1 << 31)])
def test_a_parent_outside_its_range_sets_the_status(bad):
    """A forest that is not ours: parent[2] leaves [0, 2].  Neither the unions nor the flatten follow it."""
    parent = dev([0, 0, bad, 2], torch.int32)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.cc_flatten(parent)
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert lib.cc_flatten(parent, info=info).cpu().tolist() == [0, 0, -1, -1] and int(info.cpu()) == 2
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.cc_union_runs(dev([1, 1], torch.int64), dev([1, 3], torch.int64), parent.clone())
    assert lib.cc_flatten(dev([0, 0, 1, 2], torch.int32)).cpu().tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("start", [[0, 3, 2, 5], [0, 2, 2, 5], [-1, 2, 4, 5], [0, 2, 4, 6], [0, 2, 1 << 40, 5], [2, -(1 << 62), 4, 5]])
def test_a_segment_outside_its_range_sets_the_status(start):
    x = dev([1.0, 2.0, 3.0, 4.0, 5.0], torch.float64)
    with pytest.raises(lib.VfnError, match="outside its range"):
        lib.cc_segment_sums(x, dev(start, torch.int64))
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = lib.cc_segment_sums(x, dev(start, torch.int64), info=info).cpu().numpy()
    ok = [0 <= b < e <= 5 for b, e in zip(start[:-1], start[1:])]
    assert int(info.cpu()) == 2 and np.array_equal(np.isnan(out), ~np.array(ok))
    good = [float(sum(range(b + 1, e + 1))) for b, e, fine in zip(start[:-1], start[1:], ok) if fine]
    assert out[np.array(ok)].tolist() == good
