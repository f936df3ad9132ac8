"""Mesh normals, welding and normal consistency on the MI355X (csrc/vfn_normals.hip through vf_nerf_amd/meshops.py and metrics3d.py)
against the NumPy restatement of their contracts (tests/meshops_restatement.py): every comparison with the restatement is bit for bit —
the int64 views of the doubles."""
import functools
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, mesh, meshops, metrics3d, ply, synthetic, tsdf  # noqa: E402
import meshops_restatement as M  # noqa: E402
from helpers import build_model, load_fixture  # noqa: E402
from test_meshops_host import OCTA_F, OCTA_V, weld_cases  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -53


def bits(x):
    x = x.detach().cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return x.view(torch.int64) if x.dtype == torch.float64 else x


def assert_bits(got, want, what):
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype in (torch.float64, torch.int64), what
    want = np.asarray(want)
    assert tuple(got.shape) == want.shape, f"{what}: shape {tuple(got.shape)} against {want.shape}"
    bad = int((bits(got) != bits(want)).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} words differ"


def assert_normals(v, f, what):
    mesh_ = (v, f)
    assert_bits(meshops.face_normals(mesh_, normalise=False), M.face_normals(v, f, False), f"{what}: raw face normals")
    assert_bits(meshops.face_normals(mesh_), M.face_normals(v, f, True), f"{what}: unit face normals")
    assert_bits(meshops.vertex_normals(mesh_), M.vertex_normals(v, f), f"{what}: vertex normals")
    row_start, incident = meshops.vertex_faces(torch.from_numpy(f).to(DEV), v.shape[0])
    want = M.csr(M.vertex_faces(f, v.shape[0]))
    assert row_start.is_cuda and np.array_equal(row_start.cpu().numpy(), want[0]) and np.array_equal(incident.cpu().numpy(), want[1]), what


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: face and vertex normals
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 255, 256, 257, 100003])
def test_normals_of_random_meshes_equal_restatement(m):
    """Wave and block edges and one size of many blocks; n = max(3, m // 2) vertices in [-2, 2]^3 and random index triples: repeated and
    degenerate faces occur by construction."""
    g = np.random.default_rng(m)
    n = max(3, m // 2)
    v, f = g.uniform(-2, 2, (n, 3)), g.integers(0, n, (m, 3))
    if m == 100003:
        assert (f[:, 0] == f[:, 1]).any() and np.unique(f).shape[0] < n
    assert_normals(v, f, f"m = {m}")


def test_fan_unused_vertex_and_zero_area_face():
    """A fan of 1000 faces around vertex 0 (a row longer than a wave: the ascending-face order shows in the bits), a vertex no face
    uses, a face without area among faces with it."""
    g = np.random.default_rng(1000)
    n = 1203
    v = g.uniform(-2, 2, (n, 3))
    rim = g.integers(1, n - 1, (1000, 2))
    fan = np.concatenate((np.zeros((1000, 1), dtype=np.int64), rim), axis=1)
    v[5], v[6], v[7] = (0.25, 0.5, -1.0), (0.75, 1.5, -3.0), (0.5, 1.0, -2.0)              # collinear, exactly: the cross product is zero
    f = np.concatenate((fan[:500], [[5, 6, 7]], fan[500:], [[5, 6, 8], [9, 5, 7]]))
    assert not (f == n - 1).any()
    assert_normals(v, f, "fan")
    raw = meshops.face_normals((v, f), normalise=False).cpu().numpy()
    assert np.array_equal(raw[500], [0.0, 0.0, 0.0]) and np.array_equal(meshops.face_normals((v, f)).cpu().numpy()[500], [0.0, 0.0, 0.0])
    vn = meshops.vertex_normals((v, f)).cpu().numpy()
    assert np.array_equal(vn[n - 1], [0.0, 0.0, 1.0])
    # the order of the fan's sum is visible: the same faces added in the opposite order give other bits
    rows = M.vertex_faces(f, n)
    assert len(rows[0]) == 1000
    fn = M.face_normals(v, f, False)
    backwards = functools.reduce(lambda s, j: s + fn[j], rows[0][-2::-1], fn[rows[0][-1]].copy())
    assert not np.array_equal(M.unit(backwards[None], (0.0, 0.0, 1.0))[0][0], vn[0])
    # the zero-area face adds exact zeros: the vertices it shares with other faces have the normals they have without it
    without = np.delete(f, 500, axis=0)
    assert np.array_equal(meshops.vertex_normals((v, without)).cpu().numpy()[[5, 7]], vn[[5, 7]])


def test_octahedron_comes_out_exactly():
    assert_bits(meshops.vertex_normals((OCTA_V, OCTA_F)), OCTA_V, "octahedron vertex normals")
    assert_normals(OCTA_V, OCTA_F, "octahedron")
    from_torch = meshops.vertex_normals((torch.from_numpy(OCTA_V).to(DEV).float(), torch.from_numpy(OCTA_F).to(torch.int32)))
    assert_bits(from_torch, OCTA_V, "float32 vertices on the device, int32 faces on the host")
    assert tuple(meshops.vertex_normals((np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)), device=DEV).shape) == (0, 3)
    assert meshops.vertex_normals((OCTA_V, np.zeros((0, 3), dtype=np.int64)), device=DEV).cpu().tolist() == [[0.0, 0.0, 1.0]] * 6
    assert tuple(meshops.face_normals((OCTA_V, np.zeros((0, 3), dtype=np.int64)), device=DEV).shape) == (0, 3)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_coordinates_are_refused(bad):
    v = OCTA_V.copy()
    v[3, 1] = bad
    for call in (meshops.face_normals, meshops.vertex_normals, functools.partial(meshops.face_normals, normalise=False)):
        with pytest.raises(lib.VfnError, match="non-finite"):
            call((v, OCTA_F))
    with pytest.raises(ValueError, match="non-finite"):
        meshops.weld((v, OCTA_F))
    unit = torch.from_numpy(OCTA_V).to(DEV)
    index = torch.arange(6, device=DEV)
    with pytest.raises(lib.VfnError, match="non-finite"):
        lib.normal_dots(torch.from_numpy(v).to(DEV), unit, index)
    with pytest.raises(lib.VfnError, match="non-finite"):
        lib.normal_dots(unit, torch.from_numpy(v).to(DEV), index)
    assert_bits(lib.normal_dots(unit, unit, index), np.ones(6), "the finite case")


def test_overflowing_length_is_refused():
    big = OCTA_V * 1e200                                                           # finite coordinates, a cross product beyond the doubles
    for normalise in (True, False):
        with pytest.raises(lib.VfnError, match="overflow"):
            meshops.face_normals((big, OCTA_F), normalise=normalise)
    with pytest.raises(lib.VfnError, match="overflow"):
        meshops.vertex_normals((big, OCTA_F))
    # |c|^2 overflows although c does not: the raw normals are written, the unit ones refused
    raw = meshops.face_normals((OCTA_V * 1e80, OCTA_F), normalise=False)
    assert_bits(raw, M.face_normals(OCTA_V * 1e80, OCTA_F, False), "1e160")
    with pytest.raises(lib.VfnError, match="overflow"):
        meshops.face_normals((OCTA_V * 1e80, OCTA_F))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2: weld
# ---------------------------------------------------------------------------------------------------------------------------------
def assert_weld(v, f, digits, what):
    want = M.weld(v, f, digits)
    got = meshops.weld((v, f), digits=digits, device=DEV)
    again = meshops.weld((torch.from_numpy(np.ascontiguousarray(v)).to(DEV), f), digits=digits)
    for g in (got, again):
        assert_bits(g[0], want[0], f"{what}: vertices")
        assert_bits(g[1], want[1], f"{what}: faces")
        assert_bits(g[2], want[2], f"{what}: inverse")
    return want


@pytest.mark.parametrize("name", list(weld_cases()))
@pytest.mark.parametrize("digits", [None, 8, 0])
def test_weld_host_cases_on_the_device(name, digits):
    v, f = weld_cases()[name]
    assert_weld(v, f, digits, name)


@pytest.mark.parametrize("jitter", [False, True])
@pytest.mark.parametrize("digits", [None, 8])
def test_weld_lattice_soup(digits, jitter):
    """10^5 vertices on the points of a 40 x 40 x 40 lattice (many duplicates) and random triples; with ``jitter`` every coordinate is
    moved by up to 3e-9, which digits = 8 rounds away and digits = None does not."""
    g = np.random.default_rng(40 + jitter)
    n, m = 100000, 60000
    v = g.integers(0, 40, (n, 3)).astype(np.float64) / 8.0 - 2.5
    if jitter:
        v = v + g.uniform(-3e-9, 3e-9, (n, 3))
    f = g.integers(0, n, (m, 3))
    want = assert_weld(v, f, digits, f"lattice soup, digits {digits}, jitter {jitter}")
    classes = want[0].shape[0]
    print(f"digits {digits}, jitter {jitter}: {np.unique(f).shape[0]} referenced vertices -> {classes}")
    assert classes <= 64000 if (digits == 8 or not jitter) else classes > 80000


def test_weld_extremes():
    g = np.random.default_rng(9)
    one = np.tile(np.array([[0.1, -0.2, 0.3]]), (4096, 1))                          # every vertex equal: one table slot takes them all
    f = g.integers(0, 4096, (3000, 3))
    f[0] = (4095, 17, 4094)
    want = assert_weld(one, f, None, "4096 equal vertices")
    assert want[0].shape[0] == 1 and (want[1] == 0).all()
    assert_weld(one, f, 8, "4096 equal vertices, digits 8")
    distinct = g.permutation(5000).astype(np.float64)[:, None] * np.array([[1.0, 0.5, 0.25]])        # no duplicates at all
    f = g.integers(0, 5000, (7000, 3))
    want = assert_weld(distinct, f, 8, "no duplicates")
    assert want[0].shape[0] == np.unique(f).shape[0]
    for n in (1, 64, 65):
        v = g.integers(0, 3, (n, 3)).astype(np.float64)
        f = np.stack((np.arange(n), (np.arange(n) + 1) % n, (np.arange(n) + 2) % n), axis=1)
        assert_weld(v, f, None, f"n = {n}")
        assert_weld(v, f, 8, f"n = {n}, digits 8")
    empty = meshops.weld((OCTA_V, np.zeros((0, 3), dtype=np.int64)), device=DEV)
    assert tuple(empty[0].shape) == (0, 3) and tuple(empty[1].shape) == (0, 3) and empty[2].cpu().tolist() == [-1] * 6


def synthetic_decoder(points):
    """A sphere's shell and a slab, as a vector field that converges on them."""
    d = points - torch.tensor([0.05, -0.1, 0.02], device=points.device)
    r = d.norm(dim=1, keepdim=True).clamp_min(1e-6)
    v = -torch.sign(r - 0.6) * d / r * (0.2 + (r - 0.6).abs())
    v = v + 0.5 * torch.sign(torch.sin(5.0 * points[:, :1])) * torch.tensor([[1.0, 0.0, 0.0]], device=points.device) * (points[:, 1:2] > 0.4)
    return torch.cat((v, torch.zeros_like(v[:, :1])), dim=1).float()


def test_extract_mesh_weld():
    args = dict(scale=1.1, translation=torch.tensor([0.05, -0.02, 0.01]), centroid=torch.tensor([0.0, 0.1, -0.05]))
    plain = mesh.extract_mesh(synthetic_decoder, 16, **args)
    explicit = mesh.extract_mesh(synthetic_decoder, 16, weld=False, **args)
    welded = mesh.extract_mesh(synthetic_decoder, 16, weld=True, **args)
    assert plain.faces.shape[0] > 100
    for a, b in zip(plain, explicit):
        assert torch.equal(bits(a), bits(b))
    v32 = plain.vertices.float().double()
    wv, wf, inverse = meshops.weld((v32, plain.faces), digits=8)
    assert torch.equal(bits(welded.vertices), bits(wv)) and torch.equal(welded.faces, wf) and welded.faces.shape == plain.faces.shape
    t, c = args["translation"].to(DEV, torch.float64), args["centroid"].to(DEV, torch.float64)
    assert torch.equal(bits(welded.vertices_scaled), bits(wv * 1.1 + t + c))
    want = M.weld(v32.cpu().numpy(), plain.faces.cpu().numpy(), 8)
    assert_bits(welded.vertices, want[0], "welded extraction")
    assert_bits(welded.faces, want[1], "welded extraction")
    with pytest.raises(ValueError):
        mesh.extract_mesh(synthetic_decoder, 16, weld=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: normal consistency
# ---------------------------------------------------------------------------------------------------------------------------------
KEYS = ("pred_to_ref", "ref_to_pred", "mean")


def random_mesh(seed, n=1000, m=2000):
    g = np.random.default_rng(seed)
    return g.uniform(-2, 2, (n, 3)), g.integers(0, n, (m, 3))


def lattice_mesh(seed, n=300, m=700):
    """Vertices on multiples of 1/8 in [-2, 2]: with barycentric coordinates on multiples of 1/1024 a sample is exact."""
    g = np.random.default_rng(seed)
    return g.integers(-16, 17, (n, 3)).astype(np.float64) / 8.0, g.integers(0, n, (m, 3))


def uniforms(count, seed, dyadic=False):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(count, 3, dtype=torch.float64, generator=g)
    if dyadic:
        u[:, 1:] = torch.randint(0, 1024, (count, 2), generator=g).double() / 1024.0
    return u


def test_a_mesh_against_itself():
    """Every sample's nearest sample of the other set is its own copy: every dot is a unit normal's squared length.  First order: the
    squared length carries at most 6 u, the stated dot adds at most 3 u."""
    for mesh_ in (random_mesh(1), (OCTA_V, OCTA_F)):
        out = metrics3d.normal_consistency(mesh_, mesh_, num_points=20000, uniforms=uniforms(20000, 3))
        print({k: (out[k] - 1.0) / U for k in KEYS}, "x 2^-53")
        assert set(out) == set(KEYS) and all(type(out[k]) is float for k in KEYS)
        assert all(1.0 - 10 * U <= out[k] <= 1.0 + 10 * U for k in KEYS)


def test_flipped_winding_changes_no_bit():
    """b x a = -(a x b) exactly, so a flipped face has the negated normal and every |dot| is what it was — given the same samples.  A
    flipped face (v0, v2, v1) swaps the roles of the two barycentric coordinates; on lattice meshes with dyadic coordinates a sample
    is exact, so (1) both meshes flipped with the two columns swapped and (2) one mesh flipped with the two columns equal sample the
    same points."""
    a, b = lattice_mesh(11), lattice_mesh(12)
    flip = lambda mesh_: (mesh_[0], np.ascontiguousarray(mesh_[1][:, [0, 2, 1]]))          # noqa: E731
    n = 20000
    u = uniforms(n, 5, dyadic=True)
    first = metrics3d.normal_consistency(a, b, num_points=n, uniforms=u)
    assert 0.2 < first["mean"] < 0.8
    assert metrics3d.normal_consistency(flip(a), flip(b), num_points=n, uniforms=u[:, [0, 2, 1]]) == first
    p1, f1 = metrics3d.sample_surface(*a, n, uniforms=u)
    p2, f2 = metrics3d.sample_surface(*flip(a), n, uniforms=u[:, [0, 2, 1]])
    assert torch.equal(bits(p1), bits(p2)) and torch.equal(f1, f2)
    assert torch.equal(meshops.face_normals(a), -meshops.face_normals(flip(a)))          # (as values: a face without area has +0.0 both ways)
    u[:, 2] = u[:, 1]
    second = metrics3d.normal_consistency(a, b, num_points=n, uniforms=u)
    assert metrics3d.normal_consistency(flip(a), b, num_points=n, uniforms=u) == second
    assert metrics3d.normal_consistency(a, flip(b), num_points=n, uniforms=u) == second


def test_tilted_square():
    """A flat square of 2 x 32 x 32 triangles against its copy turned by 0.3 rad about an in-plane axis through its centre: every dot is
    cos 0.3 up to rounding."""
    k = 32
    ax = np.linspace(-1.0, 1.0, k + 1)
    x, y = np.meshgrid(ax, ax, indexing="ij")
    v = np.stack((x.reshape(-1), y.reshape(-1), np.zeros((k + 1) ** 2)), axis=1)
    i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    q = (i * (k + 1) + j).reshape(-1)
    f = np.concatenate((np.stack((q, q + k + 1, q + 1), axis=1), np.stack((q + 1, q + k + 1, q + k + 2), axis=1)))
    assert f.shape[0] == 2 * k * k
    c, s = math.cos(0.3), math.sin(0.3)
    turned = v @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]).T
    out = metrics3d.normal_consistency((v, f), (turned, f), num_points=20000, uniforms=uniforms(20000, 8))
    print({key: out[key] - c for key in KEYS})
    assert all(abs(out[key] - c) <= 1e-12 for key in KEYS)


def test_normal_consistency_equals_restatement_on_the_devices_samples():
    a, b = random_mesh(21), random_mesh(22)
    n = 5000
    u = uniforms(n, 23)
    got = metrics3d.normal_consistency(a, b, num_points=n, uniforms=u)
    pp, pf = metrics3d.sample_surface(*a, n, uniforms=u)
    rp, rf = metrics3d.sample_surface(*b, n, uniforms=u)
    pn = M.face_normals(*a, True)[pf.cpu().numpy()]
    rn = M.face_normals(*b, True)[rf.cpu().numpy()]
    to_ref, _ = metrics3d.nearest(pp, rp)
    to_pred, _ = metrics3d.nearest(rp, pp)
    want = M.normal_consistency(pn, rn, to_ref.cpu().numpy(), to_pred.cpu().numpy())
    print(got, want)
    assert got == want and 0.3 < got["mean"] < 0.7 and got["pred_to_ref"] != got["ref_to_pred"]
    # the dots themselves, and a direction whose sum has more than one partial
    index = to_ref
    assert_bits(lib.normal_dots(torch.from_numpy(pn).to(DEV), torch.from_numpy(rn).to(DEV), index), M.normal_dots(pn, rn, index.cpu().numpy()), "dots")
    with pytest.raises(lib.VfnError, match="index"):
        lib.normal_dots(torch.from_numpy(pn).to(DEV), torch.from_numpy(rn[:10]).to(DEV), index.clamp_min(10))
    info = torch.zeros(1, dtype=torch.int64, device=DEV)
    index = index.clone()
    index[[0, 77, 4999]] = torch.tensor([-1, n, 1 << 40], device=DEV)
    dots = lib.normal_dots(torch.from_numpy(pn).to(DEV), torch.from_numpy(rn).to(DEV), index, info=info).cpu().numpy()
    assert int(info.cpu()) == 2 and dots[[0, 77, 4999]].tolist() == [0.0, 0.0, 0.0] and (dots[1:77] > 0).all()


def test_score_mesh_with_normals():
    a, b = random_mesh(31), random_mesh(32)
    n = 5000
    g = torch.Generator(device=DEV)
    entries, states = {}, {}
    for key, kw in {"plain": {}, "grid": {"search": "grid"}, "false": {"normals": False}, "normals": {"normals": True},
                    "normals grid": {"normals": True, "search": "grid"}}.items():
        g.manual_seed(41)
        entries[key] = metrics3d.score_mesh(a, b, num_points=n, distance_thresh=0.2, generator=g, **kw)
        states[key] = g.get_state()
    assert all(torch.equal(states["plain"], s) for s in states.values())                # the same draws, whatever the keywords
    assert entries["plain"] == entries["false"] == entries["grid"] and "normal consistency" not in entries["plain"]
    for key in ("normals", "normals grid"):
        rest = {k: v for k, v in entries[key].items() if k != "normal consistency"}
        assert rest == entries["plain"] and list(rest) == list(entries["plain"])         # every other key, bit for bit
    assert entries["normals"] == entries["normals grid"] and 0 < entries["plain"]["precision"] < 1
    # the draws are what they were: pred first, then ref
    g.manual_seed(41)
    pp, _ = metrics3d.sample_surface(*a, n, generator=g)
    rp, _ = metrics3d.sample_surface(*b, n, generator=g)
    assert tuple(entries["plain"]["chamfer distance"][k] for k in ("mean", "median", "min", "max")) == metrics3d.chamfer_from_points(pp, rp)
    g.manual_seed(41)
    assert entries["normals"]["normal consistency"] == metrics3d.normal_consistency(a, b, num_points=n, generator=g)


def test_score_mesh_with_normals_after_icp():
    """A bumpy sheet against itself turned by a known rotation: ICP takes the turn back, the pred normals turn with the points, and the
    consistency is the unturned pair's."""
    k = 24
    ax = np.linspace(-1.0, 1.0, k + 1)
    x, y = np.meshgrid(ax, ax, indexing="ij")
    z = 0.3 * np.sin(2.5 * x + 0.3) * np.cos(1.7 * y) + 0.2 * x * y
    v = np.stack((x.reshape(-1), y.reshape(-1), z.reshape(-1)), axis=1)
    i, j = np.meshgrid(np.arange(k), np.arange(k), indexing="ij")
    q = (i * (k + 1) + j).reshape(-1)
    f = np.concatenate((np.stack((q, q + k + 1, q + 1), axis=1), np.stack((q + 1, q + k + 1, q + k + 2), axis=1)))
    axis = np.array([0.2, 1.0, 0.3]) / np.linalg.norm([0.2, 1.0, 0.3])
    angle = math.radians(4.0)
    kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    rot = np.eye(3) + math.sin(angle) * kx + (1 - math.cos(angle)) * kx @ kx
    turned = v @ rot.T + np.array([0.02, -0.01, 0.015])
    n = 20000
    u = uniforms(n, 51)
    straight = metrics3d.score_mesh((v, f), (v, f), num_points=n, distance_thresh=0.05, uniforms=u, normals=True)
    tilted = metrics3d.score_mesh((turned, f), (v, f), num_points=n, distance_thresh=0.05, uniforms=u, normals=True)
    out = metrics3d.score_mesh((turned, f), (v, f), num_points=n, distance_thresh=0.05, uniforms=u, normals=True, icp_align=True, icp_threshold=0.3)
    assert "icp" in out and "normal consistency" in out
    print(straight["normal consistency"], tilted["normal consistency"], out["normal consistency"], out["icp"]["inlier_rmse"])
    assert tilted["normal consistency"]["mean"] < 1.0 - 1e-4                            # without the alignment the turn shows
    assert all(abs(out["normal consistency"][key] - straight["normal consistency"][key]) <= 1e-9 for key in KEYS)
    plain = metrics3d.score_mesh((turned, f), (v, f), num_points=n, distance_thresh=0.05, uniforms=u, icp_align=True, icp_threshold=0.3)
    assert {key: val for key, val in out.items() if key != "normal consistency"} == plain


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: the evaluator's switch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_evaluator_switch_writes_the_vertex_normals(tmp_path, monkeypatch):
    """The synthetic model (random weights: the geometry means nothing): two views of 16 x 12 pixels rendered, left on disk as
    render_images leaves them and fused by evaluator.tsdf_mesh with the reference's dataset module stood in for.  With the switch set
    tsdf.ply holds float32(meshops.vertex_normals(the fused mesh)); its vertices, faces and colours are the file's without the switch."""
    from PIL import Image
    from vf_nerf_amd import evaluator
    fx, d = load_fixture("c1_perturb")
    model = build_model(fx, d, device=DEV)
    w, h = 16, 12
    poses = torch.stack([synthetic.orbit_pose(20.0, 8.0, 0.9), synthetic.orbit_pose(-35.0, 15.0, 1.0)])
    k4 = torch.eye(4)
    k4[0, 0] = k4[1, 1] = 15.0
    k4[0, 2], k4[1, 2] = (w - 1) / 2, (h - 1) / 2
    model.rng_seed, model._rng_offset = 5, 0
    depths, images = tsdf.render_rgbd_maps(model, poses, k4, h, w, 0)
    depths = torch.where(depths < 0, torch.zeros_like(depths), depths).cpu().numpy().astype(np.float64)
    os.makedirs(tmp_path / "rendered_images")
    for i in range(2):
        np.save(tmp_path / "rendered_images" / f"depth-{i}.npy", depths[i][..., None])
        Image.fromarray(images[i].cpu().numpy()).save(tmp_path / "rendered_images" / f"image-{i}.png")

    class Dataset:
        def __init__(self, config):
            self.intrinsics, self.poses = k4, poses

    coarse = functools.partial(tsdf.fuse_rgbd_maps, voxel_length=0.05, sdf_trunc=0.15)          # (the evaluator's own 4/512 needs a real scene)
    fused = []
    monkeypatch.setattr(tsdf, "fuse_rgbd_maps", lambda *a, **kw: fused.append(coarse(*a, **kw)) or fused[-1])
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
    finally:
        for key in names:
            del sys.modules[key]
        sys.modules.update(saved)
    vertices, faces, _ = fused[1]
    assert faces.shape[0] > 100 and files[False][3] is None
    want = meshops.vertex_normals((vertices, faces)).cpu().numpy().astype(np.float32)
    assert np.array_equal(files[True][3].astype(np.float32).view(np.int32), want.view(np.int32))
    assert_bits(meshops.vertex_normals((vertices, faces)), M.vertex_normals(vertices.cpu().numpy(), faces.cpu().numpy()), "fused mesh")
    assert all(np.array_equal(a, b) for a, b in zip(files[False][:3], files[True][:3]))
    assert np.array_equal(files[True][0].astype(np.float32), vertices.cpu().numpy().astype(np.float32))
