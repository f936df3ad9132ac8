"""The block-sparse TSDF volume on the device (csrc/vfn_tsdf.hip: vfn_tsdf_sparse_*; tsdf.SparseTSDFVolume) against the NumPy restatement
(tests/tsdf_sparse_restatement.py) bit for bit — the blocks and their numbers, the voxels, the mesh with its numbering and colours — and
against the device's own dense volume over the same lattice."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, tsdf  # noqa: E402
import tsdf_restatement as R  # noqa: E402
import tsdf_colour_restatement as C  # noqa: E402
import tsdf_sparse_restatement as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

SCENES = {
    "sphere32": lambda: R.sphere_scene(),
    "room32": lambda: R.room_scene(),
    "room_odd": lambda: R.room_scene((33, 17, 70)),
    "sphere64": lambda: R.sphere_scene((64, 64, 64)),
    "room64": lambda: R.room_scene((64, 64, 64)),
    "sphere128": lambda: R.sphere_scene((128, 128, 128), h=96, w=128),
    "room128": lambda: R.room_scene((128, 128, 128), h=60, w=80),
    "far": S.far_scene,
}
_CACHE = {}


def tables():
    if "tables" not in _CACHE:
        _, edge_vertex, tri = lib.mesh_tables()
        _CACHE["tables"] = (tri, edge_vertex)
    return _CACHE["tables"]


def scene(name):
    if ("scene", name) not in _CACHE:
        _CACHE[("scene", name)] = SCENES[name]()
    return _CACHE[("scene", name)]


def images(name):
    if ("rgb", name) not in _CACHE:
        _CACHE[("rgb", name)] = C.scene_images(scene(name))
    return _CACHE[("rgb", name)]


def restated(name, colour=False):
    """The one-call restated state of a scene: computed once, never written to."""
    key = ("state", name, colour)
    if key not in _CACHE:
        _CACHE[key] = S.fuse(scene(name), rgbs=images(name) if colour else None)
    return _CACHE[key]


def device_volume(s, rgbs=None, calls=None, allocate_first=False, sparse=True):
    cls = tsdf.SparseTSDFVolume if sparse else tsdf.TSDFVolume
    vol = cls(s.origin, s.dims, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV, colour=rgbs is not None)
    k = s.intrinsics_matrices()
    if allocate_first:
        vol.allocate(s.depths, k, s.poses)
    for sl in ([slice(None)] if calls is None else calls):
        more = {"allocate": False} if allocate_first else {}
        vol.integrate(s.depths[sl], k[sl], s.poses[sl], rgb=None if rgbs is None else rgbs[sl], **more)
    return vol


def bits(x):
    x = x.detach().cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int64)


def assert_blocks(vol, state, what=""):
    assert vol.block_coords.dtype == torch.int32 and vol.block_of.dtype == torch.int32 and vol.block_of.is_cuda
    assert vol.n_blocks == state.n_blocks, f"{what}: {vol.n_blocks} blocks, restated {state.n_blocks}"
    assert np.array_equal(vol.block_coords.cpu().numpy(), state.block_coords), what
    assert np.array_equal(vol.block_of.cpu().numpy(), state.block_of), what


def assert_state_bits(vol, state, what=""):
    assert_blocks(vol, state, what)
    pairs = [(vol.tsdf, state.tsdf), (vol.weight, state.weight)] + ([] if state.colour is None else [(vol.colour, state.colour)])
    bad = [int((bits(a) != bits(b)).sum()) for a, b in pairs]
    print(f"{what}: {vol.n_blocks} blocks, differing words {bad}; observed {int((state.weight > 0).sum())} of {state.weight.size} voxels")
    assert not any(bad), what


def assert_mesh_bits(got, want, what=""):
    assert len(got) == len(want)
    v, f = got[:2]
    assert v.dtype == torch.float64 and f.dtype == torch.int64 and v.is_cuda and f.is_cuda
    assert tuple(v.shape) == want[0].shape and tuple(f.shape) == want[1].shape, f"{what}: {tuple(v.shape)} {tuple(f.shape)} vs {want[0].shape} {want[1].shape}"
    assert torch.equal(bits(v), bits(want[0])) and np.array_equal(f.cpu().numpy(), want[1]), what
    if len(got) == 3:
        bad = int((bits(got[2]) != bits(want[2])).sum())
        print(f"{what}: {bad} of {want[2].size} colour words differ")
        assert bad == 0 and tuple(got[2].shape) == want[2].shape, what


# ---- allocation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere32", "room32", "room_odd", "sphere128"])
def test_allocation_equals_the_restatement(name):
    s = scene(name)
    state = S.State(s.dims)
    n = S.allocate(state, s.origin, s.vl, s.trunc, s.depths, s.k4s, s.e12s)
    vol = tsdf.SparseTSDFVolume(s.origin, s.dims, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    assert vol.n_blocks == 0 and vol.allocate(s.depths, s.intrinsics_matrices(), s.poses) == n
    assert_blocks(vol, state, name)
    assert n > 50 and tuple(vol.tsdf.shape) == (n, 8, 8, 8) and not bool(vol.tsdf.any()) and not bool(vol.weight.any())
    assert vol.allocate(s.depths, s.intrinsics_matrices(), s.poses) == 0 and vol.n_blocks == n          # nothing is opened twice
    assert vol.memory_bytes == vol.block_of.numel() * 4 + n * 12 + 2 * n * 512 * 4
    if name in ("room_odd", "sphere128"):
        assert n < vol.block_of.numel()                                                                 # (some blocks stay absent)


def test_allocation_in_two_calls_numbers_by_call_then_c_order():
    s = scene("sphere128")
    state = S.State(s.dims)
    counts = [S.allocate(state, s.origin, s.vl, s.trunc, s.depths[sl], s.k4s[sl], s.e12s[sl]) for sl in (slice(0, 2), slice(2, 7))]
    vol = tsdf.SparseTSDFVolume(s.origin, s.dims, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    k = s.intrinsics_matrices()
    got = [vol.allocate(s.depths[sl], k[sl], s.poses[sl]) for sl in (slice(0, 2), slice(2, 7))]
    assert got == counts and min(counts) > 50
    assert_blocks(vol, state, "two calls")
    one = restated("sphere128") if ("state", "sphere128", False) in _CACHE else None
    assert one is None or one.n_blocks == vol.n_blocks


# ---- voxel bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere32", "room32", "room_odd"])
def test_one_call_holds_the_dense_bits_on_allocated_voxels(name):
    s = scene(name)
    state = restated(name)
    vol = device_volume(s)
    assert_state_bits(vol, state, name)
    t, w = s.fused()
    inside = S.allocated_mask(state)
    dt, dw = (x.cpu().numpy() for x in vol.to_dense())
    assert dt.shape == s.dims and dt.dtype == np.float32
    assert np.array_equal(dt.view(np.uint32)[inside], t.view(np.uint32)[inside]) and np.array_equal(dw.view(np.uint32)[inside], w.view(np.uint32)[inside])
    assert not dt[~inside].any() and not dw[~inside].any() and (dw > 0).sum() > 1000
    # the device's own dense volume over the same lattice
    dense = device_volume(s, sparse=False)
    m = torch.from_numpy(inside).to(DEV)
    st, sw = vol.to_dense()
    assert torch.equal(bits(st[m]), bits(dense.tsdf[m])) and torch.equal(bits(sw[m]), bits(dense.weight[m]))
    # voxels of edge blocks beyond dims are never updated
    _, inl = state.indices()
    assert not bool(vol.weight.cpu()[torch.from_numpy(~inl)].any())


def test_colour_holds_the_dense_bits_on_allocated_voxels():
    s, rgbs = scene("sphere64"), images("sphere64")
    state = restated("sphere64", colour=True)
    vol = device_volume(s, rgbs)
    assert_state_bits(vol, state, "sphere64 with colour")
    if "dense_rgb64" not in _CACHE:
        _CACHE["dense_rgb64"] = C.scene_fused_rgb(s, rgbs)
    t, w, c = _CACHE["dense_rgb64"]
    inside = S.allocated_mask(state)
    dt, dw, dc = (x.cpu().numpy() for x in vol.to_dense())
    for got, want in ((dt, t), (dw, w), (dc, c)):
        assert np.array_equal(got.view(np.uint32)[inside], want.view(np.uint32)[inside]) and not got[~inside].any()
    assert len(np.unique(dc)) > 256 and vol.memory_bytes == vol.block_of.numel() * 4 + vol.n_blocks * (12 + 5 * 512 * 4)
    dense = device_volume(s, rgbs, sparse=False)
    m = torch.from_numpy(inside).to(DEV)
    sc = vol.to_dense()[2]
    assert torch.equal(bits(sc[m]), bits(dense.colour[m]))
    # geometry is the colourless volume's
    plain = device_volume(s)
    assert torch.equal(bits(plain.tsdf), bits(vol.tsdf)) and torch.equal(bits(plain.weight), bits(vol.weight)) and plain.colour is None


# ---- calls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,calls", [("sphere64", (slice(0, 3), slice(3, 7))), ("room64", (slice(0, 2), slice(2, 5)))])
def test_two_calls_follow_the_opened_at_call_rule(name, calls):
    s = scene(name)
    state = S.fuse(s, calls=list(calls))
    vol = device_volume(s, calls=list(calls))
    assert_state_bits(vol, state, f"{name} in two calls")
    one = restated(name)
    assert state.n_blocks == one.n_blocks and not np.array_equal(state.block_coords, one.block_coords)      # (the second call opened blocks)
    if name == "room64":
        assert not np.array_equal(state.weight[state.block_of[tuple(one.block_coords.T)]], one.weight)    # and they missed the first call's views


def test_allocating_first_makes_two_calls_equal_one():
    s = scene("sphere64")
    one = restated("sphere64")
    vol = device_volume(s, calls=[slice(0, 3), slice(3, 7)], allocate_first=True)
    assert_state_bits(vol, one, "allocate, then two integrate(allocate=False)")
    vol.reset()
    assert vol.n_blocks == 0 and tuple(vol.tsdf.shape) == (0, 8, 8, 8) and bool((vol.block_of == -1).all())
    assert vol.extract_mesh()[0].shape == (0, 3)
    # integrate(allocate=False) on a volume without blocks does nothing
    vol.integrate(s.depths, s.intrinsics_matrices(), s.poses, allocate=False)
    assert vol.n_blocks == 0


# ---- mesh -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere32", "room_odd"])
def test_mesh_equals_the_restatement_numbering_included(name):
    s, state = scene(name), restated(name)
    want = S.extract_sparse(state, s.origin, s.vl, tables())
    assert_mesh_bits(device_volume(s).extract_mesh(), want, name)
    assert len(want[1]) > 500
    with pytest.raises(ValueError, match="colour"):
        device_volume(s).extract_coloured_mesh()


def test_coloured_mesh_equals_the_restatement_and_the_dense_mesh():
    s, rgbs, state = scene("sphere64"), images("sphere64"), restated("sphere64", colour=True)
    want = S.extract_sparse(state, s.origin, s.vl, tables())
    vol = device_volume(s, rgbs)
    got = vol.extract_coloured_mesh()
    assert_mesh_bits(got, want, "sphere64 with colour")
    v, f = vol.extract_mesh()
    # ((1 - r) c + r c) / 255 with c = 255 may round a few ulps past 1 (tsdf_colour_restatement.CONSTANT_BOUND, derived there)
    assert torch.equal(bits(v), bits(got[0])) and torch.equal(f, got[1])
    assert float(got[2].min()) >= 0 and float(got[2].max()) <= 1 + C.CONSTANT_BOUND
    # the dense volume's coloured mesh: the same triangles, and the same colour at every vertex position
    dv, df, dc = (x.cpu().numpy() for x in device_volume(s, rgbs, sparse=False).extract_coloured_mesh())
    sv, sf, sc = (x.cpu().numpy() for x in got)
    assert S.triangle_set(sv, sf) == S.triangle_set(dv, df)
    ds, ss = np.lexsort(dv.view(np.uint64).T[::-1]), np.lexsort(sv.view(np.uint64).T[::-1])
    assert np.array_equal(dv[ds].view(np.uint64), sv[ss].view(np.uint64))
    assert np.abs(dc[ds] - sc[ss]).max() < 2.0 ** -40            # (two edges that round to one position may differ in the last bits)


@pytest.mark.parametrize("name", ["sphere128", "room128"])
def test_mesh_is_the_dense_volumes_mesh(name):
    s = scene(name)
    vol = device_volume(s)
    dense = device_volume(s, sparse=False)
    sv, sf = (x.cpu().numpy() for x in vol.extract_mesh())
    dv, df = (x.cpu().numpy() for x in dense.extract_mesh())
    print(f"{name}: {vol.n_blocks} of {vol.block_of.numel()} blocks, {len(sf)} faces sparse, {len(df)} dense; {vol.memory_bytes} B against "
          f"{2 * dense.tsdf.numel() * 4} B")
    assert len(df) > 10000 and sf.shape == df.shape and sv.shape == dv.shape
    cv, cf = S.canonical(sv, sf)
    cdv, cdf = S.canonical(dv, df)
    assert np.array_equal(cv, cdv) and np.array_equal(cf, cdf)
    assert vol.n_blocks < vol.block_of.numel() // 2 + 1


# ---- beyond the dense limit -------------------------------------------------------------------------------------------------
def test_a_lattice_beyond_the_dense_limit():
    s = scene("far")
    assert s.dims == (4096, 4096, 2048)
    with pytest.raises(ValueError, match="2\\^31"):
        tsdf.TSDFVolume(s.origin, s.dims, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    state = restated("far")
    vol = device_volume(s)
    print(f"far: {vol.n_blocks} blocks of {vol.block_of.numel()}, {vol.memory_bytes} B")
    assert 100 < vol.n_blocks < 2000
    assert_state_bits(vol, state, "far")
    lo, hi = state.block_coords.min(0), state.block_coords.max(0)
    assert (lo <= (487, 375, 187)).all() and (hi >= (487, 375, 187)).all()               # the block of voxel (3900, 3000, 1500)
    assert (state.weight > 0).sum() > 5000
    want = S.extract_sparse(state, s.origin, s.vl, tables())
    assert len(want[1]) > 500
    assert_mesh_bits(vol.extract_mesh(), want, "far")
    with pytest.raises(ValueError, match="2\\^31"):
        vol.to_dense()


# ---- shapes where indexing can go wrong -------------------------------------------------------------------------------------
def many_eyes(n):
    """n eyes on a sphere of radius 2 around the origin (a golden-angle spiral)."""
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    rad = np.sqrt(1.0 - z * z)
    return tuple((2.0 * rad[j] * np.cos(phi[j]), 2.0 * rad[j] * np.sin(phi[j]), 2.0 * z[j]) for j in range(n))


@pytest.mark.parametrize("dims,h,w,n_views", [((1, 1, 1), 1, 1, 1), ((8, 8, 8), 7, 5, 2), ((9, 9, 9), 7, 5, 3), ((5, 3, 2), 7, 5, 2),
                                              ((16, 16, 12), 1, 1, 7), ((8, 9, 17), 5, 7, 300)])
def test_shapes_where_indexing_can_go_wrong(dims, h, w, n_views):
    """One voxel and one pixel; exactly one block; one voxel more than a block on every axis; a lattice smaller than a block; maps of
    one pixel; 300 views: the third round of the view test (128 lanes per round) and, in the dense kernel, the second."""
    eyes = many_eyes(n_views) if n_views > 7 else R.SPHERE_EYES[:n_views]
    s = R.sphere_scene(dims=dims, h=h, w=w, eyes=eyes)
    if h == w == 1:
        s.depths[:] = 1.5                                           # the one pixel sees the sphere's near pole
    rgbs = C.scene_images(s)
    state = S.fuse(s, rgbs=rgbs)
    vol = device_volume(s, rgbs)
    assert_state_bits(vol, state, f"dims {dims}, maps {h} x {w}, {n_views} views")
    assert state.n_blocks >= 1 and (state.weight > 0).any()
    assert_mesh_bits(vol.extract_coloured_mesh(), S.extract_sparse(state, s.origin, s.vl, tables()), f"dims {dims}")
    dense = device_volume(s, rgbs, sparse=False)
    inside = torch.from_numpy(S.allocated_mask(state)).to(DEV)
    for a, b in zip(vol.to_dense(), (dense.tsdf, dense.weight, dense.colour)):
        assert torch.equal(bits(a[inside]), bits(b[inside]))
    if n_views == 300:
        assert state.weight.max() > 128
        less = S.fuse(R.Scene(s.dims, s.origin, s.vl, s.trunc, s.poses[:299], s.k4s[:299], s.depths[:299]), rgbs=rgbs[:299])
        assert not np.array_equal(less.weight, state.weight)        # the last view is applied


def test_a_view_that_sees_nothing_opens_nothing():
    s = scene("sphere32")
    for colour in (False, True):
        vol = tsdf.SparseTSDFVolume(s.origin, s.dims, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV, colour=colour)
        rgb = np.zeros((48, 64, 3), dtype=np.uint8) if colour else None
        vol.integrate(np.zeros((48, 64), dtype=np.float32), s.intrinsics_matrices()[0], s.poses[0], rgb=rgb)
        assert vol.n_blocks == 0 and vol.memory_bytes == vol.block_of.numel() * 4
        mesh = vol.extract_coloured_mesh() if colour else vol.extract_mesh()
        assert all(tuple(x.shape) == (0, 3) and x.is_cuda for x in mesh) and len(mesh) == (3 if colour else 2)
        assert all(not bool(x.any()) for x in vol.to_dense())
    # a view whose points all lie outside the lattice opens nothing either
    vol = tsdf.SparseTSDFVolume((50.0, 50.0, 50.0), s.dims, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    assert vol.allocate(s.depths, s.intrinsics_matrices(), s.poses) == 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    s = scene("sphere32")
    k = s.intrinsics_matrices()
    plain = tsdf.SparseTSDFVolume(s.origin, s.dims, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    coloured = tsdf.SparseTSDFVolume(s.origin, s.dims, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV, colour=True)
    with pytest.raises(ValueError, match="without colour"):
        plain.integrate(s.depths, k, s.poses, rgb=images("sphere32"))
    with pytest.raises(ValueError, match="required"):
        coloured.integrate(s.depths, k, s.poses)
    assert plain.n_blocks == 0 and coloured.n_blocks == 0
    with pytest.raises(ValueError, match="non-finite or negative"):
        plain.allocate(-s.depths, k, s.poses)
    # the three limits
    with pytest.raises(ValueError, match="2\\^24"):
        tsdf.SparseTSDFVolume(s.origin, (8, (1 << 24) + 8, 8), device=DEV)
    with pytest.raises(ValueError, match="blocks"):
        tsdf.SparseTSDFVolume(s.origin, (1 << 14, 1 << 14, 1 << 12), device=DEV)
    full = tsdf.SparseTSDFVolume(s.origin, s.dims, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    full.block_coords = torch.zeros((1 << 22) - 10, 3, dtype=torch.int32, device=DEV)     # as if 2^22 - 10 blocks were held already
    with pytest.raises(ValueError, match="2\\^31"):
        full.allocate(s.depths, k, s.poses)
    # to_dense on a lattice of 2^31 voxels or more
    with pytest.raises(ValueError, match="to_dense"):
        tsdf.SparseTSDFVolume(s.origin, (2048, 1024, 1024), device=DEV).to_dense()
    # arrays on mismatched devices
    vol = device_volume(s)
    d = torch.from_numpy(s.depths).to(DEV)
    kk, e = torch.from_numpy(s.k4s).to(DEV), torch.from_numpy(s.e12s).to(DEV)
    with pytest.raises(lib.VfnError, match="device"):
        lib.tsdf_sparse_integrate(vol.tsdf, vol.weight, None, vol.block_coords.cpu(), vol.dims, vol.origin, vol.voxel_length, vol.sdf_trunc, d, None, kk, e)
    with pytest.raises(lib.VfnError, match="device"):
        lib.tsdf_sparse_integrate(vol.tsdf, vol.weight, None, vol.block_coords, vol.dims, vol.origin, vol.voxel_length, vol.sdf_trunc, d.cpu(), None, kk, e)
    with pytest.raises(lib.VfnError, match="device"):
        lib.tsdf_sparse_extract(vol.tsdf, vol.weight, None, vol.block_of.cpu(), vol.block_coords, vol.dims, vol.origin, vol.voxel_length)
    with pytest.raises(lib.VfnError, match="device"):
        lib.tsdf_sparse_mark(torch.zeros(vol.block_dims, dtype=torch.uint8, device=DEV), vol.origin, vol.voxel_length, vol.sdf_trunc, d.cpu(),
                             tsdf.mark_cameras(kk.cpu(), e.cpu()).to(DEV))
    with pytest.raises(lib.VfnError, match="block_of"):
        lib.tsdf_sparse_extract(vol.tsdf, vol.weight, None, vol.block_of[:2], vol.block_coords, vol.dims, vol.origin, vol.voxel_length)
    with pytest.raises(lib.VfnError, match="go together"):
        lib.tsdf_sparse_integrate(vol.tsdf, vol.weight, None, vol.block_coords, vol.dims, vol.origin, vol.voxel_length, vol.sdf_trunc, d,
                                  torch.zeros(7, 48, 64, 3, dtype=torch.uint8, device=DEV), kk, e)


# ---- the surface above the class --------------------------------------------------------------------------------------------
def test_fuse_maps_with_and_without_sparse():
    s, rgbs = scene("sphere32"), images("sphere32")
    k = s.intrinsics_matrices()
    lo = np.asarray(s.origin, dtype=np.float64)
    hi = lo + np.asarray(s.dims) * np.float64(s.vl)
    box = tsdf.bounds_box((lo, hi), s.vl)
    args = dict(bounds=(lo, hi), voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    for colour in (False, True):
        hand = {}
        for sparse, cls in ((True, tsdf.SparseTSDFVolume), (False, tsdf.TSDFVolume)):
            vol = cls(box[0], box[1], voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV, colour=colour)
            vol.integrate(s.depths, k, s.poses, rgb=rgbs if colour else None)
            hand[sparse] = vol.extract_coloured_mesh() if colour else vol.extract_mesh()
            got = tsdf.fuse_rgbd_maps(s.depths, rgbs, k, s.poses, sparse=sparse, **args) if colour else \
                tsdf.fuse_depth_maps(s.depths, k, s.poses, sparse=sparse, **args)
            assert len(got) == len(hand[sparse]) == (3 if colour else 2) and got[1].shape[0] > 500
            for a, b in zip(got, hand[sparse]):
                assert a.shape == b.shape and torch.equal(bits(a), bits(b)), (colour, sparse)
        default = tsdf.fuse_rgbd_maps(s.depths, rgbs, k, s.poses, **args) if colour else tsdf.fuse_depth_maps(s.depths, k, s.poses, **args)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(default, hand[False]))               # the default stays dense
        sv, sf = (x.cpu().numpy() for x in hand[True][:2])
        dv, df = (x.cpu().numpy() for x in hand[False][:2])
        assert S.triangle_set(sv, sf) == S.triangle_set(dv, df)
    # the box found from the depths, and nothing seen
    a = tsdf.fuse_depth_maps(s.depths, k, s.poses, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV, sparse=True)
    b = tsdf.fuse_depth_maps(s.depths, k, s.poses, voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    assert S.triangle_set(*(x.cpu().numpy() for x in a)) == S.triangle_set(*(x.cpu().numpy() for x in b)) and a[1].shape[0] > 500
    none = tsdf.fuse_rgbd_maps(np.zeros_like(s.depths), rgbs, k, s.poses, device=DEV, sparse=True)
    assert len(none) == 3 and all(tuple(x.shape) == (0, 3) for x in none)


def test_fuse_maps_sparse_takes_a_box_the_dense_volume_refuses():
    s = scene("far")
    lo = np.asarray(s.origin, dtype=np.float64)
    hi = lo + np.asarray(s.dims) * np.float64(s.vl)
    k = s.intrinsics_matrices()
    with pytest.raises(ValueError, match="2\\^31"):
        tsdf.fuse_depth_maps(s.depths, k, s.poses, bounds=(lo, hi), voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    v, f = tsdf.fuse_depth_maps(s.depths, k, s.poses, bounds=(lo, hi), voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV, sparse=True)
    hv, hf = device_volume(s).extract_mesh()
    assert torch.equal(bits(v), bits(hv)) and torch.equal(f, hf) and f.shape[0] > 500


def test_refuse_passes_sparse_through():
    from vf_nerf_amd import refuse
    s = scene("sphere32")
    k = s.intrinsics_matrices()
    mesh = device_volume(s).extract_mesh()
    args = dict(voxel_length=s.vl, sdf_trunc=s.trunc, device=DEV)
    a = refuse.refuse(mesh, k, s.poses, 48, 64, sparse=True, **args)
    b = refuse.refuse(mesh, k, s.poses, 48, 64, **args)
    assert a[1].shape[0] > 500 and S.triangle_set(*(x.cpu().numpy() for x in a)) == S.triangle_set(*(x.cpu().numpy() for x in b))
