"""The block-sparse TSDF volume, host side (no GPU): the NumPy restatement (tests/tsdf_sparse_restatement.py) agrees with the dense
restatement voxel by voxel; the allocation rule covers every cell the dense extraction triangulates; the sparse extraction gives the
dense mesh; the new exports are declared, bound and linked; the limits are refused before a device is asked for."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, tsdf  # noqa: E402
import tsdf_restatement as R  # noqa: E402
import tsdf_colour_restatement as C  # noqa: E402
import tsdf_sparse_restatement as S  # noqa: E402

NEW_EXPORTS = ("vfn_tsdf_sparse_mark", "vfn_tsdf_sparse_integrate", "vfn_tsdf_sparse_integrate_rgb", "vfn_tsdf_sparse_count",
               "vfn_tsdf_sparse_emit", "vfn_tsdf_sparse_emit_colours")

SCENES = {
    "sphere32": lambda: R.sphere_scene(),
    "room32": lambda: R.room_scene(),
    "sphere64": lambda: R.sphere_scene((64, 64, 64)),
    "room64": lambda: R.room_scene((64, 64, 64)),
    "room_odd": lambda: R.room_scene((33, 17, 70)),
    "sphere128": lambda: R.sphere_scene((128, 128, 128), h=96, w=128),
    "room128": lambda: R.room_scene((128, 128, 128), h=60, w=80),
}
# the block counts of the prototype of the rule (a cross-check, not a contract)
PROTOTYPE_BLOCKS = {"sphere128": (1489, 4096), "room128": (2004, 4096), "sphere64": (402, 512), "room_odd": (74, 135)}
_CACHE = {}


def tables():
    _, edge_vertex, tri = lib.mesh_tables()
    return tri, edge_vertex


def fused(name):
    """The scene, its dense restated volume and its one-call sparse state: computed once, never written to."""
    if name not in _CACHE:
        s = SCENES[name]()
        _CACHE[name] = (s, s.fused(), S.fuse(s))
    return _CACHE[name]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_tsdf_sparse_mark"] == ("int", ["uint8_t*", "int32_t", "int32_t", "int32_t", "float", "float", "float", "float", "float",
                                                      "const float*", "int32_t", "int32_t", "const double*", "int32_t", "void*"])
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    # the argument checks answer before any launch
    assert handle.vfn_tsdf_sparse_integrate(None, None, None, 1, (1 << 24) + 1, 1, 1, 0.0, 0.0, 0.0, 1.0, 1.0, None, 1, 1, None, None, 1, None) != 0
    assert b"2^24" in handle.vfn_last_error()
    assert handle.vfn_tsdf_sparse_count(None, None, None, None, 1 << 22, 4096, 4096, 4096, None, None, None, None, 0, None) != 0
    assert b"blocks" in handle.vfn_last_error()
    assert handle.vfn_tsdf_sparse_mark(None, 2048, 2048, 512, 0.0, 0.0, 0.0, 1.0, 1.0, None, 1, 1, None, 1, None) != 0
    assert b"2^31" in handle.vfn_last_error()


@pytest.mark.parametrize("name", ["sphere32", "room32"])
def test_integrate_at_is_the_dense_restatement_on_every_voxel(name):
    s, (t, w), _ = fused(name)
    idx = np.stack(np.meshgrid(*(np.arange(n) for n in s.dims), indexing="ij"), axis=-1).reshape(-1, 3)
    ts, wt = np.zeros(len(idx), dtype=np.float32), np.zeros(len(idx), dtype=np.float32)
    S.integrate_at(idx, ts, wt, s.origin, s.vl, s.trunc, s.depths, s.k4s, s.e12s)
    assert np.array_equal(bits(ts.reshape(s.dims)), bits(t)) and np.array_equal(bits(wt.reshape(s.dims)), bits(w))
    assert (w > 0).sum() > t.size // 4
    # and with colour: the colour restatement's bits
    rgbs = C.scene_images(s)
    tc, wc, cc = C.scene_fused_rgb(s, rgbs)
    ts, wt, col = np.zeros(len(idx), dtype=np.float32), np.zeros(len(idx), dtype=np.float32), np.zeros((len(idx), 3), dtype=np.float32)
    S.integrate_at(idx, ts, wt, s.origin, s.vl, s.trunc, s.depths, s.k4s, s.e12s, col, rgbs)
    assert np.array_equal(bits(ts.reshape(s.dims)), bits(tc)) and np.array_equal(bits(col.reshape(s.dims + (3,))), bits(cc))


@pytest.mark.parametrize("name", list(SCENES))
def test_the_allocation_covers_every_cell_the_dense_extraction_triangulates(name):
    s, (t, w), state = fused(name)
    total = int(np.prod(state.block_of.shape))
    uncovered = S.uncovered_cells(state, t, w)
    active = int(S.active_cells(t, w).sum())
    # no voxel of the truncation band lies outside a block either
    band = (w > 0) & (np.abs(t) < 1) & ~S.allocated_mask(state)
    print(f"{name}: {state.n_blocks} of {total} blocks, {active} active cells, {uncovered} uncovered, {int(band.sum())} band voxels outside a block")
    assert active > 100
    assert uncovered == 0
    assert int(band.sum()) == 0
    if name in PROTOTYPE_BLOCKS:
        assert (state.n_blocks, total) == PROTOTYPE_BLOCKS[name]
    # the one-call state holds the dense bits on allocated voxels and zero elsewhere
    inside = S.allocated_mask(state)
    dt, dw = S.to_dense(state)
    assert np.array_equal(bits(dt)[inside], bits(t)[inside]) and np.array_equal(bits(dw)[inside], bits(w)[inside])
    assert not dt[~inside].any() and not dw[~inside].any()


@pytest.mark.parametrize("name", ["sphere32", "room32", "sphere64", "room64"])
def test_the_sparse_mesh_is_the_dense_mesh(name):
    s, (t, w), state = fused(name)
    v, f = S.extract_sparse(state, s.origin, s.vl, tables())
    dv, df = R.extract(t, w, s.origin, s.vl, tables())
    assert len(df) > 500 and f.shape == df.shape and v.shape == dv.shape
    assert S.triangle_set(v, f) == S.triangle_set(dv, df)
    cv, cf = S.canonical(v, f)
    cdv, cdf = S.canonical(dv, df)
    assert np.array_equal(cv, cdv) and np.array_equal(cf, cdf)


def test_blocks_are_numbered_by_call_then_c_order_and_open_at_their_call():
    s = fused("room64")[0]
    one = fused("room64")[2]
    two = S.fuse(s, calls=[slice(0, 2), slice(2, 5)])
    assert two.n_blocks == one.n_blocks and np.array_equal(two.block_of >= 0, one.block_of >= 0)
    first = S.State(s.dims)
    n0 = S.allocate(first, s.origin, s.vl, s.trunc, s.depths[:2], s.k4s[:2], s.e12s[:2])
    assert 0 < n0 < two.n_blocks and np.array_equal(two.block_coords[:n0], first.block_coords)
    for part in (two.block_coords[:n0], two.block_coords[n0:]):
        keys = (part[:, 0].astype(np.int64) * 64 + part[:, 1]) * 64 + part[:, 2]
        assert (np.diff(keys) > 0).all()
    # blocks of the first call hold all five views, blocks of the second only views 2 .. 4 — which the first two also saw
    t7, w7 = s.fused()
    t4, w4 = s.fused(slice(2, 5))
    dt, dw = S.to_dense(two)
    early = np.repeat(np.repeat(np.repeat((two.block_of >= 0) & (two.block_of < n0), 8, 0), 8, 1), 8, 2)[:s.dims[0], :s.dims[1], :s.dims[2]]
    late = np.repeat(np.repeat(np.repeat(two.block_of >= n0, 8, 0), 8, 1), 8, 2)[:s.dims[0], :s.dims[1], :s.dims[2]]
    assert early.any() and late.any()
    assert np.array_equal(bits(dt)[early], bits(t7)[early]) and np.array_equal(bits(dw)[early], bits(w7)[early])
    assert np.array_equal(bits(dt)[late], bits(t4)[late]) and np.array_equal(bits(dw)[late], bits(w4)[late])
    assert not np.array_equal(bits(w4)[late], bits(w7)[late])
    # allocating everything first makes two calls equal one
    ahead = S.fuse(s, calls=[slice(0, 2), slice(2, 5)], allocate_first=True)
    assert np.array_equal(ahead.block_coords, one.block_coords)
    assert np.array_equal(bits(ahead.tsdf), bits(one.tsdf)) and np.array_equal(bits(ahead.weight), bits(one.weight))


def test_edge_blocks_keep_voxels_beyond_dims_untouched():
    s, _, state = fused("room_odd")
    g, inside = state.indices()
    assert (~inside).any() and not state.weight[~inside].any() and not state.tsdf[~inside].any()
    assert state.block_of.shape == (5, 3, 9)


def test_limits_are_refused_before_a_device_is_asked_for():
    big = tsdf._check_sparse_dims((4096, 4096, 2048))
    assert big == (4096, 4096, 2048)
    with pytest.raises(ValueError, match="2\\^31"):
        tsdf._check_dims(big)                                      # the dense volume's wall
    with pytest.raises(ValueError, match="2\\^24"):
        tsdf.SparseTSDFVolume((0, 0, 0), ((1 << 24) + 1, 1, 1))
    with pytest.raises(ValueError, match="blocks"):
        tsdf.SparseTSDFVolume((0, 0, 0), (1 << 14, 1 << 14, 1 << 12))      # 2048 x 2048 x 512 blocks = 2^31
    for bad in ((0, 1, 1), (1, 1), (1.5, 1, 1), (True, 1, 1)):
        with pytest.raises(ValueError, match="dims"):
            tsdf.SparseTSDFVolume((0, 0, 0), bad)
    with pytest.raises(ValueError, match="voxel_length"):
        tsdf.SparseTSDFVolume((0, 0, 0), (8, 8, 8), voxel_length=0.0)
    with pytest.raises(ValueError, match="origin"):
        tsdf.SparseTSDFVolume((0, float("nan"), 0), (8, 8, 8))
    # a box beyond the dense limit passes the sparse check of the fusion's box and fails the dense one
    box = ((0.0, 0.0, 0.0), (16.0, 16.0, 16.0))
    assert tsdf.bounds_box(box, tsdf.VOXEL_LENGTH, sparse=True)[1] == (2048, 2048, 2048)
    with pytest.raises(ValueError, match="2\\^31"):
        tsdf.bounds_box(box, tsdf.VOXEL_LENGTH)
    assert lib.tsdf_block_lattice((1, 8, 9)) == (1, 1, 2) and tsdf.BLOCK == lib.TSDF_BLOCK == S.BLOCK == 8


def test_mark_cameras_invert_the_float32_extrinsic():
    import torch
    s = fused("room32")[0]
    cams = tsdf.mark_cameras(torch.from_numpy(s.k4s), torch.from_numpy(s.e12s)).numpy()
    assert cams.dtype == np.float64 and cams.shape == (len(s.k4s), 17)
    for i in range(len(s.k4s)):
        c, fx, fy, cx, cy, q = S.cameras(s.k4s[i], s.e12s[i])
        assert np.array_equal(cams[i, :12].view(np.uint64), c.reshape(12).view(np.uint64))
        assert np.array_equal(cams[i, 12:].view(np.uint64), np.array([fx, fy, cx, cy, q]).view(np.uint64))
        assert np.abs(c[:, :3] @ s.e12s[i].astype(np.float64).reshape(3, 4)[:, :3] - np.eye(3)).max() < 1e-6


def test_the_evaluator_switch_is_set_by_the_dropin():
    import importlib
    import types
    from vf_nerf_amd import evaluator
    assert evaluator.TSDF_SPARSE is False
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in ("models", "evaluation")}
    fake_pkg, fake = types.ModuleType("evaluation"), types.ModuleType("evaluation.methods")
    fake_pkg.__path__ = []
    fake.render_images, fake.metrics, fake.tsdf_mesh = (lambda *a, **k: "r"), (lambda *a, **k: "m"), (lambda *a, **k: "t")
    try:
        sys.modules["evaluation"], sys.modules["evaluation.methods"] = fake_pkg, fake
        dropin = importlib.import_module("vf_nerf_amd.dropin")
        dropin.install()
        assert evaluator.TSDF_SPARSE is False                                     # None leaves it as it is
        dropin.install(tsdf_sparse=True)
        assert evaluator.TSDF_SPARSE is True
        dropin.install()
        assert evaluator.TSDF_SPARSE is True
        dropin.install(tsdf_sparse=False)
        assert evaluator.TSDF_SPARSE is False
    finally:
        evaluator.TSDF_SPARSE = False
        import vf_nerf_amd.dropin as dropin
        dropin.uninstall_clip_grad_norm()
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "evaluation")]:
            del sys.modules[k]
        sys.modules.update(saved)


def test_evaluator_tsdf_mesh_asks_for_the_sparse_volume_only_when_switched(tmp_path, monkeypatch):
    """evaluator.tsdf_mesh with the reference's modules stood in for and the fusion stubbed: the switch adds sparse=True to the call and
    nothing else; off, the call carries no keyword at all."""
    import types
    import torch
    from PIL import Image
    from vf_nerf_amd import evaluator
    os.makedirs(tmp_path / "rendered_images")
    np.save(tmp_path / "rendered_images" / "depth-0.npy", np.full((3, 4, 1), 1.25))
    Image.fromarray(np.zeros((3, 4, 3), dtype=np.uint8)).save(tmp_path / "rendered_images" / "image-0.png")

    class Dataset:
        def __init__(self, config):
            self.intrinsics, self.poses = torch.eye(4), torch.eye(4)[None]

    calls = []

    def fuse_rgbd_maps(d, c, intrinsics, poses, **kwargs):
        calls.append(kwargs)
        v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64)
        return v, torch.tensor([[0, 1, 2]]), torch.zeros(3, 3, dtype=torch.float64)

    monkeypatch.setattr(tsdf, "fuse_rgbd_maps", fuse_rgbd_maps)
    names = ("datasets", "datasets.normal_datasets")
    saved = {key: sys.modules[key] for key in names if key in sys.modules}
    fakes = {key: types.ModuleType(key) for key in names}
    fakes["datasets"].__path__ = []
    fakes["datasets.normal_datasets"].dataset_dict = {"fake": Dataset}
    try:
        sys.modules.update(fakes)
        for switch in (False, True):
            monkeypatch.setattr(evaluator, "TSDF_SPARSE", switch)
            evaluator.tsdf_mesh(str(tmp_path), types.SimpleNamespace(dataset_name="fake"))
    finally:
        for key in names:
            del sys.modules[key]
        sys.modules.update(saved)
    assert calls == [{}, {"sparse": True}]
    assert os.path.exists(tmp_path / "tsdf-mesh" / "tsdf.ply")
