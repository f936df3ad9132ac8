"""Colour in the TSDF unit, host side: the new entry points are declared, bound and linked; the NumPy restatement of the colour
contract (tests/tsdf_colour_restatement.py) on constant images, on hand-set volumes and on the analytic sphere; the argument checks
that run before any launch; the PLY writer and reader byte for byte; evaluator.tsdf_mesh with the reference's modules stood in for."""
import importlib
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, ply, refuse, tsdf  # noqa: E402
import tsdf_restatement as R  # noqa: E402
import tsdf_colour_restatement as C  # noqa: E402

NEW_EXPORTS = ("vfn_tsdf_integrate_rgb", "vfn_tsdf_emit_colours", "vfn_tsdf_vertex_colours")


def tables():
    _, edge_vertex, tri = lib.mesh_tables()
    return tri, edge_vertex


@pytest.fixture(scope="module")
def sphere():
    """The sphere scene fused with the pattern images, and its coloured mesh: computed once, never written to."""
    s = R.sphere_scene()
    rgbs = C.scene_images(s)
    t, w, c = C.scene_fused_rgb(s, rgbs)
    return s, rgbs, t, w, c, C.extract_coloured(t, w, c, s.origin, s.vl, tables())


def test_new_exports_are_declared_bound_and_linked():
    protos = lib.header_prototypes()
    for name in NEW_EXPORTS:
        assert name in protos and name in lib.EXPORTS, name
    assert protos["vfn_tsdf_integrate_rgb"] == ("int", ["float*", "float*", "float*", "int32_t", "int32_t", "int32_t", "float", "float", "float",
                                                        "float", "float", "const float*", "const uint8_t*", "int32_t", "int32_t", "const float*",
                                                        "const float*", "int32_t", "void*"])
    assert protos["vfn_tsdf_emit_colours"] == ("int", ["const float*", "const float*", "const float*", "int32_t", "int32_t", "int32_t",
                                                       "const int32_t*", "const int32_t*", "double*", "void*"])
    assert protos["vfn_tsdf_vertex_colours"] == ("int", ["const int64_t*", "int64_t", "const double*", "int32_t*", "int64_t", "double*", "void*"])
    assert lib.header_abi_version() == 5                                            # additions only
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    symbols = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW_EXPORTS) <= symbols, set(NEW_EXPORTS) - symbols
    handle = lib.load()
    for name in NEW_EXPORTS:
        assert getattr(handle, name).argtypes is not None
    # the argument checks of the exports answer before any launch: no device is needed to be refused
    assert handle.vfn_tsdf_integrate_rgb(None, None, None, 0, 1, 1, 0.0, 0.0, 0.0, 1.0, 1.0, None, None, 1, 1, None, None, 1, None) != 0
    assert b"dims" in handle.vfn_last_error()
    assert handle.vfn_tsdf_integrate_rgb(None, None, None, 1, 1, 1, 0.0, 0.0, 0.0, 1.0, 1.0, None, None, 1, 1, None, None, 1, None) != 0
    assert b"NULL volume" in handle.vfn_last_error()
    assert handle.vfn_tsdf_emit_colours(None, None, None, 2, 2, 0, None, None, None, None) != 0
    assert b"dims" in handle.vfn_last_error()
    assert handle.vfn_tsdf_vertex_colours(None, 3, None, None, 4, None, None) != 0       # more vertices than slots
    assert b"limits" in handle.vfn_last_error()
    assert handle.vfn_tsdf_vertex_colours(None, 3, None, None, 1, None, None) != 0
    assert b"NULL" in handle.vfn_last_error()
    assert {"tsdf_integrate_rgb", "tsdf_extract_coloured"} <= set(dir(lib))


def test_restatement_keeps_the_geometry_bits_and_float32():
    s = R.sphere_scene()
    rgbs = C.scene_images(s)
    t, w, c = C.scene_fused_rgb(s, rgbs)                                          # (asserts per view that tsdf / weight are R.integrate_view's)
    rt, rw = s.fused()
    assert np.array_equal(t.view(np.uint32), rt.view(np.uint32)) and np.array_equal(w.view(np.uint32), rw.view(np.uint32))
    assert c.dtype == np.float32 and c.shape == s.dims + (3,)
    assert not c[w == 0].any() and (c[w > 0] >= 0).all() and (c[w > 0] <= 255).all() and len(np.unique(c[w > 0])) > 1000
    with pytest.raises(AssertionError):                                            # the widening check is alive in this module too
        C.integrate_view_rgb(t.copy(), w.copy(), c.astype(np.float64), s.origin, s.vl, s.trunc, s.depths[0], rgbs[0], s.k4s[0], s.e12s[0])
    # neighbouring pixels, channels and views of the pattern all differ
    assert (rgbs[:, 1:] != rgbs[:, :-1]).all() and (rgbs[:, :, 1:] != rgbs[:, :, :-1]).all() and (rgbs[1:] != rgbs[:-1]).all()
    assert (rgbs[..., 0] != rgbs[..., 1]).mean() > 0.99 and (rgbs[..., 1] != rgbs[..., 2]).mean() > 0.99


def test_one_view_colour_is_the_pixel_the_depth_was_read_from():
    """After ONE view every observed voxel holds exactly the byte triple of one pixel of that view: (0 x 0 + p) / 1 = p."""
    s = R.sphere_scene()
    rgbs = C.scene_images(s)
    t, w, c = C.scene_fused_rgb(s, rgbs, slice(2, 3))
    seen = c[w > 0]
    assert len(seen) > 1000 and np.array_equal(seen, np.rint(seen))
    pixels = {tuple(p) for p in rgbs[2].reshape(-1, 3)}
    assert all(tuple(int(x) for x in p) in pixels for p in seen[::37])


def test_constant_colour_is_exact():
    """The running mean of equal integers <= 255 with integer weights is exact in float32: every observed voxel holds c to the bit.
    Every vertex holds c / 255 up to the interpolation's own roundings: the contract's ((1 - r) c + r c) / 255 rounds 1 - r, the two
    products, the sum and the quotient once each — nothing of it is exact for 0 < r < 1 (with r = 1/3 and c = 255 the sum is one ulp
    off 255) — so the relative error is below (1 + 2^-53)^5 - 1 < 2^-50 on a value of at most 1; a channel of 0 stays 0 exactly."""
    s = R.sphere_scene()
    for colour in C.CONSTANT_COLOURS:
        rgbs = C.constant_images(len(s.depths), *s.depths.shape[1:], colour)
        t, w, c = C.scene_fused_rgb(s, rgbs)
        assert w.max() >= 3
        assert np.array_equal(c[w > 0], np.broadcast_to(np.float32(colour), c[w > 0].shape)) and not c[w == 0].any()
        v, f, vc = C.extract_coloured(t, w, c, s.origin, s.vl, tables())
        want = np.float64(colour) / 255.0
        print(f"colour {colour}: {int((vc != want).sum())} of {vc.size} vertex channels differ from c / 255, by at most {np.abs(vc - want).max():.3g}")
        assert len(v) > 1000 and np.abs(vc - want).max() <= C.CONSTANT_BOUND
        zero = np.asarray(colour) == 0
        assert not vc[:, zero].any()


def test_vertex_colours_are_first_slot_colours(sphere):
    s, rgbs, t, w, c, (v, f, vc) = sphere
    slots = C.slot_colours(t, w, c, tables())
    ids = f.reshape(-1)
    assert len(slots) == len(ids) and vc.shape == v.shape
    uniq, first = np.unique(ids, return_index=True)                                # the lowest slot of every id
    assert np.array_equal(uniq, np.arange(len(v)))
    want = np.stack([slots[i][1] for i in first])
    assert np.array_equal(vc.view(np.uint64), want.view(np.uint64))
    assert (vc >= 0).all() and (vc <= 1).all() and len(np.unique(vc)) > 1000
    # all the slots of a vertex lie on ONE edge here (no absorbed offsets in this scene) and carry equal colours
    edge_of = {}
    for vid, (edge, col) in zip(ids, slots):
        assert edge_of.setdefault(vid, edge) == edge and np.array_equal(col, vc[vid])


def test_absorbed_positions_take_the_first_slots_colour():
    t, w, c, origin, vl = C.absorbed_cell()
    v, f, vc = C.extract_coloured(t, w, c, origin, vl, tables())
    assert np.array_equal(f, [[0, 0, 0]]) and np.array_equal(v, [[2.0 ** 60] * 3])
    slots = C.slot_colours(t, w, c, tables())
    assert [s[0] for s in slots] == [((0, 0, 0), 1), ((0, 0, 0), 2), ((0, 0, 0), 0)]
    assert len({tuple(s[1]) for s in slots}) == 3
    r = 0.25
    assert np.array_equal(vc[0], ((1.0 - r) * c[0, 0, 0].astype(np.float64) + r * c[0, 1, 0].astype(np.float64)) / 255.0)


def test_edges_meeting_at_a_zero_corner_give_its_colour():
    """The cut edge from voxel (0,0,0) up to the zero voxel has r = 1, the one from the zero voxel up to (0,2,0) has r = 0: both give the
    zero voxel's colour / 255 EXACTLY, on the one vertex the two cells share."""
    t, w, c = C.zero_corner_volume()
    v, f, vc = C.extract_coloured(t, w, c, (0.0, 0.0, 0.0), 1.0, tables())
    assert v.shape == (5, 3) and f.shape == (2, 3)
    on_corner = np.flatnonzero(np.all(v == [0.5, 1.5, 0.5], axis=1))
    assert len(on_corner) == 1
    assert np.array_equal(vc[on_corner[0]], c[0, 1, 0].astype(np.float64) / 255.0)
    slots = C.slot_colours(t, w, c, tables())
    at = [col for vid, (edge, col) in zip(f.reshape(-1), slots) if vid == on_corner[0]]
    edges = {edge for vid, (edge, col) in zip(f.reshape(-1), slots) if vid == on_corner[0]}
    assert edges == {((0, 0, 0), 1), ((0, 1, 0), 1)} and all(np.array_equal(a, at[0]) for a in at)


def test_arguments_are_refused_before_any_launch():
    depth = np.ones((2, 4, 5), dtype=np.float32)
    rgb = np.zeros((2, 4, 5, 3), dtype=np.uint8)
    k = np.array([[4.0, 0, 2], [0, 4, 1.5], [0, 0, 1]], dtype=np.float32)
    poses = np.tile(np.eye(4), (2, 1, 1))
    bounds = ((-1, -1, -1), (1, 1, 1))
    assert tuple(tsdf._stack_rgb(rgb, depth.shape).shape) == (2, 4, 5, 3)
    assert tuple(tsdf._stack_rgb(rgb[0], (1, 4, 5)).shape) == (1, 4, 5, 3)
    assert tsdf._stack_rgb(torch.zeros(2, 4, 5, 3), depth.shape).dtype == torch.float32
    bad_rgbs = (rgb.astype(np.float64), rgb.astype(np.int32), rgb.astype(np.float16), rgb.astype(bool),      # dtype
                rgb[..., :2], rgb.reshape(2, 4, 15), rgb.transpose(0, 3, 1, 2), rgb.reshape(-1),             # shape
                rgb[:1], rgb[:, :3], rgb[:, :, :4], np.zeros((2, 5, 4, 3), dtype=np.uint8))                  # size differing from the depth's
    for bad in bad_rgbs:
        with pytest.raises(ValueError):
            tsdf._stack_rgb(bad, depth.shape)
        with pytest.raises(ValueError):
            tsdf.fuse_rgbd_maps(depth, bad, k, poses, bounds=bounds)
    with pytest.raises(TypeError):
        tsdf.fuse_rgbd_maps(depth, rgb.tolist(), k, poses, bounds=bounds)
    with pytest.raises(ValueError):
        tsdf.fuse_rgbd_maps(depth, None, k, poses, bounds=bounds)
    with pytest.raises(ValueError):
        tsdf.fuse_rgbd_maps(depth, rgb, k, poses[:1], bounds=bounds)                                        # the depth path's refusals stay
    # a volume refuses rgb it cannot use, and a missing one, before it looks at anything else (no device behind these two objects)
    plain, coloured = object.__new__(tsdf.TSDFVolume), object.__new__(tsdf.TSDFVolume)
    plain.colour, coloured.colour = None, torch.zeros(1, 1, 1, 3)
    with pytest.raises(ValueError, match="without colour"):
        plain.integrate(depth, k, poses, rgb=rgb)
    with pytest.raises(ValueError, match="required"):
        coloured.integrate(depth, k, poses)
    for bad in bad_rgbs:
        with pytest.raises(ValueError):
            coloured.integrate(depth, k, poses, rgb=bad)
    with pytest.raises(ValueError):
        plain.extract_coloured_mesh()
    mesh = (np.zeros((3, 3)), np.array([[0, 1, 2]]))
    with pytest.raises(ValueError):
        refuse.refuse_rgbd(mesh, None, k, poses, 4, 5)
    with pytest.raises(ValueError):
        refuse.refuse_rgbd(mesh, rgb[:1], k, poses, 4, 5)
    with pytest.raises(ValueError):
        refuse.refuse_rgbd(mesh, rgb.astype(np.float64), k, poses, 4, 5)
    with pytest.raises(TypeError):
        refuse.refuse_rgbd(mesh, rgb, k, poses, 4, 5, no_such_argument=1)
    if not torch.cuda.is_available():
        with pytest.raises(lib.VfnError):
            tsdf.TSDFVolume((0, 0, 0), (4, 4, 4), colour=True)                                               # no device: no fallback
        with pytest.raises(lib.VfnError):
            tsdf.fuse_rgbd_maps(depth, rgb, k, poses, bounds=bounds)
        with pytest.raises(lib.VfnError):
            lib.tsdf_integrate_rgb(torch.zeros(2, 2, 2), torch.zeros(2, 2, 2), torch.zeros(2, 2, 2, 3), (0, 0, 0), 1.0, 1.0,
                                   torch.zeros(1, 2, 2), torch.zeros(1, 2, 2, 3, dtype=torch.uint8), torch.zeros(1, 4), torch.zeros(1, 12))


# ---- PLY --------------------------------------------------------------------------------------------------------------
TRI_V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 2.0, -1.25]])
TRI_F = np.array([[0, 1, 2]])
TRI_C = np.array([[255, 0, 0], [0, 128, 0], [1, 2, 3]], dtype=np.uint8)


def header(fmt, vtype, colour):
    lines = ["ply", f"format {fmt} 1.0", "element vertex 3", f"property {vtype} x", f"property {vtype} y", f"property {vtype} z"]
    if colour:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    lines += ["element face 1", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def test_ply_bytes_of_one_triangle(tmp_path):
    path = str(tmp_path / "t.ply")
    ply.write_ply(path, TRI_V, TRI_F, binary=False)
    assert open(path, "rb").read() == header("ascii", "float", False) + b"0.0 0.0 0.0\n1.0 0.0 0.5\n0.0 2.0 -1.25\n3 0 1 2\n"
    ply.write_ply(path, TRI_V, TRI_F, TRI_C / 255.0, binary=False)
    assert open(path, "rb").read() == (header("ascii", "float", True) +
                                       b"0.0 0.0 0.0 255 0 0\n1.0 0.0 0.5 0 128 0\n0.0 2.0 -1.25 1 2 3\n3 0 1 2\n")
    face = b"\x03" + np.array([0, 1, 2], dtype="<i4").tobytes()
    ply.write_ply(path, TRI_V, TRI_F)
    assert open(path, "rb").read() == header("binary_little_endian", "float", False) + TRI_V.astype("<f4").tobytes() + face
    ply.write_ply(path, torch.from_numpy(TRI_V), torch.from_numpy(TRI_F), TRI_C)
    body = b"".join(TRI_V[i].astype("<f4").tobytes() + TRI_C[i].tobytes() for i in range(3))
    assert open(path, "rb").read() == header("binary_little_endian", "float", True) + body + face
    ply.write_ply(path, TRI_V, TRI_F, TRI_C, vertex_dtype="f8")
    body = b"".join(TRI_V[i].astype("<f8").tobytes() + TRI_C[i].tobytes() for i in range(3))
    assert open(path, "rb").read() == header("binary_little_endian", "double", True) + body + face


@pytest.mark.parametrize("binary", [True, False])
def test_ply_round_trip(tmp_path, binary):
    g = np.random.default_rng(5)
    v = g.standard_normal((50, 3)) * np.array([1e-3, 1.0, 1e6])
    f = g.integers(0, 50, (80, 3))
    c = g.random((50, 3))
    path = str(tmp_path / "m.ply")
    ply.write_ply(path, v, f, c, binary=binary, vertex_dtype="f8")
    rv, rf, rc = ply.read_ply(path)
    assert rv.dtype == np.float64 and rf.dtype == np.int64 and rc.dtype == np.uint8
    assert np.array_equal(rv.view(np.uint64), v.view(np.uint64)) and np.array_equal(rf, f)
    assert np.array_equal(rc, np.clip(np.rint(c * 255.0), 0, 255).astype(np.uint8))
    ply.write_ply(path, v, f, binary=binary)
    rv, rf, rc = ply.read_ply(path)
    assert rc is None and np.array_equal(rf, f) and np.array_equal(rv.astype(np.float32), v.astype(np.float32))
    assert np.array_equal(rv, v.astype(np.float32).astype(np.float64)) or not binary
    # an empty mesh is a file too
    ply.write_ply(path, np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3)), binary=binary)
    rv, rf, rc = ply.read_ply(path)
    assert rv.shape == (0, 3) and rf.shape == (0, 3) and rc.shape == (0, 3)


def test_ply_colour_bytes_recover_every_byte(tmp_path):
    b = np.arange(256)
    c = np.stack([b / 255.0, b[::-1] / 255.0, (b / 255.0).astype(np.float32).astype(np.float64)], axis=1)
    assert np.array_equal(ply.colour_bytes(c), np.stack([b, b[::-1], b], axis=1).astype(np.uint8))
    assert np.array_equal(ply.colour_bytes(np.array([[-0.5, 1.5, 0.4999 / 255]])), [[0, 255, 0]])
    u = np.stack([b, b, b], axis=1).astype(np.uint8)
    assert ply.colour_bytes(u) is not None and np.array_equal(ply.colour_bytes(u), u)
    path = str(tmp_path / "c.ply")
    ply.write_ply(path, np.zeros((256, 3)), np.zeros((0, 3), dtype=np.int64), c)
    assert np.array_equal(ply.read_ply(path)[2], np.stack([b, b[::-1], b], axis=1).astype(np.uint8))
    for bad in (np.array([[np.nan, 0, 0]]), np.zeros((2, 4)), np.zeros((2, 3), dtype=np.int32)):
        with pytest.raises(ValueError):
            ply.colour_bytes(bad)


def test_ply_reads_a_ground_truth_layout(tmp_path):
    """Extra vertex properties (normals, alpha) are skipped, uint indices and the name vertex_index accepted, comments ignored — ASCII and
    binary."""
    head = ("ply\nformat {} 1.0\ncomment made by a scanner\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
            "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            "property uchar alpha\nelement face 1\nproperty list uchar uint vertex_index\nend_header\n")
    path = str(tmp_path / "gt.ply")
    rec = np.zeros(3, dtype=[("p", "<f4", (3,)), ("n", "<f4", (3,)), ("c", "u1", (4,))])
    rec["p"], rec["n"], rec["c"][:, :3], rec["c"][:, 3] = TRI_V, 0.577, TRI_C, 255
    with open(path, "wb") as fh:
        fh.write(head.format("binary_little_endian").encode() + rec.tobytes() + b"\x03" + np.array([2, 1, 0], dtype="<u4").tobytes())
    v, f, c = ply.read_ply(path)
    assert np.array_equal(v, TRI_V) and np.array_equal(f, [[2, 1, 0]]) and np.array_equal(c, TRI_C)
    with open(path, "wb") as fh:
        rows = "".join(f"{p[0]} {p[1]} {p[2]} 0.5 0.5 0.7 {q[0]} {q[1]} {q[2]} 255\n" for p, q in zip(TRI_V, TRI_C))
        fh.write((head.format("ascii") + rows + "3 2 1 0\n").encode())
    v, f, c = ply.read_ply(path)
    assert np.array_equal(v, TRI_V) and np.array_equal(f, [[2, 1, 0]]) and np.array_equal(c, TRI_C)


def test_ply_refusals_are_raised_by_name(tmp_path):
    path = str(tmp_path / "bad.ply")

    def refused(text, match, tail=b""):
        with open(path, "wb") as fh:
            fh.write(text.encode() + tail)
        with pytest.raises(ply.PlyError, match=match):
            ply.read_ply(path)

    vertex = "element vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
    refused("ply\nformat binary_big_endian 1.0\n" + vertex + "end_header\n", "big-endian")
    refused("ply\nformat ascii 1.0\n" + vertex + "element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n4 0 0 0 0\n",
            "non-triangle")
    refused("ply\nformat binary_little_endian 1.0\n" + vertex + "element face 1\nproperty list uchar int vertex_indices\nend_header\n",
            "non-triangle", np.zeros(3, dtype="<f4").tobytes() + b"\x04" + np.zeros(4, dtype="<i4").tobytes())
    refused("plx\n", "not a PLY")
    refused("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n0 0\n", "x, y and z")
    refused("ply\nformat ascii 1.0\nelement edge 1\nproperty int a\n" + vertex + "end_header\n", "vertex")
    refused("ply\nformat ascii 1.0\n" + vertex + "element face 1\nproperty list uchar float vertex_indices\nend_header\n0 0 0\n3 0 0 0\n",
            "int or uint")
    refused("ply\nformat ascii 1.0\n" + vertex + "end_header\n", "ends before")
    for kwargs, err in ((dict(vertex_dtype="f2"), ValueError), (dict(colours=np.zeros((2, 3))), ValueError)):
        with pytest.raises(err):
            ply.write_ply(path, TRI_V, TRI_F, **kwargs)
    with pytest.raises(ValueError):
        ply.write_ply(path, TRI_V, np.array([[0, 1, 3]]))
    with pytest.raises(ValueError):
        ply.write_ply(path, TRI_V.astype(np.int64), TRI_F)


# ---- the evaluator's drop-in ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset_name,per_view", [("fake", False), ("dtu", True)])
def test_evaluator_tsdf_mesh_writes_the_references_file(tmp_path, monkeypatch, dataset_name, per_view):
    """evaluator.tsdf_mesh with the reference's modules stood in for and the device call stubbed: three views on disk as render_images
    leaves them (depth-i.npy [H,W,1] float64, image-i.png); the fusion receives the reference's depth (millimetre round trip), the PNGs'
    bytes, the dataset's intrinsics (shared, or per view for dtu) and poses; tsdf-mesh/tsdf.ply holds what it returned."""
    from PIL import Image
    from vf_nerf_amd import evaluator
    h, w, n = 5, 7, 3
    g = np.random.default_rng(23)
    depths = g.random((n, h, w, 1)) * 12.0
    images = g.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    os.makedirs(tmp_path / "rendered_images")
    for i in range(n):
        np.save(tmp_path / "rendered_images" / f"depth-{i}.npy", depths[i])
        Image.fromarray(images[i]).save(tmp_path / "rendered_images" / f"image-{i}.png")
    k = torch.eye(4)
    k[0, 0], k[1, 1], k[0, 2], k[1, 2] = 6.0, 6.5, 3.0, 2.0

    class Dataset:
        def __init__(self, config):
            self.intrinsics = torch.stack([k * (i + 1) for i in range(n)]) if per_view else k
            self.poses = torch.stack([torch.eye(4) + i for i in range(n)])

    calls = []

    def fuse_rgbd_maps(d, c, intrinsics, poses, **kwargs):
        calls.append((d, c, intrinsics, poses, kwargs))
        return torch.from_numpy(TRI_V), torch.from_numpy(TRI_F), torch.from_numpy(TRI_C / 255.0)

    monkeypatch.setattr(tsdf, "fuse_rgbd_maps", fuse_rgbd_maps)
    names = ("datasets", "datasets.normal_datasets")
    saved = {key: sys.modules[key] for key in names if key in sys.modules}
    fakes = {key: types.ModuleType(key) for key in names}
    fakes["datasets"].__path__ = []
    fakes["datasets.normal_datasets"].dataset_dict = {dataset_name: Dataset}
    try:
        sys.modules.update(fakes)
        evaluator.tsdf_mesh(str(tmp_path), types.SimpleNamespace(dataset_name=dataset_name))
    finally:
        for key in names:
            del sys.modules[key]
        sys.modules.update(saved)
    (d, c, intrinsics, poses, kwargs), = calls
    assert kwargs == {}                                                           # the reference's voxel length and truncation: the defaults
    assert np.array_equal(np.asarray(d), R.reference_depth(depths[..., 0])) and (np.asarray(d) == 0).any()
    assert np.asarray(c).dtype == np.uint8 and np.array_equal(np.asarray(c), images)
    want_k = torch.stack([(k * (i + 1))[:3, :3] for i in range(n)]) if per_view else k[:3, :3].expand(n, 3, 3)
    assert torch.equal(intrinsics.float(), want_k) and torch.equal(poses.float(), torch.stack([torch.eye(4) + i for i in range(n)]))
    v, f, col = ply.read_ply(str(tmp_path / "tsdf-mesh" / "tsdf.ply"))
    assert np.array_equal(v, TRI_V) and np.array_equal(f, TRI_F) and np.array_equal(col, TRI_C)
    with open(tmp_path / "tsdf-mesh" / "tsdf.ply", "rb") as fh:
        assert fh.read().startswith(header("binary_little_endian", "float", True))


def test_install_patches_tsdf_mesh_only_when_asked():
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in ("models", "evaluation")}
    fake_pkg, fake = types.ModuleType("evaluation"), types.ModuleType("evaluation.methods")
    fake_pkg.__path__ = []
    reference = lambda *a, **k: "reference tsdf_mesh"          # noqa: E731
    fake.render_images, fake.metrics, fake.tsdf_mesh = (lambda *a, **k: "r"), (lambda *a, **k: "m"), reference
    try:
        sys.modules["evaluation"], sys.modules["evaluation.methods"] = fake_pkg, fake
        dropin = importlib.import_module("vf_nerf_amd.dropin")
        from vf_nerf_amd import evaluator
        dropin.install()
        assert fake.tsdf_mesh is reference and not hasattr(fake, "_reference_tsdf_mesh")           # off by default
        dropin.install(patch_tsdf_mesh=False)
        assert fake.tsdf_mesh is reference
        dropin.install(patch_tsdf_mesh=True)
        assert fake.tsdf_mesh is evaluator.tsdf_mesh and fake._reference_tsdf_mesh is reference
        dropin.install(patch_tsdf_mesh=True)                                                       # twice: the reference's is kept
        assert fake._reference_tsdf_mesh is reference and fake.tsdf_mesh is evaluator.tsdf_mesh
        dropin.install()
        assert fake.tsdf_mesh is reference
    finally:
        import vf_nerf_amd.dropin as dropin
        dropin.uninstall_clip_grad_norm()
        for k in [k for k in sys.modules if k.split(".")[0] in ("models", "evaluation")]:
            del sys.modules[k]
        sys.modules.update(saved)
