"""Host tests of vf_nerf_amd.geomargs: what each shared argument check accepts and refuses, and that every geometry unit refuses a
device that is not a GPU with lib.VfnError before anything is launched."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from vf_nerf_amd import geomargs, lib, mesh, metrics3d, raster, tsdf  # noqa: E402

V = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
F = np.array([[0, 1, 2]])


def test_limit():
    assert geomargs.LIMIT == 1 << 31 and tsdf.LIMIT is geomargs.LIMIT and raster.LIMIT is geomargs.LIMIT and metrics3d.LIMIT is geomargs.LIMIT


def test_as_tensor():
    t = torch.ones(2, 3, requires_grad=True)
    out = geomargs.as_tensor(t, "t")
    assert not out.requires_grad and out.data_ptr() == t.data_ptr()
    a = np.arange(6.0).reshape(2, 3)[:, ::2]                     # not contiguous
    out = geomargs.as_tensor(a, "a")
    assert out.dtype == torch.float64 and out.is_contiguous() and np.array_equal(out.numpy(), a)
    for bad in ([[0.0, 1.0]], 3.0, None, "mesh.ply"):
        with pytest.raises(TypeError, match="x: expected a numpy array or a torch tensor"):
            geomargs.as_tensor(bad, "x")


def test_device_refuses_what_is_not_a_gpu():
    for bad in ("cpu", torch.device("cpu"), "meta"):
        with pytest.raises(lib.VfnError, match="TSDF fusion runs on the device"):
            geomargs.device(bad, "TSDF fusion")
    assert geomargs.device("cuda:1", "x") == torch.device("cuda", 1)          # (naming a device asks nothing of it)
    assert geomargs.device(torch.device("cuda", 0), "x") == torch.device("cuda:0")
    if not torch.cuda.is_available():
        with pytest.raises(lib.VfnError, match="mesh scoring runs on the device .* no GPU is visible"):
            geomargs.device(None, "mesh scoring")
    else:
        assert geomargs.device(None, "x") == torch.device("cuda", torch.cuda.current_device())


@pytest.mark.parametrize("call", [
    lambda: mesh.triangulate(np.zeros((8, 28), dtype=np.float32), res=2, device="cpu"),
    lambda: metrics3d.nearest_distances(V, V, device="cpu"),
    lambda: tsdf.TSDFVolume((0.0, 0.0, 0.0), (2, 2, 2), device="cpu"),
    lambda: raster.rasterize_depth(V, F, np.eye(3), np.eye(4), 4, 4, device="cpu"),
], ids=["mesh", "metrics3d", "tsdf", "raster"])
def test_every_unit_refuses_the_cpu_up_front(call):
    with pytest.raises(lib.VfnError, match="no CPU fallback.*got device cpu"):
        call()


def test_empty_mesh():
    v, f = geomargs.empty_mesh("cpu")
    assert tuple(v.shape) == (0, 3) and v.dtype == torch.float64 and tuple(f.shape) == (0, 3) and f.dtype == torch.int64


def test_check_mesh_accepts_both_forms():
    m = mesh.Mesh(torch.zeros(3, 3, dtype=torch.float64), torch.tensor([[0, 1, 2]]), torch.ones(3, 3, dtype=torch.float64))
    v, f = geomargs.check_mesh(m, "m")
    assert torch.equal(v, m.vertices_scaled) and torch.equal(f, m.faces)
    for pair in ((V, F), [torch.from_numpy(V).float(), torch.from_numpy(F).int()]):
        v, f = geomargs.check_mesh(pair, "m", allow_empty=False)
        assert tuple(v.shape) == (3, 3) and tuple(f.shape) == (1, 3)
    # a mesh of nothing is a mesh where the caller allows it, and only there
    for pair in ((V, np.zeros((0, 3), dtype=np.int64)), (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))):
        v, f = geomargs.check_mesh(pair)
        assert f.shape[0] == 0
        with pytest.raises(ValueError, match="m has no (faces|vertices)"):
            geomargs.check_mesh(pair, "m", allow_empty=False)
    with pytest.raises(ValueError, match="m has no vertices"):
        geomargs.check_mesh((np.zeros((0, 3)), F), "m", allow_empty=False)


@pytest.mark.parametrize("bad,exc", [
    ("mesh.ply", TypeError), ((V, F, F), TypeError), (V, TypeError), (([[0.0, 0, 0]], F), TypeError),
    ((V[:, :2], F), ValueError), ((V.reshape(-1), F), ValueError), ((V.astype(np.int64), F), ValueError),
    ((V, F.astype(np.float64)), ValueError), ((V, F.astype(bool)), ValueError), ((V, F.reshape(-1)), ValueError), ((V, F[:, :2]), ValueError),
])
def test_check_mesh_refuses(bad, exc):
    with pytest.raises(exc):
        geomargs.check_mesh(bad, "m")


def test_positive_int():
    assert geomargs.positive_int(1, "n") == 1 and geomargs.positive_int(np.int64(7), "n") == 7
    assert type(geomargs.positive_int(np.int32(7), "n")) is int
    assert geomargs.positive_int(geomargs.LIMIT - 1, "n") == geomargs.LIMIT - 1
    for bad in (0, -3, 2.0, 2.5, True, "4", None, geomargs.LIMIT, np.float32(3)):
        with pytest.raises(ValueError, match="^n "):
            geomargs.positive_int(bad, "n")


def test_real32():
    assert geomargs.real32(0, "x") == 0.0 and geomargs.real32(-2.5, "x") == -2.5 and geomargs.real32(np.float64(0.5), "x") == 0.5
    assert geomargs.real32(0.1, "x") == float(np.float32(0.1))                 # the float32's value, not the argument's
    assert geomargs.real32(1e-60, "x") == 0.0                                   # (underflow is finite)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e39, -1e39, True, "1.0", None, 1 + 0j):
        with pytest.raises(ValueError, match="^x "):
            geomargs.real32(bad, "x")


def test_positive32():
    assert geomargs.positive32(4.0 / 512.0, "vl") == 4.0 / 512.0 and geomargs.positive32(3, "vl") == 3.0
    assert geomargs.positive32(0.04, "vl") == float(np.float32(0.04))
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-60, True, "1.0", None):
        with pytest.raises(ValueError, match="^vl "):
            geomargs.positive32(bad, "vl")
