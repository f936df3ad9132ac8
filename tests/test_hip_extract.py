"""GPU tests of the extraction driver both triangulating units share (lib._extract over csrc/vfn_mc_extract.h), at the smallest shapes
where its bookkeeping can go wrong: no triangle at all (nothing to emit, nothing to merge) and exactly one (one count, one slot
triple), for the mesh source and for the TSDF source.  The larger shapes are tests/test_hip_mesh.py and tests/test_hip_tsdf.py."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from vf_nerf_amd import mesh, tsdf  # noqa: E402
import mesh_restatement as MR  # noqa: E402
import tsdf_restatement as TR  # noqa: E402
from test_mesh_host import TABLES  # noqa: E402

pytestmark = pytest.mark.gpu


def assert_empty_device_mesh(v, f):
    assert v.is_cuda and f.is_cuda
    assert tuple(v.shape) == (0, 3) and v.dtype == torch.float64
    assert tuple(f.shape) == (0, 3) and f.dtype == torch.int64


def assert_bits(v, f, ev, ef):
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert v.dtype == np.float64 and f.dtype == np.int64
    assert v.shape == ev.shape and f.shape == ef.shape, (v.shape, ev.shape, f.shape, ef.shape)
    assert np.array_equal(v.view(np.uint64), ev.view(np.uint64)) and np.array_equal(f, ef)


def test_mesh_source_without_a_triangle():
    """The dense raster of res = 2 (8 cells) with an all-zero comb: max 0 <= 0.5 in every cell."""
    v, f = mesh.triangulate(np.zeros((8, 28), dtype=np.float32), res=2)
    assert_empty_device_mesh(v, f)


def test_tsdf_source_without_a_triangle():
    """One cell whose corners were never observed."""
    vol = tsdf.TSDFVolume((0.0, 0.0, 0.0), (2, 2, 2), voxel_length=1.0, sdf_trunc=1.0)
    assert float(vol.weight.abs().max()) == 0.0
    assert_empty_device_mesh(*vol.extract_mesh())


def test_tsdf_source_with_one_triangle():
    """The hand-set cell of tests/test_tsdf_host.py: corner 0 inside, the others outside."""
    t = np.full((2, 2, 2), 0.75, dtype=np.float32)
    t[0, 0, 0] = -0.25
    w = np.ones((2, 2, 2), dtype=np.float32)
    origin, vl = (1.0, 2.0, 3.0), 0.5
    vol = tsdf.TSDFVolume(origin, (2, 2, 2), voxel_length=vl, sdf_trunc=1.0)
    vol.tsdf.copy_(torch.from_numpy(t))
    vol.weight.copy_(torch.from_numpy(w))
    ev, ef = TR.extract(t, w, origin, vl, TABLES)
    assert ef.shape == (1, 3) and ev.shape == (3, 3)
    v, f = vol.extract_mesh()
    assert v.is_cuda and f.is_cuda
    assert_bits(v, f, ev, ef)


def test_mesh_source_with_one_triangle():
    """One cell of the general form, named by ``selected_indices``: the comb of a cell whose corner 1 sides against the seven others
    (pair (a, b) is 1 iff exactly one of a, b is corner 1), so the values are +|udf| at corner 1 and -|udf| elsewhere: one triangle."""
    comb = np.array([[1.0 if (a == 1) != (b == 1) else 0.0 for a, b in MR.PAIRS]])
    mags = np.array([0.3, 0.7, 0.2, 0.9, 0.4, 0.6, 0.8, 0.1])
    udf = np.zeros((1, 28, 2))
    udf[0, 0, 0] = mags[0]
    udf[0, :7, 1] = mags[1:]
    cells = np.array([[1, 2, 0]])
    ev, ef = MR.triangulate_general(comb, udf, cells, 3, 2.0, 0.0, TABLES)
    assert ef.shape == (1, 3) and ev.shape == (3, 3)
    v, f = mesh.triangulate(comb, udf=udf, selected_indices=cells, res=3, size=2.0, isovalue=0.0)
    assert v.is_cuda and f.is_cuda
    assert_bits(v, f, ev, ef)
