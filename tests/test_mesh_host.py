"""Mesh triangulation, host side: the embedded case tables, the CPU restatement against the reference's recorded meshes, the drop-in
patch, and the argument checks that run before any launch (tests/golden/mesh_stages.npz, written by make_mesh_golden.py)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, mesh  # noqa: E402
import mesh_restatement as R  # noqa: E402

FIX = np.load(os.path.join(REPO, "tests", "golden", "mesh_stages.npz"))
TABLES = (FIX["tables.tri"], FIX["tables.edge_vertex"])


def field_inputs(tag):
    """(res, sides, norms) of a recorded field stage; norms not recorded are torch.norm of the (unsmoothed) field, as methods.py:223."""
    res = int(tag.split(".")[0][1:])
    norms = FIX[f"{tag}.norms"] if f"{tag}.norms" in FIX.files else torch.norm(torch.from_numpy(FIX[f"f{res}.pred"]), dim=1).numpy()
    return res, FIX[f"{tag}.sides"], norms


def assert_same_mesh(v, f, tag):
    ev, ef = FIX[f"{tag}.vs"], FIX[f"{tag}.fs"] - 1
    assert v.shape == ev.shape and f.shape == ef.shape, (tag, v.shape, ev.shape, f.shape, ef.shape)
    assert np.array_equal(v.view(np.uint64), ev.view(np.uint64)), tag         # bit for bit, signed zeros included
    assert np.array_equal(f, ef), tag


def test_embedded_tables_equal_the_recorded_ones():
    et, ev, tt = lib.mesh_tables()
    assert np.array_equal(et, FIX["tables.edge"])
    assert np.array_equal(ev, FIX["tables.edge_vertex"])
    assert np.array_equal(tt, FIX["tables.tri"])


def test_header_documents_the_mesh_entry_points():
    protos = lib.header_prototypes()
    for name in ("vfn_mesh_tables", "vfn_mesh_scan_workspace_bytes", "vfn_mesh_count", "vfn_mesh_emit", "vfn_mesh_dedup", "vfn_mesh_number",
                 "vfn_mesh_field_norms"):
        assert name in protos and name in lib.EXPORTS
    assert protos["vfn_mesh_count"][1][9:11] == ["double", "double"]


@pytest.mark.parametrize("tag", [str(t) for t in FIX["index.fields"]])
def test_restatement_reproduces_recorded_fields(tag):
    res, sides, norms = field_inputs(tag)
    assert_same_mesh(*R.triangulate_fused(sides, norms, res, TABLES), tag)
    if f"{tag}.comb" in FIX.files:
        assert_same_mesh(*R.triangulate_general(FIX[f"{tag}.comb"], FIX[f"{tag}.udf"], FIX[f"{tag}.cells"], res, 2.0, 0.0, TABLES), tag)
        comb, udf = R.comb_udf_from_sides(sides, norms, res, FIX[f"{tag}.cells"])
        assert np.array_equal(comb, FIX[f"{tag}.comb"]) and np.array_equal(udf, FIX[f"{tag}.udf"])


@pytest.mark.parametrize("name", [str(t) for t in FIX["index.general"]])
def test_restatement_reproduces_recorded_general_cases(name):
    res, size, iso = FIX[f"g.{name}.args"]
    v, f = R.triangulate_general(FIX[f"g.{name}.comb"], FIX[f"g.{name}.udf"], FIX[f"g.{name}.cells"], int(res), float(size), float(iso), TABLES)
    assert_same_mesh(v, f, f"g.{name}")


@pytest.mark.parametrize("name", [str(t) for t in FIX["index.dense"]])
def test_restatement_reproduces_recorded_dense_cases(name):
    res, size, iso = FIX[f"d.{name}.args"]
    udf = FIX[f"d.{name}.udf"] if f"d.{name}.udf" in FIX.files else None
    v, f = R.triangulate_general(FIX[f"d.{name}.comb"], udf, None, int(res), float(size), float(iso), TABLES)
    assert_same_mesh(v, f, f"d.{name}")


def test_snap_case_shares_corner_vertices():
    """The |v1 - v2| <= 1e-5 case really exercises the snap: vertices on grid corners, each used by several faces."""
    v, f = FIX["g.snap.vs"], FIX["g.snap.fs"]
    res = int(FIX["g.snap.args"][0])
    on_corner = np.all(np.isclose((v + 1.0) * res / 2.0, np.round((v + 1.0) * res / 2.0), atol=0, rtol=0), axis=1)
    assert on_corner.sum() > 10
    uses = np.bincount(f.reshape(-1) - 1, minlength=len(v))
    assert (uses[on_corner] >= 3).any()


def test_install_patches_and_restores_marching_cubes():
    from vf_nerf_amd import dropin
    names = ("evaluation", "evaluation.utils", "evaluation.utils.marching_cubes_vt")
    saved = {n: sys.modules.get(n) for n in names}
    try:
        def reference_fn(*a, **k):
            return "reference"
        for n in names[:2]:
            pkg = types.ModuleType(n)
            pkg.__path__ = []
            sys.modules[n] = pkg
        stub = types.ModuleType(names[2])
        stub.contrastive_marching_cubes = reference_fn
        sys.modules[names[2]] = stub
        sys.modules["evaluation.utils"].marching_cubes_vt = stub
        dropin.install(patch_evaluator=False, patch_clip=False, patch_mesh=True)
        assert stub.contrastive_marching_cubes is mesh.contrastive_marching_cubes
        dropin.install(patch_evaluator=False, patch_clip=False, patch_mesh=True)          # twice: the reference's function stays remembered
        dropin.install(patch_evaluator=False, patch_clip=False, patch_mesh=False)
        assert stub.contrastive_marching_cubes is reference_fn
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
        dropin.uninstall_clip_grad_norm()


def test_arguments_are_refused_before_any_launch():
    comb = np.zeros((4, 28), dtype=np.float32)
    udf = np.zeros((4, 28, 2), dtype=np.float32)
    cells = np.zeros((4, 3), dtype=np.int64)
    with pytest.raises(ValueError):
        mesh.triangulate(comb[:, :27], res=8, udf=udf, selected_indices=cells)               # wrong comb shape
    with pytest.raises(ValueError):
        mesh.triangulate(comb, res=8, udf=udf[:3], selected_indices=cells)                  # wrong udf shape
    with pytest.raises(ValueError):
        mesh.triangulate(comb, res=8, udf=udf, selected_indices=cells[:, :2])               # cells not [M,3]
    with pytest.raises(ValueError):
        mesh.triangulate(comb, res=8, udf=None, selected_indices=cells)                     # the reference's branch needs udf
    with pytest.raises(ValueError):
        mesh.triangulate(comb, res=8)                                                       # dense needs res^3 rows
    with pytest.raises(ValueError):
        mesh.triangulate(comb, res=0, udf=udf, selected_indices=cells)
    field = torch.zeros(7 ** 3, 3)
    with pytest.raises(ValueError):
        mesh.field_to_mesh(field, 7)                                                        # odd resolution
    with pytest.raises(lib.VfnError):
        mesh.field_to_mesh(torch.zeros(8 ** 3, 3), 8)                                       # host tensor where the device is required
    with pytest.raises(ValueError):
        mesh.extract_mesh(None, 9)
