"""Mesh triangulation on the MI355X (csrc/vfn_mesh.hip through vf_nerf_amd/mesh.py) against the reference's recorded meshes
(tests/golden/mesh_stages.npz) and against the CPU restatement (tests/mesh_restatement.py).  Every comparison is exact: vertex bits,
key order, faces."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import grid, lib, mesh  # noqa: E402
import mesh_restatement as R  # noqa: E402
import grid_margins as GM  # noqa: E402
from helpers import synthetic_field  # noqa: E402
from test_mesh_host import FIX, TABLES, assert_same_mesh, field_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def recorded_ref(tag):
    v, f = FIX[f"{tag}.vs"], FIX[f"{tag}.fs"]
    return {tuple(row): i + 1 for i, row in enumerate(v)}, f.tolist()


def assert_same_dict(vs, fs, tag):
    evs, efs = recorded_ref(tag)
    assert list(vs.values()) == list(range(1, len(vs) + 1))
    keys = np.array(list(vs.keys()), dtype=np.float64).reshape(-1, 3)
    assert np.array_equal(keys.view(np.uint64), FIX[f"{tag}.vs"].view(np.uint64)), tag
    assert vs == evs and fs == efs, tag
    assert all(type(x) is np.float64 for x in next(iter(vs))) if vs else True


def general_cases():
    for name in FIX["index.general"]:
        res, size, iso = FIX[f"g.{name}.args"]
        yield f"g.{name}", dict(comb_values=FIX[f"g.{name}.comb"], udf=FIX[f"g.{name}.udf"], selected_indices=FIX[f"g.{name}.cells"],
                                res=int(res), size=float(size), isovalue=float(iso))
    for name in FIX["index.dense"]:
        res, size, iso = FIX[f"d.{name}.args"]
        yield f"d.{name}", dict(comb_values=FIX[f"d.{name}.comb"], udf=FIX[f"d.{name}.udf"] if f"d.{name}.udf" in FIX.files else None,
                                res=int(res), size=float(size), isovalue=float(iso))
    yield "f16", dict(comb_values=FIX["f16.comb"].reshape(-1), udf=FIX["f16.udf"].reshape(-1, 2), selected_indices=FIX["f16.cells"], res=16)


CASES = list(general_cases())


@pytest.mark.parametrize("tag,kw", CASES, ids=[c[0] for c in CASES])
def test_general_form_equals_reference(tag, kw):
    vs, fs = mesh.contrastive_marching_cubes(**kw)
    assert_same_dict(vs, fs, tag)
    v, f = mesh.triangulate(**kw)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float64 and f.dtype == torch.int64
    assert_same_mesh(v.cpu().numpy(), f.cpu().numpy(), tag)
    # torch inputs (fp64 too: widened exactly) give the same mesh
    kw64 = dict(kw, comb_values=torch.from_numpy(np.asarray(kw["comb_values"])).double(),
                udf=None if kw.get("udf") is None else torch.from_numpy(np.asarray(kw["udf"])).double().to(DEV))
    v2, f2 = mesh.triangulate(**kw64)
    assert torch.equal(v2.view(torch.int64), v.view(torch.int64)) and torch.equal(f2, f)


@pytest.mark.parametrize("tag", [str(t) for t in FIX["index.fields"]])
def test_field_to_mesh_equals_reference(tag):
    """Unsmoothed fields: divergence, side bytes, norms and the mesh equal the reference's bit for bit.  Smoothed fields: the separable
    smoothing kernels (csrc/vfn_grid.hip) round differently from the reference's CPU conv3d, so there the divergence and side bytes are
    exact, every norm lies within the smoothing bound of its float64 value (tests/grid_margins.py: smoothed_norm_reference) and within
    the sum of both bounds of the recorded one, the face count EQUALS the reference's (with equal side bytes the triangle list is a
    function of the bytes and of which norms are exactly zero) and every triangle corner lies within 2 h eps_norm of the reference's
    (h the cell size, eps_norm the largest relative norm difference found here: a vertex is p1 + h n1 / (n1 + n2) along its edge),
    except corners on an edge inside the snap band of vertex_interpolate's |v1 - v2| > 1e-5 switch, whose share is capped.  The
    triangulation itself is pinned exactly by the restatement fed with the device's own stages."""
    res, sides, norms = field_inputs(tag)
    after, all_ = tag.endswith(".after"), tag.endswith(".all")
    pred = torch.from_numpy(FIX[f"f{res}.pred"]).to(DEV)
    st = mesh.field_stages(pred, res, smooth_after=after, smooth_all=all_)
    assert torch.equal(st.divergence.cpu().reshape(-1), torch.from_numpy(FIX[f"{tag}.div"]).reshape(-1)), "divergence"
    assert np.array_equal(st.sides.cpu().numpy(), sides), "side bytes"
    v, f = mesh.field_to_mesh(pred, res, smooth_after=after, smooth_all=all_)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    if not (after or all_):
        assert np.array_equal(st.norms.cpu().numpy().view(np.uint32), np.asarray(norms, dtype=np.float32).view(np.uint32)), "norms"
        assert_same_mesh(v, f, tag)
    else:
        got = st.norms.cpu().double()
        rec = torch.from_numpy(np.asarray(norms)).double()
        norm64, tol, tol_conv3d = GM.smoothed_norm_reference(torch.from_numpy(FIX[f"f{res}.pred"]), res, after, all_)
        print(f"{tag}: norms err / tol against float64 {float(((got - norm64).abs() / tol).max()):.3f}, against the recorded ones "
              f"{float(((got - rec).abs() / (tol + tol_conv3d)).max()):.3f}; smallest norm {float(norm64.min()):.4f}")
        assert bool(((got - norm64).abs() <= tol).all()), "norms against float64"
        assert bool(((got - rec).abs() <= tol + tol_conv3d).all()), "norms against the recorded ones"
        assert np.allclose(got.numpy(), norms, rtol=1e-4, atol=0), "norms"            # the earlier fence stays
        eps_norm = float(((got - rec).abs() / rec).max())
        ref_v, ref_f = FIX[f"{tag}.vs"], FIX[f"{tag}.fs"] - 1
        assert len(f) == len(ref_f), f"{len(f)} faces, the reference has {len(ref_f)}"
        cut, band, segments = GM.edge_snap_margin(sides, norms, res, eps_norm, TABLES[1])
        assert cut > 100 and band <= GM.CAP_SNAP_BAND * cut, (cut, band)
        mine, theirs = GM.triangle_corners(v, f), GM.triangle_corners(ref_v, ref_f)
        skip = GM.corners_on_segments(theirs, segments, res)
        dist = np.abs(mine - theirs).max(axis=-1)
        h = 2.0 / res
        print(f"{tag}: eps_norm {eps_norm:.3e}, {cut} cut edges, {band} in the snap band, largest corner distance {dist[~skip].max():.3e} "
              f"(bound {2 * h * eps_norm:.3e})")
        assert float(dist[~skip].max()) <= 2 * h * eps_norm, tag
    rv, rf = R.triangulate_fused(st.sides.cpu().numpy(), st.norms.cpu().numpy(), res, TABLES)
    assert np.array_equal(rv.view(np.uint64), v.view(np.uint64)) and np.array_equal(rf, f)


def test_field_norms_match_torch_cpu():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1 << 21, 3, generator=g) * torch.logspace(-20, 20, 1 << 21).unsqueeze(1)
    x[:7] = 0
    n, u = lib.mesh_field_norms(x.to(DEV))
    assert torch.equal(n.cpu(), torch.norm(x, dim=1))
    assert torch.equal(u.cpu(), torch.nn.functional.normalize(x, dim=1))


@pytest.mark.parametrize("res", [64, 130, 256])
def test_fused_equals_general_on_device_tables(res):
    pred = synthetic_field(res, res).to(DEV)
    st = mesh.field_stages(pred, res)
    v, f = mesh.field_to_mesh(pred, res)
    assert f.shape[0] > 1000
    # the general form fed with the device's own make_comb_format tables, the reference's cell order and selection
    choice = lib.grid_unify_direction(st.divergence.reshape(-1), lib.mesh_field_norms(pred)[1], res)
    comb, pn = lib.grid_comb_format(choice, st.norms, res)
    del choice
    order = torch.from_numpy(R.block_order(res)).to(DEV)
    flat = (order[:, 0] * res + order[:, 1]) * res + order[:, 2]
    comb, pn = comb[flat], pn[flat]
    keep = comb.sum(-1) > 0
    v2, f2 = mesh.triangulate(comb[keep], udf=pn[keep], selected_indices=order[keep], res=res)
    assert torch.equal(v2.view(torch.int64), v.view(torch.int64)) and torch.equal(f2, f)
    if res == 64:
        rv, rf = R.triangulate_fused(st.sides.cpu().numpy(), st.norms.cpu().numpy(), res, TABLES)
        assert np.array_equal(rv.view(np.uint64), v.cpu().numpy().view(np.uint64)) and np.array_equal(rf, f.cpu().numpy())


def test_extract_mesh_equals_queries_then_field_to_mesh():
    import vf_nerf_amd
    res, scale = 64, 1.1
    translation, centroid = torch.tensor([0.05, -0.02, 0.01]), torch.tensor([0.0, 0.1, -0.05])
    torch.manual_seed(0)
    model = vf_nerf_amd.VectorFieldNerf(vf_nerf_amd.shipped_config(DEV, n_samples=32, n_importance=32, perturb=False, dir_to_normal_th=-0.2))
    model.eval()
    raw = np.load(os.path.join(REPO, "tests", "golden", "trained_256.npz"))
    for tag, mod in (("vf", model.vector_field_network), ("rn", model.rendering_network), ("density", model.density)):
        mod.load_state_dict({k[len(f"w.{tag}."):]: torch.from_numpy(raw[k]) for k in raw.files if k.startswith(f"w.{tag}.")})
    model.to(DEV)
    model._invalidate_packs()
    dec = model.vector_field_network
    got = mesh.extract_mesh(dec, res, scale=scale, translation=translation, centroid=centroid)
    # the reference's lattice on the host (evaluation/methods.py:190-208), its queries, then the device stages
    idx = torch.arange(0, res ** 3, 1, out=torch.LongTensor())
    samples = torch.zeros(res ** 3, 3)
    samples[:, 2] = idx % res
    samples[:, 1] = (idx.long() // res) % res
    samples[:, 0] = ((idx.long() // res) // res) % res
    vs_ = scale * 2.0 / (res - 1)
    samples[:, 0] = (samples[:, 0] * vs_) + -scale + translation[0] + centroid[0]
    samples[:, 1] = (samples[:, 1] * vs_) + -scale + translation[1] + centroid[1]
    samples[:, 2] = (samples[:, 2] * vs_) + -scale + translation[2] + centroid[2]
    a0, a1, a2 = mesh.lattice_axes(res, scale, translation, centroid)
    assert torch.equal(samples[0::res * res, 0], a0) and torch.equal(samples[0:res * res:res, 1], a1) and torch.equal(samples[0:res, 2], a2)
    pred = grid.get_set_predictions(dec, samples, 100000, DEV).to(DEV)
    v, f = mesh.field_to_mesh(pred, res)
    assert f.shape[0] > 100
    assert torch.equal(got.vertices.view(torch.int64), v.view(torch.int64)) and torch.equal(got.faces, f)
    v32 = v.cpu().numpy().astype(np.float32).astype(np.float64)
    want = v32 * scale + translation.numpy().astype(np.float64) + centroid.numpy().astype(np.float64)
    assert np.array_equal(got.vertices_scaled.cpu().numpy(), want)


def test_non_finite_field_is_refused():
    res = 16
    pred = torch.from_numpy(FIX["f16.pred"]).clone()
    pred[(5 * res + 6) * res + 7] = float("nan")
    with pytest.raises(lib.VfnError, match="non-finite"):
        mesh.field_to_mesh(pred.to(DEV), res)
    udf = FIX["f16.udf"].copy()
    udf[:, :, :] = np.inf
    with pytest.raises(lib.VfnError, match="non-finite"):
        mesh.triangulate(FIX["f16.comb"], udf=udf, selected_indices=FIX["f16.cells"], res=res)
    cells = FIX["f16.cells"].copy()
    cells[3, 1] = res
    with pytest.raises(lib.VfnError, match="outside"):
        mesh.triangulate(FIX["f16.comb"], udf=FIX["f16.udf"], selected_indices=cells, res=res)
