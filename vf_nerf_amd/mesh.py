"""Mesh extraction on the device: contrastive marching cubes (csrc/vfn_mesh.hip) and the whole of evaluation/methods.py:140-322
(``marching_cubes_mesh``) without files.

* ``contrastive_marching_cubes`` — same signature and results as evaluation/utils/marching_cubes_vt.py:186-315: a dict of position
  tuples -> 1-based ids in order of first appearance, and a list of 1-based faces.  numpy or torch inputs.
* ``triangulate`` — the same computation, device tensors out (``vertices`` float64 [V,3], ``faces`` int64 [F,3], 0-based), no Python
  containers built.
* ``field_to_mesh`` — a device field [res^3,3] through methods.py:212-290 (smoothing, divergence, norms, side bytes) into the FUSED
  triangulation: the [res^3,28] comb and [res^3,28,2] pair-norm tables are never written, nothing res^3-sized crosses PCIe.
* ``extract_mesh`` — decoder -> lattice (regenerated on the device from its axis tables) -> queries -> ``field_to_mesh``.

Exactness: every vertex is the reference's float64 expression evaluated in the same order without contraction, so positions,
key order and faces equal the reference's bit for bit (tests/test_mesh_*.py).  Two documented departures: a non-finite norm /
udf value in a triangulated cell is refused (the reference's dict cannot merge NaN vertices in any meaningful way — ``nan != nan``,
so every NaN vertex would become a vertex of its own), and ``field_to_mesh`` refuses any non-finite norm in the grid.  By default
``vertices`` / ``faces`` are the PLY file's content, before trimesh; ``extract_mesh(..., weld=True)`` merges the vertices the way
trimesh's default (``process=True`` in methods.py:305) is remembered to — ``meshops.weld``, a specification not verified against trimesh.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import geomargs, grid, lib, meshops

N_COMBS = 28
ORIENT_REFERENCES = ("first", "majority", "volume")          # meshops.REFERENCES that need nothing but the mesh
ORIENT = None          # None, or one of ORIENT_REFERENCES: ``contrastive_marching_cubes`` then rewinds its faces (dropin.install(mesh_orient=))


def _check_even(res: int) -> None:
    # evaluation/methods.py:184-188 builds (res/2)^3 blocks of 2x2x2 cells and reshapes their res^3 rows: an odd res raises there
    if res % 2:
        raise ValueError(f"resolution must be even (the reference's 2x2x2 block order has no odd form), got {res}")


def triangulate(comb_values, isovalue: float = 0.0, res: int = 100, size: float = 2.0, udf=None, selected_indices=None, device=None):
    """The GENERAL form: comb [M,28] (+ udf [M,28,2]) with cell indices [M,3], or, ``selected_indices=None``, the dense raster of
    res^3 cells (``udf`` may then be None: corner values 0 / 1).  fp32 inputs stay fp32 on the device (the kernel widens them exactly);
    any other dtype is converted to float64 (exact for the integer / fp16 / bool tables the reference accepts).
    -> (vertices float64 [V,3], faces int64 [F,3], 0-based), on the device."""
    res = geomargs.positive_int(res, "res")
    comb = geomargs.as_tensor(comb_values, "comb_values")
    u = None if udf is None else geomargs.as_tensor(udf, "udf")
    cells = None
    if selected_indices is not None:
        cells = geomargs.as_tensor(selected_indices, "selected_indices")
        if cells.dim() != 2 or cells.shape[1] != 3:
            raise ValueError(f"selected_indices must be [M,3], got {tuple(cells.shape)}")
        if cells.dtype.is_floating_point or cells.dtype == torch.bool:
            raise ValueError(f"selected_indices must be integers, got {cells.dtype}")
        m = cells.shape[0]
        if u is None:
            # (the reference reshapes udf unconditionally in this branch: udf=None raises AttributeError there)
            raise ValueError("selected_indices given without udf: the reference's branch needs udf")
    else:
        m = res ** 3
    if comb.numel() != m * N_COMBS:
        raise ValueError(f"comb_values has {comb.numel()} values, expected {m} cells x {N_COMBS}")
    if u is not None and u.numel() != m * N_COMBS * 2:
        raise ValueError(f"udf has {u.numel()} values, expected {m} cells x {N_COMBS} x 2")
    if m >= geomargs.LIMIT:
        raise ValueError(f"{m} cells exceed the 2^31 limit of one call")
    dev = geomargs.device(device, "mesh triangulation")
    dt = torch.float32 if comb.dtype == torch.float32 and (u is None or u.dtype == torch.float32) else torch.float64
    comb = comb.reshape(m, N_COMBS).to(dev, dt).contiguous()
    if u is not None:
        u = u.reshape(m, N_COMBS, 2).to(dev, dt).contiguous()
    if cells is not None:
        cells = cells.to(dev, torch.int64).contiguous()
    if m == 0:
        return geomargs.empty_mesh(dev)
    return lib.mesh_triangulate(lib.MESH_GENERAL, m, res, float(size), float(isovalue), comb=comb, udf=u, cells=cells, device=dev)


def to_reference(vertices: torch.Tensor, faces: torch.Tensor):
    """(vertices, faces) of ``triangulate`` -> the reference's (vs, fs): {(x, y, z): id} with 1-based ids in order of first appearance
    (tuples of numpy float64, as ``tuple(row)`` of the reference's float64 arrays) and a list of 1-based [a, b, c] faces."""
    v = vertices.cpu().numpy()
    vs = {tuple(row): i + 1 for i, row in enumerate(v)}
    fs = (faces.cpu().numpy() + 1).tolist()
    return vs, fs


def _check_orient(orient):
    if orient is not None and orient not in ORIENT_REFERENCES:
        raise ValueError(f"orient must be None or one of {ORIENT_REFERENCES}, got {orient!r}")
    return orient


def contrastive_marching_cubes(comb_values, isovalue=0.0, res=100, size=2.0, udf=None, selected_indices=None):
    """Drop-in for evaluation/utils/marching_cubes_vt.contrastive_marching_cubes (same arguments, same (vs, fs)).  With the module's
    ``ORIENT`` set (None by default: nothing changes) the faces are rewound by ``meshops.orient`` before they are listed: same vertices,
    same faces in the same order, columns 1 and 2 of some exchanged."""
    vertices, faces = triangulate(comb_values, isovalue=isovalue, res=res, size=size, udf=udf, selected_indices=selected_indices)
    if ORIENT is not None:
        _, faces, _ = meshops.orient((vertices, faces), reference=_check_orient(ORIENT))
    return to_reference(vertices, faces)


def _dev_field(prediction: torch.Tensor, resolution: int) -> torch.Tensor:
    if not isinstance(prediction, torch.Tensor) or not prediction.is_cuda:
        raise lib.VfnError("field_to_mesh runs on the device: pass the device-resident field (no CPU fallback)")
    if prediction.numel() != resolution ** 3 * 3:
        raise ValueError(f"field has {prediction.numel()} values, expected {resolution}^3 x 3")
    if prediction.dtype != torch.float32:
        raise ValueError(f"field must be float32, got {prediction.dtype}")
    return prediction.reshape(resolution ** 3, 3).contiguous()


class FieldStages(NamedTuple):
    divergence: torch.Tensor     # [res,res,res] float32
    norms: torch.Tensor          # [res^3] float32
    sides: torch.Tensor          # [res^3] uint8 (bit q = corner q's side)


def field_stages(prediction: torch.Tensor, resolution: int, smooth_after: bool = False, smooth_all: bool = False) -> FieldStages:
    """evaluation/methods.py:212-255 on the device, up to the side bytes: smoothing (k=3 if smooth_all), divergence, smoothing (k=9 if
    smooth_after or smooth_all), norms + normalised field, side bytes."""
    res = geomargs.positive_int(resolution, "resolution")
    _check_even(res)
    pred = _dev_field(prediction, res)
    if smooth_all:
        pred = grid.smooth_vf(pred.reshape(res, res, res, 3), k=3, sigma=1).reshape(res ** 3, 3)
    divergence = grid.extract_divergence(pred, res)
    if smooth_after or smooth_all:
        pred = grid.smooth_vf(pred.reshape(res, res, res, 3), k=9, sigma=2).reshape(res ** 3, 3)
    norms, unit = lib.mesh_field_norms(pred)
    sides, _ = lib.grid_unify_direction_sides(divergence.reshape(-1), unit, res, want_table=False)
    return FieldStages(divergence, norms, sides)


def field_to_mesh(prediction: torch.Tensor, resolution: int, smooth_after: bool = False, smooth_all: bool = False):
    """Device field [res^3,3] -> (vertices float64 [V,3], faces int64 [F,3], 0-based): evaluation/methods.py:212-290 in the reference's
    order, the triangulation in its FUSED form (side bytes + norms).  Refuses a non-finite norm anywhere in the grid."""
    res = geomargs.positive_int(resolution, "resolution")
    st = field_stages(prediction, res, smooth_after=smooth_after, smooth_all=smooth_all)
    return lib.mesh_triangulate(lib.MESH_FUSED, res ** 3, res, 2.0, 0.0, sides=st.sides, norms=st.norms)


def lattice_axes(resolution: int, scale: float = 1.0, translation=0, centroid=0):
    """The three axis tables of evaluation/methods.py:190-208's lattice, with the same fp32 torch operations in the same order (column c
    of cell (i,j,k) depends on one index only; the reference writes index * voxel_size + origin + translation[c] + centroid[c])."""
    voxel_origin = [-scale, -scale, -scale]
    voxel_size = scale * 2.0 / (resolution - 1)
    t = torch.as_tensor(translation, dtype=torch.float32).expand(3)
    c = torch.as_tensor(centroid, dtype=torch.float32).expand(3)
    idx = torch.arange(0, resolution, 1, out=torch.LongTensor()).to(torch.float32)
    # (the reference's samples[:, 0] uses voxel_origin[2], [:, 2] voxel_origin[0]: all three are -scale)
    a0 = (idx * voxel_size) + voxel_origin[2] + t[0] + c[0]
    a1 = (idx * voxel_size) + voxel_origin[1] + t[1] + c[1]
    a2 = (idx * voxel_size) + voxel_origin[0] + t[2] + c[2]
    return a0, a1, a2


class Mesh(NamedTuple):
    vertices: torch.Tensor          # float64 [V,3], unit frame (the reference's vs keys)
    faces: torch.Tensor             # int64 [F,3], 0-based
    vertices_scaled: torch.Tensor   # float64 [V,3]: float64(float32(v)) * scale + translation + centroid


@torch.no_grad()
def extract_mesh(decoder, resolution: int, scale: float = 1.0, translation=0, centroid=0, smooth_after: bool = False,
                 smooth_all: bool = False, max_batch: int = 100000, device=None, weld: bool = False, orient=None) -> Mesh:
    """evaluation/methods.py:140-322 (``marching_cubes_mesh``) without files: lattice -> queries -> ``field_to_mesh``.  The lattice is
    regenerated on the device from its axis tables (no res^3 host grid), the queries stay device-resident.  ``vertices_scaled`` is
    what the PLY's f4 vertices become after ``apply_scale`` / ``apply_translation(translation)`` / ``apply_translation(centroid)``
    (:314-316).  ``weld=True``: ``vertices``, ``faces`` and ``vertices_scaled`` are those of ``meshops.weld`` (``digits=8``) applied to
    float64(float32(vertices)) before scaling — where the reference's ``trimesh.Trimesh(...)`` merges: after the PLY's f4 rounding and
    before ``apply_scale``.  The default changes nothing.  ``orient`` ("first", "majority" or "volume"; None: the faces as extracted):
    the faces are those of ``meshops.orient(mesh, reference=orient)`` applied to the mesh this call would otherwise return — the cells
    choose their sides locally, so the extracted faces are not consistently wound; the vertices are untouched."""
    if not isinstance(weld, bool):
        raise ValueError(f"weld must be a bool, got {weld!r}")
    _check_orient(orient)
    res = geomargs.positive_int(resolution, "resolution")
    _check_even(res)
    if res < 2:
        raise ValueError("resolution must be >= 2")
    dev = geomargs.device(device, "mesh triangulation")
    axes = tuple(a.to(dev) for a in lattice_axes(res, scale, translation, centroid))
    n = res ** 3
    pred = torch.empty(n, 3, device=dev)
    # the queries are pointwise: max_batch (the reference's activation-memory bound) does not change a value, so the launches go in
    # chunks of grid.DEVICE_CHUNK points
    step = max(int(max_batch), grid.DEVICE_CHUNK)
    for lo in range(0, n, step):
        cnt = min(step, n - lo)
        pts = lib.grid_lattice_points(axes, res, lo, cnt)
        pred[lo:lo + cnt] = decoder(pts, vector_only=True) if grid._accepts_vector_only(decoder) else decoder(pts)[:, :3]
    vertices, faces = field_to_mesh(pred, res, smooth_after=smooth_after, smooth_all=smooth_all)
    t = torch.as_tensor(translation).to(dev, torch.float64).expand(3)
    c = torch.as_tensor(centroid).to(dev, torch.float64).expand(3)
    if weld:
        vertices, faces, _ = meshops.weld((vertices.to(torch.float32).to(torch.float64), faces), digits=meshops.WELD_DIGITS, device=dev)
    scaled = vertices.to(torch.float32).to(torch.float64) * float(scale) + t + c
    if orient is not None:
        _, faces, _ = meshops.orient(Mesh(vertices, faces, scaled), reference=orient, device=dev)
    return Mesh(vertices, faces, scaled)
