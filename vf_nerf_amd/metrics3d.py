"""Scoring a mesh against a mesh on the device (csrc/vfn_metrics.hip): the geometry of evaluation/methods.py:747-801
(``metrics_3d_no_vf``) — ``utils.get_chamfer_distance`` (utils/utils.py:327-367) and precision / recall / F-score at a distance
threshold — without copying either mesh to the host.

* ``nearest_distances`` — every query's distance to its nearest target: all pairs in float64, bit-equal to
  ``scipy.spatial.cKDTree(targets).query(queries)[0]`` (tests/test_metrics3d_host.py, tests/test_hip_metrics3d.py).  No index.
* ``nearest`` — the same distance WITH the index of the target that attains it (ties to the lowest index), by a uniform grid over the
  targets searched ring by ring (csrc/vfn_nn.hip, include/vfn.h: ``vfn_nn_nearest``): exact, unbounded, and bit-equal to the all-pairs
  search whatever the grid — an exact lower bound on every unvisited target's distance ends a query's search; a query it has not
  ended after ``max_rings`` rings is served by all pairs.  ``nearest_grid`` builds the grid of a target set once for several searches.
* ``search="grid"`` on ``nearest_distances``, ``chamfer_from_points``, ``chamfer_distance``, ``precision_recall_fscore`` and
  ``score_mesh`` runs their searches through that kernel instead of all pairs (the default, ``"all_pairs"``): one grid per point set
  and direction, and the same numbers to the bit — only the time differs (DESIGN 6i has the measurements).
* ``sample_surface`` — area-weighted surface samples (face by cumulative area, folded-square barycentric coordinates).
* ``chamfer_from_points`` / ``chamfer_distance`` — the reference's four numbers with the reference's combination.
* ``precision_recall_fscore`` — shares of points within a threshold of the other set.
* ``score_mesh`` — both from one sampling and one search per direction, shaped like an entry of the reference's ``3d-metrics.json``.
* ``normal_consistency`` — the mean |n(p) . n(nearest point of the other surface)| in both directions, the third number beside chamfer
  distance and F-score: a sample's normal is the unit normal of the face it was drawn from (``meshops.face_normals``), the neighbour
  comes with its index from the grid search, the dots from csrc/vfn_normals.hip, the sums along the fixed tree.
  ``score_mesh(..., normals=True)`` adds it to the entry as "normal consistency" from the same samples and searches.

Inputs are numpy arrays or torch tensors on any device; a mesh is a ``mesh.Mesh`` (its ``vertices_scaled`` are used) or a
``(vertices, faces)`` pair.  No CPU fallback: ``lib.VfnError`` when no device is visible.

The mesh that ``metrics_3d`` scores for a VF-NeRF run, ``tsdf_mesh``'s, comes from ``vf_nerf_amd.tsdf`` (``fuse_depth_maps`` /
``fuse_rendered_views``) in the form ``score_mesh`` accepts; the other three meshes it scores (smoothed, refused, both) and its whole
dictionary come from ``vf_nerf_amd.refuse`` (``reconstruction_meshes``, ``metrics_3d``).

``score_mesh(..., icp_align=True)`` first aligns the pred samples to the ref samples with ``vf_nerf_amd.icp.align`` (point-to-point ICP,
a specification of ours: not verified against Open3D or the ``evaluate_3d_reconstruction`` package).

``voxel_down_sample`` is the first step of the ``evaluate_3d_reconstruction`` package's protocol (vf_nerf_amd/voxel.py,
csrc/vfn_voxel.hip): one point per occupied voxel, the mean of the voxel's points.  ``precision_recall_fscore``, ``score_mesh`` and
``refuse.metrics_3d`` take ``voxel_size=`` and then count on the down-sampled clouds, where every occupied voxel votes once;
``icp.align_stages`` is that protocol's staged registration.  All of it is a specification of ours that imitates Open3D's
``voxel_down_sample`` as remembered, not verified against Open3D or the package.

``score_mesh(..., min_component_faces=, keep_largest=)`` first culls the small detached pieces of the pred mesh
(``meshops.filter_components``, csrc/vfn_cc.hip: connected components by shared edges), so that floaters draw no samples.

Out of scope: scale in ICP, and the ``evaluate_3d_reconstruction`` package's cropping, histograms and coloured error clouds.
Trimesh's vertex merging is ``meshops.weld``, PLY reading / writing ``vf_nerf_amd.ply``.
The random numbers are torch's, not
numpy's: a sampled point set is distributed as trimesh's, it is not the same set.
"""
from __future__ import annotations

import functools
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import geomargs, icp, lib, meshops, voxel
from .geomargs import LIMIT

SEARCHES = ("all_pairs", "grid")
MAX_RINGS = 8                      # rings a query of the grid search visits before it is left to all pairs (speed only)
GRID_TARGETS_PER_CELL = 8          # the default grid has about sqrt(m / 8) cells along the longest axis (speed only)

# this unit's forms of the shared checks (module attributes, so a test can stand in for the device)
_device = functools.partial(geomargs.device, what="mesh scoring")
_check_mesh = functools.partial(geomargs.check_mesh, allow_empty=False)          # nothing can be sampled on an empty mesh


def _check_points(x, name: str) -> torch.Tensor:
    """Shape / dtype / size checks on the host tensor, before any device call."""
    t = geomargs.as_tensor(x, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be [n,3], got {tuple(t.shape)}")
    if not (t.dtype.is_floating_point or t.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)):
        raise ValueError(f"{name} must be real numbers, got {t.dtype}")
    if t.shape[0] < 1:
        raise ValueError(f"{name} is empty")
    if t.shape[0] >= LIMIT:
        raise ValueError(f"{name}: {t.shape[0]} rows exceed the 2^31 limit of one call")
    return t


def _check_threshold(threshold) -> float:
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise ValueError(f"threshold must be a real number, got {threshold!r}")
    if not math.isfinite(float(threshold)) or float(threshold) < 0:
        raise ValueError(f"threshold must be finite and >= 0, got {threshold!r}")
    return float(threshold)


def _check_search(search) -> str:
    if search not in SEARCHES:
        raise ValueError(f"search must be one of {SEARCHES}, got {search!r}")
    return search


def _search_kw(search) -> dict:
    """The checked ``search`` as the keyword of ``_both_directions``: none for the default, whose call stays what it was."""
    return {} if _check_search(search) == "all_pairs" else {"search": search}


def _check_max_rings(max_rings) -> int:
    if isinstance(max_rings, bool) or not isinstance(max_rings, (int, np.integer)) or int(max_rings) < 0:
        raise ValueError(f"max_rings must be a non-negative integer, got {max_rings!r}")
    return int(max_rings)


def _check_cells(cells) -> Optional[int]:
    cap = lib.icp_grid_limits()[0]
    if cells is None:
        return None
    if isinstance(cells, bool) or not isinstance(cells, (int, np.integer)) or not 1 <= int(cells) <= cap:
        raise ValueError(f"cells must be None or an integer in [1, {cap}], got {cells!r}")
    return int(cells)


def _dev_points(t: torch.Tensor, dev: torch.device) -> torch.Tensor:
    return t.to(dev, torch.float64).contiguous()


VoxelDownSample = voxel.VoxelDownSample


def voxel_down_sample(points, voxel_size, normals=None, colours=None, device=None) -> VoxelDownSample:
    """points[n,3] -> a ``VoxelDownSample``: ``points`` [V,3], the mean of the points of every occupied voxel of edge ``voxel_size``
    (voxels in ascending (c_0, c_1, c_2), c_k = floor((p_k - origin_k) / voxel_size), origin = the bounding box's lower corner less
    half a voxel); ``normals`` / ``colours`` ([n,3]) averaged with them as plain means, not re-normalised; ``counts`` [V],
    ``voxel_of_point`` [n], and the host values ``origin`` and ``dims``.  A mean is the serial sum in ascending original index over
    the count (include/vfn.h: vfn_voxel_means).  Imitates Open3D's ``voxel_down_sample`` as remembered; not verified against it.
    ``vf_nerf_amd.voxel.down_sample`` has the details and the refusals."""
    return voxel.down_sample(points, voxel_size, normals=normals, colours=colours, device=device)


def _check_voxel(voxel_size) -> Optional[float]:
    return None if voxel_size is None else voxel.check_voxel_size(voxel_size)


def _voxel_pair(pred_points, ref_points, voxel_size: float, device=None):
    """Both point sets on the device, each down-sampled at ``voxel_size`` in its own frame -> (pred, ref, the "voxel" entry)."""
    p, r = _check_points(pred_points, "pred_points"), _check_points(ref_points, "ref_points")
    dev = _device(device)
    p, r = (voxel.down_sample_device(_dev_points(x, dev), voxel_size).points for x in (p, r))
    return p, r, {"size": voxel_size, "pred_points": int(p.shape[0]), "ref_points": int(r.shape[0])}


def _check_components(min_component_faces, keep_largest) -> Optional[dict]:
    """The two culling keywords of ``score_mesh``, checked -> the keywords of ``_cull_components``, or None when both are None."""
    min_faces = meshops._check_count(min_component_faces, "min_component_faces", 0)
    keep_largest = meshops._check_count(keep_largest, "keep_largest", 1)
    return None if min_faces is None and keep_largest is None else {"min_faces": min_faces, "keep_largest": keep_largest}


def _cull_components(vertices: torch.Tensor, faces: torch.Tensor, min_faces, keep_largest, device=None):
    """A checked mesh where it is -> (vertices, faces, the "components" entry): ``meshops.filter_components`` by edge connectivity."""
    v, f = meshops._mesh_on_device((vertices, faces), device, "pred_mesh", "mesh scoring")
    (kept_vertices, kept_faces, kept_index, _), c, keep = meshops._filter(v, f, min_faces, None, keep_largest, "faces", "edge", areas=True)
    if kept_faces.shape[0] < 1:
        raise ValueError(f"pred_mesh: none of its {c.n_components} components is left after the culling (min_component_faces={min_faces!r}, "
                         f"keep_largest={keep_largest!r})")
    removed = c.area[~keep].cpu().tolist()
    entry = {"connectivity": "edge", "found": c.n_components, "kept": c.n_components - len(removed),
             "faces_removed": int(f.shape[0] - kept_faces.shape[0]), "area_removed": math.fsum(removed)}
    return kept_vertices, kept_faces, entry


def grid_edge(extent, m: int, cells: Optional[int] = None) -> float:
    """The cell edge of the unbounded search's grid over m targets whose bounding box has the three ``extent``s (host arithmetic):
    ``cells`` cells along the longest axis — by default min(128, max(1, ceil(sqrt(m / 8)))), about eight targets a cell when they lie
    on a surface — so h = longest / cells (1 + 2^-20); h = 1.0 for a box without extent.  Only speed depends on it."""
    cap, margin = lib.icp_grid_limits()
    if cells is None:
        cells = min(cap, max(1, math.ceil(math.sqrt(m / GRID_TARGETS_PER_CELL))))
    longest = max(extent)
    return longest / cells * margin if longest > 0 else 1.0


def _grid(targets: torch.Tensor, cells: Optional[int]) -> "icp.Grid":
    """Device targets -> their grid for the unbounded search (``icp.build_grid``'s plumbing with ``grid_edge``'s cell edge; no radius)."""
    return icp.build_grid(targets, 0.0, edge=lambda extent: grid_edge(extent, targets.shape[0], cells))


def nearest_grid(targets, cells: Optional[int] = None, device=None) -> "icp.Grid":
    """targets[m,3] -> the ``icp.Grid`` that ``nearest`` builds for them: the targets sorted by the cell of a uniform grid with
    ``cells`` cells along the longest axis of their bounding box (None: ``grid_edge``'s default; at most 128).  Give it to ``nearest``
    in place of the targets to search the same set several times."""
    t = _check_points(targets, "targets")
    cells = _check_cells(cells)
    dev = _device(device)
    with torch.cuda.device(dev):
        return _grid(_dev_points(t, dev), cells)


def _nearest_sq(q: torch.Tensor, t: torch.Tensor, search: str, info: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Device queries and targets -> the squared nearest distances by the chosen search: the same bits either way."""
    if search == "all_pairs":
        return lib.nn_sqdist(q, t, info=info)
    with torch.cuda.device(q.device):
        grid = _grid(t, None)
        return lib.nn_nearest(q, grid.nearest_args(), MAX_RINGS, order=icp.query_order(q, None, grid), info=info)[1]


def nearest(queries, targets, device=None, max_rings: int = MAX_RINGS, cells: Optional[int] = None):
    """queries[n,3], targets[m,3] (or a ``nearest_grid`` of them) -> (index int64 [n], distance float64 [n]) on the device: for every
    query the index of its nearest target over ALL targets and the distance to it — ``nearest_distances`` to the bit; among targets at
    the same squared distance the lowest index.  ``max_rings`` (>= 0) and ``cells`` change the time, never a bit: a query whose search
    the ring bound has not ended after ring ``max_rings`` goes to an all-pairs pass.  A NaN / inf coordinate raises ``lib.VfnError``."""
    q = _check_points(queries, "queries")
    max_rings, cells = _check_max_rings(max_rings), _check_cells(cells)
    grid = targets if isinstance(targets, icp.Grid) else None
    if grid is not None and cells is not None:
        raise ValueError("cells is the grid's own: give it to nearest_grid")
    t = None if grid is not None else _check_points(targets, "targets")
    dev = grid.targets.device if grid is not None else _device(device)
    with torch.cuda.device(dev):
        q = _dev_points(q, dev)
        if grid is None:
            grid = _grid(_dev_points(t, dev), cells)
        index, sqdist, _ = lib.nn_nearest(q, grid.nearest_args(), max_rings, order=icp.query_order(q, None, grid))
    return index, torch.sqrt(sqdist)


def nearest_distances(queries, targets, device=None, search: str = "all_pairs") -> torch.Tensor:
    """queries[n,3], targets[m,3] -> float64 [n] on the device: the distance of every query to its nearest target (sqrt of the kernel's
    exact minimum of squared distances).  ``search``: "all_pairs" or "grid" (``nearest``'s kernel; the same bits).  A NaN / inf
    coordinate raises ``lib.VfnError``."""
    q, t = _check_points(queries, "queries"), _check_points(targets, "targets")
    search = _check_search(search)
    dev = _device(device)
    return torch.sqrt(_nearest_sq(_dev_points(q, dev), _dev_points(t, dev), search))


def face_areas(vertices, faces, device=None) -> torch.Tensor:
    """-> areas[F] float64 on the device (csrc: vfn_tri_areas)."""
    v, f = _check_mesh((vertices, faces), "mesh")
    dev = _device(device)
    return lib.tri_areas(_dev_points(v, dev), f.to(dev, torch.int64).contiguous())


def sample_surface(vertices, faces, count: int, generator: Optional[torch.Generator] = None, uniforms=None, device=None):
    """``count`` area-weighted points on the surface -> (points[count,3] float64, face_index[count] int64), device tensors.  A face is
    chosen by its share of the cumulative area (a zero-area face never), the point by the folded-square barycentric rule.  ``uniforms``
    ([count,3] in [0,1)) replaces the device's own random numbers; otherwise they come from ``generator`` (a device generator, or the
    device's default one).  ValueError on no faces, on zero total area and on count < 1."""
    v, f = _check_mesh((vertices, faces), "mesh")
    count = geomargs.positive_int(count, "count")
    u = None
    if uniforms is not None:
        u = geomargs.as_tensor(uniforms, "uniforms")
        if tuple(u.shape) != (count, 3) or not u.dtype.is_floating_point:
            raise ValueError(f"uniforms must be floating point [{count},3], got {u.dtype} {tuple(u.shape)}")
    dev = _device(device)
    v, f = _dev_points(v, dev), f.to(dev, torch.int64).contiguous()
    cum = cumulative_areas(v, f)
    if u is None:
        u = torch.rand(count, 3, dtype=torch.float64, device=dev, generator=generator)
    u = _dev_points(u, dev)
    points, face_index, info = lib.sample_surface(v, f, cum, u)
    return points, face_index


def cumulative_areas(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """Device vertices / faces -> the inclusive cumulative-area table [F]: vfn_tri_areas, the fixed-tree scan vfn_cumsum_f64, then a
    running maximum over the prefixes of the faces WITH area.  A tree scan rounds neighbouring prefixes along different paths, so
    the raw prefixes may step down by an ulp, or up across a zero-area face; the running maximum (exact, so any evaluation order
    gives the same bits) makes the table non-decreasing and level across every zero-area face — such a face can never be selected —
    and keeps each entry within the scan's error bound (the maximum is a prefix of an earlier face, whose exact sum is no larger,
    and at least the prefix of the last face with area, whose exact sum is the same).  One value crosses to the host: the total, to
    refuse a surface without area."""
    areas = lib.tri_areas(vertices, faces)
    cum = lib.cumsum_f64(areas)
    cum = torch.cummax(torch.where(areas > 0, cum, torch.zeros_like(cum)), dim=0).values
    total = float(cum[-1].cpu())
    if not total > 0.0:
        raise ValueError("the mesh has zero total area: nothing to sample")
    if not math.isfinite(total):
        raise lib.VfnError("the mesh's total area is not finite")
    return cum


def _median_pair(sq: torch.Tensor) -> torch.Tensor:
    """The two middle values of sq (equal for an odd count) as a device tensor [2]: np.median is their mean."""
    n = sq.shape[0]
    s = torch.sort(sq).values
    return torch.stack((s[(n - 1) // 2], s[n // 2]))


def _direction(dist: torch.Tensor, threshold: float) -> torch.Tensor:
    """Nearest distances of one direction -> device [7]: sum, min, max of the SQUARED distances (the reference squares the KD-tree's
    distances, utils.py:353-356), the two middle squares, n, number of distances < threshold."""
    sq = dist * dist
    s = lib.reduce_stats(sq, math.inf)
    c = lib.reduce_stats(dist, threshold)
    n = torch.tensor([float(dist.shape[0])], dtype=torch.float64, device=dist.device)
    return torch.cat((s[:3], _median_pair(sq), n, c[3:4]))


def _chamfer(one, two):
    """Two host rows of ``_direction`` (ref -> pred, pred -> ref) -> (mean, median, min, max), utils.py:366-367."""
    mean = one[0] / one[5] + two[0] / two[5]
    median = (one[3] + one[4]) / 2.0 + (two[3] + two[4]) / 2.0
    return float(mean), float(median), float(min(one[1], two[1])), float(max(one[2], two[2]))


def _prf(pred_row, ref_row) -> dict:
    n_p, n_r = int(pred_row[6]), int(ref_row[6])
    p, r = n_p / int(pred_row[5]), n_r / int(ref_row[5])
    return {"precision": p, "recall": r, "fscore": 2 * p * r / (p + r) if p + r > 0 else 0.0, "pred_within": n_p, "ref_within": n_r}


def _both_directions(pred_points, ref_points, threshold: float, device=None, search: str = "all_pairs"):
    """-> host float64 [2,7]: row 0 = the ref points against the pred set, row 1 = the pred points against the ref set.  One read
    of the results (the grid search adds its own: a box per grid, a count per search)."""
    p, r = _check_points(pred_points, "pred_points"), _check_points(ref_points, "ref_points")
    dev = _device(device)
    p, r = _dev_points(p, dev), _dev_points(r, dev)
    info = torch.zeros(1, dtype=torch.int64, device=dev)
    one = _direction(torch.sqrt(_nearest_sq(r, p, search, info=info)), threshold)
    two = _direction(torch.sqrt(_nearest_sq(p, r, search, info=info)), threshold)
    host = torch.cat((one, two, info.to(torch.float64))).cpu().numpy()
    lib.nn_check(int(host[14]))
    return host[:14].reshape(2, 7)


def _normal_direction(q: torch.Tensor, qn: torch.Tensor, t: torch.Tensor, tn: torch.Tensor, threshold: float, info: torch.Tensor,
                      ninfo: torch.Tensor) -> torch.Tensor:
    """One direction WITH normals -> device [8]: ``_direction``'s seven numbers from the grid search's distances (the all-pairs kernel's
    to the bit), then the sum of |qn . tn[nearest]| along the fixed tree."""
    with torch.cuda.device(q.device):
        grid = _grid(t, None)
        index, sq, _ = lib.nn_nearest(q, grid.nearest_args(), MAX_RINGS, order=icp.query_order(q, None, grid), info=info)
    dots = lib.normal_dots(qn, tn, index, info=ninfo)
    return torch.cat((_direction(torch.sqrt(sq), threshold), lib.reduce_stats(dots, math.inf)[:1]))


def _both_directions_normals(p: torch.Tensor, pn: torch.Tensor, r: torch.Tensor, rn: torch.Tensor, threshold: float):
    """Device points and unit normals of both sample sets -> (host [2,7] as ``_both_directions``, the "normal consistency" entry).  Both
    searches go through the grid kernel: the all-pairs kernel has no index.  One read of the results, the two sums of dots with it."""
    dev = p.device
    info = torch.zeros(1, dtype=torch.int64, device=dev)
    ninfo = torch.zeros(1, dtype=torch.int64, device=dev)
    one = _normal_direction(r, rn, p, pn, threshold, info, ninfo)
    two = _normal_direction(p, pn, r, rn, threshold, info, ninfo)
    host = torch.cat((one, two, info.to(torch.float64), ninfo.to(torch.float64))).cpu().numpy()
    lib.nn_check(int(host[16]))
    lib.normals_check(int(host[17]), "normal consistency")
    a, b = float(host[15] / p.shape[0]), float(host[7] / r.shape[0])
    return np.stack((host[0:7], host[8:15])), {"pred_to_ref": a, "ref_to_pred": b, "mean": (a + b) / 2.0}


def _sample_normals(vertices, faces, face_index: torch.Tensor) -> torch.Tensor:
    """The unit normal of the face every sample was drawn from (a torch gather), on the samples' device."""
    return meshops.face_normals((vertices, faces), normalise=True, device=face_index.device)[face_index].contiguous()


def _rotate(normals: torch.Tensor, transformation: np.ndarray) -> torch.Tensor:
    """Normals under the 3 x 3 block of a [4,4] rigid transformation: ``icp.transform_points``'s kernel with the translation zero."""
    rotation = np.array(transformation, dtype=np.float64, copy=True)
    rotation[:3, 3] = 0.0
    return icp.transform_points(normals, rotation, device=normals.device)


def normal_consistency(pred_mesh, ref_mesh, num_points: int = 1000000, generator: Optional[torch.Generator] = None, uniforms=None,
                       device=None) -> dict:
    """{"pred_to_ref", "ref_to_pred", "mean"}: ``num_points`` samples of each surface (pred first, then ref, from the same generator, or
    the same ``uniforms`` for both), every sample with the unit normal of its face; per direction the mean of |n(p) . n(q)| over the
    samples p of one surface with q the nearest sample of the other (ties to the lowest index), and the mean of the two means.  The
    absolute value because neither mesh's winding is trusted.  Sums along the fixed tree (``lib.reduce_stats``), divided on the host."""
    pv, pf = _check_mesh(pred_mesh, "pred_mesh")
    rv, rf = _check_mesh(ref_mesh, "ref_mesh")
    num_points = geomargs.positive_int(num_points, "num_points")
    pred_points, pred_face = sample_surface(pv, pf, num_points, generator=generator, uniforms=uniforms, device=device)
    ref_points, ref_face = sample_surface(rv, rf, num_points, generator=generator, uniforms=uniforms, device=device)
    return _both_directions_normals(pred_points, _sample_normals(pv, pf, pred_face), ref_points, _sample_normals(rv, rf, ref_face), 0.0)[1]


def chamfer_from_points(pred_points, ref_points, device=None, search: str = "all_pairs") -> Tuple[float, float, float, float]:
    """utils.py:350-367 on two point sets -> (mean, median, min, max) as Python floats: per direction the mean / median / min / max of
    the squared nearest distances, then the sum of the means, the sum of the medians, the min of the mins, the max of the maxes.  The
    median is np.median's (the mean of the two middle values for an even count).  ``search`` as in ``nearest_distances``."""
    rows = _both_directions(pred_points, ref_points, 0.0, device, **_search_kw(search))
    return _chamfer(rows[0], rows[1])


def chamfer_distance(pred_mesh, ref_mesh, num_points: int = 2500000, generator: Optional[torch.Generator] = None, device=None,
                     search: str = "all_pairs"):
    """``utils.get_chamfer_distance``: ``num_points`` samples of each surface (pred first, then ref, from the same generator), then
    ``chamfer_from_points`` (``search`` goes there)."""
    search = _check_search(search)
    pv, pf = _check_mesh(pred_mesh, "pred_mesh")
    rv, rf = _check_mesh(ref_mesh, "ref_mesh")
    num_points = geomargs.positive_int(num_points, "num_points")
    pred_points, _ = sample_surface(pv, pf, num_points, generator=generator, device=device)
    ref_points, _ = sample_surface(rv, rf, num_points, generator=generator, device=device)
    return chamfer_from_points(pred_points, ref_points, device=device, search=search)


def precision_recall_fscore(pred_points, ref_points, threshold: float, device=None, search: str = "all_pairs", voxel_size=None) -> dict:
    """precision = the share of pred points whose nearest ref point is closer than ``threshold`` (distance < threshold), recall = the
    share of ref points whose nearest pred point is closer than ``threshold``, fscore = 2 P R / (P + R), 0 when P + R = 0.  The counts
    are returned too (``pred_within``, ``ref_within``).  ``search`` as in ``nearest_distances``.

    With ``voxel_size=None`` this is the plain definition on the two point sets as given: a share of POINTS, so a region with many
    points weighs more.  With a value both sets are first replaced by their ``voxel_down_sample`` at that edge, each in its own frame,
    so that every occupied voxel votes once, as the external ``evaluate_3d_reconstruction`` package the reference calls does before it
    counts; the result gains "voxel": {"size", "pred_points", "ref_points"}.  That package's choice of the edge is ``threshold / 2``
    — as remembered, not verified.  Neither form is claimed equal to that package's numbers: the down-sampling imitates Open3D's as
    remembered, and the package's cropping is not done here."""
    threshold = _check_threshold(threshold)
    search_kw = _search_kw(search)
    voxel_size = _check_voxel(voxel_size)
    if voxel_size is None:
        rows = _both_directions(pred_points, ref_points, threshold, device, **search_kw)
        return _prf(rows[1], rows[0])
    p, r, entry = _voxel_pair(pred_points, ref_points, voxel_size, device)
    rows = _both_directions(p, r, threshold, p.device, **search_kw)
    out = _prf(rows[1], rows[0])
    out["voxel"] = entry
    return out


def score_mesh(pred_mesh, ref_mesh, num_points: int = 1000000, distance_thresh: float = 0.05, generator: Optional[torch.Generator] = None,
               uniforms=None, device=None, icp_align: bool = False, icp_threshold: Optional[float] = None, search: str = "all_pairs",
               normals: bool = False, voxel_size=None, min_component_faces=None, keep_largest=None) -> dict:
    """One entry of the reference's ``3d-metrics.json`` (methods.py:794-801): {"chamfer distance": {mean, median, min, max}, "precision",
    "recall", "fscore"} (plus the two counts), from ONE sampling of each mesh and ONE nearest-neighbour search per direction shared
    by both metrics.  ``uniforms`` ([num_points,3]) is used for BOTH meshes when given.

    ``icp_align=True``: the pred samples are aligned to the ref samples with ``icp.align`` (correspondences within ``icp_threshold``;
    None = ``distance_thresh`` — that default is ours, not the external package's), moved by the result and scored as above; the
    entry gains "icp": {"transformation" (nested lists), "fitness", "inlier_rmse", "iterations"}.  With ``icp_align=False`` nothing
    changes: the same keys, values and draws from the generator as without the keyword.

    ``search="grid"``: the two scoring searches go through the grid kernel (``nearest``); the dictionary is the same to the bit.

    ``normals=True``: the entry gains "normal consistency": {"pred_to_ref", "ref_to_pred", "mean"} (``normal_consistency``, from the same
    samples; with ``icp_align`` the pred normals are rotated by the result's 3 x 3 block).  The two scoring searches then go through the
    grid kernel whatever ``search`` says — the all-pairs kernel has no index — and every other key is what it is without ``normals``,
    bit for bit.  With ``normals=False`` nothing changes.

    ``voxel_size``: both sample sets are replaced by their ``voxel_down_sample`` at that edge — after the sampling, and after the ICP
    move when ``icp_align=True`` (the alignment itself runs on the samples as drawn, so the "icp" entry does not depend on the keyword)
    — and chamfer distance, precision, recall and F-score are taken on the results, through ``search`` as given; the entry gains
    "voxel": {"size", "pred_points", "ref_points"}.  Every occupied voxel then votes once, as in the external
    ``evaluate_3d_reconstruction`` package, whose edge is ``distance_thresh / 2`` — as remembered, not verified.  Together with
    ``normals=True`` it raises ``ValueError``: a voxel's normal for normal consistency is not defined here.  With ``voxel_size=None``
    nothing changes: the same keys, bits and draws from the generator as without the keyword.

    ``min_component_faces`` / ``keep_largest``: ``pred_mesh`` alone is first replaced by its ``meshops.filter_components`` (edge
    connectivity; ``min_faces=min_component_faces``, ``keep_largest`` ranked by faces) — before the sampling, so that detached pieces of
    a fused mesh ("floaters") draw no samples — and the entry gains "components": {"connectivity", "found", "kept", "faces_removed",
    "area_removed"} (``area_removed``: the correctly rounded sum of the removed components' areas).  ``ValueError`` if nothing is left.
    With both None nothing changes: the same keys, bits and draws from the generator as without the keywords."""
    search = _check_search(search)
    if not isinstance(normals, (bool, np.bool_)):
        raise ValueError(f"normals must be a bool, got {normals!r}")
    voxel_size = _check_voxel(voxel_size)
    if voxel_size is not None and normals:
        raise ValueError("voxel_size together with normals=True: a voxel's normal for normal consistency is not defined here (the mean of "
                         "unit normals is no unit normal, and no face belongs to a voxel)")
    components_kw = _check_components(min_component_faces, keep_largest)
    pv, pf = _check_mesh(pred_mesh, "pred_mesh")
    rv, rf = _check_mesh(ref_mesh, "ref_mesh")
    num_points = geomargs.positive_int(num_points, "num_points")
    threshold = _check_threshold(distance_thresh)
    if not isinstance(icp_align, (bool, np.bool_)):
        raise ValueError(f"icp_align must be a bool, got {icp_align!r}")
    if icp_align:
        icp_radius = icp._check_radius(threshold if icp_threshold is None else icp_threshold, "icp_threshold")
    if components_kw is not None:
        pv, pf, components_entry = _cull_components(pv, pf, device=device, **components_kw)
    pred_points, pred_face = sample_surface(pv, pf, num_points, generator=generator, uniforms=uniforms, device=device)
    ref_points, ref_face = sample_surface(rv, rf, num_points, generator=generator, uniforms=uniforms, device=device)
    if normals:
        pred_normals, ref_normals = _sample_normals(pv, pf, pred_face), _sample_normals(rv, rf, ref_face)
    aligned = None
    if icp_align:
        aligned = icp.align(pred_points, ref_points, icp_radius, device=pred_points.device)
        pred_points = icp.transform_points(pred_points, aligned.transformation, device=pred_points.device)
        if normals:
            pred_normals = _rotate(pred_normals, aligned.transformation)
    if normals:
        rows, consistency = _both_directions_normals(pred_points, pred_normals, ref_points, ref_normals, threshold)
    elif voxel_size is not None:
        pred_points, ref_points, voxel_entry = _voxel_pair(pred_points, ref_points, voxel_size, pred_points.device)
        rows = _both_directions(pred_points, ref_points, threshold, pred_points.device, **_search_kw(search))
    else:
        rows = _both_directions(pred_points, ref_points, threshold, device, **_search_kw(search))
    mean, median, mn, mx = _chamfer(rows[0], rows[1])
    out = {"chamfer distance": {"mean": mean, "median": median, "min": mn, "max": mx}}
    out.update(_prf(rows[1], rows[0]))
    if normals:
        out["normal consistency"] = consistency
    if voxel_size is not None:
        out["voxel"] = voxel_entry
    if components_kw is not None:
        out["components"] = components_entry
    if aligned is not None:
        out["icp"] = {"transformation": aligned.transformation.tolist(), "fitness": aligned.fitness, "inlier_rmse": aligned.inlier_rmse,
                      "iterations": aligned.iterations}
    return out
