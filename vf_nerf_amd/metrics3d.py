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

* ``closest_point`` — every point's nearest point ON a mesh, its distance and the face it lies on (csrc/vfn_proximity.hip, include/vfn.h:
  ``vfn_closest_on_triangle``, ``vfn_tri_nearest``): exact point-to-triangle, on a uniform grid of the faces with ``nearest``'s ring bound,
  bit-equal to testing every face.  ``triangle_grid`` builds the grid once; ``surface_distances`` returns the distances alone;
  ``surface_deviation`` the one-sided mean / rms / max / median from one surface to another — what a mesh operation moved.
* ``surface="mesh"`` on ``chamfer_distance``, ``score_mesh`` and ``normal_consistency`` (and ``refuse.metrics_3d``) measures the samples of
  each surface against the other MESH instead of against its samples: no sampling floor under the score, and the neighbour's normal is
  its face's.  The default ``"samples"`` leaves every call, key and bit as it was.  A specification of ours that follows trimesh's and
  Open3D's closest-point queries as remembered, verified against neither.

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

Out of scope: scale in ICP, and the ``evaluate_3d_reconstruction`` package's cropping, histograms and coloured error clouds; of the
closest point: its barycentric coordinates and attribute interpolation, signed distance and inside / outside, ray queries.
Trimesh's vertex merging is ``meshops.weld``, PLY reading / writing ``vf_nerf_amd.ply``.
The random numbers are torch's, not
numpy's: a sampled point set is distributed as trimesh's, it is not the same set.
"""
from __future__ import annotations

import dataclasses
import functools
import math
from typing import NamedTuple, Optional, Tuple

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
                       device=None, surface: str = "samples") -> dict:
    """{"pred_to_ref", "ref_to_pred", "mean"}: ``num_points`` samples of each surface (pred first, then ref, from the same generator, or
    the same ``uniforms`` for both), every sample with the unit normal of its face; per direction the mean of |n(p) . n(q)| over the
    samples p of one surface with q the nearest sample of the other (ties to the lowest index), and the mean of the two means.  The
    absolute value because neither mesh's winding is trusted.  Sums along the fixed tree (``lib.reduce_stats``), divided on the host.
    ``surface="mesh"``: q is the nearest point of the other MESH and n(q) the unit normal of the face it lies on (``closest_point``)."""
    surface = _check_surface(surface)
    pv, pf = _check_mesh(pred_mesh, "pred_mesh")
    rv, rf = _check_mesh(ref_mesh, "ref_mesh")
    num_points = geomargs.positive_int(num_points, "num_points")
    pred_points, pred_face = sample_surface(pv, pf, num_points, generator=generator, uniforms=uniforms, device=device)
    ref_points, ref_face = sample_surface(rv, rf, num_points, generator=generator, uniforms=uniforms, device=device)
    if surface == "mesh":
        return _both_directions_mesh(pred_points, ref_points, (pv, pf), (rv, rf), 0.0, _sample_normals(pv, pf, pred_face),
                                     _sample_normals(rv, rf, ref_face))[1]
    return _both_directions_normals(pred_points, _sample_normals(pv, pf, pred_face), ref_points, _sample_normals(rv, rf, ref_face), 0.0)[1]


def chamfer_from_points(pred_points, ref_points, device=None, search: str = "all_pairs") -> Tuple[float, float, float, float]:
    """utils.py:350-367 on two point sets -> (mean, median, min, max) as Python floats: per direction the mean / median / min / max of
    the squared nearest distances, then the sum of the means, the sum of the medians, the min of the mins, the max of the maxes.  The
    median is np.median's (the mean of the two middle values for an even count).  ``search`` as in ``nearest_distances``."""
    rows = _both_directions(pred_points, ref_points, 0.0, device, **_search_kw(search))
    return _chamfer(rows[0], rows[1])


def chamfer_distance(pred_mesh, ref_mesh, num_points: int = 2500000, generator: Optional[torch.Generator] = None, device=None,
                     search: str = "all_pairs", surface: str = "samples"):
    """``utils.get_chamfer_distance``: ``num_points`` samples of each surface (pred first, then ref, from the same generator), then
    ``chamfer_from_points`` (``search`` goes there).  ``surface="mesh"``: the same samples, each set measured against the other MESH
    (``closest_point``) instead of the other set, combined in the same way; ``search`` is then not used."""
    search = _check_search(search)
    surface = _check_surface(surface)
    pv, pf = _check_mesh(pred_mesh, "pred_mesh")
    rv, rf = _check_mesh(ref_mesh, "ref_mesh")
    num_points = geomargs.positive_int(num_points, "num_points")
    pred_points, _ = sample_surface(pv, pf, num_points, generator=generator, device=device)
    ref_points, _ = sample_surface(rv, rf, num_points, generator=generator, device=device)
    if surface == "mesh":
        rows, _ = _both_directions_mesh(pred_points, ref_points, (pv, pf), (rv, rf), 0.0)
        return _chamfer(rows[0], rows[1])
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
               normals: bool = False, voxel_size=None, min_component_faces=None, keep_largest=None, surface: str = "samples") -> dict:
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
    With both None nothing changes: the same keys, bits and draws from the generator as without the keywords.

    ``surface="mesh"``: the samples of each surface are measured against the other MESH (``closest_point``), not against its samples:
    the pred samples against the ref mesh (chamfer's pred -> ref half, precision), the ref samples against the pred mesh — the one
    after the culling — (the ref -> pred half, recall).  A surface scored against itself then scores 0 up to rounding, whatever
    ``num_points``.  Sampling, ICP, ``voxel_size`` and the culling act as above on the sample sets and the pred mesh.  With
    ``icp_align`` the moved pred samples are measured against the ref mesh, and the ref samples are moved by the INVERSE of the
    result ([R^T | -R^T t]) before they are measured against the pred mesh, which stays where it is; with ``normals=True`` the
    neighbour's normal is the unit normal of the face found (``meshops.face_normals`` at ``face[i]``), and the ref normals are rotated
    by R^T with their samples.  ``search`` is not used: the grid search serves both directions.  The entry gains "surface": "mesh".
    With ``surface="samples"`` (the default) nothing changes."""
    search = _check_search(search)
    surface = _check_surface(surface)
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
    if surface == "mesh":
        ref_there = ref_points            # the ref samples in the pred mesh's frame
        if aligned is not None:
            inverse = _rigid_inverse(aligned.transformation)
            ref_there = icp.transform_points(ref_points, inverse, device=ref_points.device)
        if voxel_size is not None:
            pred_points, ref_there, voxel_entry = _voxel_pair(pred_points, ref_there, voxel_size, pred_points.device)
        ref_there_normals = None
        if normals:
            ref_there_normals = ref_normals if aligned is None else _rotate(ref_normals, inverse)
        rows, consistency = _both_directions_mesh(pred_points, ref_there, (pv, pf), (rv, rf), threshold,
                                                  pred_normals if normals else None, ref_there_normals)
    elif normals:
        rows, consistency = _both_directions_normals(pred_points, pred_normals, ref_points, ref_normals, threshold)
    elif voxel_size is not None:
        pred_points, ref_points, voxel_entry = _voxel_pair(pred_points, ref_points, voxel_size, pred_points.device)
        rows = _both_directions(pred_points, ref_points, threshold, pred_points.device, **_search_kw(search))
    else:
        rows = _both_directions(pred_points, ref_points, threshold, device, **_search_kw(search))
    mean, median, mn, mx = _chamfer(rows[0], rows[1])
    out = {"chamfer distance": {"mean": mean, "median": median, "min": mn, "max": mx}}
    out.update(_prf(rows[1], rows[0]))
    if surface == "mesh":
        out["surface"] = "mesh"
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


# ---------------------------------------------------------------------------------------------------------------------------------
# the closest point ON a mesh (csrc/vfn_proximity.hip; include/vfn.h: vfn_tri_nearest)
# ---------------------------------------------------------------------------------------------------------------------------------
SURFACES = ("samples", "mesh")
BIG_FACE_CELLS = 64                # a face whose box touches more cells is tested by every query instead of registered (speed only)


class ClosestPoint(NamedTuple):
    """``closest_point``'s result, device tensors: the point of the surface nearest to every query, its squared distance (the kernel's
    number), the distance (its square root, rounded once) and the face the point lies on (the lowest index among equals)."""
    points: torch.Tensor               # [n,3] float64
    sqdist: torch.Tensor               # [n] float64
    distance: torch.Tensor             # [n] float64
    face: torch.Tensor                 # [n] int64


@dataclasses.dataclass
class TriangleGrid:
    """The faces of a mesh registered in the cells of a uniform grid (include/vfn.h: vfn_tri_cell_ranges, vfn_tri_cell_pairs)."""
    n_vertices: int
    tri: torch.Tensor                  # [F,9] float64: every face's three vertices
    ncells: torch.Tensor               # [F] int32: the cells its box touches (0: a face with a bad index, never evaluated)
    pair_face: torch.Tensor            # [n_pairs] int32: the faces of the (cell, face) pairs in ascending cell key
    cell_start: torch.Tensor           # [cells + 1] int32
    large: torch.Tensor                # [n_large] int64: the faces with ncells > big_face_cells, ascending
    box: Tuple[float, ...]             # min[3], max[3] over the vertices that some face names, cell edge
    dims: Tuple[int, int, int]
    big_face_cells: int

    @property
    def n_faces(self) -> int:
        return int(self.tri.shape[0])

    @property
    def n_pairs(self) -> int:
        return int(self.pair_face.shape[0])

    @property
    def n_large(self) -> int:
        return int(self.large.shape[0])

    def args(self):
        return self.tri, self.ncells, self.pair_face, self.cell_start, self.large, self.box, self.dims


def _check_surface(surface) -> str:
    if surface not in SURFACES:
        raise ValueError(f"surface must be one of {SURFACES}, got {surface!r}")
    return surface


def _check_big_face_cells(big_face_cells) -> int:
    if big_face_cells is None:
        return BIG_FACE_CELLS
    if isinstance(big_face_cells, bool) or not isinstance(big_face_cells, (int, np.integer)) or int(big_face_cells) < 0:
        raise ValueError(f"big_face_cells must be None or a non-negative integer, got {big_face_cells!r}")
    return int(big_face_cells)


def _check_pair_count(n_pairs: int, dims, big_face_cells: int) -> int:
    if n_pairs >= LIMIT:
        raise ValueError(f"the faces touch {n_pairs} cells of the {dims[0]} x {dims[1]} x {dims[2]} grid, beyond the 2^31 limit of one pair "
                         f"list: lower `cells` (fewer cells a face) or `big_face_cells` = {big_face_cells} (more faces on the large list)")
    return n_pairs


def _triangle_grid(v: torch.Tensor, f: torch.Tensor, cells: Optional[int], big_face_cells: int, pairs: bool = True,
                   info: Optional[torch.Tensor] = None) -> TriangleGrid:
    """Device vertices [V,3] float64 and faces [F,3] int64 -> their ``TriangleGrid``.  The kernels compute the faces' cell ranges and write
    the pairs; the plumbing between them is torch's, as for points (``icp.build_grid``): the box over the named vertices (six values
    cross to the host), the exclusive prefix sums, a stable sort by cell key, the table of first positions.  One more host read: the
    number of pairs with the status word.  ``pairs=False`` leaves the pair list empty and every face off the large list (what the
    all-pairs search needs: ``tri`` and ``ncells``).  With the caller's zero-filled ``info`` the status bits stay there; without it a
    set bit raises."""
    dev, nv, nf = v.device, v.shape[0], f.shape[0]
    named = f[((f >= 0) & (f < nv)).all(dim=1)].reshape(-1)
    if named.shape[0] == 0:
        lib.proximity_check(lib.GEOM_STATUS_INDEX, nv)
    named = v[named]
    box = torch.cat((named.min(dim=0).values, named.max(dim=0).values)).cpu().tolist()
    if not all(math.isfinite(b) for b in box):
        lib.proximity_check(lib.GEOM_STATUS_NONFINITE, nv)
    extent = [box[3 + k] - box[k] for k in range(3)]
    if not all(math.isfinite(e) for e in extent):
        raise lib.VfnError("closest point: the mesh's bounding box overflows float64")
    cap = lib.icp_grid_limits()[0]
    h = grid_edge(extent, nf, cells)
    dims = tuple(min(cap, int(math.floor(e / h)) + 1) for e in extent)
    box = tuple(box) + (h,)
    own = info is None
    if own:
        info = torch.zeros(1, dtype=torch.int64, device=dev)
    tri, cell_lo, cell_hi, ncells = lib.tri_cell_ranges(v, f, box, dims, info)
    n_cells = dims[0] * dims[1] * dims[2]
    pair_face = torch.empty(0, dtype=torch.int32, device=dev)
    cell_start = torch.zeros(n_cells + 1, dtype=torch.int32, device=dev)
    large = torch.empty(0, dtype=torch.int64, device=dev)
    if pairs:
        count = ncells.to(torch.int64)
        is_large = count > big_face_cells
        small = torch.where(is_large, torch.zeros_like(count), count)
        inclusive = torch.cumsum(small, dim=0)
        n_pairs, status = (int(x) for x in torch.stack((inclusive[-1], info[0])).cpu())
        if own:
            lib.proximity_check(status, nv)
        _check_pair_count(n_pairs, dims, big_face_cells)
        large = torch.nonzero(is_large).reshape(-1).contiguous()
        if n_pairs:
            key, face = lib.tri_cell_pairs(cell_lo, cell_hi, ncells, (inclusive - small).contiguous(), big_face_cells, dims, n_pairs, info)
            sorted_key, perm = torch.sort(key, stable=True)
            pair_face = face[perm].contiguous()
            cell_start = torch.searchsorted(sorted_key, torch.arange(n_cells + 1, dtype=torch.int32, device=dev)).to(torch.int32).contiguous()
    elif own:
        lib.proximity_check(int(info.cpu()), nv)
    return TriangleGrid(nv, tri, ncells, pair_face, cell_start, large, box, dims, big_face_cells)


def triangle_grid(mesh, cells: Optional[int] = None, big_face_cells: Optional[int] = None, device=None) -> TriangleGrid:
    """mesh -> the ``TriangleGrid`` that ``closest_point`` builds for it, to search the same mesh several times: every face registered in
    each cell its bounding box touches, on a uniform grid with ``cells`` cells along the longest axis of the box of the vertices the
    faces name (None: ``grid_edge``'s default for the number of faces; at most 128).  A face that touches more than ``big_face_cells``
    cells (None: 64) is kept on a list of its own that every query tests.  ``n_pairs``, ``n_large`` and ``dims`` tell how it came out;
    both keywords change the time only.  ``ValueError`` (it names ``cells``) when the pair list would reach 2^31 entries: the count comes
    from the range kernel, so that launch and the [F,9] table (72 bytes a face) precede the refusal; the pair kernel, the sort and every
    search come after it."""
    v, f = _check_mesh(mesh, "mesh")
    cells, big_face_cells = _check_cells(cells), _check_big_face_cells(big_face_cells)
    dev = _device(device)
    with torch.cuda.device(dev):
        return _triangle_grid(_dev_points(v, dev), f.to(dev, torch.int64).contiguous(), cells, big_face_cells)


def _closest(q: torch.Tensor, grid: TriangleGrid, max_rings: Optional[int], info: Optional[torch.Tensor] = None):
    """Device queries and a grid -> ``lib.tri_nearest``'s (face, closest, sqdist, leftover_count); ``max_rings`` None = all pairs."""
    with torch.cuda.device(q.device):
        order = None if max_rings is None else torch.argsort(icp._cells(q, grid.box, grid.dims, q.device)).contiguous()
        return lib.tri_nearest(q, grid.args(), max_rings, grid.n_vertices, order=order, info=info)


def closest_point(mesh, points, search: str = "grid", max_rings: int = MAX_RINGS, cells: Optional[int] = None,
                  big_face_cells: Optional[int] = None, device=None) -> ClosestPoint:
    """mesh (or a ``triangle_grid`` of it), points[n,3] -> a ``ClosestPoint`` on the device: for every point the nearest point of the
    SURFACE (not of a sample of it), over ALL faces; the squared distance to it, the distance, and the face it lies on — among faces
    at the same squared distance the lowest index.  The pair routine is include/vfn.h's ``vfn_closest_on_triangle``: float64, a
    fixed order of operations, exact for a vertex, never NaN for a degenerate face.  ``search="grid"`` walks a uniform grid of the faces
    ring by ring and ends a query's search by an exact lower bound; a query not ended after ``max_rings`` rings is served by all pairs,
    as ``nearest`` serves its leftovers.  ``search="all_pairs"`` tests every face for every query.  ``search``, ``max_rings``, ``cells``
    and ``big_face_cells`` change the time, never a bit.  A NaN / inf coordinate or a face index outside the vertices raises
    ``lib.VfnError``.  A specification of ours, following trimesh's ``proximity.closest_point`` and Open3D's
    ``RaycastingScene.compute_closest_points`` as remembered; verified against neither."""
    grid = mesh if isinstance(mesh, TriangleGrid) else None
    if grid is None:
        v, f = _check_mesh(mesh, "mesh")
    q = _check_points(points, "points")
    search, max_rings = _check_search(search), _check_max_rings(max_rings)
    if grid is not None and (cells is not None or big_face_cells is not None):
        raise ValueError("cells and big_face_cells are the grid's own: give them to triangle_grid")
    cells, big_face_cells = _check_cells(cells), _check_big_face_cells(big_face_cells)
    dev = grid.tri.device if grid is not None else _device(device)
    with torch.cuda.device(dev):
        if grid is None:
            grid = _triangle_grid(_dev_points(v, dev), f.to(dev, torch.int64).contiguous(), cells, big_face_cells, pairs=search == "grid")
        face, closest, sqdist, _ = _closest(_dev_points(q, dev), grid, max_rings if search == "grid" else None)
    return ClosestPoint(closest, sqdist, torch.sqrt(sqdist), face)


def surface_distances(points, mesh, search: str = "grid", device=None) -> torch.Tensor:
    """points[n,3], mesh -> float64 [n] on the device: every point's distance to the surface (``closest_point``'s ``distance``)."""
    return closest_point(mesh, points, search=search, device=device).distance


def _deviation(dist: torch.Tensor) -> dict:
    """Distances [n] on the device -> {"mean", "rms", "max", "median"}: sums and the maximum along the fixed tree (``lib.reduce_stats``),
    the median from the two middle values; one read."""
    n = dist.shape[0]
    host = torch.cat((lib.reduce_stats(dist, math.inf)[:3], lib.reduce_stats(dist * dist, math.inf)[:1], _median_pair(dist))).cpu().numpy()
    return {"mean": float(host[0] / n), "rms": float(math.sqrt(host[3] / n)), "max": float(host[2]), "median": float((host[4] + host[5]) / 2.0)}


def surface_deviation(mesh_a, mesh_b, num_points: int = 1000000, generator: Optional[torch.Generator] = None, uniforms=None,
                      vertices: bool = False, search: str = "grid", device=None) -> dict:
    """{"mean", "rms", "max", "median"} of the distances from surface ``a`` to surface ``b``: ONE-SIDED — ``num_points`` area-weighted
    samples of ``a`` (``sample_surface``; ``uniforms`` replaces the random numbers), or with ``vertices=True`` the vertices of ``a`` that
    its faces name, in ascending index, each measured against the surface of ``b`` itself (``closest_point``).  What a mesh operation
    moved: ``surface_deviation(simplified, original)``.  rms = sqrt(sum d^2 / n); the median is np.median's."""
    av, af = _check_mesh(mesh_a, "mesh_a")
    bv, bf = _check_mesh(mesh_b, "mesh_b")
    if not isinstance(vertices, (bool, np.bool_)):
        raise ValueError(f"vertices must be a bool, got {vertices!r}")
    search = _check_search(search)
    if not vertices:
        num_points = geomargs.positive_int(num_points, "num_points")
    dev = _device(device)
    if vertices:
        named = torch.unique(af.to(dev, torch.int64).reshape(-1))
        if int(named[0]) < 0 or int(named[-1]) >= av.shape[0]:
            lib.proximity_check(lib.GEOM_STATUS_INDEX, av.shape[0])
        points = _dev_points(av, dev)[named].contiguous()
    else:
        points, _ = sample_surface(av, af, num_points, generator=generator, uniforms=uniforms, device=dev)
    return _deviation(closest_point((bv, bf), points, search=search, device=dev).distance)


def _rigid_inverse(transformation: np.ndarray) -> np.ndarray:
    """[4,4] rigid -> its inverse [R^T | -R^T t] in float64 (numpy on the host)."""
    m = np.asarray(transformation, dtype=np.float64)
    inverse = np.eye(4)
    inverse[:3, :3] = m[:3, :3].T
    inverse[:3, 3] = -(m[:3, :3].T @ m[:3, 3])
    return inverse


def _mesh_direction(q: torch.Tensor, qn: Optional[torch.Tensor], mesh, threshold: float, info: torch.Tensor, ninfo: torch.Tensor) -> torch.Tensor:
    """One direction against a MESH -> device [7] as ``_direction``; with the queries' normals ``qn`` [8]: then the sum of
    |qn . n(face[i])| with n = ``meshops.face_normals`` of the mesh."""
    v, f = mesh
    dev = q.device
    with torch.cuda.device(dev):
        v, f = _dev_points(v, dev), f.to(dev, torch.int64).contiguous()
        grid = _triangle_grid(v, f, None, BIG_FACE_CELLS, info=info)
        face, _, sq, _ = _closest(q, grid, MAX_RINGS, info=info)
    row = _direction(torch.sqrt(sq), threshold)
    if qn is None:
        return row
    dots = lib.normal_dots(qn, lib.face_normals(v, f, True, info=ninfo), face, info=ninfo)
    return torch.cat((row, lib.reduce_stats(dots, math.inf)[:1]))


def _both_directions_mesh(pred_points: torch.Tensor, ref_points: torch.Tensor, pred_mesh, ref_mesh, threshold: float,
                          pred_normals: Optional[torch.Tensor] = None, ref_normals: Optional[torch.Tensor] = None):
    """``surface="mesh"``: the ref points against the pred MESH (row 0), the pred points against the ref MESH (row 1) -> (host [2,7] as
    ``_both_directions``, the "normal consistency" entry or None).  The points arrive in the frame of the mesh they are measured
    against.  One read of the results."""
    dev = pred_points.device
    info = torch.zeros(1, dtype=torch.int64, device=dev)
    ninfo = torch.zeros(1, dtype=torch.int64, device=dev)
    one = _mesh_direction(ref_points, ref_normals, pred_mesh, threshold, info, ninfo)
    two = _mesh_direction(pred_points, pred_normals, ref_mesh, threshold, info, ninfo)
    k = one.shape[0]
    host = torch.cat((one, two, info.to(torch.float64), ninfo.to(torch.float64))).cpu().numpy()
    lib.proximity_check(int(host[2 * k]), max(pred_mesh[0].shape[0], ref_mesh[0].shape[0]))
    lib.normals_check(int(host[2 * k + 1]), "normal consistency")
    rows = np.stack((host[0:7], host[k:k + 7]))
    if pred_normals is None:
        return rows, None
    a, b = float(host[k + 7] / pred_points.shape[0]), float(host[7] / ref_points.shape[0])
    return rows, {"pred_to_ref": a, "ref_to_pred": b, "mean": (a + b) / 2.0}
