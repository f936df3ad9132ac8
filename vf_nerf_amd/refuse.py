"""The tail of the reference's ``metrics_3d`` (evaluation/methods.py:667-744) on the device: the four meshes it scores — ``tsdf``,
``tsdf-smoothed``, ``refused-tsdf``, ``refused-tsdf-smoothed`` — from the one ``vf_nerf_amd.tsdf`` produces, and their scores.

* ``refuse`` — methods.py:33-72: the mesh's depth from every view (``raster.rasterize_depth`` in place of the OpenGL renderer), depths
  at or beyond ``depth_trunc`` dropped (depth_scale 1, no uint16 step: methods.py:61-62), the maps re-fused by
  ``tsdf.fuse_depth_maps`` (voxel length 4/512, ``sdf_trunc`` 0.04).  Whatever no camera sees disappears.
* ``smooth_laplacian`` — methods.py:690 (``filter_smooth_laplacian(number_of_iterations=10)``): uniform-weight Laplacian smoothing,
  Jacobi steps ``v + lam (mean of the neighbours - v)`` over the edge-neighbours of every vertex.  ``iterations = 10`` and
  ``lam = 0.5`` are Open3D's filter as remembered, not verified; Open3D's neighbour sets have no fixed summation order, so ours
  (ascending neighbour index, include/vfn.h) is a specification.
* ``reconstruction_meshes`` — the four meshes; ``metrics_3d`` — the dictionary of methods.py:732-741, every entry a
  ``metrics3d.score_mesh``.

Everything stays on the device between the stages; a mesh is ``(vertices float64 [n,3], faces int64 [m,3])``.  No CPU fallback.

``metrics_3d(..., icp_align=True)`` aligns every mesh's samples to the ground truth's before scoring (``vf_nerf_amd.icp``, a
specification of ours, not verified against Open3D).

``refuse_rgbd`` is ``refuse`` with the views' images fused along with the depth, as the reference's ``refuse()`` does (nothing it reports
depends on the colour; the mesh it returns is coloured) -> (vertices, faces, vertex colours); ``vf_nerf_amd.ply`` reads and writes PLY
files (with vertex normals, if given: ``meshops.vertex_normals``); trimesh's vertex merging is ``meshops.weld``.

``metrics_3d(..., normals=True)`` adds "normal consistency" to every entry (``metrics3d.normal_consistency``).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import geomargs, lib, metrics3d, raster, tsdf

DEPTH_TRUNC = 5.0                  # evaluation/methods.py:62
ITERATIONS, LAM = 10, 0.5
MESH_NAMES = ("tsdf", "refused_tsdf", "tsdf_smoothed", "refused_tsdf_smoothed")      # the order of methods.py:732-736


def refuse(mesh, intrinsics, poses, height: int, width: int, bounds=None, voxel_length: float = tsdf.VOXEL_LENGTH,
           sdf_trunc: float = tsdf.SDF_TRUNC, depth_trunc: float = DEPTH_TRUNC, near: float = raster.NEAR, far: float = raster.FAR,
           pixel_centre: float = raster.PIXEL_CENTRE, device=None, sparse: bool = False):
    """Render the mesh's depth from every view, drop depths >= ``depth_trunc``, fuse the maps again -> (vertices, faces).  ``bounds`` as
    in ``tsdf.fuse_depth_maps`` (None: the back-projected depth points, padded by ``sdf_trunc``).  Two empty tensors when no camera
    sees anything.  ``sparse`` goes to the fusion (``tsdf.fuse_depth_maps``: the block-sparse volume)."""
    return _refuse(mesh, None, intrinsics, poses, height, width, bounds=bounds, voxel_length=voxel_length, sdf_trunc=sdf_trunc,
                   depth_trunc=depth_trunc, near=near, far=far, pixel_centre=pixel_centre, device=device, sparse=sparse)


def refuse_rgbd(mesh, rgb, intrinsics, poses, height: int, width: int, **refuse_args):
    """``refuse`` WITH the views' images, what the reference's ``refuse()`` fuses (methods.py:56-62: the dataset's rgb as bytes next to the
    mesh's rendered depth) -> (vertices, faces, vertex_colours float64 [n,3] in [0,1]).  ``rgb`` is uint8 [V,height,width,3] (or
    [height,width,3] for one view), or float32 in [0, 1] quantised as ``metrics2d.quantize_rgb8`` does — trunc(x 255), the reference's
    ``(rgb * 255).astype(np.uint8)``.  ``refuse_args`` are ``refuse``'s; the vertices and faces are ``refuse``'s."""
    if rgb is None:
        raise ValueError("rgb is required (refuse re-fuses depth alone)")
    return _refuse(mesh, rgb, intrinsics, poses, height, width, **refuse_args)


def _refuse(mesh, rgb, intrinsics, poses, height, width, bounds=None, voxel_length=tsdf.VOXEL_LENGTH, sdf_trunc=tsdf.SDF_TRUNC,
            depth_trunc=DEPTH_TRUNC, near=raster.NEAR, far=raster.FAR, pixel_centre=raster.PIXEL_CENTRE, device=None, sparse=False):
    if isinstance(depth_trunc, bool) or not isinstance(depth_trunc, (int, float, np.integer, np.floating)) or not float(depth_trunc) > 0:
        raise ValueError(f"depth_trunc must be a positive number, got {depth_trunc!r}")
    vl, _ = geomargs.positive32(voxel_length, "voxel_length"), geomargs.positive32(sdf_trunc, "sdf_trunc")
    if bounds is not None:
        tsdf.bounds_box(bounds, vl, bool(sparse))                          # every refusal that needs no device comes before the first launch
    if rgb is not None:
        n_views = 1 if geomargs.as_tensor(poses, "poses").dim() == 2 else int(geomargs.as_tensor(poses, "poses").shape[0])
        tsdf._stack_rgb(rgb, (n_views, height, width))
    depth = raster.rasterize_depth_counted(mesh, intrinsics, poses, height, width, near=near, far=far, pixel_centre=pixel_centre, device=device)[0]
    depth = torch.where(depth >= float(depth_trunc), torch.zeros_like(depth), depth)
    if rgb is None:
        return tsdf.fuse_depth_maps(depth, intrinsics, poses, bounds=bounds, voxel_length=voxel_length, sdf_trunc=sdf_trunc, device=depth.device,
                                    sparse=bool(sparse))
    return tsdf.fuse_rgbd_maps(depth, rgb, intrinsics, poses, bounds=bounds, voxel_length=voxel_length, sdf_trunc=sdf_trunc, device=depth.device,
                               sparse=bool(sparse))


def vertex_adjacency(faces: torch.Tensor, n_vertices: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """faces[m,3] (int64, every index in [0, n)) -> the CSR of the edge-neighbours (row_start[n+1], neighbours), on faces' device: the
    three undirected edges of every face, self-edges dropped, duplicates removed, a vertex's neighbours in ascending order."""
    a = torch.cat([faces[:, 0], faces[:, 1], faces[:, 2], faces[:, 1], faces[:, 2], faces[:, 0]])
    b = torch.cat([faces[:, 1], faces[:, 2], faces[:, 0], faces[:, 0], faces[:, 1], faces[:, 2]])
    keep = a != b
    keys = torch.unique(a[keep] * n_vertices + b[keep])                  # sorted: by vertex, then by neighbour
    rows = torch.div(keys, n_vertices, rounding_mode="floor")
    row_start = torch.zeros(n_vertices + 1, dtype=torch.int64, device=faces.device)
    row_start[1:] = torch.cumsum(torch.bincount(rows, minlength=n_vertices), dim=0)
    return row_start, (keys - rows * n_vertices).contiguous()


def smooth_laplacian(mesh, iterations: int = ITERATIONS, lam: float = LAM, device=None):
    """``iterations`` Jacobi steps of uniform Laplacian smoothing -> (vertices, faces) on the device; the faces are the input's.  A vertex
    that no face uses (or only degenerate ones) stays where it is."""
    v, f = geomargs.check_mesh(mesh)
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or int(iterations) < 0:
        raise ValueError(f"iterations must be a non-negative integer, got {iterations!r}")
    if isinstance(lam, bool) or not isinstance(lam, (int, float, np.integer, np.floating)) or not math.isfinite(float(lam)):
        raise ValueError(f"lam must be a finite number, got {lam!r}")
    dev = geomargs.device(device if device is not None else (v.device if v.is_cuda else None), "Laplacian smoothing")
    v, f = v.to(dev, torch.float64).contiguous(), f.to(dev, torch.int64).contiguous()
    n = v.shape[0]
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= n):
        raise lib.VfnError(f"Laplacian smoothing: a face index lies outside [0, {n})")
    row_start, neighbours = vertex_adjacency(f, n)
    return lib.smooth_laplacian(v, row_start, neighbours, int(iterations), float(lam)), f


def reconstruction_meshes(tsdf_mesh, intrinsics, poses, height: int, width: int, iterations: int = ITERATIONS, lam: float = LAM,
                          **refuse_args) -> Dict[str, tuple]:
    """The four meshes ``metrics_3d`` scores (methods.py:686-709) from the TSDF mesh and the dataset's cameras: ``tsdf`` (as given),
    ``tsdf_smoothed``, ``refused_tsdf`` = refuse(tsdf), ``refused_tsdf_smoothed`` = refuse(tsdf_smoothed).  ``refuse_args`` go to
    ``refuse`` (bounds, voxel_length, sdf_trunc, depth_trunc, near, far, pixel_centre, device)."""
    smoothed = smooth_laplacian(tsdf_mesh, iterations=iterations, lam=lam, device=refuse_args.get("device"))
    dev = smoothed[0].device
    v, f = geomargs.check_mesh(tsdf_mesh)
    plain = (v.to(dev, torch.float64).contiguous(), smoothed[1])
    return {"tsdf": plain, "tsdf_smoothed": smoothed,
            "refused_tsdf": refuse(plain, intrinsics, poses, height, width, **refuse_args),
            "refused_tsdf_smoothed": refuse(smoothed, intrinsics, poses, height, width, **refuse_args)}


def metrics_3d(tsdf_mesh, gt_mesh, intrinsics, poses, height: int, width: int, num_points: int = 1000000, distance_thresh: float = 0.01,
               generator: Optional[torch.Generator] = None, uniforms=None, iterations: int = ITERATIONS, lam: float = LAM,
               icp_align: bool = False, icp_threshold: Optional[float] = None, search: str = "all_pairs", normals: bool = False, voxel_size=None,
               min_component_faces=None, keep_largest=None, surface: str = "samples", **refuse_args) -> Dict[str, dict]:
    """The dictionary the reference writes to ``3d-metrics.json`` (methods.py:732-741): keys ``tsdf``, ``refused_tsdf``,
    ``tsdf_smoothed``, ``refused_tsdf_smoothed``, each ``metrics3d.score_mesh(mesh, gt_mesh)`` — {"chamfer distance": {mean, median,
    min, max}, "precision", "recall", "fscore", ...} — scored in that order with the one ``generator`` (or the same ``uniforms``).  ``icp_align`` / ``icp_threshold`` go to
    ``metrics3d.score_mesh`` (every entry then has an "icp" key), and so does ``search`` ("all_pairs" or "grid": the eight searches
    through the grid kernel, the same dictionary to the bit), ``normals`` (True: every entry gains "normal consistency") and
    ``voxel_size`` (a value: every entry is scored on the voxel-down-sampled clouds and gains "voxel"; None changes nothing).
    ``min_component_faces`` / ``keep_largest`` go there too (a value: every one of the four meshes is scored without its small detached
    pieces, ``meshops.filter_components``, and every entry gains "components"; both None change nothing).  ``surface`` goes there as
    well ("mesh": every one of the four meshes and ``gt_mesh`` are measured as surfaces, ``metrics3d.closest_point``, not through
    their samples, and every entry gains "surface": "mesh"; "samples", the default, changes nothing)."""
    search = metrics3d._check_search(search)
    surface = metrics3d._check_surface(surface)
    voxel_size = metrics3d._check_voxel(voxel_size)
    if voxel_size is not None and normals:
        raise ValueError("voxel_size together with normals=True: a voxel's normal for normal consistency is not defined here")
    components_kw = metrics3d._check_components(min_component_faces, keep_largest)
    components_kw = {} if components_kw is None else {"min_component_faces": min_component_faces, "keep_largest": keep_largest}
    meshes = reconstruction_meshes(tsdf_mesh, intrinsics, poses, height, width, iterations=iterations, lam=lam, **refuse_args)
    dev = meshes["tsdf"][0].device
    return {name: metrics3d.score_mesh(meshes[name], gt_mesh, num_points=num_points, distance_thresh=distance_thresh, generator=generator,
                                       uniforms=uniforms, device=dev, icp_align=icp_align, icp_threshold=icp_threshold, search=search,
                                       **({"normals": True} if normals else {}), **({} if voxel_size is None else {"voxel_size": voxel_size}), **components_kw,
                                       **({} if surface == "samples" else {"surface": surface}))
            for name in MESH_NAMES}
