"""The depth of a triangle mesh as pinhole cameras see it, on the device (csrc/vfn_raster.hip): the renderer half of
evaluation/methods.py:33-72 (``refuse``), which renders the mesh's depth from every dataset view with an OpenGL renderer
(evaluation/utils/renderer.py: pyrender, faces not culled) before re-fusing it.  ``vf_nerf_amd.refuse`` is the chain built on it.

``rasterize_depth`` gives, per view and pixel, the z-depth of the nearest surface or 0 where there is none — no colour, no face index.
The arithmetic is a specification, not a recording of pyrender / OpenGL (neither publishes one): ray / triangle intersection written
as homogeneous edge functions in float64, stated operation for operation in include/vfn.h, restated in NumPy in
tests/raster_restatement.py, and the device equals the restatement bit for bit.  A face that crosses the camera plane needs no
clipping (the datasets' cameras stand inside the scene mesh), a closed surface has no holes, and no bit depends on the order of the
faces.

Defaults: ``near = 0.05`` and ``far = 100.0`` are THIS MODULE's defaults — pyrender's camera defaults as remembered, not verified (the
reference sets neither).  ``pixel_centre = 0.5``: OpenGL samples a pixel at its centre, while the fusion's own projection
(``vfn_tsdf_integrate``) and the datasets' rays treat integer coordinates as centres, which is ``pixel_centre = 0.0``.  The reference
chain carries that half-pixel inconsistency; the parameter keeps it visible and defaults to the reference's 0.5.

A mesh is a ``mesh.Mesh`` or ``(vertices [n,3], faces [m,3])`` as in ``metrics3d`` / ``tsdf``; cameras are intrinsics ([3,3] / [4,4],
shared or per view) and camera-to-world poses ([V,4,4]; +z forward, x right, y down) as in ``tsdf``.  No CPU fallback:
``lib.VfnError`` when no device is visible.
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import geomargs, lib
from .geomargs import LIMIT
from .tsdf import extrinsics_from_poses, split_intrinsics

NEAR, FAR, PIXEL_CENTRE = 0.05, 100.0, 0.5


def check_view_args(n_views: int, height, width, near, far, pixel_centre) -> Tuple[int, int, float, float, float]:
    h, w = geomargs.positive_int(height, "height"), geomargs.positive_int(width, "width")
    if n_views * h * w >= LIMIT:
        raise ValueError(f"{n_views} views of {h} x {w} pixels reach the 2^31 limit of one call")
    near, far, c = geomargs.real32(near, "near"), geomargs.real32(far, "far"), geomargs.real32(pixel_centre, "pixel_centre")
    if not (0.0 < near < far):
        raise ValueError(f"need 0 < near < far as float32, got near {near!r} and far {far!r}")
    return h, w, near, far, c


def _n_views(poses) -> int:
    p = geomargs.as_tensor(poses, "poses")
    if p.dim() == 2:
        return 1
    if p.dim() != 3:
        raise ValueError(f"poses must be [4,4] or [V,4,4], got {tuple(p.shape)}")
    return int(p.shape[0])


def rasterize_depth_counted(mesh, intrinsics, poses, height: int, width: int, near: float = NEAR, far: float = FAR,
                            pixel_centre: float = PIXEL_CENTRE, device=None):
    """``rasterize_depth`` with the kernel's counters: -> (depth, {"fragments": kept (face, pixel) candidates, "atomics": atomics sent,
    "cooperative": (face, view) pairs walked by a whole wave})."""
    v, f = geomargs.check_mesh(mesh)
    n = _n_views(poses)
    k = split_intrinsics(intrinsics, n)
    e = extrinsics_from_poses(poses, n)
    h, w, near, far, c = check_view_args(n, height, width, near, far, pixel_centre)
    # (every refusal above needs no device)
    dev = geomargs.device(device if device is not None else (v.device if v.is_cuda else None), "the depth rasteriser")
    if n == 0 or f.shape[0] == 0:
        return torch.zeros(n, h, w, dtype=torch.float32, device=dev), {"fragments": 0, "atomics": 0, "cooperative": 0}
    return lib.raster_depth(v.to(dev, torch.float64).contiguous(), f.to(dev, torch.int64).contiguous(), k.to(dev), e.to(dev), h, w, near, far, c)


def rasterize_depth(vertices, faces=None, intrinsics=None, poses=None, height=None, width=None, near: float = NEAR, far: float = FAR,
                    pixel_centre: float = PIXEL_CENTRE, device=None) -> torch.Tensor:
    """The mesh ``(vertices, faces)`` — or a ``mesh.Mesh`` as ``vertices`` with ``faces=None`` — seen by V pinhole cameras ->
    depth[V,height,width] float32 on the device: the z-depth of the nearest surface, 0 where there is none.  All views in ONE kernel
    launch (faces and vertices are read once per call).  ``near`` / ``far`` bound the depths that count (this module's defaults, see
    above); ``pixel_centre`` is the offset of a pixel's sample point from its integer coordinate (0.5: OpenGL's; 0.0: the fusion's).
    An empty mesh gives all zeros.  A face index outside the vertices or a non-finite vertex raises ``lib.VfnError``."""
    mesh = vertices if faces is None else (vertices, faces)
    if intrinsics is None or poses is None or height is None or width is None:
        raise TypeError("rasterize_depth needs intrinsics, poses, height and width")
    return rasterize_depth_counted(mesh, intrinsics, poses, height, width, near=near, far=far, pixel_centre=pixel_centre, device=device)[0]
