"""Fusing depth maps into a mesh on the device (csrc/vfn_tsdf.hip): the stage of evaluation/methods.py:613-665 (``tsdf_mesh``) between
``render-images`` and ``3d-metrics`` — the mesh that ``metrics_3d`` scores for a trained VF-NeRF — without leaving the device.

* ``TSDFVolume`` — a dense truncated-signed-distance volume: ``integrate`` fuses one depth map or a stack of them in ONE pass over the
  volume, ``extract_mesh`` triangulates the zero level set with classic marching cubes.  ``TSDFVolume(..., colour=True)`` fuses every
  view's RGB image together with its depth (the reference's ``TSDFVolumeColorType.RGB8``); ``extract_coloured_mesh`` adds a colour per
  vertex.
* ``SparseTSDFVolume`` — the same lattice held as blocks of 8^3 voxels opened near the back-projected depth points: no 2^31 voxel limit,
  memory that grows with the surface, every held voxel with the dense volume's bits and — on the allocation rule of include/vfn.h — the
  dense volume's mesh.  ``sparse=True`` on the ``fuse_*`` functions fuses into it; the default stays dense.
* ``reference_depth`` — a depth map as ``tsdf_mesh`` hands it to the fusion: millimetres as uint16, truncated at ``depth_trunc``.
* ``fuse_depth_maps`` — depth maps + cameras -> mesh; the box defaults to the back-projected valid depth points, padded by ``sdf_trunc``.
  ``fuse_rgbd_maps`` — the same with the views' images -> (vertices, faces, vertex colours).
* ``fuse_rendered_views`` — a model's views rendered (``VectorFieldNerf.render_chunked``, as ``evaluator.render_view``), their depth
  maps kept on the device and fused; only the mesh leaves it.  ``fuse_rendered_rgbd`` keeps the rendered rgb too (as the bytes of the
  PNG ``render_images`` writes) and returns the coloured mesh; ``vf_nerf_amd.ply.write_ply`` writes it as the reference's ``tsdf.ply``.

The semantics are modelled on a uniform TSDF volume's integration and extraction as ``tsdf_mesh`` drives one (voxel length 4/512,
``sdf_trunc`` 0.04, extrinsic = inv(pose)); include/vfn.h states the arithmetic operation for operation and tests/tsdf_restatement.py
restates it in NumPy (tests/tsdf_colour_restatement.py: the colour; tests/tsdf_sparse_restatement.py: the blocks), which the device equals
bit for bit.  One deliberate difference from the reference's fusion:

* ``TSDFVolume`` is DENSE over a box the caller gives, not hashed 16^3 blocks opened near back-projected points.  A voxel in free space
  in front of a surface therefore collects ``tsdf = 1`` observations here in cases where the hashed volume would never have allocated it;
  the zero crossing lies inside the truncation band either way.  ``SparseTSDFVolume`` opens blocks near the points as the hashed volume
  does, but blocks of 8^3 voxels of the dense lattice, by a rule under which its mesh is the dense one.

A mesh is ``(vertices float64 [n,3], faces int64 [m,3])``, 0-based, on the device — the form ``mesh.triangulate`` returns and
``metrics3d.score_mesh`` accepts; a coloured mesh adds ``colours float64 [n,3]`` in [0, 1].  A volume without colour keeps its kernels
and its bits; the geometry of a coloured volume is bit-equal to the colourless one's.  No CPU fallback: ``lib.VfnError`` when no device
is visible.

``refuse()`` and Laplacian smoothing (``tsdf-smoothed.ply``) are ``vf_nerf_amd.refuse``: a mesh's depth rasterised on the device
(``vf_nerf_amd.raster``) and re-fused by this volume.  PLY reading / writing is ``vf_nerf_amd.ply``, the vertex
normals the reference computes before writing (``compute_vertex_normals()``) are ``meshops.vertex_normals``.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import geomargs, lib
from .geomargs import LIMIT

VOXEL_LENGTH = 4.0 / 512.0        # evaluation/methods.py:624
SDF_TRUNC = 0.04                  # :625
DEPTH_SCALE, DEPTH_TRUNC = 1000.0, 10.0


def _three_dims(dims) -> Tuple[int, int, int]:
    d = tuple(dims)
    if len(d) != 3 or any(isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 1 for n in d):
        raise ValueError(f"dims must be three positive integers, got {dims!r}")
    return tuple(int(n) for n in d)


def _check_dims(dims) -> Tuple[int, int, int]:
    d = _three_dims(dims)
    if d[0] * d[1] * d[2] >= LIMIT:
        raise ValueError(f"a volume of {d[0]} x {d[1]} x {d[2]} voxels exceeds the 2^31 limit")
    return d


BLOCK = 8                         # the edge of a block of the sparse volume, a compile-time constant of csrc/vfn_tsdf.hip
DIM_LIMIT = 1 << 24               # a lattice index is exact as float32 up to here


def _check_sparse_dims(dims) -> Tuple[int, int, int]:
    """``_check_dims`` for the block-sparse volume: no bound on the voxels; each dim <= 2^24 and fewer than 2^31 blocks of 8^3."""
    d = _three_dims(dims)
    if max(d) > DIM_LIMIT:
        raise ValueError(f"a sparse volume of {d[0]} x {d[1]} x {d[2]} voxels exceeds 2^24 voxels along an axis")
    nb = lib.tsdf_block_lattice(d)
    if nb[0] * nb[1] * nb[2] >= LIMIT:
        raise ValueError(f"a sparse volume of {d[0]} x {d[1]} x {d[2]} voxels has {nb[0]} x {nb[1]} x {nb[2]} blocks: beyond the 2^31 limit")
    return d


def _check_depth_values(d: torch.Tensor, name: str) -> None:
    """One reduction on whatever device the map lives on: non-finite or negative depths are refused."""
    if d.numel() and not bool((torch.isfinite(d) & (d >= 0)).all()):
        raise ValueError(f"{name} holds non-finite or negative values")


def split_intrinsics(intrinsics, n_views: int) -> torch.Tensor:
    """[3,3] / [4,4] shared or [V,3,3] / [V,4,4] per view -> float32 [V,4] = fx fy cx cy (host).  Skew is refused: the projection of
    include/vfn.h has none."""
    k = geomargs.as_tensor(intrinsics, "intrinsics").cpu()
    if k.dim() == 2:
        k = k.unsqueeze(0).expand(n_views, -1, -1)
    if k.dim() != 3 or k.shape[0] != n_views or tuple(k.shape[1:]) not in ((3, 3), (4, 4)):
        raise ValueError(f"intrinsics must be [3,3], [4,4] or one of those per view ({n_views}), got {tuple(geomargs.as_tensor(intrinsics, 'intrinsics').shape)}")
    k = k.to(torch.float32)
    out = torch.stack([k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2]], dim=1).contiguous()
    if not bool(torch.isfinite(out).all()) or not bool((out[:, :2] > 0).all()):
        raise ValueError("intrinsics need finite values and positive focal lengths")
    if bool((k[:, 0, 1] != 0).any()):
        raise ValueError("intrinsics with skew are not supported")
    return out


def extrinsics_from_poses(poses, n_views: int) -> torch.Tensor:
    """Camera-to-world poses [4,4] / [V,4,4] -> float32 [V,12]: the first three rows of float32(inv(float64 pose)) (host)."""
    p = geomargs.as_tensor(poses, "pose").cpu()
    if p.dim() == 2:
        p = p.unsqueeze(0)
    if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4) or p.shape[0] != n_views:
        raise ValueError(f"poses must be [4,4] per view ({n_views}), got {tuple(geomargs.as_tensor(poses, 'pose').shape)}")
    p64 = p.to(torch.float64).numpy()
    if not np.isfinite(p64).all():
        raise ValueError("a pose holds non-finite values")
    out = np.empty((n_views, 12), dtype=np.float32)
    for i in range(n_views):
        try:
            inv = np.linalg.inv(p64[i])
        except np.linalg.LinAlgError:
            raise ValueError(f"pose {i} is singular") from None
        e = inv.astype(np.float32)
        if not np.isfinite(e).all() or np.linalg.matrix_rank(p64[i]) < 4:
            raise ValueError(f"pose {i} is singular")
        out[i] = e[:3].reshape(12)
    return torch.from_numpy(out)


def _stack_depths(depth, name: str = "depth") -> torch.Tensor:
    d = geomargs.as_tensor(depth, name)
    if d.dim() == 2:
        d = d.unsqueeze(0)
    if d.dim() == 4 and d.shape[-1] == 1:
        d = d[..., 0]
    if d.dim() != 3 or d.shape[1] < 1 or d.shape[2] < 1:
        raise ValueError(f"{name} must be [H,W] or [V,H,W], got {tuple(geomargs.as_tensor(depth, name).shape)}")
    if not d.dtype.is_floating_point:
        raise ValueError(f"{name} must be floating point (metres), got {d.dtype}")
    if d.shape[1] * d.shape[2] >= LIMIT:
        raise ValueError(f"{name}: a map of {d.shape[1]} x {d.shape[2]} pixels exceeds the 2^31 limit")
    return d


def _stack_rgb(rgb, views_shape, name: str = "rgb") -> torch.Tensor:
    """The images that go with depth maps of ``views_shape`` = (V, H, W): uint8 or float32, [V,H,W,3] (or [H,W,3] for one view) ->
    [V,H,W,3] as given (any device, not yet bytes).  Any other dtype or shape is refused."""
    c = geomargs.as_tensor(rgb, name)
    if c.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{name} must be uint8 (bytes) or float32 (in [0, 1], quantised as the PNG is), got {c.dtype}")
    if c.dim() == 3:
        c = c.unsqueeze(0)
    if c.dim() != 4 or c.shape[-1] != 3:
        raise ValueError(f"{name} must be [H,W,3] or [V,H,W,3], got {tuple(geomargs.as_tensor(rgb, name).shape)}")
    if tuple(c.shape[:3]) != tuple(views_shape):
        raise ValueError(f"{name} of {tuple(c.shape[:3])} views x pixels does not go with depth maps of {tuple(views_shape)}")
    return c


def _rgb_bytes(c: torch.Tensor, dev) -> torch.Tensor:
    """``_stack_rgb``'s result as contiguous uint8 on ``dev``; float32 goes through ``metrics2d.quantize_rgb8`` (the PNG's bytes)."""
    if c.dtype == torch.float32:
        from . import metrics2d
        return metrics2d.quantize_rgb8(c, device=dev).contiguous()
    return c.to(dev).contiguous()


def reference_depth(depth_map, depth_scale: float = DEPTH_SCALE, depth_trunc: float = DEPTH_TRUNC) -> torch.Tensor:
    """A depth map in metres as ``tsdf_mesh`` feeds it to the fusion (evaluation/methods.py:651-657): q = trunc(float64(depth) depth_scale) as
    uint16, d = float32(q) / float32(depth_scale), d = 0 where d >= depth_trunc.  Non-finite, negative or >= 65.536 m (at the default
    scale: anything whose q leaves uint16) inputs are refused — NumPy's out-of-range cast is undefined and not inherited.  Stays on
    the input's device."""
    d = geomargs.as_tensor(depth_map, "depth_map")
    if not d.dtype.is_floating_point:
        raise ValueError(f"depth_map must be floating point (metres), got {d.dtype}")
    _check_depth_values(d, "depth_map")
    q = torch.trunc(d.to(torch.float64) * float(depth_scale))      # (the reference multiplies the float64 array it loads from depth-i.npy)
    if d.numel() and bool((q > 65535).any()):
        raise ValueError(f"depth_map holds values of {65536 / depth_scale} m or more: their millimetres leave uint16")
    out = q.to(torch.float32) / torch.tensor(depth_scale, dtype=torch.float32, device=d.device)
    return torch.where(out >= depth_trunc, torch.zeros_like(out), out)


class _LatticeVolume:
    """What both volumes share: the lattice arguments, taken as float32, and the checks of a call's views.  ``dims`` arrive checked."""

    def __init__(self, origin, dims, voxel_length, sdf_trunc, device):
        self.dims = dims
        self.voxel_length = geomargs.positive32(voxel_length, "voxel_length")
        self.sdf_trunc = geomargs.positive32(sdf_trunc, "sdf_trunc")
        o = np.asarray(origin.detach().cpu() if isinstance(origin, torch.Tensor) else origin, dtype=np.float64).reshape(-1)
        if o.shape != (3,) or not np.isfinite(o.astype(np.float32)).all():
            raise ValueError(f"origin must be three finite numbers, got {origin!r}")
        self.origin = tuple(float(x) for x in o.astype(np.float32))
        self.device = geomargs.device(device, "TSDF fusion")

    def _views(self, depth, intrinsics, pose, rgb, need_rgb: bool = True):
        """The arguments of ``integrate`` checked -> (depth maps [V,H,W] where they live, images as given or None, float32 fx fy cx cy
        [V,4] and extrinsic rows [V,12] on the host): what ``_integrate_prepared`` takes."""
        d = _stack_depths(depth)
        v = d.shape[0]
        if need_rgb and (rgb is None) != (self.colour is None):
            raise ValueError("rgb is required by a volume with colour" if rgb is None else "rgb was given to a volume without colour")
        c = None if rgb is None else _stack_rgb(rgb, d.shape)
        k = split_intrinsics(intrinsics, v)
        e = extrinsics_from_poses(pose, v)
        _check_depth_values(d, "depth")
        return d, c, k, e


class TSDFVolume(_LatticeVolume):
    """A dense TSDF volume of ``dims = (nx, ny, nz)`` voxels of ``voxel_length`` whose first voxel's corner is ``origin``: voxel (i, j, k)
    has its centre at origin + (index + 0.5) voxel_length.  ``tsdf`` / ``weight`` are float32 [nx,ny,nz] device tensors, zero until a
    view has been integrated.  ``colour=True`` adds ``colour`` float32 [nx,ny,nz,3] in byte units (else None): every ``integrate`` then
    needs the views' images."""

    def __init__(self, origin, dims, voxel_length: float = VOXEL_LENGTH, sdf_trunc: float = SDF_TRUNC, device=None, colour: bool = False):
        super().__init__(origin, _check_dims(dims), voxel_length, sdf_trunc, device)
        self.tsdf = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(self.dims, dtype=torch.float32, device=self.device)
        self.colour = torch.zeros(self.dims + (3,), dtype=torch.float32, device=self.device) if colour else None

    def reset(self) -> None:
        self.tsdf.zero_()
        self.weight.zero_()
        if self.colour is not None:
            self.colour.zero_()

    def integrate(self, depth, intrinsics, pose, rgb=None) -> None:
        """One depth map [H,W] or a stack [V,H,W] (float metres, 0 = no measurement; host or device tensors or NumPy) with intrinsics
        [3,3] / [4,4] shared or per view and camera-to-world poses [4,4] / [V,4,4].  The V views are fused in index order by ONE kernel
        that reads and writes the volume once: the bits of V single-view calls.  ``rgb`` — required exactly when the volume has colour —
        is the views' images, uint8 [V,H,W,3] / [H,W,3], or float32 in [0, 1] sent through ``metrics2d.quantize_rgb8``."""
        self._integrate_prepared(*self._views(depth, intrinsics, pose, rgb))

    def _integrate_prepared(self, d, c, k, e) -> None:
        """``integrate`` of views that ``_views`` (or a caller with the same checks) has passed."""
        dev = self.device
        d = d.to(dev, torch.float32).contiguous()
        if c is None:
            lib.tsdf_integrate(self.tsdf, self.weight, self.origin, self.voxel_length, self.sdf_trunc, d, k.to(dev), e.to(dev))
        else:
            lib.tsdf_integrate_rgb(self.tsdf, self.weight, self.colour, self.origin, self.voxel_length, self.sdf_trunc, d, _rgb_bytes(c, dev),
                                   k.to(dev), e.to(dev))

    def extract_mesh(self):
        """-> (vertices float64 [n,3], faces int64 [m,3], 0-based) on the device; two empty tensors when nothing crosses zero."""
        return lib.tsdf_extract(self.tsdf, self.weight, self.origin, self.voxel_length)

    def extract_coloured_mesh(self):
        """``extract_mesh`` of a volume with colour -> (vertices, faces, colours float64 [n,3] in [0,1]): the same vertices and faces."""
        if self.colour is None:
            raise ValueError("extract_coloured_mesh needs a volume with colour (TSDFVolume(..., colour=True))")
        return lib.tsdf_extract_coloured(self.tsdf, self.weight, self.colour, self.origin, self.voxel_length)


def mark_cameras(k: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """What the allocation kernel reads per view, float64 [V,17] (host): C[12], the first three rows of ``numpy.linalg.inv`` of the 4x4 built
    from the float32 extrinsic rows ``e`` [V,12] promoted to float64 — the allocation inverts exactly the matrix the integration uses —,
    then fx fy cx cy (the float32 intrinsics ``k`` [V,4] promoted) and q = sqrt(1 / (fx fx) + 1 / (fy fy))."""
    k64, e64 = k.numpy().astype(np.float64), e.numpy().astype(np.float64)
    out = np.empty((k64.shape[0], 17), dtype=np.float64)
    for i in range(k64.shape[0]):
        m = np.eye(4, dtype=np.float64)
        m[:3] = e64[i].reshape(3, 4)
        out[i, :12] = np.linalg.inv(m)[:3].reshape(12)
        fx, fy = k64[i, 0], k64[i, 1]
        out[i, 12:16] = k64[i]
        out[i, 16] = np.sqrt(np.float64(1.0) / (fx * fx) + np.float64(1.0) / (fy * fy))
    return torch.from_numpy(out)


class SparseTSDFVolume(_LatticeVolume):
    """A block-sparse TSDF volume over the lattice of ``TSDFVolume(origin, dims, voxel_length)``: the same ``origin`` / ``dims`` /
    ``voxel_length`` taken as float32, voxel (i, j, k) centred at origin + ((float)index + 0.5f) voxel_length with the GLOBAL index — so
    every voxel it holds carries the bits of the dense volume over the same lattice — but only blocks of ``BLOCK``^3 = 8^3 voxels near
    the back-projected depth points exist.  ``dims`` are not bound by 2^31 voxels: each dim is <= 2^24, the block lattice
    nb = ceil(dims / 8) has fewer than 2^31 blocks, and the allocated blocks hold fewer than 2^31 voxels.

    The block edge is 8, not the 16 of the reference's hashed volume (which is not reproduced bit for bit anyway): 8 wastes about 30 %
    fewer voxels around a band of +-(sdf_trunc + one voxel), and one block is two waves of lanes owning 4 consecutive k voxels each.

    State, all on the device: ``block_of`` int32 [nbx,nby,nbz] (-1: absent), ``block_coords`` int32 [n_blocks,3], ``tsdf`` / ``weight``
    float32 [n_blocks,8,8,8] and ``colour`` float32 [n_blocks,8,8,8,3] in byte units (None without colour).  Block ids are given in order
    of allocation call and, within a call, in ascending C order of the block lattice (``torch.nonzero`` of the marks; no atomics decide a
    number); they never change, growth is a ``torch.cat``.  Voxels of an edge block whose global index is >= dims are never updated and
    keep weight == 0.

    Allocation rule (include/vfn.h, vfn_tsdf_sparse_mark; DESIGN 6p has the argument): a pixel with depth d > 0 opens every block that
    the axis-aligned cube of half edge r = sdf_trunc + 0.5 (d + sdf_trunc) q + 2 voxel_length around its back-projected point touches,
    q = sqrt(1 / fx^2 + 1 / fy^2).  With it, every cell the dense extraction triangulates has its eight corners in allocated blocks:
    after ONE ``integrate`` of all views the mesh is the dense volume's mesh.  A voxel of a block holds the bits of a dense volume
    that was zero until the call that opened the block."""

    def __init__(self, origin, dims, voxel_length: float = VOXEL_LENGTH, sdf_trunc: float = SDF_TRUNC, device=None, colour: bool = False):
        super().__init__(origin, _check_sparse_dims(dims), voxel_length, sdf_trunc, device)
        self.block_dims = lib.tsdf_block_lattice(self.dims)
        self._has_colour = bool(colour)
        self.reset()

    def reset(self) -> None:
        """Back to no blocks."""
        dev, blk = self.device, (BLOCK,) * 3
        self.block_of = torch.full(self.block_dims, -1, dtype=torch.int32, device=dev)
        self.block_coords = torch.zeros(0, 3, dtype=torch.int32, device=dev)
        self.tsdf = torch.zeros((0,) + blk, dtype=torch.float32, device=dev)
        self.weight = torch.zeros((0,) + blk, dtype=torch.float32, device=dev)
        self.colour = torch.zeros((0,) + blk + (3,), dtype=torch.float32, device=dev) if self._has_colour else None

    @property
    def n_blocks(self) -> int:
        return int(self.block_coords.shape[0])

    @property
    def memory_bytes(self) -> int:
        """The bytes of the state: table, coordinates and voxel arrays."""
        return sum(t.numel() * t.element_size() for t in (self.block_of, self.block_coords, self.tsdf, self.weight, self.colour) if t is not None)

    def _allocate(self, d: torch.Tensor, k: torch.Tensor, e: torch.Tensor) -> int:
        marks = torch.zeros(self.block_dims, dtype=torch.uint8, device=self.device)
        lib.tsdf_sparse_mark(marks, self.origin, self.voxel_length, self.sdf_trunc, d, mark_cameras(k, e).to(self.device))
        new = marks.bool() & (self.block_of < 0)
        coords = torch.nonzero(new)                               # ascending C order; its size is the one host read
        n_new, n_old = int(coords.shape[0]), self.n_blocks
        if n_new == 0:
            return 0
        if (n_old + n_new) * BLOCK ** 3 >= LIMIT:
            raise ValueError(f"{n_old + n_new} blocks of {BLOCK}^3 voxels exceed the 2^31 limit")
        self.block_of[new] = torch.arange(n_old, n_old + n_new, dtype=torch.int32, device=self.device)
        self.block_coords = torch.cat([self.block_coords, coords.to(torch.int32)])
        blk = (n_new,) + (BLOCK,) * 3
        self.tsdf = torch.cat([self.tsdf, torch.zeros(blk, dtype=torch.float32, device=self.device)])
        self.weight = torch.cat([self.weight, torch.zeros(blk, dtype=torch.float32, device=self.device)])
        if self.colour is not None:
            self.colour = torch.cat([self.colour, torch.zeros(blk + (3,), dtype=torch.float32, device=self.device)])
        return n_new

    def allocate(self, depth, intrinsics, pose) -> int:
        """Opens the blocks near the back-projected points of the views (arguments as ``integrate``) -> the number of new blocks."""
        d, _, k, e = self._views(depth, intrinsics, pose, None, False)
        return self._allocate(d.to(self.device, torch.float32).contiguous(), k, e)

    def integrate(self, depth, intrinsics, pose, rgb=None, allocate: bool = True) -> None:
        """``TSDFVolume.integrate``'s arguments.  First opens the blocks of all its views (unless ``allocate=False``), then applies all
        its views, in index order, to EVERY block allocated so far — one pass over the blocks, whatever V is."""
        self._integrate_prepared(*self._views(depth, intrinsics, pose, rgb), allocate=allocate)

    def _integrate_prepared(self, d, c, k, e, allocate: bool = True) -> None:
        """``integrate`` of views that ``_views`` (or a caller with the same checks) has passed."""
        dev = self.device
        d = d.to(dev, torch.float32).contiguous()
        if allocate:
            self._allocate(d, k, e)
        if self.n_blocks == 0:
            return
        lib.tsdf_sparse_integrate(self.tsdf, self.weight, self.colour, self.block_coords, self.dims, self.origin, self.voxel_length,
                                  self.sdf_trunc, d, None if c is None else _rgb_bytes(c, dev), k.to(dev), e.to(dev))

    def extract_mesh(self):
        """-> (vertices float64 [n,3], faces int64 [m,3], 0-based) on the device: blocks in id order, cells in local C order, vertices
        numbered by first appearance, each with the dense extraction's position bits."""
        if self.n_blocks == 0:
            return geomargs.empty_mesh(self.device)
        return lib.tsdf_sparse_extract(self.tsdf, self.weight, None, self.block_of, self.block_coords, self.dims, self.origin, self.voxel_length)

    def extract_coloured_mesh(self):
        """``extract_mesh`` of a volume with colour -> (vertices, faces, colours float64 [n,3] in [0,1])."""
        if self.colour is None:
            raise ValueError("extract_coloured_mesh needs a volume with colour (SparseTSDFVolume(..., colour=True))")
        if self.n_blocks == 0:
            return geomargs.empty_mesh(self.device) + (torch.empty(0, 3, dtype=torch.float64, device=self.device),)
        return lib.tsdf_sparse_extract(self.tsdf, self.weight, self.colour, self.block_of, self.block_coords, self.dims, self.origin,
                                       self.voxel_length)

    def to_dense(self):
        """-> (tsdf, weight[, colour]) as [nx,ny,nz] (colour [nx,ny,nz,3]) device tensors, absent voxels zero — for tests and small
        scenes: a lattice of 2^31 voxels or more is refused."""
        nx, ny, nz = self.dims
        if nx * ny * nz >= LIMIT:
            raise ValueError(f"to_dense: a lattice of {nx} x {ny} x {nz} voxels exceeds the 2^31 limit")
        nb = self.block_dims
        bi, bj, bk = (self.block_coords[:, c].long() for c in range(3))

        def spread(blocks, tail=()):
            out = torch.zeros((nb[0], BLOCK, nb[1], BLOCK, nb[2], BLOCK) + tail, dtype=blocks.dtype, device=self.device)
            out[bi, :, bj, :, bk, :] = blocks
            return out.reshape((nb[0] * BLOCK, nb[1] * BLOCK, nb[2] * BLOCK) + tail)[:nx, :ny, :nz].contiguous()

        dense = (spread(self.tsdf), spread(self.weight))
        return dense if self.colour is None else dense + (spread(self.colour, (3,)),)


def depth_bounds(depths: torch.Tensor, k: torch.Tensor, poses: torch.Tensor) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
    """min / max (float64 [3] each, host) of the valid depth points of depths[V,H,W] back-projected through fx fy cx cy and the
    camera-to-world poses — torch on the depth maps' device; None when no pixel is valid."""
    dev = depths.device
    v, h, w = depths.shape
    k = k.to(dev, torch.float64)
    p = poses.to(dev, torch.float64)
    lo = torch.full((3,), float("inf"), dtype=torch.float64, device=dev)
    hi = -lo
    uu = torch.arange(w, dtype=torch.float64, device=dev)[None, :]
    vv = torch.arange(h, dtype=torch.float64, device=dev)[:, None]
    for i in range(v):
        d = depths[i].to(torch.float64)
        valid = d > 0
        if not bool(valid.any()):
            continue
        cam = torch.stack([(uu - k[i, 2]) / k[i, 0] * d, (vv - k[i, 3]) / k[i, 1] * d, d], dim=-1)[valid]      # [n,3]
        world = cam @ p[i, :3, :3].T + p[i, :3, 3]
        lo, hi = torch.minimum(lo, world.min(dim=0).values), torch.maximum(hi, world.max(dim=0).values)
    if not bool(torch.isfinite(lo).all()):
        return None
    return lo.cpu(), hi.cpu()


def bounds_box(bounds, vl: float, sparse: bool = False):
    """(min[3], max[3]) -> (origin float64 [3], dims): ceil(extent / voxel_length) voxels per axis, at least one.  ``sparse``: the dims
    are held to the block-sparse volume's limits, not to the dense volume's 2^31 voxels."""
    if len(bounds) != 2:
        raise ValueError("bounds must be (min[3], max[3])")
    lo, hi = (np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64).reshape(-1) for b in bounds)
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all()) or not (hi > lo).all():
        raise ValueError(f"bounds must be two finite [3] corners with max > min, got {bounds!r}")
    extent = (hi - lo) / vl
    if not (extent < LIMIT).all():
        raise ValueError(f"a box of {extent} voxels exceeds the 2^31 limit")
    return lo, (_check_sparse_dims if sparse else _check_dims)(tuple(max(1, int(math.ceil(float(x)))) for x in extent))


_box = bounds_box          # (the name before it became public)


def fuse_depth_maps(depths, intrinsics, poses, bounds=None, voxel_length: float = VOXEL_LENGTH, sdf_trunc: float = SDF_TRUNC, device=None,
                    sparse: bool = False):
    """Depth maps [V,H,W] (or one [H,W]) with their cameras -> (vertices, faces): one volume, one integration pass, one extraction.
    ``bounds`` = (min[3], max[3]) of the box; None: the min / max of the back-projected valid depth points, padded by ``sdf_trunc``.
    The box is covered by ceil(extent / voxel_length) voxels per axis (at least one).  ``sparse=True`` fuses into a
    ``SparseTSDFVolume`` over the same box and lattice — held to its limits, not to 2^31 voxels — and returns its mesh."""
    return _fuse_maps(depths, None, intrinsics, poses, bounds, voxel_length, sdf_trunc, device, sparse)


def fuse_rgbd_maps(depths, colours, intrinsics, poses, bounds=None, voxel_length: float = VOXEL_LENGTH, sdf_trunc: float = SDF_TRUNC,
                   device=None, sparse: bool = False):
    """``fuse_depth_maps`` with the views' images ``colours`` (uint8 [V,H,W,3] / [H,W,3], or float32 in [0, 1] quantised as the PNG is)
    -> (vertices, faces, vertex_colours float64 [n,3] in [0,1]); the vertices and faces are ``fuse_depth_maps``' for the same depths.
    ``sparse`` as in ``fuse_depth_maps``."""
    if colours is None:
        raise ValueError("colours is required (fuse_depth_maps fuses depth alone)")
    return _fuse_maps(depths, colours, intrinsics, poses, bounds, voxel_length, sdf_trunc, device, sparse)


def _fuse_maps(depths, colours, intrinsics, poses, bounds, voxel_length, sdf_trunc, device, sparse=False):
    vl, tr = geomargs.positive32(voxel_length, "voxel_length"), geomargs.positive32(sdf_trunc, "sdf_trunc")
    d = _stack_depths(depths, "depths")
    v = d.shape[0]
    c = None if colours is None else _stack_rgb(colours, d.shape, "colours")
    k = split_intrinsics(intrinsics, v)
    e = extrinsics_from_poses(poses, v)
    _check_depth_values(d, "depths")                           # (on whatever device the maps live)
    box = None if bounds is None else bounds_box(bounds, vl, sparse)         # every refusal that needs no device comes before the device is asked for
    dev = geomargs.device(device if device is not None else (d.device if d.is_cuda else None), "TSDF fusion")
    d = d.to(dev, torch.float32).contiguous()
    if box is None:
        p = geomargs.as_tensor(poses, "poses").cpu()
        found = depth_bounds(d, k, p.unsqueeze(0) if p.dim() == 2 else p)
        if found is None:
            return geomargs.empty_mesh(dev) + (() if c is None else (torch.empty(0, 3, dtype=torch.float64, device=dev),))
        box = bounds_box((found[0].numpy() - tr, found[1].numpy() + tr), vl, sparse)
    vol = (SparseTSDFVolume if sparse else TSDFVolume)(box[0], box[1], voxel_length=vl, sdf_trunc=tr, device=dev, colour=c is not None)
    vol._integrate_prepared(d, c, k, e)                        # (the views were checked above, under this function's argument names)
    return vol.extract_mesh() if c is None else vol.extract_coloured_mesh()


@torch.no_grad()
def render_depth_maps(model, poses, intrinsics, height: int, width: int, epoch: int, split_size: int = 512, white: bool = False,
                      n_streams: int = 2, min_chunk: Optional[int] = None) -> torch.Tensor:
    """Every pixel of every view rendered as ``evaluator.render_view`` renders it (``VectorFieldNerf.render_chunked`` with sparse
    colours, chunks of max(split_size, min_chunk) rays) -> depth maps [V,height,width] float32 that stay on the device."""
    return _render_maps(model, poses, intrinsics, height, width, epoch, split_size, white, n_streams, min_chunk, False)[0]


@torch.no_grad()
def render_rgbd_maps(model, poses, intrinsics, height: int, width: int, epoch: int, split_size: int = 512, white: bool = False,
                     n_streams: int = 2, min_chunk: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``render_depth_maps`` keeping the rgb ``render_chunked`` returns next to the depth -> (depth maps [V,height,width] float32, images
    [V,height,width,3] uint8 — ``metrics2d.quantize_rgb8``: the bytes of the PNG ``render_images`` writes), both on the device.  The
    depth maps are ``render_depth_maps``' for the same random stream."""
    from . import metrics2d
    depth, rgb = _render_maps(model, poses, intrinsics, height, width, epoch, split_size, white, n_streams, min_chunk, True)
    return depth, metrics2d.quantize_rgb8(rgb, device=depth.device)


def _render_maps(model, poses, intrinsics, height, width, epoch, split_size, white, n_streams, min_chunk, keep_rgb):
    from . import evaluator
    p = geomargs.as_tensor(poses, "poses").to(torch.float32)
    p = p.unsqueeze(0) if p.dim() == 2 else p
    if p.dim() != 3 or tuple(p.shape[1:]) != (4, 4):
        raise ValueError(f"poses must be [V,4,4], got {tuple(p.shape)}")
    v = p.shape[0]
    k = geomargs.as_tensor(intrinsics, "intrinsics").to(torch.float32)
    if k.dim() == 2:
        k = k.unsqueeze(0).expand(v, -1, -1)
    if k.dim() != 3 or k.shape[0] != v or tuple(k.shape[1:]) not in ((3, 3), (4, 4)):
        raise ValueError(f"intrinsics must be [3,3], [4,4] or one of those per view ({v}), got {tuple(k.shape)}")
    if k.shape[1] == 3:
        k4 = torch.eye(4).repeat(v, 1, 1)
        k4[:, :3, :3] = k.cpu()
        k = k4
    if height < 1 or width < 1:
        raise ValueError(f"bad image size {height} x {width}")
    dev = geomargs.device(getattr(model.config.cuda_config, "device", None), "TSDF fusion")
    vv, uu = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32), indexing="ij")
    uv = torch.stack([uu.reshape(-1), vv.reshape(-1)], dim=1).to(dev)
    chunk = max(int(split_size), int(evaluator.MIN_CHUNK if min_chunk is None else min_chunk))
    out = torch.empty(v, height, width, dtype=torch.float32, device=dev)
    images = torch.empty(v, height, width, 3, dtype=torch.float32, device=dev) if keep_rgb else None
    keep = getattr(model, "sparse_colours", False)
    model.sparse_colours = bool(evaluator.SPARSE_COLOURS) or keep
    try:
        for i in range(v):
            rgb, depth = model.render_chunked(p[i].to(dev), uv, k[i].to(dev), epoch, chunk=chunk, n_streams=n_streams, white=white)
            out[i] = depth.reshape(height, width)
            if keep_rgb:
                images[i] = rgb.reshape(height, width, 3)
    finally:
        model.sparse_colours = keep
    return out, images


@torch.no_grad()
def fuse_rendered_views(model, poses, intrinsics, height: int, width: int, epoch: int, bounds=None, voxel_length: float = VOXEL_LENGTH,
                        sdf_trunc: float = SDF_TRUNC, as_reference: bool = True, depth_scale: float = DEPTH_SCALE,
                        depth_trunc: float = DEPTH_TRUNC, split_size: int = 512, white: bool = False, n_streams: int = 2,
                        min_chunk: Optional[int] = None, sparse: bool = False):
    """render-images -> tsdf-mesh in one call: the model's views (camera-to-world ``poses`` [V,4,4], ``intrinsics`` shared or per view)
    rendered at ``height`` x ``width``, their depth maps — as ``tsdf_mesh`` stores them when ``as_reference`` (``reference_depth``) —
    fused into a volume over ``bounds`` and triangulated.  The depth maps never leave the device; -> (vertices, faces).

    A rendered depth below zero (compositing can leave one on a ray without a surface) is no measurement and becomes 0 — where the
    reference's unchecked uint16 cast in practice wraps it past ``depth_trunc``, which zeroes it too.  Non-finite depths are refused.
    ``sparse`` as in ``fuse_depth_maps``."""
    depths = render_depth_maps(model, poses, intrinsics, height, width, epoch, split_size=split_size, white=white, n_streams=n_streams,
                               min_chunk=min_chunk)
    depths = torch.where(depths < 0, torch.zeros_like(depths), depths)
    if as_reference:
        depths = reference_depth(depths, depth_scale=depth_scale, depth_trunc=depth_trunc)
    return fuse_depth_maps(depths, intrinsics, poses, bounds=bounds, voxel_length=voxel_length, sdf_trunc=sdf_trunc, device=depths.device,
                           sparse=sparse)


@torch.no_grad()
def fuse_rendered_rgbd(model, poses, intrinsics, height: int, width: int, epoch: int, bounds=None, voxel_length: float = VOXEL_LENGTH,
                       sdf_trunc: float = SDF_TRUNC, as_reference: bool = True, depth_scale: float = DEPTH_SCALE,
                       depth_trunc: float = DEPTH_TRUNC, split_size: int = 512, white: bool = False, n_streams: int = 2,
                       min_chunk: Optional[int] = None, sparse: bool = False):
    """``fuse_rendered_views`` with colour: the same arguments and the same depth handling, the rendered rgb kept as the PNG's bytes
    (``render_rgbd_maps``) and fused with the depth -> (vertices, faces, vertex_colours).  The vertices and faces are
    ``fuse_rendered_views``' for the same random stream; ``ply.write_ply`` writes the result as the reference's ``tsdf.ply``.
    ``sparse`` as in ``fuse_depth_maps``."""
    depths, images = render_rgbd_maps(model, poses, intrinsics, height, width, epoch, split_size=split_size, white=white, n_streams=n_streams,
                                      min_chunk=min_chunk)
    depths = torch.where(depths < 0, torch.zeros_like(depths), depths)
    if as_reference:
        depths = reference_depth(depths, depth_scale=depth_scale, depth_trunc=depth_trunc)
    return fuse_rgbd_maps(depths, images, intrinsics, poses, bounds=bounds, voxel_length=voxel_length, sdf_trunc=sdf_trunc, device=depths.device,
                          sparse=sparse)
