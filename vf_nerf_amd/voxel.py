"""Voxel down-sampling of a point set on the device (csrc/vfn_voxel.hip): the first step of the ``evaluate_3d_reconstruction`` protocol
that the reference's ``metrics_3d`` / ``metrics_3d_no_vf`` call — both clouds are down-sampled before they are registered and before
precision and recall are counted, so that every occupied voxel votes once however many points fell into it.

``down_sample`` (public as ``metrics3d.voxel_down_sample``) replaces the points of every occupied voxel by their mean, and averages
normals and colours with them.  The contract is include/vfn.h's (``vfn_voxel_keys``, ``vfn_voxel_means``):

* the frame, in Python floats: ``origin_k = min_k - 0.5 h`` (Open3D's ``voxel_min_bound``), ``dims_k = floor((max_k - origin_k) / h) + 1``;
* a point's voxel ``c_k = floor((p_k - origin_k) / h)``, its key ``(c_0 << 42) | (c_1 << 21) | c_2``;
* voxels numbered in ascending key, the points of a voxel in ascending original index (a STABLE sort of the keys);
* a mean is the serial sum in that order, started from the first point, over the count.

This is a specification of ours that imitates Open3D's ``voxel_down_sample`` AS REMEMBERED: neither Open3D nor the external package is
available to compare against, and Open3D's hash map fixes no order of summation.  tests/voxel_restatement.py restates the contract in
NumPy and the device is held to it bit for bit.

Inputs are numpy arrays or torch tensors on any device.  No CPU fallback: ``lib.VfnError`` when no device is visible.
"""
from __future__ import annotations

import dataclasses
import functools
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import geomargs, lib
from .geomargs import LIMIT

BOX_TILE = 1024          # rows of a tile of the bounding box's two-step reduction (speed only)
_device = functools.partial(geomargs.device, what="voxel down-sampling")          # (a module attribute, so a test can stand in for the device)


@dataclasses.dataclass
class VoxelDownSample:
    """What ``down_sample`` returns: device tensors, except ``origin`` and ``dims``."""
    points: torch.Tensor                       # [V,3] float64: the mean of every occupied voxel's points, voxels in ascending key
    normals: Optional[torch.Tensor]            # [V,3] plain means, NOT re-normalised (as Open3D averages them); None when not given
    colours: Optional[torch.Tensor]            # [V,3] plain means; None when not given
    counts: torch.Tensor                       # [V] int64: points per voxel
    voxel_of_point: torch.Tensor               # [n] int64: the output row every input point went to
    origin: Tuple[float, float, float]         # host: the lower corner of the points' bounding box less half a voxel
    dims: Tuple[int, int, int]                 # host: voxels per axis of the frame


def check_voxel_size(voxel_size, name: str = "voxel_size") -> float:
    """A finite real number > 0 whose square is a normal float64 -> float."""
    if isinstance(voxel_size, bool) or not isinstance(voxel_size, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a real number, got {voxel_size!r}")
    h = float(voxel_size)
    if not math.isfinite(h) or h <= 0 or not math.isfinite(h * h) or h * h < 2.0 ** -1022:
        raise ValueError(f"{name} must be finite and > 0 with a normal square, got {voxel_size!r}")
    return h


def frame(lower, upper, voxel_size: float):
    """The bounding box's two corners (finite Python floats) and the checked voxel edge -> (origin[3], dims[3]) in host arithmetic:
    origin_k = lower_k - 0.5 h, dims_k = floor((upper_k - origin_k) / h) + 1.  ValueError when an axis needs more than 2^21 voxels."""
    h = float(voxel_size)
    origin = tuple(float(lo) - 0.5 * h for lo in lower)
    cells = [math.floor((float(hi) - o) / h) if math.isfinite((float(hi) - o) / h) else math.inf for hi, o in zip(upper, origin)]
    cap = lib.voxel_limits()[0]
    if any(c + 1 > cap for c in cells):
        raise ValueError(f"voxel_size {h!r}: the bounding box needs {tuple(c + 1 for c in cells)} voxels, more than 2^{cap.bit_length() - 1} "
                         "on an axis; choose a larger voxel")
    return origin, tuple(int(c) + 1 for c in cells)


def _check_rows(x, name: str, n: Optional[int] = None) -> torch.Tensor:
    t = geomargs.as_tensor(x, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be [n,3], got {tuple(t.shape)}")
    if not (t.dtype.is_floating_point or t.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)):
        raise ValueError(f"{name} must be real numbers, got {t.dtype}")
    if t.shape[0] < 1:
        raise ValueError(f"{name} is empty")
    if t.shape[0] >= LIMIT:
        raise ValueError(f"{name}: {t.shape[0]} rows exceed the 2^31 limit of one call")
    if n is not None and t.shape[0] != n:
        raise ValueError(f"{name} must have the points' {n} rows, got {t.shape[0]}")
    return t


def bounding_box(t: torch.Tensor):
    """points [n,3] where they are (any device, any real dtype) -> (lower[3], upper[3]) as Python floats: ONE read when they are on a
    device.  The minimum of the float64 values is the float64 value of the minimum (the conversion is monotonic).  A NaN / inf
    coordinate raises ``lib.VfnError``.  Minima and maxima are exact, so the order they are taken in changes no bit: tiles of
    BOX_TILE rows are reduced first, then the tiles' results (torch's reduction of a tall [n,3] array along its rows in one step
    takes 1.2 ms at 10^6 rows on an MI355X, the two steps 0.06 ms: DESIGN 6q)."""
    lo = hi = t
    whole = t.shape[0] // BOX_TILE * BOX_TILE
    if whole >= 2 * BOX_TILE:
        tiles = t[:whole].reshape(-1, BOX_TILE, 3)
        lo, hi = torch.cat((tiles.amin(dim=1), t[whole:])), torch.cat((tiles.amax(dim=1), t[whole:]))
    box = torch.cat((lo.amin(dim=0), hi.amax(dim=0))).to(torch.float64).cpu().tolist()
    if not all(math.isfinite(b) for b in box):
        lib.voxel_check(lib.GEOM_STATUS_NONFINITE)
    return box[:3], box[3:]


def table(keys: torch.Tensor, info: torch.Tensor):
    """Device keys [n] -> (perm[n], start[V+1], voxel_of_point[n], counts[V]), all int64: a stable sort, a voxel per run of equal keys in
    ascending key, the first sorted position of every voxel and n.  Plumbing in torch, as ``icp.build_grid``'s.  ONE read: the number
    of voxels with the status word of the keys, which is checked here."""
    n = keys.shape[0]
    dev = keys.device
    sorted_key, perm = torch.sort(keys, stable=True)
    voxel_sorted = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(sorted_key[1:] != sorted_key[:-1], dim=0)))
    last, status = (int(x) for x in torch.cat((voxel_sorted[-1:], info.reshape(-1)[:1])).cpu())          # the one read
    lib.voxel_check(status)
    start = torch.searchsorted(voxel_sorted, torch.arange(last + 2, dtype=torch.int64, device=dev)).contiguous()
    voxel_of_point = torch.empty(n, dtype=torch.int64, device=dev)
    voxel_of_point[perm] = voxel_sorted
    return perm, start, voxel_of_point, start[1:] - start[:-1]


def _down(p: torch.Tensor, h: float, origin, dims, extras=(None, None)) -> VoxelDownSample:
    """Device float64 points [n,3] in their frame (and up to two more [n,3] device float64 arrays) -> ``VoxelDownSample``.  The rows are
    gathered ONCE into sorted order by torch, all channels side by side, so that adjacent lanes of the means kernel read adjacent
    segments; its status is not read: the table comes from ``table`` one line above, whose segments are non-empty, ascending and end at
    n by construction."""
    dev = p.device
    with torch.cuda.device(dev):
        info = torch.zeros(1, dtype=torch.int64, device=dev)
        keys = lib.voxel_keys(p, origin, h, info=info)
        perm, start, voxel_of_point, counts = table(keys, info)
        given = [x for x in extras if x is not None]
        values = p if not given else torch.cat([p] + given, dim=1)
        means = lib.voxel_means(values[perm].contiguous(), start, info=torch.zeros(1, dtype=torch.int64, device=dev))
    blocks = iter([means[:, c:c + 3].contiguous() for c in range(0, means.shape[1], 3)])
    mean_points = next(blocks)
    mean_normals, mean_colours = (None if x is None else next(blocks) for x in extras)
    return VoxelDownSample(mean_points, mean_normals, mean_colours, counts, voxel_of_point, tuple(origin), tuple(dims))


def down_sample_device(points: torch.Tensor, voxel_size: float) -> VoxelDownSample:
    """Device float64 points [n,3] and a CHECKED voxel edge -> ``VoxelDownSample`` (what ``metrics3d`` and ``icp.align_stages`` call on the
    clouds they already hold on the device)."""
    origin, dims = frame(*bounding_box(points), voxel_size)
    return _down(points, voxel_size, origin, dims)


def down_sample(points, voxel_size, normals=None, colours=None, device=None) -> VoxelDownSample:
    """points[n,3] -> their ``VoxelDownSample`` at voxel edge ``voxel_size``: one output point per occupied voxel, the mean of the
    voxel's points; ``normals`` / ``colours`` ([n,3] each) are averaged the same way — plain means, a normal is NOT made a unit vector
    again (Open3D averages them so, as remembered).  Voxels in ascending (c_0, c_1, c_2); ``voxel_of_point`` names every input point's
    output row.  Two host reads: the bounding box, then the number of voxels with the status.  ValueError before any launch on a
    ``voxel_size`` that is not finite and > 0 with a normal square, and on a box that needs more than 2^21 voxels on an axis; a NaN / inf
    coordinate raises ``lib.VfnError``."""
    p = _check_rows(points, "points")
    nrm = None if normals is None else _check_rows(normals, "normals", p.shape[0])
    col = None if colours is None else _check_rows(colours, "colours", p.shape[0])
    h = check_voxel_size(voxel_size)
    origin, dims = frame(*bounding_box(p), h)
    dev = _device(device)
    to_dev = lambda t: None if t is None else t.to(dev, torch.float64).contiguous()          # noqa: E731
    return _down(to_dev(p), h, origin, dims, (to_dev(nrm), to_dev(col)))
