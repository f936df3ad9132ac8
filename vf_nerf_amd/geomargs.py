"""The argument checks the geometry units share (``mesh``, ``metrics3d``, ``tsdf``, ``raster``, ``refuse``): what a tensor, a device, a mesh
and a scalar parameter must look like before anything is launched.  Host code only: importable without a device.

Refusals are ``TypeError`` for a wrong container, ``ValueError`` for a wrong shape / dtype / value, and ``lib.VfnError`` for a device that
is not one (the HIP path has no CPU fallback).
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np
import torch

from .lib import VfnError

LIMIT = 1 << 31          # rows, cells, pixels or voxels of one call: the kernels index with int32 counts


def as_tensor(x, name: str) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.detach()
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x))
    raise TypeError(f"{name}: expected a numpy array or a torch tensor, got {type(x).__name__}")


def device(device, what: str) -> torch.device:
    """The device a unit runs on: ``device`` if given (it must be a GPU), else the current one.  ``what`` names the unit in the refusal."""
    if device is not None:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise VfnError(f"{what} runs on the device (no CPU fallback), got device {dev}")
        return dev
    if not torch.cuda.is_available():
        raise VfnError(f"{what} runs on the device (no CPU fallback) and no GPU is visible")
    return torch.device("cuda", torch.cuda.current_device())


def empty_mesh(dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """The mesh of nothing: (vertices float64 [0,3], faces int64 [0,3]) on ``dev``."""
    return torch.empty(0, 3, dtype=torch.float64, device=dev), torch.empty(0, 3, dtype=torch.int64, device=dev)


def check_mesh(m, name: str = "mesh", allow_empty: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """A ``mesh.Mesh`` (its ``vertices_scaled`` are used) or a ``(vertices, faces)`` pair -> (vertices, faces) as given (any device), shapes
    and dtypes checked.  With ``allow_empty`` an empty face or vertex array is a mesh (of nothing)."""
    from .mesh import Mesh                  # (mesh imports this module)
    if isinstance(m, Mesh):
        vertices, faces = m.vertices_scaled, m.faces
    elif isinstance(m, (tuple, list)) and len(m) == 2:
        vertices, faces = m
    else:
        raise TypeError(f"{name}: expected a mesh.Mesh or a (vertices, faces) pair, got {type(m).__name__}")
    v, f = as_tensor(vertices, f"{name} vertices"), as_tensor(faces, f"{name} faces")
    if v.dim() != 2 or v.shape[1] != 3 or not v.dtype.is_floating_point:
        raise ValueError(f"{name} vertices must be floating point [n,3], got {v.dtype} {tuple(v.shape)}")
    if f.dim() != 2 or f.shape[1] != 3 or f.dtype.is_floating_point or f.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError(f"{name} faces must be integers [m,3], got {f.dtype} {tuple(f.shape)}")
    if not allow_empty and (f.shape[0] < 1 or v.shape[0] < 1):
        raise ValueError(f"{name} has no faces" if f.shape[0] < 1 else f"{name} has no vertices")
    if v.shape[0] >= LIMIT or f.shape[0] >= LIMIT:
        raise ValueError(f"{name}: {v.shape[0]} vertices / {f.shape[0]} faces exceed the 2^31 limit")
    return v, f


def positive_int(x, name: str) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or int(x) < 1:
        raise ValueError(f"{name} must be a positive integer, got {x!r}")
    if int(x) >= LIMIT:
        raise ValueError(f"{name} {x} exceeds the 2^31 limit of one call")
    return int(x)


def real32(x, name: str) -> float:
    """A finite real number that is still finite as float32 -> that float32's value."""
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(float(x)):
        raise ValueError(f"{name} must be a finite number, got {x!r}")
    f = float(np.float32(x))
    if not math.isfinite(f):
        raise ValueError(f"{name} = {x!r} is not a finite float32")
    return f


def positive32(x, name: str) -> float:
    """A positive finite number that is still positive and finite as float32 -> that float32's value."""
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(float(x)) or float(x) <= 0:
        raise ValueError(f"{name} must be a positive finite number, got {x!r}")
    f = float(np.float32(x))
    if not (f > 0 and math.isfinite(f)):
        raise ValueError(f"{name} = {x!r} is not a positive float32")
    return f
