"""Normals and welded vertices of a triangle mesh on the device (csrc/vfn_normals.hip, include/vfn.h): what the reference leaves to
Open3D's ``compute_vertex_normals()`` before it writes ``tsdf.ply`` (evaluation/methods.py:664-665) and to trimesh's ``process=True``
when it loads a mesh (methods.py:305).

* ``face_normals`` — the cross product of two edges of every face (its length is twice the area), a unit vector by default; a face
  without area gets (0, 0, 0).
* ``vertex_faces`` — the CSR of every vertex's faces (ascending, each once): torch plumbing, as ``refuse.vertex_adjacency``.
* ``vertex_normals`` — the unnormalised normals of a vertex's faces added in ascending face order, then made a unit vector: area
  weighting, Open3D's ``compute_vertex_normals()`` AS REMEMBERED — not verified against Open3D, whose sums have no fixed order.  A vertex
  without faces (or whose sum has no length) gets (0, 0, 1).
* ``weld`` — vertices with equal coordinates (``digits=None``) or equal ``round_half_even(v * 10**digits)`` merged into the one with the
  lowest index, unreferenced vertices dropped, faces remapped.  A specification of ours that follows trimesh's ``merge_vertices`` AS
  REMEMBERED — not verified against trimesh.  The merge is ``lib.mesh_dedup``'s (csrc/vfn_mesh.hip): no new hash table.

Inputs are numpy arrays or torch tensors on any device; a mesh is a ``mesh.Mesh`` (its ``vertices_scaled`` are used) or a
``(vertices, faces)`` pair.  Outputs are device tensors.  No CPU fallback: ``lib.VfnError`` when no device is visible.  A face index
outside [0, n) is refused on the host (``ValueError``) before anything is launched.

Out of scope: angle-weighted or uniform vertex normals, orienting a mesh, removing degenerate or duplicate faces.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import geomargs, lib

WELD_DIGITS = 8                    # trimesh's merge_vertices default (digits_vertex), as remembered


def _check_indices(f: torch.Tensor, n: int, name: str) -> None:
    """Every face index in [0, n), checked where the faces are (no device is needed for host faces)."""
    if f.numel() and (int(f.min()) < 0 or int(f.max()) >= n):
        raise ValueError(f"{name}: a face index lies outside [0, {n})")


def _check_digits(digits) -> Optional[int]:
    if digits is None:
        return None
    if isinstance(digits, bool) or not isinstance(digits, (int, np.integer)) or not 0 <= int(digits) <= 15:
        raise ValueError(f"digits must be None or an integer in [0, 15], got {digits!r}")
    return int(digits)


def _mesh_on_device(mesh, device, name: str, what: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """The checks that need no device, then (vertices float64, faces int64) contiguous on the device."""
    v, f = geomargs.check_mesh(mesh, name)
    _check_indices(f, v.shape[0], name)
    dev = geomargs.device(device if device is not None else (v.device if v.is_cuda else None), what)
    return v.to(dev, torch.float64).contiguous(), f.to(dev, torch.int64).contiguous()


def face_normals(mesh, normalise: bool = True, device=None) -> torch.Tensor:
    """-> float64 [m,3] on the device: per face c = (v1 - v0) x (v2 - v0), as it is (``normalise=False``: |c| is twice the area) or as
    a unit vector ((0, 0, 0) for a face without area).  A NaN / inf coordinate, or a length that overflows, raises ``lib.VfnError``."""
    if not isinstance(normalise, (bool, np.bool_)):
        raise ValueError(f"normalise must be a bool, got {normalise!r}")
    v, f = _mesh_on_device(mesh, device, "mesh", "face normals")
    return lib.face_normals(v, f, bool(normalise))


def _vertex_faces(faces: torch.Tensor, n_vertices: int) -> Tuple[torch.Tensor, torch.Tensor]:
    m = faces.shape[0]
    row_start = torch.zeros(n_vertices + 1, dtype=torch.int64, device=faces.device)
    if m == 0:
        return row_start, torch.empty(0, dtype=torch.int64, device=faces.device)
    face = torch.arange(m, dtype=torch.int64, device=faces.device)
    keys = torch.unique(torch.cat([faces[:, 0] * m + face, faces[:, 1] * m + face, faces[:, 2] * m + face]))      # sorted: by vertex, then by face
    rows = torch.div(keys, m, rounding_mode="floor")
    row_start[1:] = torch.cumsum(torch.bincount(rows, minlength=n_vertices), dim=0)
    return row_start, (keys - rows * m).contiguous()


def vertex_faces(faces, n_vertices: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """faces[m,3] (integers, every index in [0, n_vertices)) -> the CSR of every vertex's faces (row_start[n+1], incident), int64 on
    faces' device: the keys ``vertex * m + face`` of the three corners through ``torch.unique`` — a vertex's faces in ascending order,
    and a face that names a vertex twice once in that vertex's row."""
    f = geomargs.as_tensor(faces, "faces")
    if f.dim() != 2 or f.shape[1] != 3 or f.dtype.is_floating_point or f.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError(f"faces must be integers [m,3], got {f.dtype} {tuple(f.shape)}")
    if isinstance(n_vertices, bool) or not isinstance(n_vertices, (int, np.integer)) or not 0 <= int(n_vertices) < geomargs.LIMIT:
        raise ValueError(f"n_vertices must be an integer in [0, 2^31), got {n_vertices!r}")
    _check_indices(f, int(n_vertices), "faces")
    return _vertex_faces(f.to(torch.int64), int(n_vertices))


def vertex_normals(mesh, device=None) -> torch.Tensor:
    """-> float64 [n,3] on the device: unit(sum of the unnormalised normals of the vertex's faces, in ascending face order), (0, 0, 1)
    for a vertex without faces.  One read of the status word.  A NaN / inf coordinate or an overflowing length raises ``lib.VfnError``."""
    v, f = _mesh_on_device(mesh, device, "mesh", "vertex normals")
    with torch.cuda.device(v.device):
        info = torch.zeros(2, dtype=torch.int64, device=v.device)          # a word per stage: the first stage's complaint names the cause
        raw = lib.face_normals(v, f, False, info=info[0:1])
        row_start, incident = _vertex_faces(f, v.shape[0])
        out = lib.vertex_normals(raw, row_start, incident, info=info[1:2])
        if v.shape[0]:
            faces_status, vertices_status = (int(x) for x in info.cpu())
            lib.normals_check(faces_status, "vertex normals (face stage)")
            lib.normals_check(vertices_status, "vertex normals")
    return out


def weld(mesh, digits: Optional[int] = WELD_DIGITS, device=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (vertices float64 [V',3], faces int64 [m,3], inverse int64 [n]) on the device.  Only the vertices some face uses take part;
    the others are dropped (``inverse`` -1).  The key of a vertex is its coordinates (``digits=None``; -0.0 equals +0.0) or
    ``round_half_even(v * 10.0**digits)`` per component in float64 (``digits`` an integer in [0, 15]); vertices with equal keys form a
    class whose representative is its lowest vertex index.  The output vertices are the representatives' original bits in ascending
    representative index, ``inverse`` maps every input vertex to its output vertex, and the faces are the input's remapped: same
    count, same order, faces the merge makes degenerate kept.  A non-finite coordinate (or key) is refused (``ValueError``)."""
    digits = _check_digits(digits)
    v, f = _mesh_on_device(mesh, device, "mesh", "vertex welding")
    dev, n = v.device, v.shape[0]
    with torch.cuda.device(dev):
        inverse = torch.full((n,), -1, dtype=torch.int64, device=dev)
        if f.shape[0] == 0 or n == 0:
            return torch.empty(0, 3, dtype=torch.float64, device=dev), f, inverse
        used = torch.zeros(n, dtype=torch.bool, device=dev)
        used[f.reshape(-1)] = True
        referenced = torch.nonzero(used).reshape(-1)                      # ascending vertex index
        vr = v[referenced].contiguous()
        keys = vr if digits is None else torch.round(vr * 10.0 ** digits)
        if not bool(torch.isfinite(keys).all()):
            raise ValueError("weld: a non-finite vertex coordinate (or a key that overflows)")
        _, ids = lib.mesh_dedup(keys.contiguous())                         # class numbers in order of first appearance = ascending representative
        count = int(ids.max()) + 1
        position = torch.arange(referenced.shape[0], dtype=torch.int64, device=dev)
        first = torch.full((count,), referenced.shape[0], dtype=torch.int64, device=dev).scatter_reduce(0, ids, position, reduce="amin")
        inverse[referenced] = ids
        return vr[first].contiguous(), inverse[f].contiguous(), inverse
