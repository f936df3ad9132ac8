"""Decimating a triangle mesh to a face count on the device: quadric edge collapse (csrc/vfn_collapse.hip, csrc/vfn_collapse_core.h;
include/vfn.h has the specification).  What the reference asks of trimesh in ``get_dominant_bases``
(``mesh.simplify_quadratic_decimation(decimation * len(mesh.faces))``, utils/utils.py:227), for which ``meshops.simplify_to_faces`` is a
stand-in by vertex clustering.

* ``simplify_edge_collapse`` — the call: rounds of ``collapse_round`` until the face count is at or below ``target_faces``, no edge may
  collapse within ``max_error``, or ``max_rounds`` rounds have run.
* ``collapse_round`` — one round, a pure function of (positions, faces, the remaining budget): planes of the faces and of the boundary
  edges, a quadric per vertex, per edge the minimiser of the two ends' quadrics with its cost and a flip test over both 1-rings, a
  selection of edges whose 1-rings share no moving vertex, and of those the cheapest the budget needs.

A round-based, memoryless quadric-error decimation AS SPECIFIED BY US, not verified against trimesh / Open3D: it is NOT the serial
priority-queue order of those libraries.  Known limit of the specification: the link condition is not tested, so a collapse may make
two faces name the same vertex set; the later one is then dropped by the duplicate rule (``meshops.remove_duplicate_faces``), nothing
else guards against it.  tests/collapse_restatement.py restates the contract in NumPy twice and the device is held to it bit for bit.

Inputs are numpy arrays or torch tensors on any device; a mesh is a ``mesh.Mesh`` or a ``(vertices, faces)`` pair.  Outputs are device
tensors.  No CPU fallback: ``lib.VfnError`` when no device is visible.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import geomargs, lib, voxel

MAX_ROUNDS = 256


class Collapsed(NamedTuple):
    """What ``simplify_edge_collapse`` returns: device tensors, except the last three."""
    vertices: torch.Tensor                     # [V',3] float64: the vertices some remaining face names, in the input's order
    faces: torch.Tensor                        # [m',3] int64: the remaining faces over the output vertices, in the input's order and winding
    kept_faces: torch.Tensor                   # [m'] int64: the faces of the INPUT they are
    inverse: torch.Tensor                      # [n] int64: input vertex -> output vertex along the collapse chain; -1 where nothing is left
    colours: Optional[torch.Tensor]            # [V',3] float64, interpolated along every collapsed edge; None when not given
    normals: Optional[torch.Tensor]            # [V',3] float64, likewise, NOT made unit vectors again; None when not given
    cost: torch.Tensor                         # [V'] float64: the largest collapse cost the vertex has absorbed; +0.0 if none
    rounds: int                                # rounds run
    collapsed: int                             # edges collapsed
    reached: bool                              # m' <= target_faces; always False without a target


class Round(NamedTuple):
    """What ``collapse_round`` returns: device tensors, except the last."""
    planes: torch.Tensor                       # [m + B,5] float64: the face planes, then the boundary planes in ascending edge key
    edge_a: torch.Tensor                       # [E] int64: the unique undirected edges (a < b) in ascending key a n + b
    edge_b: torch.Tensor
    run: torch.Tensor                          # [E] int64: the corner pairs that hold the edge (1: boundary, 2: manifold, more: neither)
    item_row: torch.Tensor                     # [k] int64: every vertex's plane rows, ascending
    start: torch.Tensor                        # [n + 1] int64
    quadrics: torch.Tensor                     # [n,10] float64
    point: torch.Tensor                        # [E,3] float64: where the collapse of the edge would put its vertex
    cost: torch.Tensor                         # [E] float64, >= +0.0
    s: torch.Tensor                            # [E] float64 in [0, 1]: the attribute parameter from a to b
    flags: torch.Tensor                        # [E] uint8: ``lib.COLLAPSE_*``; bit 1 = a candidate
    best_edge: torch.Tensor                    # [n] int64: the edge every vertex chose; ``lib.COLLAPSE_NO_EDGE`` where none
    proposed: torch.Tensor                     # [E] bool: both ends chose it
    withdrawn: torch.Tensor                    # [E] bool: a face saw it beside a lower proposal
    taken: torch.Tensor                        # [E] bool: proposed, not withdrawn, and inside the budget
    n_taken: int                               # host: how many


def _check_real(x, name: str, none_ok: bool = False) -> Optional[float]:
    if x is None and none_ok:
        return None
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(float(x)) or float(x) < 0:
        raise ValueError(f"{name} must be {'None or ' if none_ok else ''}a finite number >= 0, got {x!r}")
    return float(x)


def _check_arguments(target_faces, max_error, boundary_weight, rcond, reach, max_rounds):
    from . import meshops
    target = None if target_faces is None else geomargs.positive_int(target_faces, "target_faces")
    max_error = _check_real(max_error, "max_error", none_ok=True)
    if target is None and max_error is None:
        raise ValueError("at least one of target_faces and max_error must be given")
    reach = _check_real(reach, "reach")
    if not math.isfinite(reach * reach):
        raise ValueError(f"reach must have a finite square, got {reach!r}")
    return target, max_error, _check_real(boundary_weight, "boundary_weight"), meshops._check_rcond(rcond), reach, \
        geomargs.positive_int(max_rounds, "max_rounds")


def collapse_round(vertices: torch.Tensor, faces: torch.Tensor, origin, target_faces: Optional[int] = None, max_error: Optional[float] = None,
                   boundary_weight: float = 1.0, rcond: float = 1e-9, reach: float = 2.0) -> Round:
    """One round (include/vfn.h, steps 1 to 5) on device tensors: ``vertices`` [n,3] float64, ``faces`` [m,3] int64 with m >= 1, none naming
    a vertex twice and no two one vertex set, every index in [0, n) (the caller's: ``simplify_edge_collapse`` cleans first), ``origin`` three
    host floats.  Without ``target_faces`` every edge that stays is taken.  Nothing is applied: the positions and the faces are read only.
    One host read: the four status words with the number of taken edges.  The edges and the items come from torch's sorts; the planes,
    the quadrics, the candidates and the selection are the unit's kernels."""
    v, f = vertices, faces
    if not (v.is_cuda and f.is_cuda and v.dtype == torch.float64 and f.dtype == torch.int64 and v.dim() == 2 and f.dim() == 2
            and v.shape[1] == 3 and f.shape[1] == 3 and f.shape[0] >= 1 and v.shape[0] >= 1 and len(origin) == 3):
        raise ValueError("collapse_round: vertices must be float64 [n,3] and faces int64 [m,3] with m >= 1, on the device, and origin three values")
    dev, n, m = v.device, v.shape[0], f.shape[0]
    v, f = v.contiguous(), f.contiguous()
    limit = math.inf if max_error is None else float(max_error)
    with torch.cuda.device(dev):
        info = torch.zeros(5, dtype=torch.int64, device=dev)          # a word per stage, then the number of taken edges
        face_planes = lib.face_planes(v, f, origin, info=info[0:1])
        # the unique undirected edges, in ascending key, with the length of their runs
        first_end = torch.cat((f[:, 0], f[:, 1], f[:, 2]))
        second_end = torch.cat((f[:, 1], f[:, 2], f[:, 0]))
        keys, order = torch.sort(torch.minimum(first_end, second_end) * n + torch.maximum(first_end, second_end), stable=True)
        edge_key, run = torch.unique_consecutive(keys, return_counts=True)
        n_edges = int(edge_key.shape[0])
        edge_a = torch.div(edge_key, n, rounding_mode="floor")
        edge_b = (edge_key - edge_a * n).contiguous()
        edge_a = edge_a.contiguous()
        run = run.contiguous()
        boundary = torch.nonzero(run == 1).reshape(-1)                # ascending edge: ascending key
        n_boundary = int(boundary.shape[0])
        rows = m + n_boundary
        face = torch.arange(m, dtype=torch.int64, device=dev)
        item_keys = [f[:, 0] * rows + face, f[:, 1] * rows + face, f[:, 2] * rows + face]
        planes = face_planes
        if n_boundary:
            pair = order[(torch.cumsum(run, dim=0) - run)[boundary]]  # the one corner pair of every boundary edge
            along = lib.boundary_planes(v, face_planes, (pair % m).contiguous(), first_end[pair].contiguous(), second_end[pair].contiguous(),
                                        origin, boundary_weight, info=info[1:2])
            planes = torch.cat((face_planes, along)).contiguous()
            row = m + torch.arange(n_boundary, dtype=torch.int64, device=dev)
            item_keys += [edge_a[boundary] * rows + row, edge_b[boundary] * rows + row]
        item_key = torch.sort(torch.cat(item_keys))[0]                # ascending (vertex, row); every key once
        item_vertex = torch.div(item_key, rows, rounding_mode="floor")
        item_row = (item_key - item_vertex * rows).contiguous()
        start = torch.searchsorted(item_vertex, torch.arange(n + 1, dtype=torch.int64, device=dev)).contiguous()
        quadrics = lib.vertex_quadrics(planes, item_row, start, info=info[2:3])
        point, cost, s, flags = lib.edge_collapse_candidates(v, f, quadrics, item_row, start, rows, edge_a, edge_b, run, origin, rcond, reach, limit,
                                                             info=info[2:3])
        best_edge, proposed, withdrawn = lib.collapse_select(cost, flags, edge_a, edge_b, f, n, info=info[3:4])
        proposed, withdrawn = proposed != 0, withdrawn != 0
        # the budget: the edges that stay, ascending by (cost, edge); the shortest prefix whose runs add up to the faces still to go
        stays = torch.nonzero(proposed & ~withdrawn).reshape(-1)
        stays = stays[torch.sort(cost[stays], stable=True)[1]]
        taken = torch.zeros(n_edges, dtype=torch.bool, device=dev)
        if target_faces is None:
            taken[stays] = True
        elif stays.shape[0] and m > int(target_faces):
            removed = torch.cumsum(run[stays], dim=0)
            count = torch.searchsorted(removed, torch.full((1,), m - int(target_faces), dtype=torch.int64, device=dev)) + 1
            taken[stays] = torch.arange(stays.shape[0], dtype=torch.int64, device=dev) < count
        info[4] = taken.sum()
        plane_status, boundary_status, edge_status, select_status, n_taken = (int(x) for x in info.cpu())          # the one read
        lib.collapse_check(plane_status, "edge collapse (face planes)")
        lib.collapse_check(boundary_status, "edge collapse (boundary planes)")
        lib.collapse_check(edge_status, "edge collapse (quadrics and candidates)")
        lib.collapse_check(select_status, "edge collapse (selection)")
    return Round(planes, edge_a, edge_b, run, item_row, start, quadrics, point, cost, s, flags, best_edge, proposed, withdrawn, taken, n_taken)


def simplify_edge_collapse(mesh, target_faces=None, max_error=None, boundary_weight=1.0, rcond=1e-9, reach=2.0, colours=None, normals=None,
                           max_rounds=MAX_ROUNDS, device=None) -> Collapsed:
    """-> ``Collapsed`` on the device: the mesh decimated by quadric edge collapse (csrc/vfn_collapse.hip; include/vfn.h has the
    specification, operation by operation).  At least one of ``target_faces`` (stop at or below that many faces) and ``max_error`` (never
    collapse an edge whose quadric cost exceeds it) must be given; with ``max_error`` alone the call runs until no edge may collapse.

    The faces that name a vertex twice and the later ones of a sorted triple are dropped first (``remove_degenerate_faces``,
    ``remove_duplicate_faces``); the frame's origin is the lower corner of the bounding box of the vertices some face names.  Then
    ROUNDS (``collapse_round``): every face gives its plane, weighted by its area, and every boundary edge a plane through it
    perpendicular to its face, weighted ``boundary_weight`` times that area, so that outlines hold; every vertex adds the quadrics of its
    planes in a fixed order; every edge (a < b) finds the minimiser of Q_a + Q_b by the adjugate — accepted when the determinant exceeds
    ``rcond`` times the cube of the mean diagonal and the minimiser lies within ``reach`` edge lengths of the midpoint, else the best of
    (midpoint, a, b) — and is a candidate unless more than two faces share it, its cost exceeds ``max_error`` or a face of either 1-ring
    would turn over; every vertex chooses its cheapest candidate, an edge both of whose ends chose it is proposed, and a face that sees
    two proposals withdraws the dearer: what stays may be applied at once, in any order.  With a target the cheapest of them that the
    remaining budget needs are taken.  A taken edge moves b onto a at the chosen point; ``colours`` / ``normals`` ([n,3]) are interpolated
    along it, ``cost`` keeps the largest cost a vertex absorbed.  ``faces`` keep the input's order and winding.

    A round-based, memoryless quadric-error decimation AS SPECIFIED BY US, not verified against trimesh / Open3D, and NOT their serial
    priority-queue order.  Known limit: the link condition is not tested — a collapse may make two faces name the same vertex set, and
    the later one is dropped by the duplicate rule.  One host read a round beside those inside torch's compactions.  ValueError before any
    launch on bad arguments; a NaN / inf coordinate raises ``lib.VfnError``.  A mesh without faces returns empty tensors."""
    from . import meshops
    target, max_error, boundary_weight, rcond, reach, max_rounds = _check_arguments(target_faces, max_error, boundary_weight, rcond, reach, max_rounds)
    n_rows = geomargs.check_mesh(mesh, "mesh")[0].shape[0]
    col, nrm = meshops._check_attribute(colours, "colours", n_rows), meshops._check_attribute(normals, "normals", n_rows)
    v, f = meshops._mesh_on_device(mesh, device, "mesh", "edge-collapse decimation")
    dev, n = v.device, v.shape[0]
    with torch.cuda.device(dev):
        extras = [None if x is None else x.to(dev, torch.float64).clone() for x in (col, nrm)]
        f, kept = meshops._without_degenerate(v, f)
        f, sub = meshops._without_duplicates(f)
        kept = kept[sub]
        position = v.clone()
        owner = torch.arange(n, dtype=torch.int64, device=dev)        # where every input vertex has gone
        absorbed = torch.zeros(n, dtype=torch.float64, device=dev)
        rounds = collapsed = 0
        if f.shape[0]:
            origin = voxel.bounding_box(v[meshops._referenced(f, n)])[0]          # (a non-finite coordinate raises here)
        while f.shape[0] and (target is None or f.shape[0] > target) and rounds < max_rounds:
            r = collapse_round(position, f, origin, target, max_error, boundary_weight, rcond, reach)
            rounds += 1
            if r.n_taken == 0:
                break
            edge = torch.nonzero(r.taken).reshape(-1)
            a, b, s = r.edge_a[edge], r.edge_b[edge], r.s[edge][:, None]
            position[a] = r.point[edge]
            for x in extras:
                if x is not None:
                    x[a] = (1.0 - s) * x[a] + s * x[b]
            absorbed[a] = torch.maximum(torch.maximum(absorbed[a], absorbed[b]), r.cost[edge])
            remap = torch.arange(n, dtype=torch.int64, device=dev)
            remap[b] = a
            owner = remap[owner]
            f, sub = meshops._without_degenerate(position, remap[f])
            kept = kept[sub]
            f, sub = meshops._without_duplicates(f)
            kept = kept[sub]
            collapsed += r.n_taken
        used = meshops._referenced(f, n)
        number = torch.where(used, torch.cumsum(used, dim=0) - 1, torch.full((n,), -1, dtype=torch.int64, device=dev))
        out_colours, out_normals = (None if x is None else x[used].contiguous() for x in extras)
        return Collapsed(position[used].contiguous(), number[f].reshape(-1, 3).contiguous(), kept.contiguous(), number[owner].contiguous(),
                         out_colours, out_normals, absorbed[used].contiguous(), rounds, collapsed, target is not None and f.shape[0] <= target)
