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

* ``connected_components`` — what a mesh consists of (csrc/vfn_cc.hip, include/vfn.h): the faces are the nodes, two faces are connected
  when they share an edge (``connectivity="edge"``) or a vertex (``"vertex"``); a concurrent union-find on the device over the sorted
  half-edge keys (the vertex incidences), components numbered in ascending lowest face, with exact face counts and areas added in
  a fixed order.  A specification of ours that follows Open3D's ``cluster_connected_triangles`` and trimesh's ``split`` AS REMEMBERED —
  not verified against either; neither fixes a numbering or an order of summation.  tests/cc_restatement.py restates it in NumPy and
  the device is held to it bit for bit.
* ``filter_components`` — the mesh without its small pieces ("floaters"): by face count, by area, or the k largest.
* ``remove_degenerate_faces`` / ``remove_duplicate_faces`` / ``clean`` — faces that name a vertex twice (or have no area), faces that
  repeat an earlier face's vertex triple, and the four steps in one call.  Torch plumbing, no kernel of their own.
* ``orientation`` / ``orient`` — the faces rewound so that two faces sharing a manifold edge traverse it in opposite directions
  (csrc/vfn_orient.hip, include/vfn.h): the components' union-find with one more bit per node, a parity forest under compare-and-swap,
  exact and independent of the schedule; the sign of every component by its first face, the majority, the enclosed volume or the
  nearest viewpoints; a non-orientable component is reported and left alone.  What the contrastive marching-cubes mesh needs before
  ``vertex_normals`` means anything on it (``mesh.extract_mesh(..., orient=)``).  As specified by us, NOT verified against trimesh's
  ``fix_normals`` or Open3D's ``orient_triangles``; tests/orient_restatement.py restates it in NumPy twice and the device is held to
  it bit for bit.  ``inconsistent_edges`` counts the manifold edges wound the same way from both sides.
* ``simplify_vertex_clustering`` — vertex-clustering simplification (csrc/vfn_simplify.hip, include/vfn.h): the vertices of every
  occupied voxel contracted into one — ``voxel.down_sample``'s cells, numbering and means —, the faces that collapse dropped; with
  ``contraction="quadric"`` a cluster's vertex stands at the minimiser of its faces' plane quadrics (ten sums a cluster added by one
  wave in a fixed order, a 3 x 3 adjugate solve, accepted inside the cell only), so that corners and creases survive.  What the
  reference does before it takes ``vertex_normals`` in ``get_dominant_bases`` (utils/utils.py:216-233).  A specification of ours that
  follows Open3D's ``simplify_vertex_clustering`` (Average / Quadric) AS REMEMBERED — not verified against Open3D or trimesh;
  tests/simplify_restatement.py restates it in NumPy twice and the device is held to it bit for bit.
* ``dominant_bases`` — the reference's ``get_dominant_bases`` (utils/utils.py:216-233) on the device: an optional ``orient``, an optional
  decimation (``simplify_vertex_clustering`` at a voxel edge, or ``simplify_to_faces``: a fixed bisection of the voxel edge towards a
  face count, AS SPECIFIED BY US), ``vertex_normals``, then Lloyd's k-means over them (csrc/vfn_kmeans.hip through ``cluster.kmeans``:
  float64, sums along the fixed tree, bit for bit tests/kmeans_restatement.py), the bases in descending order of their counts.  From
  the same seeds the iteration agrees with scikit-learn's; the seeding is ours and trimesh's edge-collapse decimation is not imitated.
  With the module switch ``DECIMATION = "collapse"`` the decimation is ``simplify_edge_collapse`` instead.
* ``simplify_edge_collapse`` — decimation to a face count by quadric edge collapse (``vf_nerf_amd/decimate.py``, csrc/vfn_collapse.hip,
  include/vfn.h), re-exported here: rounds of plane quadrics per vertex (the faces' and, weighted by ``boundary_weight``, the boundary
  edges'), per edge the minimiser of the two ends' quadrics with a flip test over both 1-rings, a selection of edges whose 1-rings
  share no moving vertex, and of those the cheapest the remaining budget needs.  A round-based, memoryless quadric-error decimation
  AS SPECIFIED BY US, not verified against trimesh / Open3D; tests/collapse_restatement.py restates it in NumPy twice and the device
  is held to it bit for bit.

Inputs are numpy arrays or torch tensors on any device; a mesh is a ``mesh.Mesh`` (its ``vertices_scaled`` are used) or a
``(vertices, faces)`` pair.  Outputs are device tensors.  No CPU fallback: ``lib.VfnError`` when no device is visible.  A face index
outside [0, n) is refused on the host (``ValueError``) before anything is launched.

Out of scope: angle-weighted or uniform vertex normals, signed normal consistency (``vfn_normal_dots`` takes ``fabs`` by contract), filling
holes, trimesh's / Open3D's serial priority-queue edge-collapse order and the link condition, scikit-learn's greedy k-means++ and its
random stream, a scale in ICP.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import cluster, geomargs, lib, voxel

WELD_DIGITS = 8                    # trimesh's merge_vertices default (digits_vertex), as remembered
CONNECTIVITIES = ("edge", "vertex")
SIZES = ("faces", "area")          # what ``keep_largest`` ranks by
REFERENCES = ("first", "majority", "volume", "viewpoints")          # what fixes the sign of an orientation component
CONTRACTIONS = ("average", "quadric")          # where ``simplify_vertex_clustering`` puts a cluster's vertex
DECIMATIONS = ("clustering", "collapse")
# how ``dominant_bases(decimation=)`` reaches its face count: "clustering" (``simplify_to_faces``) or "collapse"
# (``simplify_edge_collapse``).  dropin.install(dominant_bases_decimation=...) sets it.
DECIMATION = "clustering"


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


def _referenced(faces: torch.Tensor, n_vertices: int) -> torch.Tensor:
    """Device faces (any shape, checked) -> used[n] bool: the vertices some face names."""
    used = torch.zeros(n_vertices, dtype=torch.bool, device=faces.device)
    used[faces.reshape(-1)] = True
    return used


def _incidences(faces: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """faces[m,3], m >= 1 -> (vertex, face) of every incidence, each once, ascending by vertex then by face."""
    m = faces.shape[0]
    face = torch.arange(m, dtype=torch.int64, device=faces.device)
    keys = torch.unique(torch.cat([faces[:, 0] * m + face, faces[:, 1] * m + face, faces[:, 2] * m + face]))      # sorted: by vertex, then by face
    rows = torch.div(keys, m, rounding_mode="floor")
    return rows, (keys - rows * m).contiguous()


def _vertex_faces(faces: torch.Tensor, n_vertices: int) -> Tuple[torch.Tensor, torch.Tensor]:
    row_start = torch.zeros(n_vertices + 1, dtype=torch.int64, device=faces.device)
    if faces.shape[0] == 0:
        return row_start, torch.empty(0, dtype=torch.int64, device=faces.device)
    rows, incident = _incidences(faces)
    row_start[1:] = torch.cumsum(torch.bincount(rows, minlength=n_vertices), dim=0)
    return row_start, incident


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
        referenced = torch.nonzero(_referenced(f, n)).reshape(-1)          # ascending vertex index
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


# ------------------------------------------------------------------------------------------------
# connected components (csrc/vfn_cc.hip, include/vfn.h)
# ------------------------------------------------------------------------------------------------
class Components(NamedTuple):
    """What ``connected_components`` returns: device tensors, except ``n_components``."""
    face_label: torch.Tensor                   # [m] int64: the component of every face, components numbered in ascending lowest face
    vertex_label: torch.Tensor                 # [n] int64: the lowest label among the vertex's faces; -1 for a vertex no face names
    n_components: int                          # K (host)
    face_count: torch.Tensor                   # [K] int64, exact
    area: Optional[torch.Tensor]               # [K] float64 in the fixed order of include/vfn.h; None with ``areas=False``
    first_face: torch.Tensor                   # [K] int64: every component's lowest face index, ascending


def _check_connectivity(connectivity) -> str:
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity must be one of {CONNECTIVITIES}, got {connectivity!r}")
    return connectivity


def _check_count(x, name: str, least: int) -> Optional[int]:
    if x is None:
        return None
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not least <= int(x) < geomargs.LIMIT:
        raise ValueError(f"{name} must be None or an integer in [{least}, 2^31), got {x!r}")
    return int(x)


def _check_area(x, name: str) -> Optional[float]:
    if x is None:
        return None
    if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not math.isfinite(float(x)) or float(x) < 0:
        raise ValueError(f"{name} must be None or a finite number >= 0, got {x!r}")
    return float(x)


def _check_filter(min_faces, min_area, keep_largest, by, connectivity):
    if by not in SIZES:
        raise ValueError(f"by must be one of {SIZES}, got {by!r}")
    return (_check_count(min_faces, "min_faces", 0), _check_area(min_area, "min_area"), _check_count(keep_largest, "keep_largest", 1), by,
            _check_connectivity(connectivity))


def component_items(faces: torch.Tensor, n_vertices: int, connectivity: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device faces[m,3] (m >= 1, checked) -> (keys, nodes) as ``lib.cc_union_runs`` takes them, int64: the faces that hold one key stand
    next to each other.  "edge": the first two of ``orient_items`` (its direction bytes are not made).  "vertex": the rows of ``_vertex_faces``, key = the vertex."""
    if connectivity == "vertex":
        return _incidences(faces)
    return _edge_items(faces, n_vertices, False)[:2]


def _label_segments(face_label: torch.Tensor, face_count: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (order[m], start[K+1]) as ``lib.cc_segment_sums`` takes them: the faces sorted stably by label — a component's faces in
    ascending face index — and where every component's segment starts, the last one's end behind them."""
    order = torch.sort(face_label, stable=True)[1]
    start = torch.cat((torch.zeros(1, dtype=torch.int64, device=face_label.device), torch.cumsum(face_count, dim=0))).contiguous()
    return order, start


def _components(v: torch.Tensor, f: torch.Tensor, connectivity: str, areas: bool) -> Components:
    """Device vertices / faces, checked -> ``Components``.  Two host reads: the number of components (inside ``torch.unique``) and the
    four status words, together."""
    dev, n, m = v.device, v.shape[0], f.shape[0]
    with torch.cuda.device(dev):
        if m == 0:
            none = torch.empty(0, dtype=torch.int64, device=dev)
            return Components(none, torch.full((n,), -1, dtype=torch.int64, device=dev), 0, none.clone(),
                              torch.empty(0, dtype=torch.float64, device=dev) if areas else None, none.clone())
        info = torch.zeros(4, dtype=torch.int64, device=dev)          # a word per stage: the first stage's complaint names the cause
        keys, nodes = component_items(f, n, connectivity)
        parent = torch.arange(m, dtype=torch.int32, device=dev)
        lib.cc_union_runs(keys, nodes, parent, info=info[0:1])
        root = lib.cc_flatten(parent, info=info[1:2])
        first_face, face_label = torch.unique(root, return_inverse=True)          # ascending root: the numbering.  The read for K.
        k = int(first_face.shape[0])
        vertex_label = torch.full((n,), k, dtype=torch.int64, device=dev).scatter_reduce(0, f.reshape(-1), face_label.repeat_interleave(3),
                                                                                        reduce="amin")
        vertex_label = torch.where(vertex_label == k, torch.full_like(vertex_label, -1), vertex_label)
        face_count = torch.bincount(face_label, minlength=k)
        area = None
        if areas:
            per_face = lib.tri_areas(v, f, info=info[2:3])
            order, start = _label_segments(face_label, face_count)
            area = lib.cc_segment_sums(per_face[order].contiguous(), start, info=info[3:4])
        unions, chains, triangles, sums = (int(x) for x in info.cpu())          # the one read of the status words
        lib.cc_check(unions, "connected components (unions)")
        lib.cc_check(chains, "connected components (flatten)")
        lib.tri_areas_check(triangles, n)
        lib.cc_check(sums, "connected components (areas)")
    return Components(face_label, vertex_label, k, face_count, area, first_face)


def connected_components(mesh, connectivity: str = "edge", areas: bool = True, device=None) -> Components:
    """-> ``Components`` on the device.  The nodes are the faces; with ``connectivity="edge"`` two faces are connected when they share an
    undirected edge {a, b}, a != b (a corner pair that names one vertex twice is no edge; an edge shared by three or more faces
    connects them all), with ``"vertex"`` when they name a common vertex.  The root of a component is its lowest face index and the
    components are numbered 0..K-1 in ascending root: ``first_face`` holds the roots, ``face_label`` every face's number,
    ``vertex_label`` the lowest label among a vertex's faces (-1: no face names it), ``face_count`` the exact counts and ``area`` the
    ``vfn_tri_areas`` values of a component's faces in ascending face index, added in the fixed order of include/vfn.h
    (vfn_cc_segment_sums: 64 strided serial sums, then a fold by halves).  No output depends on the schedule of the union-find.
    Follows Open3D's ``cluster_connected_triangles`` and trimesh's ``split`` as remembered; not verified against either."""
    connectivity = _check_connectivity(connectivity)
    if not isinstance(areas, (bool, np.bool_)):
        raise ValueError(f"areas must be a bool, got {areas!r}")
    v, f = _mesh_on_device(mesh, device, "mesh", "connected components")
    return _components(v, f, connectivity, bool(areas))


def _keep_mask(c: Components, min_faces, min_area, keep_largest, by) -> torch.Tensor:
    """-> keep[K] bool: count >= min_faces, area >= min_area, and among the ``keep_largest`` greatest by ``by`` (ties to the lower label:
    a stable descending sort)."""
    keep = torch.ones(c.n_components, dtype=torch.bool, device=c.face_label.device)
    if min_faces is not None:
        keep &= c.face_count >= min_faces
    if min_area is not None:
        keep &= c.area >= min_area
    if keep_largest is not None and c.n_components:
        size = c.face_count if by == "faces" else c.area
        top = torch.zeros_like(keep)
        top[torch.sort(size, descending=True, stable=True)[1][:keep_largest]] = True
        keep &= top
    return keep


def _select_faces(v: torch.Tensor, f: torch.Tensor, face_keep: torch.Tensor):
    """The faces of the mask in their order, the vertices they name in their order and bits -> (vertices, faces, kept_faces, inverse)."""
    kept_faces = torch.nonzero(face_keep).reshape(-1)
    kept = f[kept_faces]
    used = _referenced(kept, v.shape[0])
    inverse = torch.where(used, torch.cumsum(used, dim=0) - 1, torch.full((v.shape[0],), -1, dtype=torch.int64, device=v.device))
    return v[used].contiguous(), inverse[kept].reshape(-1, 3).contiguous(), kept_faces, inverse


def _filter(v, f, min_faces, min_area, keep_largest, by, connectivity, areas: bool = False):
    """The checked arguments on device tensors -> (``filter_components``' tuple, the ``Components``, keep[K])."""
    c = _components(v, f, connectivity, areas or min_area is not None or (keep_largest is not None and by == "area"))
    keep = _keep_mask(c, min_faces, min_area, keep_largest, by)
    with torch.cuda.device(v.device):
        return _select_faces(v, f, keep[c.face_label]), c, keep


def filter_components(mesh, min_faces=None, min_area=None, keep_largest=None, by: str = "faces", connectivity: str = "edge", device=None):
    """-> (vertices float64 [V',3], faces int64 [m',3], kept_faces int64 [m'], inverse int64 [n]) on the device: the mesh without the
    components that fail a criterion.  A component stays if its face count is >= ``min_faces`` and its area is >= ``min_area``; with
    ``keep_largest=k`` it must also be among the k greatest of ALL components by ``by`` ("faces" or "area"), ties going to the lower
    label.  The faces that stay keep their order, ``kept_faces`` names them in the input; vertices that no remaining face names are
    dropped, the others keep their order and bits; ``inverse`` maps every input vertex to its output vertex or -1, as ``weld``'s —
    colours and normals follow by indexing with ``inverse >= 0``.  With every criterion None: the mesh less its unreferenced vertices.
    Components are ``connected_components``' (its caveats apply)."""
    min_faces, min_area, keep_largest, by, connectivity = _check_filter(min_faces, min_area, keep_largest, by, connectivity)
    v, f = _mesh_on_device(mesh, device, "mesh", "component filtering")
    return _filter(v, f, min_faces, min_area, keep_largest, by, connectivity)[0]


# ------------------------------------------------------------------------------------------------
# orientation (csrc/vfn_orient.hip, include/vfn.h)
# ------------------------------------------------------------------------------------------------
class Orientation(NamedTuple):
    """What ``orientation`` returns: device tensors, except ``n_components`` and ``inconsistent_edges``."""
    flip: torch.Tensor                         # [m] bool: the faces whose columns 1 and 2 change places
    face_label: torch.Tensor                   # [m] int64: the orientation component of every face, numbered in ascending lowest face
    n_components: int                          # K (host)
    first_face: torch.Tensor                   # [K] int64: every component's lowest face index, ascending
    face_count: torch.Tensor                   # [K] int64, exact
    orientable: torch.Tensor                   # [K] bool: False for a component whose constraints contradict each other (left as it is)
    flipped_count: torch.Tensor                # [K] int64: the faces of the component that ``flip`` names
    inconsistent_edges: int                    # the manifold edges of the INPUT whose two faces traverse them the same way (host)
    votes: Optional[torch.Tensor]              # [K] float64: the vote sums of "volume" / "viewpoints"; None otherwise


def _check_reference(reference, viewpoints):
    """The checks of ``reference`` / ``viewpoints`` that need no device -> (reference, viewpoints tensor or None, wherever it is)."""
    if reference not in REFERENCES:
        raise ValueError(f"reference must be one of {REFERENCES}, got {reference!r}")
    if reference != "viewpoints":
        if viewpoints is not None:
            raise ValueError(f"viewpoints are taken with reference='viewpoints' only, not with {reference!r}")
        return reference, None
    if viewpoints is None:
        raise ValueError("reference='viewpoints' needs viewpoints [C,3]")
    p = geomargs.as_tensor(viewpoints, "viewpoints")
    if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1 or not p.dtype.is_floating_point:
        raise ValueError(f"viewpoints must be floating point [C,3] with C >= 1, got {p.dtype} {tuple(p.shape)}")
    if not p.is_cuda and not bool(torch.isfinite(p).all()):          # (on the device the vote kernel's status word says so: no read here)
        raise ValueError("viewpoints: a non-finite coordinate")
    return reference, p


def orient_items(faces: torch.Tensor, n_vertices: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Device faces[m,3] (m >= 1, checked) -> (keys, nodes, dirs) as ``lib.orient_union_runs`` takes them: the 3m half-edges a -> b —
    all (0,1), then all (1,2), then all (2,0) — with key = min * n + max (-1 where both ends are one vertex: no edge), sorted stably
    by torch, each with its face and the direction byte (a < b).  The first two are ``component_items``' "edge" items."""
    return _edge_items(faces, n_vertices, True)


def _edge_items(faces: torch.Tensor, n_vertices: int, dirs: bool):
    """``orient_items``; without ``dirs`` the direction bytes are not made (None)."""
    m = faces.shape[0]
    a = torch.cat((faces[:, 0], faces[:, 1], faces[:, 2]))
    b = torch.cat((faces[:, 1], faces[:, 2], faces[:, 0]))
    keys = torch.where(a == b, torch.full_like(a, -1), torch.minimum(a, b) * n_vertices + torch.maximum(a, b))
    keys, order = torch.sort(keys, stable=True)
    nodes = torch.arange(m, dtype=torch.int64, device=faces.device).repeat(3)[order].contiguous()
    return keys, nodes, (a < b)[order].to(torch.uint8).contiguous() if dirs else None


def manifold_mask(keys: torch.Tensor, nodes: torch.Tensor, dirs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k items of ``orient_items`` -> (manifold[k-1], same_way[k-1]), bool, over the ADJACENT item pairs (i, i + 1): whether the pair
    is a manifold edge — a run of exactly two equal keys >= 0 whose items belong to two faces nodes[i] != nodes[i + 1] — and whether its
    two half-edges run the same way, the parity the edge asks for between the faces.  Masks over all pairs, nothing compacted: no
    host read."""
    same = (keys[1:] == keys[:-1]) & (keys[1:] >= 0)
    manifold = same & (nodes[1:] != nodes[:-1])
    manifold[1:] &= ~same[:-1]                 # the run does not begin earlier ...
    manifold[:-1] &= ~same[1:]                 # ... and does not go on
    return manifold, dirs[1:] == dirs[:-1]


def _count_by_label(face_label: torch.Tensor, flags: torch.Tensor, k: int) -> torch.Tensor:
    """-> [k] int64: how many of the flagged entries carry each label.  Exact integer additions (``torch.bincount`` would read its
    input's maximum on the host).  With few labels every addition would land on the same few words, so each label gets ``spread`` words
    (a power of two chosen on the host from k alone, at most 2^22 words in all), entry i adds into word i % spread of its label, and the
    words of a label are added at the end."""
    spread = 1 << max(0, min(8, 22 - int(k).bit_length()))
    dev = face_label.device
    words = face_label * spread + (torch.arange(face_label.shape[0], dtype=torch.int64, device=dev) & (spread - 1))
    return torch.zeros(k * spread, dtype=torch.int64, device=dev).scatter_add_(0, words, flags.to(torch.int64)).view(k, spread).sum(dim=1)


def _orientation(v: torch.Tensor, f: torch.Tensor, reference: str, viewpoints: Optional[torch.Tensor]) -> Orientation:
    """Device vertices / faces, checked -> ``Orientation``.  Two host reads: the number of components (inside ``torch.unique``), and the
    status words with the count of inconsistent edges, together.  Nothing in between is compacted (no ``nonzero``, no boolean-mask
    indexing, no ``bincount``): the pair test runs over the masks of all adjacent items."""
    dev, m = v.device, f.shape[0]
    if m >= lib.ORIENT_NODE_LIMIT:
        raise ValueError(f"orientation: {m} faces; one call takes fewer than 2^30 (a forest word holds the parent shifted by one bit)")
    with torch.cuda.device(dev):
        if m == 0:
            none = torch.empty(0, dtype=torch.int64, device=dev)
            no = torch.empty(0, dtype=torch.bool, device=dev)
            return Orientation(no, none, 0, none.clone(), none.clone(), no.clone(), none.clone(), 0,
                               torch.empty(0, dtype=torch.float64, device=dev) if reference in ("volume", "viewpoints") else None)
        info = torch.zeros(4, dtype=torch.int64, device=dev)          # a word per stage: the first stage's complaint names the cause
        keys, nodes, dirs = orient_items(f, v.shape[0])
        forest = torch.arange(0, 2 * m, 2, dtype=torch.int32, device=dev)          # x << 1: every face a root, parity 0
        lib.orient_union_runs(keys, nodes, dirs, forest, info=info[0:1])
        root, parity = lib.orient_flatten(forest, info=info[1:2])
        first_face, face_label, face_count = torch.unique(root, return_inverse=True, return_counts=True)   # ascending root: the numbering.  The read for K.
        k = int(first_face.shape[0])
        # the conflict test: a manifold edge whose two faces' parities do not differ as it asks makes its component non-orientable
        manifold, want = manifold_mask(keys, nodes, dirs)
        a, b = nodes[:-1], nodes[1:]
        wrong = manifold & (((parity[a] ^ parity[b]) != 0) != want)
        orientable = _count_by_label(face_label[a], wrong, k) == 0
        parity = torch.where(orientable[face_label], parity, torch.zeros_like(parity)).contiguous()
        sign = torch.zeros(k, dtype=torch.bool, device=dev)
        votes = None
        if reference == "majority":
            sign = 2 * _count_by_label(face_label, parity, k) > face_count                        # exact; a tie keeps the root's winding
        elif reference in ("volume", "viewpoints"):
            per_face = lib.orient_votes(v, f, parity, lib.ORIENT_VOLUME if reference == "volume" else lib.ORIENT_VIEWPOINTS, viewpoints,
                                        info=info[2:3])
            order, start = _label_segments(face_label, face_count)
            votes = lib.cc_segment_sums(per_face[order].contiguous(), start, info=info[3:4])
            sign = (votes < 0) & orientable
        flip = (parity != 0) ^ sign[face_label]
        flipped_count = _count_by_label(face_label, flip, k)
        unions, chains, faces_status, sums, inconsistent = (int(x) for x in torch.cat((info, (manifold & want).sum().reshape(1))).cpu())   # the one read
        lib.orient_check(unions, "orientation (unions)")
        lib.orient_check(chains, "orientation (flatten)")
        lib.orient_check(faces_status, "orientation (votes)")
        lib.cc_check(sums, "orientation (vote sums)")
    return Orientation(flip, face_label, k, first_face, face_count, orientable, flipped_count, inconsistent, votes)


def _rewind(f: torch.Tensor, flip: torch.Tensor) -> torch.Tensor:
    """faces with the columns 1 and 2 of the flipped faces exchanged; column 0 stays."""
    return torch.stack((f[:, 0], torch.where(flip, f[:, 2], f[:, 1]), torch.where(flip, f[:, 1], f[:, 2])), dim=1).contiguous()


def orientation(mesh, reference: str = "first", viewpoints=None, device=None) -> Orientation:
    """-> ``Orientation`` on the device: which faces to rewind so that two faces that share a manifold edge traverse it in opposite
    directions (csrc/vfn_orient.hip; include/vfn.h has the specification).  A manifold edge is an undirected edge held by exactly two
    half-edges of two different faces; boundary edges, edges of three or more faces and corner pairs naming one vertex twice impose
    nothing and connect nothing, so the orientation components are in general finer than ``connected_components("edge")``.  Components
    are numbered in ascending lowest face (``first_face``).  A component whose constraints contradict each other (a Möbius strip) has
    ``orientable`` False and none of its faces in ``flip``.  ``reference`` chooses the sign of every orientable component:
    ``"first"`` — its lowest face keeps its winding; ``"majority"`` — the sign that flips fewer faces, the lowest face keeping its winding
    on a tie; ``"volume"`` — the sign that makes six times the signed volume, sum of v0 . (v1 x v2), not negative: meaningful for CLOSED
    pieces only; ``"viewpoints"`` with ``viewpoints[C,3]`` — the sign that turns the faces' normals towards their nearest viewpoint, summed
    over the component.  The vote sums (``votes``) are float64, added in the fixed order of ``vfn_cc_segment_sums``; no output depends
    on the schedule of the union-find.  ``inconsistent_edges`` counts the manifold edges of the input whose two faces traverse them the
    same way.  As specified by us, not verified against trimesh's ``fix_normals`` or Open3D's ``orient_triangles``."""
    reference, viewpoints = _check_reference(reference, viewpoints)
    v, f = _mesh_on_device(mesh, device, "mesh", "mesh orientation")
    if viewpoints is not None:
        viewpoints = viewpoints.to(v.device, torch.float64).contiguous()
    return _orientation(v, f, reference, viewpoints)


def orient(mesh, reference: str = "first", viewpoints=None, device=None) -> Tuple[torch.Tensor, torch.Tensor, Orientation]:
    """-> (vertices float64 [n,3], faces int64 [m,3], ``Orientation``) on the device: the mesh with the faces ``orientation`` names
    rewound — their columns 1 and 2 exchanged, column 0, the order of the faces and the vertices as they were."""
    reference, viewpoints = _check_reference(reference, viewpoints)
    v, f = _mesh_on_device(mesh, device, "mesh", "mesh orientation")
    if viewpoints is not None:
        viewpoints = viewpoints.to(v.device, torch.float64).contiguous()
    o = _orientation(v, f, reference, viewpoints)
    with torch.cuda.device(v.device):
        return v, _rewind(f, o.flip), o


def inconsistent_edges(mesh, device=None) -> int:
    """-> how many manifold edges of the mesh are traversed the same way by their two faces (0: consistently wound wherever that means
    anything).  Torch plumbing over the sorted half-edges: no kernel, one host read after the index check of the input."""
    v, f = _mesh_on_device(mesh, device, "mesh", "counting inconsistent edges")
    if f.shape[0] == 0:
        return 0
    with torch.cuda.device(v.device):
        manifold, same_way = manifold_mask(*orient_items(f, v.shape[0]))
        return int((manifold & same_way).sum())


def remove_degenerate_faces(mesh, zero_area: bool = False, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (faces int64 [m',3], kept_faces int64 [m']) on the device: without the faces that name a vertex twice and, with
    ``zero_area=True``, without those whose ``face_normals(normalise=False)`` is (0, 0, 0).  The others keep their order."""
    if not isinstance(zero_area, (bool, np.bool_)):
        raise ValueError(f"zero_area must be a bool, got {zero_area!r}")
    v, f = _mesh_on_device(mesh, device, "mesh", "removing degenerate faces")
    with torch.cuda.device(v.device):
        return _without_degenerate(v, f, bool(zero_area))


def _without_degenerate(v: torch.Tensor, f: torch.Tensor, zero_area: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``remove_degenerate_faces`` on checked device tensors, the caller's device current (``v`` is read with ``zero_area`` only)."""
    bad = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
    if zero_area and f.shape[0]:
        bad |= (lib.face_normals(v, f, False) == 0).all(dim=1)
    kept = torch.nonzero(~bad).reshape(-1)
    return f[kept].contiguous(), kept


def remove_duplicate_faces(mesh, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (faces int64 [m',3], kept_faces int64 [m']) on the device: of the faces with one sorted vertex triple the lowest face index
    stays, whatever the winding.  The others keep their order."""
    v, f = _mesh_on_device(mesh, device, "mesh", "removing duplicate faces")
    with torch.cuda.device(v.device):
        return _without_duplicates(f)


def _without_duplicates(f: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``remove_duplicate_faces`` on checked device faces, the caller's device current."""
    if f.shape[0] == 0:
        return f, torch.empty(0, dtype=torch.int64, device=f.device)
    triples, triple = torch.unique(torch.sort(f, dim=1)[0], dim=0, return_inverse=True)
    position = torch.arange(f.shape[0], dtype=torch.int64, device=f.device)
    first = torch.full((triples.shape[0],), f.shape[0], dtype=torch.int64, device=f.device).scatter_reduce(0, triple, position, reduce="amin")
    kept = torch.sort(first)[0]
    return f[kept].contiguous(), kept


def clean(mesh, weld_digits=None, degenerate: bool = True, duplicates: bool = True, device=None, **filter_args):
    """``weld`` at ``weld_digits`` (None: no welding), ``remove_degenerate_faces``, ``remove_duplicate_faces``, then ``filter_components``
    with ``filter_args`` -> its tuple (vertices, faces, kept_faces, inverse): ``kept_faces`` names faces of the INPUT, ``inverse`` maps
    the INPUT's vertices (after a weld several of them share an output vertex)."""
    weld_digits = _check_digits(weld_digits)
    for name, flag in (("degenerate", degenerate), ("duplicates", duplicates)):
        if not isinstance(flag, (bool, np.bool_)):
            raise ValueError(f"{name} must be a bool, got {flag!r}")
    unknown = set(filter_args) - {"min_faces", "min_area", "keep_largest", "by", "connectivity"}
    if unknown:
        raise ValueError(f"clean: unknown arguments {sorted(unknown)}")
    checked = _check_filter(filter_args.get("min_faces"), filter_args.get("min_area"), filter_args.get("keep_largest"),
                            filter_args.get("by", "faces"), filter_args.get("connectivity", "edge"))
    v, f = _mesh_on_device(mesh, device, "mesh", "mesh cleaning")
    with torch.cuda.device(v.device):
        first = None
        if weld_digits is not None:
            v, f, first = weld((v, f), weld_digits)
        kept = torch.arange(f.shape[0], dtype=torch.int64, device=v.device)
        if degenerate:
            f, sub = remove_degenerate_faces((v, f))
            kept = kept[sub]
        if duplicates:
            f, sub = remove_duplicate_faces((v, f))
            kept = kept[sub]
        (vertices, faces, sub, inverse), _, _ = _filter(v, f, *checked)
        if first is not None and inverse.shape[0] == 0:
            inverse = torch.full_like(first, -1)
        elif first is not None:
            inverse = torch.where(first >= 0, inverse[first.clamp(min=0)], torch.full_like(first, -1))
        return vertices, faces, kept[sub], inverse


# ------------------------------------------------------------------------------------------------
# vertex-clustering simplification (csrc/vfn_simplify.hip, include/vfn.h)
# ------------------------------------------------------------------------------------------------
class Simplified(NamedTuple):
    """What ``simplify_vertex_clustering`` returns: device tensors, except ``n_clusters``."""
    vertices: torch.Tensor                     # [V',3] float64: one vertex per cluster that a remaining face names, clusters in ascending key
    faces: torch.Tensor                        # [m',3] int64: the remaining faces over the output vertices, in the input's order and winding
    kept_faces: torch.Tensor                   # [m'] int64: the faces of the INPUT they are
    inverse: torch.Tensor                      # [n] int64: input vertex -> output vertex; -1 where dropped, as ``weld``'s
    colours: Optional[torch.Tensor]            # [V',3] float64 plain cluster means; None when not given
    normals: Optional[torch.Tensor]            # [V',3] float64 plain cluster means, NOT made unit vectors again; None when not given
    placed: torch.Tensor                       # [V'] bool: the quadric's minimiser was accepted for this vertex (all False for "average")
    error: torch.Tensor                        # [V'] float64: the quadric's value at the output position; NaN for "average"
    n_clusters: int                            # K (host): the occupied cells, the dropped ones included


def _check_rcond(rcond) -> float:
    if isinstance(rcond, bool) or not isinstance(rcond, (int, float, np.integer, np.floating)) or not math.isfinite(float(rcond)) \
            or not 0.0 <= float(rcond) <= 1.0:
        raise ValueError(f"rcond must be a finite number in [0, 1], got {rcond!r}")
    return float(rcond)


def _check_attribute(x, name: str, n: int) -> Optional[torch.Tensor]:
    if x is None:
        return None
    t = geomargs.as_tensor(x, name)
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError(f"{name} must be real numbers [n,3], got {t.dtype} {tuple(t.shape)}")
    if t.shape[0] != n:
        raise ValueError(f"{name} must have the vertices' {n} rows, got {t.shape[0]}")
    return t


def _cluster_items(f: torch.Tensor, cluster_of_vertex: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Device faces[m,3] (m >= 1) and every vertex's cluster -> (item_face, start[K+1]) as ``lib.cluster_quadrics`` takes them: the
    incidences of ``_incidences`` sorted stably by the vertex's cluster, so that a cluster's items stand in ascending (vertex, face).
    No host read (``searchsorted``, not ``bincount``)."""
    rows, incident = _incidences(f)
    cluster, order = torch.sort(cluster_of_vertex[rows], stable=True)
    start = torch.searchsorted(cluster, torch.arange(k + 1, dtype=torch.int64, device=f.device))
    return incident[order].contiguous(), start.contiguous()


def simplify_vertex_clustering(mesh, voxel_size, contraction: str = "average", colours=None, normals=None, rcond: float = 1e-9,
                               device=None) -> Simplified:
    """-> ``Simplified`` on the device: the vertices of every occupied cell of edge ``voxel_size`` contracted into one, the faces that
    collapse dropped (csrc/vfn_simplify.hip; include/vfn.h has the specification).  Only the vertices some face names take part, as
    in ``weld``; the frame, the cells, the numbering of the clusters (ascending key) and their means are ``voxel.down_sample``'s over
    those vertices.  ``contraction="average"`` puts a cluster's vertex at the mean of its vertices; ``"quadric"`` at the minimiser of
    the area-weighted squared distances from the planes of the faces its vertices belong to — ten sums per cluster added by one wave
    in the fixed order of ``vfn_cc_segment_sums``, the 3 x 3 system solved by the adjugate — where that minimiser is ACCEPTED: the
    determinant exceeds ``rcond`` times the cube of the mean diagonal and the minimiser lies inside the cluster's cell (the in-cell test
    is ours); every other cluster keeps its mean, with the mean's bits.  So corners and creases survive the contraction, and a flat or
    near-singular cluster can never throw its vertex out of its cell.  ``colours`` / ``normals`` ([n,3]) follow as plain cluster means.
    The faces are the input's with every corner replaced by its cluster, less those that name a cluster twice
    (``remove_degenerate_faces``) and the later ones of a sorted triple (``remove_duplicate_faces``); winding and order are untouched,
    clusters that no remaining face names are dropped.  ``"average"`` launches neither kernel of the unit.  A mesh without faces
    returns empty tensors.

    Three host reads of its own a call — the bounding box, the number of clusters with the status of the keys, the final status words —
    beside those inside the compactions it shares with ``weld`` and ``clean`` (``nonzero``, ``unique``).  ValueError before any launch
    on a ``voxel_size`` that is not finite and > 0 with a normal square, an unknown ``contraction``, an ``rcond`` outside [0, 1],
    attributes without the vertices' row count, and a frame wider than 2^21 cells; a NaN / inf coordinate raises ``lib.VfnError``.

    A specification of ours that follows Open3D's ``simplify_vertex_clustering`` (Average / Quadric) AS REMEMBERED, not verified
    against Open3D or trimesh; tests/simplify_restatement.py restates it in NumPy twice and the device is held to it bit for bit."""
    h = voxel.check_voxel_size(voxel_size)
    if contraction not in CONTRACTIONS:
        raise ValueError(f"contraction must be one of {CONTRACTIONS}, got {contraction!r}")
    rcond = _check_rcond(rcond)
    n_rows = geomargs.check_mesh(mesh, "mesh")[0].shape[0]
    col, nrm = _check_attribute(colours, "colours", n_rows), _check_attribute(normals, "normals", n_rows)
    v, f = _mesh_on_device(mesh, device, "mesh", "mesh simplification")
    dev, n, m = v.device, v.shape[0], f.shape[0]
    extras = [None if x is None else x.to(dev, torch.float64).contiguous() for x in (col, nrm)]
    with torch.cuda.device(dev):
        if m == 0 or n == 0:
            none = lambda *shape, dtype=torch.float64: torch.empty(*shape, dtype=dtype, device=dev)          # noqa: E731
            return Simplified(none(0, 3), none(0, 3, dtype=torch.int64), none(0, dtype=torch.int64),
                              torch.full((n,), -1, dtype=torch.int64, device=dev), *(None if x is None else none(0, 3) for x in extras),
                              none(0, dtype=torch.bool), none(0), 0)
        referenced = torch.nonzero(_referenced(f, n)).reshape(-1)          # ascending vertex index
        vr = v[referenced].contiguous()
        origin, _ = voxel.frame(*voxel.bounding_box(vr), h)               # read 1 (a non-finite coordinate raises here)
        info = torch.zeros(4, dtype=torch.int64, device=dev)              # a word per stage: keys, means, planes, quadrics
        keys = lib.voxel_keys(vr, origin, h, info=info[0:1])
        perm, start, cluster_of_referenced, _ = voxel.table(keys, info[0:1])          # read 2: K with the status of the keys
        k = int(start.shape[0]) - 1
        given = [x[referenced] for x in extras if x is not None]
        values = vr if not given else torch.cat([vr] + given, dim=1)
        means = lib.voxel_means(values[perm].contiguous(), start, info=info[1:2])
        cluster_of_vertex = torch.full((n,), -1, dtype=torch.int64, device=dev)
        cluster_of_vertex[referenced] = cluster_of_referenced
        mean_points = means[:, 0:3].contiguous()
        if contraction == "quadric":
            key = keys[perm[start[:-1]]]                                  # every cluster's key: (c_0 << 42) | (c_1 << 21) | c_2
            axis_bits = lib.voxel_limits()[0].bit_length() - 1
            mask = (1 << axis_bits) - 1
            cells = torch.stack((key >> (2 * axis_bits), (key >> axis_bits) & mask, key & mask), dim=1).to(torch.float64)
            centres = ((cells + 0.5) * h + torch.tensor(origin, dtype=torch.float64, device=dev)).contiguous()
            planes = lib.face_planes(v, f, origin, info=info[2:3])
            item_face, item_start = _cluster_items(f, cluster_of_vertex, k)
            position, placed, error = lib.cluster_quadrics(planes, item_face, item_start, centres, mean_points, origin, h, rcond, info=info[3:4])
            placed = placed != 0
        else:
            position = mean_points
            placed = torch.zeros(k, dtype=torch.bool, device=dev)
            error = torch.full((k,), float("nan"), dtype=torch.float64, device=dev)
        # the faces over the clusters, cleaned; kept_faces names faces of the input
        remapped = cluster_of_vertex[f]
        proper, kept = _without_degenerate(position, remapped)
        kept = kept[_without_duplicates(proper)[1]]
        face_keep = torch.zeros(m, dtype=torch.bool, device=dev)
        face_keep[kept] = True
        vertices, faces, kept_faces, cluster_inverse = _select_faces(position, remapped, face_keep)
        stays = cluster_inverse >= 0
        inverse = torch.where(cluster_of_vertex >= 0, cluster_inverse[cluster_of_vertex.clamp(min=0)], torch.full_like(cluster_of_vertex, -1))
        blocks = iter([means[:, c:c + 3][stays].contiguous() for c in range(3, means.shape[1], 3)])
        out_colours, out_normals = (None if x is None else next(blocks) for x in extras)
        _, mean_status, plane_status, quadric_status = (int(x) for x in info.cpu())          # read 3: the final status words
        lib.voxel_check(mean_status, "mesh simplification (means)")
        lib.simplify_check(plane_status, "mesh simplification (planes)")
        lib.simplify_check(quadric_status, "mesh simplification (quadrics)")
    return Simplified(vertices, faces, kept_faces, inverse, out_colours, out_normals, placed[stays], error[stays], k)


BISECTION_STEPS = 16               # candidates ``simplify_to_faces`` evaluates
BISECTION_SPAN_LOG2 = 20           # its finest voxel edge: the largest extent / 2^20 (never evaluated: the first candidate is extent / 2^10)


def simplify_to_faces(mesh, target_faces, contraction: str = "quadric", steps: int = BISECTION_STEPS, device=None) -> Tuple[Simplified, float]:
    """-> (``Simplified``, voxel_size): ``simplify_vertex_clustering`` at a voxel edge chosen so that about ``target_faces`` faces remain.
    AS SPECIFIED BY US, a deterministic stand-in for the reference's edge-collapse decimation to a face count
    (``simplify_quadratic_decimation``, utils/utils.py:227), which stays out of scope: a fixed geometric bisection.  With E the largest
    extent of the bounding box of the vertices some face names, lo = E / 2^20 and hi = E (Python floats); each of the ``steps`` steps
    evaluates the candidate h = sqrt(lo hi) and goes to the coarser half (lo = h) iff its face count is above the target, to the finer
    one (hi = h) otherwise.  Returned is the evaluated candidate with the most faces <= ``target_faces`` — of equals the one evaluated
    first — or, if none qualifies, the coarsest one evaluated.  Every candidate costs the host reads of ``simplify_vertex_clustering``.
    ValueError on a mesh without faces or without extent."""
    target = geomargs.positive_int(target_faces, "target_faces")
    steps = geomargs.positive_int(steps, "steps")
    if contraction not in CONTRACTIONS:
        raise ValueError(f"contraction must be one of {CONTRACTIONS}, got {contraction!r}")
    if geomargs.check_mesh(mesh, "mesh")[1].shape[0] < 1:
        raise ValueError("simplify_to_faces: the mesh has no faces")
    v, f = _mesh_on_device(mesh, device, "mesh", "mesh simplification")
    with torch.cuda.device(v.device):
        used = _referenced(f, v.shape[0])
        lower, upper = voxel.bounding_box(v[used])
    extent = max(hi - lo for lo, hi in zip(lower, upper))
    if not extent > 0:
        raise ValueError("simplify_to_faces: the mesh has no extent")
    lo, hi = extent / 2.0 ** BISECTION_SPAN_LOG2, extent
    fitting, coarsest = None, None          # (faces, h, Simplified)
    for _ in range(steps):
        h = math.sqrt(lo * hi)
        s = simplify_vertex_clustering((v, f), h, contraction)
        count = int(s.faces.shape[0])
        if count > target:
            lo = h
        else:
            hi = h
            if fitting is None or count > fitting[0]:
                fitting = (count, h, s)
        if coarsest is None or h > coarsest[1]:
            coarsest = (count, h, s)
    _, h, s = fitting if fitting is not None else coarsest
    return s, h


# ------------------------------------------------------------------------------------------------
# the dominant directions of a mesh (csrc/vfn_kmeans.hip through vf_nerf_amd/cluster.py)
# ------------------------------------------------------------------------------------------------
class DominantBases(NamedTuple):
    """What ``dominant_bases`` returns: device tensors, except the last six."""
    bases: torch.Tensor                        # [num_bases,3] float64: the k-means centres of the vertex normals, the dominant one first
    counts: torch.Tensor                       # [num_bases] int64: the normals of every base, descending
    labels: torch.Tensor                       # [V] int64: the base of every vertex normal (the vertices some face names, ascending)
    inertia: torch.Tensor                      # [] float64
    n_iter: int
    converged: bool
    n_vertices: int                            # V: the vertices whose normals were clustered
    n_faces: int                               # the faces of the mesh they were taken on (after the simplification, if any)
    voxel_size: Optional[float]                # the voxel edge of the simplification; None without one


def _check_decimation(decimation) -> Optional[float]:
    if decimation is None:
        return None
    if isinstance(decimation, bool) or not isinstance(decimation, (int, float, np.integer, np.floating)) or not 0.0 < float(decimation) <= 1.0:
        raise ValueError(f"decimation must be None or a number in (0, 1], got {decimation!r}")
    return float(decimation)


def dominant_bases(mesh, num_bases, voxel_size=None, decimation=None, orient=None, unit: bool = False, init="farthest", n_init: int = 1,
                   seed=None, max_iter: int = cluster.MAX_ITER, device=None) -> DominantBases:
    """-> ``DominantBases`` on the device: the reference's ``get_dominant_bases`` (utils/utils.py:216-233) — decimate the mesh, take its
    vertex normals, fit k-means to them, return the centres.  The steps: (1) with ``orient`` ("first", "majority" or "volume") the
    faces are rewound consistently first (``orient``: what a contrastive marching-cubes mesh needs before its vertex normals mean
    anything); (2) an optional simplification, by ``voxel_size`` (``simplify_vertex_clustering``, "quadric") or by ``decimation``
    (``simplify_to_faces`` with ``target_faces = floor(decimation * faces)``, at least 1 — or, with the module switch
    ``DECIMATION = "collapse"``, ``simplify_edge_collapse`` at that target, and ``voxel_size`` is then None), not both; (3) ``vertex_normals`` of what is left,
    restricted to the vertices some face names; (4) ``cluster.kmeans`` with ``init`` / ``n_init`` / ``seed`` / ``max_iter``; (5) the bases
    ordered by descending count with a stable sort, so that the dominant one is first, ``labels`` renumbered with them; (6) with
    ``unit=True`` each base divided by its length ``sqrt((x x + y y) + z z)``, a base without length left as it is.

    The k-means is ``cluster.kmeans``' (it agrees with scikit-learn's Lloyd iteration from the same seeds; its seeding is ours, NOT
    scikit-learn's greedy k-means++ nor its random stream), the decimation is vertex clustering AS SPECIFIED BY US, not trimesh's
    edge collapse: the bases are this project's, not a recording of the reference's.  ValueError before any launch on bad arguments and
    on a mesh of which nothing is left to cluster; a NaN / inf coordinate raises ``lib.VfnError``."""
    k, init, n_init, max_iter, seed = cluster.check_arguments(num_bases, init, n_init, max_iter, seed)
    decimation = _check_decimation(decimation)
    h = None if voxel_size is None else voxel.check_voxel_size(voxel_size)
    if h is not None and decimation is not None:
        raise ValueError("dominant_bases takes voxel_size or decimation, not both")
    if orient is not None and orient not in REFERENCES[:3]:
        raise ValueError(f"orient must be None or one of {REFERENCES[:3]}, got {orient!r}")
    if not isinstance(unit, (bool, np.bool_)):
        raise ValueError(f"unit must be a bool, got {unit!r}")
    if DECIMATION not in DECIMATIONS:
        raise ValueError(f"meshops.DECIMATION must be one of {DECIMATIONS}, got {DECIMATION!r}")
    if geomargs.check_mesh(mesh, "mesh")[1].shape[0] < 1:
        raise ValueError("dominant_bases: the mesh has no faces")
    v, f = _mesh_on_device(mesh, device, "mesh", "dominant bases")
    with torch.cuda.device(v.device):
        if orient is not None:
            f = _rewind(f, _orientation(v, f, orient, None).flip)
        if h is not None:
            s = simplify_vertex_clustering((v, f), h, "quadric")
            v, f = s.vertices, s.faces
        elif decimation is not None and DECIMATION == "collapse":
            s = simplify_edge_collapse((v, f), target_faces=max(1, math.floor(decimation * f.shape[0])))
            v, f = s.vertices, s.faces
        elif decimation is not None:
            s, h = simplify_to_faces((v, f), max(1, math.floor(decimation * f.shape[0])))
            v, f = s.vertices, s.faces
        if f.shape[0] < 1:
            raise ValueError(f"dominant_bases: the simplification at voxel edge {h!r} leaves no face")          # (None: by edge collapse)
        used = _referenced(f, v.shape[0])
        normals = vertex_normals((v, f))[used].contiguous()
        km = cluster.kmeans(normals, k, init, n_init, max_iter, seed)
        counts, order = torch.sort(km.counts, descending=True, stable=True)
        rank = torch.empty_like(order)
        rank[order] = torch.arange(k, dtype=torch.int64, device=v.device)
        bases = km.centres[order].contiguous()
        if unit:
            length = torch.sqrt((bases[:, 0] * bases[:, 0] + bases[:, 1] * bases[:, 1]) + bases[:, 2] * bases[:, 2])[:, None]
            bases = torch.where(length > 0, bases / length, bases)
        return DominantBases(bases, counts, rank[km.labels], km.inertia, km.n_iter, km.converged, int(normals.shape[0]), int(f.shape[0]), h)


# decimation to a face count by quadric edge collapse: vf_nerf_amd/decimate.py (which takes its helpers from this module at call time)
from .decimate import Collapsed, collapse_round, simplify_edge_collapse  # noqa: E402,F401
