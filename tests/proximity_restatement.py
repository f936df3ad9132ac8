"""A CPU restatement of the closest point on a triangle mesh (include/vfn.h: vfn_closest_on_triangle, vfn_tri_nearest;
csrc/vfn_proximity_core.h, csrc/vfn_proximity.hip), in float64, twice.

* ``pair_scalar`` / ``brute_scalar`` — the DEFINITION as a plain loop over (query, face) with Python floats (IEEE doubles, one rounding
  an operation): the seven candidates, the clamp, the minimum of (d2, candidate), then over ALL faces the minimum of (d2, face).  No
  grid.  ``pair_scalar(..., candidates=4)`` is the form without the three vertex candidates, kept to show its flaw (P4).
* ``pair_matrix`` / ``brute`` — the same array-wise in numpy, and with it the grid: ``host_grid`` / ``cell_ranges`` (the box over the
  named vertices, the cell ranges and counts), ``grid_counts`` (``n_pairs`` and ``n_large`` for a ``big_face_cells``), and
  ``ring_search`` (which faces rings 0..r hold, the bound after ring r, the ring at which a query stops): the result the ring path
  alone gives, and the NUMBER of leftovers for a ``max_rings``.
* ``exact_sqdist`` — the true squared distance as a ``fractions.Fraction``: the region classification of the closest point on a
  triangle in exact rational arithmetic.

Shared inputs of tests/test_proximity_host.py (CPU) and tests/test_hip_proximity.py (device) are at the end.  Not part of the package."""
from __future__ import annotations

import functools
import math
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import lib, metrics3d  # noqa: E402

GUARD = 2.0 ** -20
SHAVE = 1.0 - 2.0 ** -20
MIN_NORMAL = 2.0 ** -1022
INF = math.inf


# ---------------------------------------------------------------------------------------------------------------------------------
# the pair routine, scalar
# ---------------------------------------------------------------------------------------------------------------------------------
def _sqdist(q, t):
    dx, dy, dz = q[0] - t[0], q[1] - t[1], q[2] - t[2]
    return (dx * dx + dy * dy) + dz * dz


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _clamp(x, lo, hi):
    if not x >= lo:
        x = lo
    if not x <= hi:
        x = hi
    return x


def _segment(q, P, Q):
    d, w = _sub(Q, P), _sub(q, P)
    dd = _dot(d, d)
    t = _dot(w, d) / dd if dd != 0.0 else math.nan          # (the C division by zero gives inf or NaN; neither is looked at)
    if dd == 0.0 or t <= 0.0:
        return P
    if t >= 1.0:
        return Q
    return (P[0] + t * d[0], P[1] + t * d[1], P[2] + t * d[2])


def _side(P1, P2, p, n):
    return _dot(_cross(_sub(P2, P1), _sub(p, P1)), n)


def pair_scalar(q, A, B, C, candidates: int = 7):
    """-> (c: 3 floats, d2, the winning candidate's number 1..7).  ``candidates=4``: without the vertices."""
    q, A, B, C = (tuple(float(x) for x in p) for p in (q, A, B, C))
    lo, hi = list(A), list(A)
    for k in range(3):
        for P in (B, C):
            if P[k] < lo[k]:
                lo[k] = P[k]
        for P in (B, C):
            if P[k] > hi[k]:
                hi[k] = P[k]
    offered = [(1, _segment(q, A, B)), (2, _segment(q, B, C)), (3, _segment(q, C, A))]
    n = _cross(_sub(B, A), _sub(C, A))
    nn = _dot(n, n)
    if nn > 0.0:
        s = _dot(_sub(q, A), n) / nn
        p = (q[0] - s * n[0], q[1] - s * n[1], q[2] - s * n[2])
        if _side(A, B, p, n) >= 0.0 and _side(B, C, p, n) >= 0.0 and _side(C, A, p, n) >= 0.0:
            offered.append((4, p))
    if candidates == 7:
        offered += [(5, A), (6, B), (7, C)]
    best = None
    for number, p in offered:
        c = tuple(_clamp(p[k], lo[k], hi[k]) for k in range(3))
        d2 = _sqdist(q, c)
        if best is None or d2 < best[1]:
            best = (c, d2, number)
    return best


def valid_faces(vertices, faces):
    f = np.asarray(faces, dtype=np.int64)
    return ((f >= 0) & (f < len(vertices))).all(axis=1)


def brute_scalar(queries, vertices, faces):
    """-> (face int64 [n], closest [n,3], sqdist [n]): the definition, pair by pair; a face with an index outside the vertices is no
    face; no face with d2 < +inf: -1, +inf, +inf."""
    q, v, f = np.asarray(queries, dtype=np.float64), np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    ok = valid_faces(v, f)
    face, closest, sqdist = np.full(len(q), -1, dtype=np.int64), np.full((len(q), 3), INF), np.full(len(q), INF)
    for i in range(len(q)):
        for j in range(len(f)):
            if not ok[j]:
                continue
            c, d2, _ = pair_scalar(q[i], v[f[j, 0]], v[f[j, 1]], v[f[j, 2]])
            if d2 < sqdist[i]:
                face[i], closest[i], sqdist[i] = j, c, d2
    return face, closest, sqdist


# ---------------------------------------------------------------------------------------------------------------------------------
# the pair routine, array-wise
# ---------------------------------------------------------------------------------------------------------------------------------
def _adot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _across(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), axis=-1)


def _asegment(q, P, Q):
    d, w = Q - P, q - P
    dd = _adot(d, d)
    t = _adot(w, d) / dd
    first = (dd == 0.0) | (t <= 0.0)
    second = ~first & (t >= 1.0)
    inner = P + t[..., None] * d
    return np.where(first[..., None], P, np.where(second[..., None], Q, inner))


def _aside(P1, P2, p, n):
    return _adot(_across(P2 - P1, p - P1), n)


def pairs_array(q, A, B, C):
    """Broadcasting arrays [..., 3] -> (c [..., 3], d2 [...]) of the pair routine."""
    with np.errstate(all="ignore"):
        lo = np.where(B < A, B, A)
        lo = np.where(C < lo, C, lo)
        hi = np.where(B > A, B, A)
        hi = np.where(C > hi, C, hi)
        n = _across(B - A, C - A)
        nn = _adot(n, n)
        s = _adot(q - A, n) / nn
        foot = q - s[..., None] * n
        inside = (nn > 0.0) & (_aside(A, B, foot, n) >= 0.0) & (_aside(B, C, foot, n) >= 0.0) & (_aside(C, A, foot, n) >= 0.0)
        best_c, best_d2 = None, None
        for p, offered in ((_asegment(q, A, B), None), (_asegment(q, B, C), None), (_asegment(q, C, A), None), (foot, inside),
                           (A, None), (B, None), (C, None)):
            c = np.where(p >= lo, p, lo)
            c = np.where(c <= hi, c, hi)
            c = np.broadcast_to(c, np.broadcast(q, A).shape)
            d = q - c
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            if best_c is None:
                best_c, best_d2 = c.copy(), d2.copy()
                continue
            take = d2 < best_d2
            if offered is not None:
                take &= offered
            best_c = np.where(take[..., None], c, best_c)
            best_d2 = np.where(take, d2, best_d2)
    return best_c, best_d2


def pair_matrix(queries, vertices, faces, chunk: int = 256):
    """-> (c [n,F,3], d2 [n,F]) with d2 = +inf where a face is no face or d2 is not below +inf (such a pair can never win)."""
    q, v, f = np.asarray(queries, dtype=np.float64), np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    ok = valid_faces(v, f)
    tri = v[np.where(ok[:, None], f, 0)]                                   # [F,3,3]
    c, d2 = np.empty((len(q), len(f), 3)), np.empty((len(q), len(f)))
    for a in range(0, len(q), chunk):
        c[a:a + chunk], d2[a:a + chunk] = pairs_array(q[a:a + chunk, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
    d2 = np.where(ok[None, :] & (d2 < INF), d2, INF)
    return c, d2


def _pick(c, d2, allowed=None):
    """Rows of the pair matrix -> (face, closest, sqdist): the lowest face among the least d2 (of the allowed pairs)."""
    m = d2 if allowed is None else np.where(allowed, d2, INF)
    best = m.min(axis=1)
    face = np.where(best < INF, np.argmax(m == best[:, None], axis=1), -1)
    closest = np.where((best < INF)[:, None], c[np.arange(len(c)), np.maximum(face, 0)], INF)
    return face.astype(np.int64), closest, best


def brute(queries, vertices, faces):
    """-> (face, closest, sqdist): the definition, array-wise."""
    return _pick(*pair_matrix(queries, vertices, faces))


# ---------------------------------------------------------------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------------------------------------------------------------
def host_grid(vertices, faces, cells=None):
    """-> (box: 7 floats, dims: 3 ints) of the grid ``metrics3d.triangle_grid`` builds: the box over the vertices that a face names."""
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    named = v[f[valid_faces(v, f)].reshape(-1)]
    lo, hi = named.min(axis=0), named.max(axis=0)
    extent = [float(hi[k]) - float(lo[k]) for k in range(3)]
    cap = lib.icp_grid_limits()[0]
    h = metrics3d.grid_edge(extent, len(f), cells)
    dims = tuple(min(cap, int(math.floor(e / h)) + 1) for e in extent)
    return tuple(float(x) for x in lo) + tuple(float(x) for x in hi) + (h,), dims


def cell_coords(points, box, dims):
    """-> (a float64 [..., 3], c int64 [..., 3]) of include/vfn.h's cell()."""
    lo, hi, h = np.array(box[0:3]), np.array(box[3:6]), np.float64(box[6])
    a = (np.fmin(np.fmax(np.asarray(points, dtype=np.float64), lo), hi) - lo) / h
    c = np.minimum(np.maximum(np.floor(a), 0.0), np.array(dims, dtype=np.float64) - 1.0).astype(np.int64)
    return a, c


def cell_ranges(vertices, faces, box, dims):
    """-> (cell_lo int64 [F,3], cell_hi [F,3], ncells [F]); a face that is none: an empty range and 0."""
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    ok = valid_faces(v, f)
    tri = v[np.where(ok[:, None], f, 0)]
    cell_lo, cell_hi = cell_coords(tri.min(axis=1), box, dims)[1], cell_coords(tri.max(axis=1), box, dims)[1]
    cell_lo, cell_hi = np.where(ok[:, None], cell_lo, 0), np.where(ok[:, None], cell_hi, -1)
    return cell_lo, cell_hi, np.where(ok, np.prod(cell_hi - cell_lo + 1, axis=1), 0)


def grid_counts(ncells, big_face_cells: int):
    """-> (n_pairs, n_large): what ``TriangleGrid`` reports."""
    large = ncells > big_face_cells
    return int(ncells[~large].sum()), int(large.sum())


def ring_search(queries, vertices, faces, box, dims, big_face_cells: int, matrix=None):
    """-> (ring int64 [n], face, closest, sqdist): for every query the ring after which the rule stops it, and the minimum of (d2, face)
    over the large faces and the faces registered in rings 0..ring — what the ring kernel writes when ``max_rings >= ring``.
    ``matrix``: the ``pair_matrix`` of the same inputs, when the caller has it already."""
    q = np.asarray(queries, dtype=np.float64)
    h = float(box[6])
    c, d2 = pair_matrix(q, vertices, faces) if matrix is None else matrix
    cell_lo, cell_hi, ncells = cell_ranges(vertices, faces, box, dims)
    a_q, c_q = cell_coords(q, box, dims)
    top = np.array(dims, dtype=np.int64) - 1
    # the first ring that holds a cell of the face: per axis the distance from the query's cell to the range; a large face: before ring 0
    first = np.maximum(np.maximum(cell_lo[None] - c_q[:, None], c_q[:, None] - cell_hi[None]), 0).max(axis=2)
    first = np.where((ncells > big_face_cells)[None], -1, first)
    first = np.where((ncells > 0)[None], first, np.iinfo(np.int64).max)
    ring = np.empty(len(q), dtype=np.int64)
    for i in range(len(q)):
        f = a_q[i] - c_q[i]
        s = float(np.min(np.fmin(f, np.fmax(1.0 - f, 0.0))))
        cover = int(max(np.max(c_q[i]), np.max(top - c_q[i])))
        seen = first[i] <= cover
        least = np.full(cover + 2, INF)
        np.minimum.at(least, first[i][seen] + 1, d2[i][seen])
        r, best = 0, float(least[0])
        while True:
            best = min(best, float(least[r + 1]))
            if r >= cover:
                break
            rs = float(r) + s
            w = rs * h
            lb = (w * w) * SHAVE
            if rs >= GUARD and lb >= MIN_NORMAL and best < lb:
                break
            r += 1
        ring[i] = r
    return (ring,) + _pick(c, d2, first <= ring[:, None])


def leftovers(ring, max_rings: int) -> int:
    return int((np.asarray(ring) > max_rings).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def exact_sqdist(q, A, B, C) -> Fraction:
    """The true squared distance from q to the (non-degenerate) triangle A B C: the Voronoi regions of the triangle's features, decided
    and evaluated in rational arithmetic (floats are rationals)."""
    q, A, B, C = ([Fraction(float(x)) for x in p] for p in (q, A, B, C))
    sub = lambda a, b: [a[k] - b[k] for k in range(3)]                      # noqa: E731
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]              # noqa: E731
    along = lambda P, d, t: [P[k] + t * d[k] for k in range(3)]             # noqa: E731
    ab, ac, bc = sub(B, A), sub(C, A), sub(C, B)
    ap, bp, cp = sub(q, A), sub(q, B), sub(q, C)
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    if d1 <= 0 and d2 <= 0:
        c = A
    elif d3 >= 0 and d4 <= d3:
        c = B
    elif vc <= 0 and d1 >= 0 and d3 <= 0:
        c = along(A, ab, d1 / (d1 - d3))
    elif d6 >= 0 and d5 <= d6:
        c = C
    elif vb <= 0 and d2 >= 0 and d6 <= 0:
        c = along(A, ac, d2 / (d2 - d6))
    elif va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        c = along(B, bc, (d4 - d3) / ((d4 - d3) + (d5 - d6)))
    else:
        total = va + vb + vc
        c = [A[k] + ab[k] * (vb / total) + ac[k] * (vc / total) for k in range(3)]
    d = sub(q, c)
    return dot(d, d)


def cube_surface_sqdist(q):
    """The squared distance of q [n,3] to the surface of the unit cube [0, 1]^3 in closed form (exact for small dyadic q)."""
    q = np.asarray(q, dtype=np.float64)
    out = np.maximum(np.maximum(-q, q - 1.0), 0.0)
    outside = (out * out).sum(axis=1)
    depth = np.minimum(q, 1.0 - q).min(axis=1)
    return np.where((out > 0).any(axis=1), outside, depth * depth)


# ---------------------------------------------------------------------------------------------------------------------------------
# the shared inputs: name -> (vertices [V,3], faces [F,3], queries [n,3])
# ---------------------------------------------------------------------------------------------------------------------------------
CUBE_V = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])


def soup(n_faces: int, size: float, seed: int, extent: float = 1.0):
    """``n_faces`` separate triangles of edge about ``size`` with their centres uniform in [-extent, extent]^3."""
    g = np.random.default_rng(seed)
    centre = g.uniform(-extent, extent, (n_faces, 1, 3))
    v = (centre + g.uniform(-size, size, (n_faces, 3, 3))).reshape(-1, 3)
    return v, np.arange(3 * n_faces, dtype=np.int64).reshape(-1, 3)


def lattice_queries():
    """The dyadic lattice from -1 to 2 in steps of 1/4: 13^3 queries."""
    t = np.arange(-4, 9) / 4.0
    return np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)


def _special_positions():
    """Two faces that share the edge (0,0,0)-(1,0,0), one in the plane z = 0 and one in the plane y = 0; queries exactly on a vertex, on
    an edge, on the first face's plane inside and outside, and on the bisector plane through the shared edge (y = z: both faces are
    equally far, the lower face wins)."""
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, 0, 1]])
    f = np.array([[0, 1, 2], [1, 0, 3]])
    q = np.array([[0.0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.25, 0, 0], [0.75, 0.5, 0], [0.5, 0.25, 0], [0.5, 0.5, 0], [2.0, 2.0, 0], [-1.0, 0.5, 0],
                  [0.5, -0.5, -0.5], [0.25, -1.0, -1.0], [0.5, 0.25, 0.25], [0.5, 2.0, 2.0], [0.5, -0.25, 0.0]])
    return v, f, q


def _degenerate():
    """Good faces with A = B, three collinear points, A = B = C and a repeated triple among them."""
    v, f = soup(20, 0.2, 3)
    g = np.random.default_rng(4)
    extra = np.array([[0.1, 0.2, 0.3], [0.6, -0.2, 0.1], [0.35, 0.0, 0.2], [-0.5, 0.5, 0.5]])       # [2] is the midpoint of [0], [1]
    n = len(v)
    v = np.concatenate((v, extra))
    f = np.concatenate((f[:10], [[n, n, n + 1], [n, n + 2, n + 1], [n + 3, n + 3, n + 3], list(f[4])], f[10:]))
    return v, f, g.uniform(-1.2, 1.2, (150, 3))


def _spanning():
    """One face from corner to corner of the box over 200 small ones."""
    v, f = soup(200, 0.05, 6)
    n = len(v)
    v = np.concatenate((v, [[-1.1, -1.1, -1.1], [1.1, 1.1, -1.1], [1.1, -1.1, 1.1]]))
    f = np.concatenate((f[:50], [[n, n + 1, n + 2]], f[50:]))
    return v, f, np.random.default_rng(7).uniform(-1.2, 1.2, (200, 3))


def _two_sets():
    """Two clusters of faces far apart, queries around both and between them."""
    v1, f1 = soup(60, 0.05, 8, extent=0.3)
    v2, f2 = soup(60, 0.05, 9, extent=0.3)
    v = np.concatenate((v1, v2 + np.array([6.0, 0.5, -0.25])))
    f = np.concatenate((f1, f2 + len(v1)))
    g = np.random.default_rng(10)
    q = np.concatenate((g.uniform(-0.5, 0.5, (60, 3)), g.uniform(-0.5, 0.5, (60, 3)) + np.array([6.0, 0.5, -0.25]),
                        g.uniform(0.5, 5.5, (40, 1)) * np.array([1.0, 0.1, 0.0])))
    return v, f, q


@functools.lru_cache(maxsize=None)
def cases():
    g = np.random.default_rng(11)
    out = {}
    for n in (1, 63, 64, 65):
        out[f"one_face_{n}_queries"] = (np.array([[0.0, 0, 0], [1, 0.25, 0], [0.25, 1, 0.5]]), np.array([[0, 1, 2]]), g.uniform(-1, 2, (n, 3)))
    for m in (255, 256, 257):
        v, f = soup(m, 0.1, m)
        out[f"{m}_faces_one_query"] = (v, f, np.array([[0.1, -0.2, 0.3]]))
    out["special_positions"] = _special_positions()
    out["degenerate"] = _degenerate()
    out["spanning"] = _spanning()
    out["two_sets"] = _two_sets()
    v, f = soup(150, 0.08, 12)
    q = g.uniform(-1, 1, (120, 3))
    out["soup"] = (v, f, q)
    out["far_queries"] = (v, f, np.concatenate((q[:40] + np.array([12.0, 0, 0]), q[40:80] * 30.0, q[80:] * np.array([1.0, 1e3, 1.0]))))
    out["cube_lattice"] = (CUBE_V, CUBE_F, lattice_queries()[::7])
    return out


def accuracy_pairs():
    """family -> [(q, A, B, C)] for the comparison with ``exact_sqdist``: 100 random pairs, 80 needle-thin triangles (aspect 10^6), 80
    tiny ones (edge 10^-6 at coordinates of order 1), 80 far queries (10^3 edges away), and 60 queries exactly ON a triangle with
    dyadic coordinates (a vertex, an edge's midpoint, an inner point): their exact d2 is 0.  Then the same two questions where rounding
    is live, on the needles and the tiny triangles: "vertex", 80 queries that ARE a vertex in its own bits (exact d2 0), and "near", 80
    rounded midpoints of an edge and rounded inner points (exact d2 positive but at the level of an ulp of the coordinates squared: only
    the absolute error against the squared edge says anything there, ``absolute_error``)."""
    g = np.random.default_rng(2024)
    out = {"random": [tuple(g.uniform(-1, 1, (4, 3))) for _ in range(100)], "needle": [], "tiny": [], "far": [], "on": []}
    for _ in range(80):
        A, d, e = g.uniform(-1, 1, (3, 3))
        across = np.cross(d, e)
        out["needle"].append((A + g.uniform(-1, 1, 3), A, A + d, A + 0.5 * d + 1e-6 * np.linalg.norm(d) * across / np.linalg.norm(across)))
        A, B, C = g.uniform(-1, 1, 3) + 1e-6 * g.uniform(-1, 1, (3, 3))
        out["tiny"].append((A + 1e-6 * g.uniform(-2, 2, 3), A, B, C))
        A, B, C = g.uniform(-1, 1, (3, 3))
        direction = g.normal(size=3)
        out["far"].append((A + 1e3 * direction / np.linalg.norm(direction), A, B, C))
    out["vertex"], out["near"] = [], []
    for k, (_, A, B, C) in enumerate(out["needle"][:40] + out["tiny"][:40]):
        out["vertex"].append(((A, B, C)[k % 3], A, B, C))
        out["near"].append((((A + B) / 2, (B + C) / 2, (A + B + 2 * C) / 4, (2 * A + B + C) / 4)[k % 4], A, B, C))
    for k in range(60):
        A, B, C = g.integers(-1024, 1025, (3, 3)) / 1024.0
        out["on"].append(((A, (A + B) / 2, (A + B + 2 * C) / 4)[k % 3], A, B, C))
    return out


def accuracy_errors(pairs):
    """-> (the largest |d2 - exact| / exact over the pairs with exact > 0, the largest d2 / (the longest edge squared) over the pairs
    with exact == 0), both as floats (0.0 for an empty class)."""
    relative, absolute = 0.0, 0.0
    for q, A, B, C in pairs:
        d2 = Fraction(pair_scalar(q, A, B, C)[1])
        exact = exact_sqdist(q, A, B, C)
        if exact > 0:
            relative = max(relative, float(abs(d2 - exact) / exact))
        else:
            edge = max(_sqdist(A, B), _sqdist(B, C), _sqdist(C, A))
            absolute = max(absolute, float(d2 / Fraction(edge)))
    return relative, absolute


def absolute_error(pairs):
    """-> the largest |d2 - exact| / (the longest edge squared) over ALL the pairs, as a float."""
    worst = 0.0
    for q, A, B, C in pairs:
        edge = max(_sqdist(A, B), _sqdist(B, C), _sqdist(C, A))
        worst = max(worst, float(abs(Fraction(pair_scalar(q, A, B, C)[1]) - exact_sqdist(q, A, B, C)) / Fraction(edge)))
    return worst


GRID_SETTINGS =tuple({"cells": c} for c in (1, 2, 7, 128)) + tuple({"big_face_cells": b} for b in (0, 1, 8, 10 ** 9)) + \
    tuple({"max_rings": r} for r in (0, 1, 8))
