"""A CPU restatement of the unbounded nearest-neighbour search (include/vfn.h: vfn_nn_nearest; csrc/vfn_nn.hip), in numpy float64.

* ``brute`` — the DEFINITION: over all targets the minimum of (d2, index); tests/icp_restatement.py's brute force with a radius beyond
  every pair.  It does not know about a grid.
* ``host_grid`` / ``cell_coords`` — the grid ``metrics3d.nearest_grid`` builds, from the same host arithmetic (``metrics3d.grid_edge``)
  and the cell expression of include/vfn.h.
* ``ring_search`` — a model of the ring rule, query by query: which targets rings 0..r hold, the bound after ring r, the ring at which
  the query stops.  From it: the result the ring path alone would give (to be held to ``brute``) and the exact number of leftovers for
  a ``max_rings`` — the contract makes that number a function of the queries, the grid and ``max_rings``.

Shared inputs of tests/test_nn_grid_host.py (CPU) and tests/test_hip_nn_grid.py (device) are at the end.  Not part of the package."""
from __future__ import annotations

import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import icp_restatement as R  # noqa: E402
from vf_nerf_amd import lib, metrics3d  # noqa: E402

BEYOND = 1e150                    # a radius beyond every pair of the tests (its square is finite)
GUARD = 2.0 ** -20                # the least r + s at which the bound is used
SHAVE = 1.0 - 2.0 ** -20
MIN_NORMAL = 2.0 ** -1022


def brute(queries, targets, workers: int = 1):
    """-> (index int64 [n], sqdist [n]): the definition."""
    return R.nearest_within(queries, targets, BEYOND, workers=workers)


def host_grid(targets, cells=None):
    """-> (box: 7 floats, dims: 3 ints) of the grid ``metrics3d.nearest_grid(targets, cells)`` builds."""
    t = np.asarray(targets, dtype=np.float64)
    lo, hi = t.min(axis=0), t.max(axis=0)
    extent = [float(hi[k]) - float(lo[k]) for k in range(3)]
    cap = lib.icp_grid_limits()[0]
    h = metrics3d.grid_edge(extent, len(t), cells)
    dims = tuple(min(cap, int(math.floor(e / h)) + 1) for e in extent)
    return tuple(float(x) for x in lo) + tuple(float(x) for x in hi) + (h,), dims


def cell_coords(points, box, dims):
    """-> (a float64 [n,3], c int64 [n,3]): a = fl(fl(min(max(x, o), e) - o) / h), c = min(max(floor(a), 0), dim - 1)."""
    lo, hi, h = np.array(box[0:3]), np.array(box[3:6]), np.float64(box[6])
    a = (np.minimum(np.maximum(np.asarray(points, dtype=np.float64), lo), hi) - lo) / h
    c = np.minimum(np.maximum(np.floor(a), 0.0), np.array(dims, dtype=np.float64) - 1.0).astype(np.int64)
    return a, c


def ring_search(queries, targets, box, dims):
    """-> (ring int64 [n], index int64 [n], sqdist [n]): for every query the ring after which the rule stops it, and the minimum of
    (d2, index) over the targets of rings 0..ring — what the ring kernel writes when ``max_rings >= ring``."""
    q, t = np.asarray(queries, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    h = float(box[6])
    a_q, c_q = cell_coords(q, box, dims)
    _, c_t = cell_coords(t, box, dims)
    top = np.array(dims, dtype=np.int64) - 1
    ring, index, sqdist = np.empty(len(q), dtype=np.int64), np.empty(len(q), dtype=np.int64), np.empty(len(q))
    for i in range(len(q)):
        f = a_q[i] - c_q[i]
        s = float(np.min(np.minimum(f, np.maximum(1.0 - f, 0.0))))
        cover = int(max(np.max(c_q[i]), np.max(top - c_q[i])))
        cheb = np.abs(c_t - c_q[i]).max(axis=1)                         # the ring of every target
        dx, dy, dz = q[i, 0] - t[:, 0], q[i, 1] - t[:, 1], q[i, 2] - t[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        least = np.full(cover + 1, np.inf)
        np.minimum.at(least, cheb, d2)
        r, best = 0, math.inf
        while True:
            best = min(best, float(least[r]))
            if r >= cover:
                break
            rs = float(r) + s
            w = rs * h
            lb = (w * w) * SHAVE
            if rs >= GUARD and lb >= MIN_NORMAL and best < lb:
                break
            r += 1
        ring[i], sqdist[i] = r, best
        hit = np.flatnonzero((cheb <= r) & (d2 == best))
        index[i] = hit[0] if len(hit) else -1
    return ring, index, sqdist


def leftovers(ring, max_rings: int) -> int:
    """The queries that have not stopped after ring ``max_rings``."""
    return int((np.asarray(ring) > max_rings).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# the shared inputs
# ---------------------------------------------------------------------------------------------------------------------------------
UNIFORM_SIZES = ((1, 1), (3, 7), (1037, 1805), (1024, 8))
MIXED = (1037, 1805)


@functools.lru_cache(maxsize=None)
def uniform_pair(n, m):
    from test_hip_icp import uniform_case
    return uniform_case(n, m)


def far_queries():
    """200 queries of the (1037, 1805) pair moved out of the targets' box: 100 shifted by +12 along x, 100 scaled by 3."""
    q, t = uniform_pair(*MIXED)
    return np.concatenate((q[:100] + np.array([12.0, 0.0, 0.0]), q[100:200] * 3.0)), t


@functools.lru_cache(maxsize=None)
def lattice_ties():
    """The 17^3 lattice of spacing 0.125 with 200 positions stored twice, in reversed order (test_hip_icp.lattice_case) -> (queries,
    targets, n_mid): n_mid queries at the centres of lattice cubes (eight targets at the same distance), then queries on lattice
    points (the duplicated positions among them: two targets at distance 0)."""
    from test_hip_icp import lattice_case
    r, targets, _, _, _, dup = lattice_case(True)
    g = np.random.default_rng(23)
    corner = (g.integers(-8, 8, (300, 3)) * r).astype(np.float64)
    mid = corner + r / 2
    on = np.concatenate((dup, (g.integers(-8, 9, (100, 3)) * r).astype(np.float64)))
    return np.concatenate((mid, on)), targets, len(mid)


def degenerate_cases():
    """name -> (queries, targets): one target; five coincident targets; 500 targets in the plane z = 0.25; the corner room moved."""
    g = np.random.default_rng(5)
    q = g.uniform(-1, 1, (300, 3))
    one = g.uniform(-1, 1, (1, 3))
    plane = g.uniform(-1, 1, (500, 3))
    plane[:, 2] = 0.25
    room = R.corner_room(2000, 4)
    return {"one": (q, one), "coincident": (q, np.repeat(one, 5, axis=0)), "plane": (q, plane),
            "room": (R.corner_room(1500, 3), R.transform(room, R.motion()))}
