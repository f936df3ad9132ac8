"""Quadric edge-collapse decimation (include/vfn.h: vfn_boundary_planes, vfn_vertex_quadrics, vfn_edge_collapse_candidates,
vfn_collapse_select; vf_nerf_amd/decimate.py: collapse_round, simplify_edge_collapse) restated in NumPy from its contract, TWICE, by two
texts that share nothing but the contract:

* ``round_loops`` / ``text="loops"`` — Python floats and Python loops over vertices, edges and faces: a dictionary from an edge to the corner
  pairs that hold it, a list of rows per vertex, the adjugate and the flip test written out for one edge at a time, the choice of every
  vertex and the withdrawal of every face as loops over tuples (cost, edge);
* ``round_arrays`` / ``text="arrays"`` — array-wise: the keys of tests/cc_restatement.py's ``items``, the planes of
  tests/simplify_restatement.py's ``planes_arrays``, every edge's solve on whole arrays, the 1-rings expanded into (edge, face) pairs,
  the selection by lexicographic sorts.

Both return the same dictionaries; tests/test_collapse_host.py holds them against each other bit for bit, round by round and over a
whole call, tests/test_hip_collapse.py holds the device to them.  A round-based, memoryless quadric-error decimation AS SPECIFIED BY US,
not verified against trimesh / Open3D, neither of which is there to compare against.  Not part of the package: tests only."""
import math

import numpy as np

import cc_restatement as CC
import simplify_restatement as SR

CANDIDATE, ACCEPTED, NONMANIFOLD, NONFINITE, OVER, FLIP = 1, 2, 4, 8, 16, 32
NO_EDGE = (1 << 63) - 1
ROUND_FIELDS = ("planes", "edge_a", "edge_b", "run", "item_row", "start", "quadrics", "point", "cost", "s", "flags", "best_edge", "proposed",
                "withdrawn", "taken")
FIELDS = ("vertices", "faces", "kept_faces", "inverse", "colours", "normals", "cost", "rounds", "collapsed", "reached")


# ---------------------------------------------------------------------------------------------------------------------------------
# the first text: loops
# ---------------------------------------------------------------------------------------------------------------------------------
def _div(a, b):
    """IEEE division of two Python floats (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _boundary_plane_loop(pa, pb, plane, origin, weight):
    nf, area = plane[:3], plane[4]
    d = [pb[k] - pa[k] for k in range(3)]
    c = [d[1] * nf[2] - d[2] * nf[1], d[2] * nf[0] - d[0] * nf[2], d[0] * nf[1] - d[1] * nf[0]]
    s = c[0] * c[0]
    s = s + c[1] * c[1]
    s = s + c[2] * c[2]
    r = math.sqrt(s)
    if not (r > 0.0 and math.isfinite(r)):
        return [0.0, 0.0, 0.0, 0.0, 0.0]
    nrm = [c[0] / r, c[1] / r, c[2] / r]
    e = nrm[0] * (pa[0] - origin[0])
    e = e + nrm[1] * (pa[1] - origin[1])
    e = e + nrm[2] * (pa[2] - origin[2])
    return nrm + [e, weight * area]


def _ten_loop(row):
    nx, ny, nz, e, w = row
    wx, wy, wz, we = w * nx, w * ny, w * nz, w * e
    return [wx * nx, wx * ny, wx * nz, wy * ny, wy * nz, wz * nz, -(we * nx), -(we * ny), -(we * nz), we * e]


def _value_loop(s, z):
    p0 = (s[0] * z[0] + s[1] * z[1]) + s[2] * z[2]
    p1 = (s[1] * z[0] + s[3] * z[1]) + s[4] * z[2]
    p2 = (s[2] * z[0] + s[4] * z[1]) + s[5] * z[2]
    return (((z[0] * p0 + z[1] * p1) + z[2] * p2) + 2.0 * ((s[6] * z[0] + s[7] * z[1]) + s[8] * z[2])) + s[9]


def _cross_loop(p0, p1, p2):
    a = [p1[k] - p0[k] for k in range(3)]
    d = [p2[k] - p0[k] for k in range(3)]
    return [a[1] * d[2] - a[2] * d[1], a[2] * d[0] - a[0] * d[2], a[0] * d[1] - a[1] * d[0]]


def _edge_loop(v, f, faces_of, quadrics, origin, a, b, run, rcond, reach, limit):
    """-> (point[3], cost, s, flags) of the edge (a, b)"""
    s = [quadrics[a][c] + quadrics[b][c] for c in range(10)]
    pa, pb = v[a], v[b]
    d = [pb[k] - pa[k] for k in range(3)]
    mid = [0.5 * (pa[k] + pb[k]) for k in range(3)]
    l2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    a00, a01, a02, a11, a12, a22, b0, b1, b2, _ = s
    m00, m01, m02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    m11, m12, m22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = (a00 * m00 + a01 * m01) + a02 * m02
    t = ((a00 + a11) + a22) / 3.0
    accepted = False
    if det > rcond * ((t * t) * t):
        y = [(m00 * b0 + m01 * b1) + m02 * b2, (m01 * b0 + m11 * b1) + m12 * b2, (m02 * b0 + m12 * b1) + m22 * b2]
        x = [-_div(y[k], det) for k in range(3)]
        r = [x[k] - (mid[k] - origin[k]) for k in range(3)]
        accepted = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2] <= (reach * reach) * l2
    if accepted:
        point, value = [origin[k] + x[k] for k in range(3)], _value_loop(s, x)
    else:
        point, value = None, math.nan
        for tried in (mid, pa, pb):
            val = _value_loop(s, [tried[k] - origin[k] for k in range(3)])
            if point is None or val < value:
                point, value = list(tried), val
    cost = value if value > 0.0 else 0.0
    gap = [point[k] - pa[k] for k in range(3)]
    par = _div((gap[0] * d[0] + gap[1] * d[1]) + gap[2] * d[2], l2)
    if not par >= 0.0:
        par = 0.0
    if par > 1.0:
        par = 1.0
    flags = ACCEPTED if accepted else 0
    if run > 2:
        flags |= NONMANIFOLD
    if not all(math.isfinite(x) for x in [value] + point):
        flags |= NONFINITE
    if cost > limit:
        flags |= OVER
    if not flags & (NONMANIFOLD | NONFINITE | OVER):
        keeps = True
        for moving, other in ((a, b), (b, a)):
            for j in faces_of[moving]:
                if not keeps or other in f[j]:
                    continue
                old = _cross_loop(*(v[i] for i in f[j]))
                if old == [0.0, 0.0, 0.0]:
                    continue
                new = _cross_loop(*(point if i == moving else v[i] for i in f[j]))
                if not (old[0] * new[0] + old[1] * new[1]) + old[2] * new[2] > 0.0:
                    keeps = False
        flags |= CANDIDATE if keeps else FLIP
    return point, cost, par, flags


def _pack(n_edges, planes, edges, runs, rows_of, quadrics, results, best, proposed, withdrawn, taken):
    start = np.concatenate(([0], np.cumsum([len(r) for r in rows_of]))).astype(np.int64)
    return {"planes": np.array(planes, dtype=np.float64).reshape(-1, 5), "edge_a": np.array([e[0] for e in edges], dtype=np.int64),
            "edge_b": np.array([e[1] for e in edges], dtype=np.int64), "run": np.array(runs, dtype=np.int64),
            "item_row": np.array([r for rows in rows_of for r in rows], dtype=np.int64), "start": start,
            "quadrics": np.array(quadrics, dtype=np.float64).reshape(-1, 10), "point": np.array([r[0] for r in results], dtype=np.float64).reshape(-1, 3),
            "cost": np.array([r[1] for r in results], dtype=np.float64), "s": np.array([r[2] for r in results], dtype=np.float64),
            "flags": np.array([r[3] for r in results], dtype=np.uint8), "best_edge": np.array(best, dtype=np.int64),
            "proposed": np.array(proposed, dtype=bool).reshape(n_edges), "withdrawn": np.array(withdrawn, dtype=bool).reshape(n_edges),
            "taken": np.array(taken, dtype=bool).reshape(n_edges), "n_taken": int(sum(taken))}


def round_loops(vertices, faces, origin, target_faces=None, max_error=None, boundary_weight=1.0, rcond=1e-9, reach=2.0):
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3).tolist()
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist()
    n, m, origin = len(v), len(f), [float(x) for x in origin]
    limit = math.inf if max_error is None else float(max_error)
    planes = [SR._plane_loop(v[t[0]], v[t[1]], v[t[2]], origin) for t in f]
    holders = {}                                            # an edge -> its corner pairs, in the order all (0,1), all (1,2), all (2,0)
    for c in range(3):
        for j in range(m):
            p, q = f[j][c], f[j][(c + 1) % 3]
            holders.setdefault((min(p, q), max(p, q)), []).append((j, p, q))
    edges = sorted(holders)
    runs = [len(holders[e]) for e in edges]
    faces_of = [[] for _ in range(n)]
    for j, tri in enumerate(f):                             # ascending face in every list
        for i in tri:
            faces_of[i].append(j)
    rows_of = [list(x) for x in faces_of]
    for e in edges:
        if len(holders[e]) == 1:
            j, p, q = holders[e][0]
            for i in e:
                rows_of[i].append(len(planes))
            planes.append(_boundary_plane_loop(v[p], v[q], planes[j], origin, float(boundary_weight)))
    quadrics = []
    for i in range(n):
        s = [0.0] * 10
        for k, row in enumerate(rows_of[i]):
            t = _ten_loop(planes[row])
            s = t if k == 0 else [x + y for x, y in zip(s, t)]
        quadrics.append(s)
    results = [_edge_loop(v, f, faces_of, quadrics, origin, a, b, run, rcond, reach, limit) for (a, b), run in zip(edges, runs)]
    # the selection
    choice = [None] * n
    for e, (a, b) in enumerate(edges):
        if results[e][3] & CANDIDATE:
            for i in (a, b):
                if choice[i] is None or (results[e][1], e) < choice[i]:
                    choice[i] = (results[e][1], e)
    best = [NO_EDGE if c is None else c[1] for c in choice]
    proposed = [bool(results[e][3] & CANDIDATE) and best[a] == e and best[b] == e for e, (a, b) in enumerate(edges)]
    withdrawn = [False] * len(edges)
    for tri in f:
        seen = {(results[best[i]][1], best[i]) for i in tri if best[i] != NO_EDGE and proposed[best[i]]}
        for _, e in sorted(seen)[1:]:
            withdrawn[e] = True
    # the budget
    stays = sorted((results[e][1], e) for e in range(len(edges)) if proposed[e] and not withdrawn[e])
    taken = [False] * len(edges)
    gone = 0
    for _, e in stays:
        if target_faces is not None and gone >= m - target_faces:
            break
        taken[e] = True
        gone += runs[e]
    return _pack(len(edges), planes, edges, runs, rows_of, quadrics, results, best, proposed, withdrawn, taken)


# ---------------------------------------------------------------------------------------------------------------------------------
# the second text: arrays
# ---------------------------------------------------------------------------------------------------------------------------------
def _cross(p0, p1, p2):
    a, d = p1 - p0, p2 - p0
    return np.stack((a[:, 1] * d[:, 2] - a[:, 2] * d[:, 1], a[:, 2] * d[:, 0] - a[:, 0] * d[:, 2], a[:, 0] * d[:, 1] - a[:, 1] * d[:, 0]), axis=1)


def _value(s, z):
    p0 = (s[:, 0] * z[:, 0] + s[:, 1] * z[:, 1]) + s[:, 2] * z[:, 2]
    p1 = (s[:, 1] * z[:, 0] + s[:, 3] * z[:, 1]) + s[:, 4] * z[:, 2]
    p2 = (s[:, 2] * z[:, 0] + s[:, 4] * z[:, 1]) + s[:, 5] * z[:, 2]
    return (((z[:, 0] * p0 + z[:, 1] * p1) + z[:, 2] * p2) + 2.0 * ((s[:, 6] * z[:, 0] + s[:, 7] * z[:, 1]) + s[:, 8] * z[:, 2])) + s[:, 9]


def _lower(cost_x, edge_x, cost_y, edge_y):
    """is (cost_x, edge_x) < (cost_y, edge_y)?"""
    return (cost_x < cost_y) | ((cost_x == cost_y) & (edge_x < edge_y))


def round_arrays(vertices, faces, origin, target_faces=None, max_error=None, boundary_weight=1.0, rcond=1e-9, reach=2.0):
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    n, m, o = len(v), len(f), np.asarray(origin, dtype=np.float64)
    limit = np.inf if max_error is None else float(max_error)
    with np.errstate(all="ignore"):
        face_planes = SR.planes_arrays(v, f, o)
        keys, nodes = CC.items(f, n, "edge")
        edge_key, first, run = np.unique(keys, return_index=True, return_counts=True)
        edge_a, edge_b = edge_key // n, edge_key % n
        n_edges = len(edge_key)
        boundary = np.nonzero(run == 1)[0]
        bface = nodes[first[boundary]]
        # the corner pair of a boundary edge inside its face: the corner after `from` is `to`
        tri = f[bface]
        forward = ((tri == edge_a[boundary, None]) & (np.roll(tri, -1, axis=1) == edge_b[boundary, None])).any(axis=1)
        start_v = np.where(forward, edge_a[boundary], edge_b[boundary])
        end_v = np.where(forward, edge_b[boundary], edge_a[boundary])
        nf, area = face_planes[bface, :3], face_planes[bface, 4]
        d = v[end_v] - v[start_v]
        c = np.stack((d[:, 1] * nf[:, 2] - d[:, 2] * nf[:, 1], d[:, 2] * nf[:, 0] - d[:, 0] * nf[:, 2], d[:, 0] * nf[:, 1] - d[:, 1] * nf[:, 0]), axis=1)
        r = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        good = (r > 0) & np.isfinite(r)
        nrm = c / np.where(good, r, 1.0)[:, None]
        rel = v[start_v] - o
        e = (nrm[:, 0] * rel[:, 0] + nrm[:, 1] * rel[:, 1]) + nrm[:, 2] * rel[:, 2]
        along = np.concatenate((nrm, e[:, None], (float(boundary_weight) * area)[:, None]), axis=1)
        along[~good] = 0.0
        planes = np.concatenate((face_planes, along))
        rows = len(planes)
        # the items: ascending (vertex, row)
        face = np.arange(m, dtype=np.int64)
        brow = m + np.arange(len(boundary), dtype=np.int64)
        item_key = np.sort(np.concatenate((f[:, 0] * rows + face, f[:, 1] * rows + face, f[:, 2] * rows + face, edge_a[boundary] * rows + brow,
                                           edge_b[boundary] * rows + brow)))
        item_vertex, item_row = item_key // rows, item_key % rows
        start = np.searchsorted(item_vertex, np.arange(n + 1)).astype(np.int64)
        degree = np.diff(start)
        nx, ny, nz, off, w = planes[item_row].T
        wx, wy, wz, we = w * nx, w * ny, w * nz, w * off
        ten = np.stack((wx * nx, wx * ny, wx * nz, wy * ny, wy * nz, wz * nz, -(we * nx), -(we * ny), -(we * nz), we * off), axis=1)
        quadrics = np.zeros((n, 10))
        for k in range(int(degree.max()) if n else 0):          # the k-th item of every vertex that has one
            has = np.nonzero(degree > k)[0]
            quadrics[has] = ten[start[has] + k] if k == 0 else quadrics[has] + ten[start[has] + k]
        # every edge
        s = quadrics[edge_a] + quadrics[edge_b]
        pa, pb = v[edge_a], v[edge_b]
        d = pb - pa
        mid = 0.5 * (pa + pb)
        l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        a00, a01, a02, a11, a12, a22, b0, b1, b2, _ = s.T
        m00, m01, m02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        m11, m12, m22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = (a00 * m00 + a01 * m01) + a02 * m02
        y = np.stack(((m00 * b0 + m01 * b1) + m02 * b2, (m01 * b0 + m11 * b1) + m12 * b2, (m02 * b0 + m12 * b1) + m22 * b2), axis=1)
        x = -(y / det[:, None])
        t = ((a00 + a11) + a22) / 3.0
        gap = x - (mid - o)
        accepted = (det > rcond * ((t * t) * t)) & ((gap[:, 0] * gap[:, 0] + gap[:, 1] * gap[:, 1]) + gap[:, 2] * gap[:, 2] <= (reach * reach) * l2)
        point, value = mid.copy(), _value(s, mid - o)
        for tried in (pa, pb):
            val = _value(s, tried - o)
            better = val < value
            point[better], value[better] = tried[better], val[better]
        point[accepted], value[accepted] = (o + x)[accepted], _value(s, x)[accepted]
        cost = np.where(value > 0, value, 0.0)
        g = point - pa
        par = ((g[:, 0] * d[:, 0] + g[:, 1] * d[:, 1]) + g[:, 2] * d[:, 2]) / l2
        par = np.where(par >= 0, par, 0.0)
        par = np.where(par > 1, 1.0, par)
        flags = np.where(accepted, ACCEPTED, 0) | np.where(run > 2, NONMANIFOLD, 0) \
            | np.where(np.isfinite(value) & np.isfinite(point).all(axis=1), 0, NONFINITE) | np.where(cost > limit, OVER, 0)
        # the flip test: every (edge, end, face of that end)
        face_degree = np.bincount(f.reshape(-1), minlength=n)          # a vertex's faces are the first items of its segment
        moving, other, of_edge = np.concatenate((edge_a, edge_b)), np.concatenate((edge_b, edge_a)), np.tile(np.arange(n_edges), 2)
        count = face_degree[moving]
        pair_edge, pair_moving, pair_other = np.repeat(of_edge, count), np.repeat(moving, count), np.repeat(other, count)
        within = np.arange(count.sum()) - np.repeat(np.cumsum(count) - count, count)
        pair_face = item_row[start[pair_moving] + within]
        tri = f[pair_face]
        corners = v[tri]                                          # [pairs, 3 corners, 3]
        moved = np.where((tri == pair_moving[:, None])[:, :, None], point[pair_edge][:, None, :], corners)
        old, new = _cross(corners[:, 0], corners[:, 1], corners[:, 2]), _cross(moved[:, 0], moved[:, 1], moved[:, 2])
        dot = (old[:, 0] * new[:, 0] + old[:, 1] * new[:, 1]) + old[:, 2] * new[:, 2]
        fails = ~(tri == pair_other[:, None]).any(axis=1) & ~(old == 0).all(axis=1) & ~(dot > 0)
        flips = np.zeros(n_edges, dtype=bool)
        flips[pair_edge[fails]] = True
        open_ = (flags & (NONMANIFOLD | NONFINITE | OVER)) == 0
        flags = (flags | np.where(open_ & flips, FLIP, 0) | np.where(open_ & ~flips, CANDIDATE, 0)).astype(np.uint8)
        # the selection: every vertex's lowest (cost, edge) among its candidates
        live = np.nonzero(flags & CANDIDATE)[0]
        end = np.concatenate((edge_a[live], edge_b[live]))
        of = np.concatenate((live, live))
        order = np.lexsort((of, cost[of], end))
        head = order[np.concatenate(([True], end[order][1:] != end[order][:-1]))] if len(order) else order
        best = np.full(n, NO_EDGE, dtype=np.int64)
        best[end[head]] = of[head]
        proposed = np.zeros(n_edges, dtype=bool)
        proposed[live] = (best[edge_a[live]] == live) & (best[edge_b[live]] == live)
        seen = best[f]                                            # [m, 3]
        seen = np.where((seen != NO_EDGE) & proposed[np.minimum(seen, n_edges - 1)], seen, NO_EDGE)
        seen_cost = np.where(seen != NO_EDGE, cost[np.minimum(seen, n_edges - 1)], np.inf)
        low, low_cost = seen[:, 0].copy(), seen_cost[:, 0].copy()
        for c in (1, 2):
            better = _lower(seen_cost[:, c], seen[:, c], low_cost, low)
            low[better], low_cost[better] = seen[better, c], seen_cost[better, c]
        withdrawn = np.zeros(n_edges, dtype=bool)
        loses = (seen != NO_EDGE) & (seen != low[:, None])
        withdrawn[seen[loses]] = True
        # the budget
        stays = np.nonzero(proposed & ~withdrawn)[0]
        stays = stays[np.argsort(cost[stays], kind="stable")]
        taken = np.zeros(n_edges, dtype=bool)
        if target_faces is None:
            taken[stays] = True
        elif len(stays) and m > target_faces:
            taken[stays[:np.searchsorted(np.cumsum(run[stays]), m - target_faces) + 1]] = True
    return {"planes": planes, "edge_a": edge_a, "edge_b": edge_b, "run": run.astype(np.int64), "item_row": item_row, "start": start,
            "quadrics": quadrics, "point": point, "cost": cost, "s": par, "flags": flags, "best_edge": best, "proposed": proposed,
            "withdrawn": withdrawn, "taken": taken, "n_taken": int(taken.sum())}


ROUNDS = {"loops": round_loops, "arrays": round_arrays}


# ---------------------------------------------------------------------------------------------------------------------------------
# the call
# ---------------------------------------------------------------------------------------------------------------------------------
def _apply_loops(r, position, extras, absorbed, owner, f):
    remap = list(range(len(position)))
    for e in np.nonzero(r["taken"])[0]:
        a, b, s = int(r["edge_a"][e]), int(r["edge_b"][e]), float(r["s"][e])
        remap[b] = a
        position[a] = r["point"][e]
        for x in extras:
            if x is not None:
                x[a] = [(1.0 - s) * p + s * q for p, q in zip(x[a].tolist(), x[b].tolist())]
        absorbed[a] = max(absorbed[a], absorbed[b], float(r["cost"][e]))
    owner[:] = [remap[i] for i in owner]
    return np.array([[remap[i] for i in tri] for tri in f.tolist()], dtype=np.int64).reshape(-1, 3)


def _apply_arrays(r, position, extras, absorbed, owner, f):
    e = np.nonzero(r["taken"])[0]
    a, b, s = r["edge_a"][e], r["edge_b"][e], r["s"][e][:, None]
    remap = np.arange(len(position))
    remap[b] = a
    position[a] = r["point"][e]
    for x in extras:
        if x is not None:
            x[a] = (1.0 - s) * x[a] + s * x[b]
    absorbed[a] = np.maximum(np.maximum(absorbed[a], absorbed[b]), r["cost"][e])
    owner[:] = remap[owner]
    return remap[f]


def collapse(vertices, faces, target_faces=None, max_error=None, boundary_weight=1.0, rcond=1e-9, reach=2.0, colours=None, normals=None,
             max_rounds=256, text="arrays", history=None):
    """``simplify_edge_collapse`` -> a dictionary of ``FIELDS``.  ``history``: a list that receives every round's dictionary, with the
    round's ``inputs`` (positions, faces, origin)."""
    assert target_faces is not None or max_error is not None
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n = len(v)
    one_round, apply = ROUNDS[text], {"loops": _apply_loops, "arrays": _apply_arrays}[text]
    f, kept = CC.remove_degenerate_faces(v, f)
    f, sub = CC.remove_duplicate_faces(f)
    kept = kept[sub]
    position, absorbed, owner = v.copy(), np.zeros(n), np.arange(n)
    extras = [None if x is None else np.array(x, dtype=np.float64) for x in (colours, normals)]
    rounds = collapsed = 0
    origin = v[np.unique(f)].min(axis=0) if len(f) else None
    while len(f) and (target_faces is None or len(f) > target_faces) and rounds < max_rounds:
        r = one_round(position, f, origin, target_faces, max_error, boundary_weight, rcond, reach)
        if history is not None:
            history.append(dict(r, inputs=(position.copy(), f.copy(), origin.copy())))
        rounds += 1
        if r["n_taken"] == 0:
            break
        f = apply(r, position, extras, absorbed, owner, f)
        f, sub = CC.remove_degenerate_faces(position, f)
        kept = kept[sub]
        f, sub = CC.remove_duplicate_faces(f)
        kept = kept[sub]
        collapsed += r["n_taken"]
    used = np.zeros(n, dtype=bool)
    used[f.reshape(-1)] = True
    number = np.where(used, np.cumsum(used) - 1, -1).astype(np.int64)
    return {"vertices": position[used], "faces": number[f].reshape(-1, 3), "kept_faces": kept.astype(np.int64), "inverse": number[owner],
            "colours": None if extras[0] is None else extras[0][used], "normals": None if extras[1] is None else extras[1][used],
            "cost": absorbed[used], "rounds": rounds, "collapsed": collapsed, "reached": target_faces is not None and len(f) <= target_faces}


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases (tests/test_collapse_host.py and tests/test_hip_collapse.py share them): the smallest at which each thing can go wrong
# ---------------------------------------------------------------------------------------------------------------------------------
def square(k=16):
    """The flat square [0,1]^2 x {0} as k x k cells of two triangles, wound upwards: every coordinate a multiple of 1/k."""
    i, j = np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing="ij")
    v = np.stack((i.reshape(-1) / k, j.reshape(-1) / k, np.zeros((k + 1) ** 2)), axis=1)
    idx = lambda p, q: (p * (k + 1) + q).reshape(-1)          # noqa: E731
    i, j = i[:-1, :-1], j[:-1, :-1]
    f = np.concatenate((np.stack((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), axis=1), np.stack((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)), axis=1)))
    return v, f.astype(np.int64)


def ribbon(k):
    """k triangles in a row over a gently waving zigzag, consistently wound: k + 2 vertices, ALL on the boundary, 2 k + 1 edges."""
    i = np.arange(k + 2)
    v = np.stack((0.5 * i, (i % 2).astype(np.float64), 0.05 * np.sin(0.7 * i)), axis=1)
    j = np.arange(k)
    f = np.where((j % 2 == 0)[:, None], np.stack((j, j + 1, j + 2), axis=1), np.stack((j + 1, j, j + 2), axis=1))
    return v, f.astype(np.int64)


def with_edges(count):
    """A mesh with exactly ``count`` unique edges: a ribbon, and for an even count a separate triangle."""
    if count % 2:
        return ribbon((count - 1) // 2)
    v, f = ribbon((count - 4) // 2)
    return np.concatenate((v, [[0.0, 3.0, 0.0], [1.0, 3.0, 0.0], [0.0, 4.0, 0.5]])), np.concatenate((f, [[len(v), len(v) + 1, len(v) + 2]]))


def moebius(k=24):
    """A Möbius strip of 2 k triangles: two rows of k vertices, closed with a half twist.  Not orientable; one boundary curve."""
    t = 2 * np.pi * np.arange(k) / k
    rows = [np.stack(((1 + w * np.cos(t / 2)) * np.cos(t), (1 + w * np.cos(t / 2)) * np.sin(t), w * np.sin(t / 2)), axis=1) for w in (-0.3, 0.3)]
    v = np.concatenate(rows)
    f = []
    for i in range(k):
        a, b = i, k + i
        c, d = (i + 1, k + i + 1) if i + 1 < k else (k, 0)          # the half twist at the seam
        f += [[a, c, b], [c, d, b]]
    return v, np.array(f, dtype=np.int64)


def book(pages=3, length=6, width=4):
    """``pages`` rectangular sheets of length x width cells that share one spine: the spine's edges are held by ``pages`` faces each."""
    g = np.random.default_rng(11)
    spine = np.stack((np.zeros(length + 1), np.zeros(length + 1), np.arange(length + 1, dtype=np.float64)), axis=1)
    vs, fs, index = [spine], [], {}
    count = length + 1
    for p in range(pages):
        angle = 2 * np.pi * p / pages + 0.1
        for i in range(length + 1):
            index[p, i, 0] = i
            for j in range(1, width + 1):
                index[p, i, j] = count
                count += 1
                vs.append([[j * np.cos(angle), j * np.sin(angle), i + 0.02 * g.uniform(-1, 1)]])
        for i in range(length):
            for j in range(width):
                a, b, c, d = index[p, i, j], index[p, i + 1, j], index[p, i + 1, j + 1], index[p, i, j + 1]
                fs += [[a, b, c], [a, c, d]]
    return np.concatenate(vs), np.array(fs, dtype=np.int64)


FAN_SIZES = (63, 64, 65, 300)
COUNTS = (255, 256, 257)
TINY = ("no_faces", "one_face", "bow_tie", "unreferenced_vertex", "repeated_vertex", "duplicate_face", "three_on_an_edge")
_cases = {}


def cases():
    """{name: (vertices, faces, keyword arguments)}, built once"""
    if _cases:
        return _cases
    out = {}
    tiny = CC._tiny()
    for name in TINY:
        out[name] = (*tiny[name], {"target_faces": 1})
    # every cost on the flat square ties at exactly 0, so every vertex chooses its lowest edge and about ONE edge a round is chosen by both
    # its ends: the free square needs 285 rounds to come down to two faces, more than the default of 256
    out["square_outline"] = (*square(16), {"max_error": 1e-12, "target_faces": 1})
    out["square_free"] = (*square(16), {"boundary_weight": 0.0, "target_faces": 2, "max_rounds": 512})
    out["ribbon_40"] = (*ribbon(40), {"target_faces": 10})
    out["cube_96"] = (*SR.cube(4), {"target_faces": 96})
    out["cube_12"] = (*SR.cube(4), {"target_faces": 12})
    out["cube_one_round"] = (*SR.cube(4), {"target_faces": 12, "max_rounds": 1})
    out["cube_two_rounds"] = (*SR.cube(4), {"target_faces": 12, "max_rounds": 2})
    out["cube_error_only"] = (*SR.cube(4), {"max_error": 1e-9})
    out["moebius"] = (*moebius(), {"target_faces": 16})
    out["book"] = (*book(), {"target_faces": 30})
    for k in FAN_SIZES:
        out[f"fan_{k}"] = (*SR.fan(k), {"target_faces": k // 2})
    for k in COUNTS:
        out[f"edges_{k}"] = (*with_edges(k), {"target_faces": k // 8})
        out[f"vertices_{k}"] = (*ribbon(k - 2), {"target_faces": k // 8})
    for tag in ("f16", "f32"):
        v, f = SR.golden(tag)
        out[f"{tag}_half"] = (v, f, {"target_faces": len(f) // 2})
        out[f"{tag}_tenth"] = (v, f, {"target_faces": len(f) // 10})
    _cases.update(out)
    return _cases


def attributes(n, seed=0):
    """Seeded colours and normals for n vertices (plain numbers)."""
    g = np.random.default_rng(99 + seed)
    return g.uniform(0.0, 1.0, (n, 3)), g.normal(size=(n, 3))
