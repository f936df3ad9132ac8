"""Vertex-clustering simplification (include/vfn.h: vfn_face_planes, vfn_cluster_quadrics; vf_nerf_amd/meshops.py:
simplify_vertex_clustering) restated in NumPy from its contract, TWICE, by two texts that share nothing but the contract:

* ``simplify_loops`` — Python floats and Python loops: a dictionary from a cell to its vertices, the planes face by face, the items
  cluster by cluster, the 64 lanes of the sum as a list, the adjugate written out for one cluster at a time;
* ``simplify_arrays`` — array-wise: the frame, the keys and the serial means of tests/voxel_restatement.py, the planes and the ten
  numbers of all items at once, every channel of every cluster through tests/cc_restatement.py's ``wave_sum``, the solve on whole arrays.

Both return the same dictionary; tests/test_simplify_host.py holds them against each other bit for bit, tests/test_hip_simplify.py holds
the device to them.  A specification of ours that follows Open3D's simplify_vertex_clustering (Average / Quadric) AS REMEMBERED: neither
Open3D nor trimesh is there to compare against.  Not part of the package: tests only."""
import math
import os

import numpy as np

import cc_restatement as CC
import voxel_restatement as V

CONTRACTIONS = ("average", "quadric")
WAVE = 64
FIELDS = ("vertices", "faces", "kept_faces", "inverse", "colours", "normals", "placed", "error", "n_clusters")


def _empty(n, colours, normals):
    none = np.zeros((0, 3))
    return {"vertices": none, "faces": np.zeros((0, 3), np.int64), "kept_faces": np.zeros(0, np.int64), "inverse": np.full(n, -1, np.int64),
            "colours": None if colours is None else none.copy(), "normals": None if normals is None else none.copy(),
            "placed": np.zeros(0, bool), "error": np.zeros(0), "n_clusters": 0, "centres": none.copy(), "items_per_cluster": np.zeros(0, np.int64),
            "cluster_of_vertex": np.full(n, -1, np.int64), "cluster": np.zeros(0, np.int64)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the first text: loops
# ---------------------------------------------------------------------------------------------------------------------------------
def _lanes_sum(xs):
    """The header's rule on a list of Python floats: 64 lanes, lane t starts from its first element; fold by halves."""
    lanes = [0.0] * WAVE
    for idx, x in enumerate(xs):
        t = idx % WAVE
        lanes[t] = x if idx < WAVE else lanes[t] + x
    for o in (32, 16, 8, 4, 2, 1):
        for t in range(o):
            lanes[t] = lanes[t] + lanes[t + o]
    return lanes[0]


def _plane_loop(p0, p1, p2, origin):
    a = [p1[k] - p0[k] for k in range(3)]
    b = [p2[k] - p0[k] for k in range(3)]
    c = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    s = c[0] * c[0]
    s = s + c[1] * c[1]
    s = s + c[2] * c[2]
    r = math.sqrt(s)
    if not (r > 0.0 and math.isfinite(r)):
        return [0.0, 0.0, 0.0, 0.0, 0.0]
    nrm = [c[0] / r, c[1] / r, c[2] / r]
    e = nrm[0] * (p0[0] - origin[0])
    e = e + nrm[1] * (p0[1] - origin[1])
    e = e + nrm[2] * (p0[2] - origin[2])
    return nrm + [e, 0.5 * r]


def _solve_loop(s, g, mean, h, rcond):
    """The ten sums of one cluster -> (position[3], accepted, error)."""
    a00, a01, a02, a11, a12, a22, b0, b1, b2, c = s
    m00, m01, m02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    m11, m12, m22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = (a00 * m00 + a01 * m01) + a02 * m02
    t = ((a00 + a11) + a22) / 3.0
    accepted, x = False, None
    if det > rcond * ((t * t) * t) and det != 0.0:          # (a determinant of 0 passes the first test for no t >= 0; a negative t cannot be)
        y = [(m00 * b0 + m01 * b1) + m02 * b2, (m01 * b0 + m11 * b1) + m12 * b2, (m02 * b0 + m12 * b1) + m22 * b2]
        x = [-(y[k] / det) for k in range(3)]
        accepted = all(abs(x[k]) <= 0.5 * h for k in range(3))
    position = [g[k] + x[k] for k in range(3)] if accepted else list(mean)
    z = x if accepted else [mean[k] - g[k] for k in range(3)]
    p = [(a00 * z[0] + a01 * z[1]) + a02 * z[2], (a01 * z[0] + a11 * z[1]) + a12 * z[2], (a02 * z[0] + a12 * z[1]) + a22 * z[2]]
    error = (((z[0] * p[0] + z[1] * p[1]) + z[2] * p[2]) + 2.0 * ((b0 * z[0] + b1 * z[1]) + b2 * z[2])) + c
    return position, accepted, error


def simplify_loops(vertices, faces, h, contraction="average", colours=None, normals=None, rcond=1e-9):
    assert contraction in CONTRACTIONS
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3).tolist()
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist()
    extra = [None if x is None else np.asarray(x, dtype=np.float64).tolist() for x in (colours, normals)]
    n, m, h = len(v), len(f), float(h)
    if m == 0 or n == 0:
        return _empty(n, colours, normals)
    referenced = sorted({i for tri in f for i in tri})
    origin = [min(v[i][k] for i in referenced) - 0.5 * h for k in range(3)]
    members = {}
    for i in referenced:                                                   # ascending index inside every cell
        cell = tuple(int(math.floor((v[i][k] - origin[k]) / h)) for k in range(3))
        members.setdefault(cell, []).append(i)
    order = sorted(members)                                               # ascending (c_0, c_1, c_2): ascending key
    k_all = len(order)
    cluster_of_vertex = [-1] * n
    for q, cell in enumerate(order):
        for i in members[cell]:
            cluster_of_vertex[i] = q
    rows = [v[i] + [x for e in extra if e is not None for x in e[i]] for i in range(n)]
    means = []
    for cell in order:
        s = list(rows[members[cell][0]])
        for i in members[cell][1:]:
            s = [a + b for a, b in zip(s, rows[i])]
        means.append([a / float(len(members[cell])) for a in s])
    centres = [[origin[k] + (cell[k] + 0.5) * h for k in range(3)] for cell in order]
    position, placed, error = [mn[:3] for mn in means], [False] * k_all, [math.nan] * k_all
    counts = [0] * k_all
    if contraction == "quadric":
        planes = [_plane_loop(v[t[0]], v[t[1]], v[t[2]], origin) for t in f]
        faces_of = [set() for _ in range(n)]
        for j, tri in enumerate(f):
            for i in tri:
                faces_of[i].add(j)
        for q, cell in enumerate(order):
            g = centres[q]
            u = [g[k] - origin[k] for k in range(3)]
            numbers = []
            for i in members[cell]:
                for j in sorted(faces_of[i]):
                    nx, ny, nz, e, w = planes[j]
                    d = nx * u[0]
                    d = d + ny * u[1]
                    d = d + nz * u[2]
                    d = d - e
                    wx, wy, wz, wd = w * nx, w * ny, w * nz, w * d
                    numbers.append([wx * nx, wx * ny, wx * nz, wy * ny, wy * nz, wz * nz, wd * nx, wd * ny, wd * nz, wd * d])
            counts[q] = len(numbers)
            sums = [_lanes_sum([row[c] for row in numbers]) for c in range(10)]
            position[q], placed[q], error[q] = _solve_loop(sums, g, means[q][:3], h, rcond)
    # the faces over the clusters
    seen, kept = set(), []
    for j, tri in enumerate(f):
        a, b, c = (cluster_of_vertex[i] for i in tri)
        if a == b or b == c or c == a:
            continue
        name = tuple(sorted((a, b, c)))
        if name in seen:
            continue
        seen.add(name)
        kept.append(j)
    named = sorted({cluster_of_vertex[i] for j in kept for i in f[j]})
    number = {q: r for r, q in enumerate(named)}
    out = {"vertices": np.array([position[q] for q in named], dtype=np.float64).reshape(-1, 3),
           "faces": np.array([[number[cluster_of_vertex[i]] for i in f[j]] for j in kept], dtype=np.int64).reshape(-1, 3),
           "kept_faces": np.array(kept, dtype=np.int64),
           "inverse": np.array([number.get(q, -1) if q >= 0 else -1 for q in cluster_of_vertex], dtype=np.int64),
           "placed": np.array([placed[q] for q in named], dtype=bool), "error": np.array([error[q] for q in named], dtype=np.float64),
           "n_clusters": k_all, "centres": np.array([centres[q] for q in named], dtype=np.float64).reshape(-1, 3),
           "items_per_cluster": np.array(counts, dtype=np.int64), "cluster_of_vertex": np.array(cluster_of_vertex, dtype=np.int64),
           "cluster": np.array(named, dtype=np.int64)}
    col = 3
    for name, e in zip(("colours", "normals"), extra):
        out[name] = None if e is None else np.array([means[q][col:col + 3] for q in named], dtype=np.float64).reshape(-1, 3)
        col += 0 if e is None else 3
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the second text: arrays
# ---------------------------------------------------------------------------------------------------------------------------------
def planes_arrays(v, f, origin):
    """-> planes[m,5] = (nrm, e, w); five +0.0 for a face without area."""
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    a, b = p1 - p0, p2 - p0
    c = np.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), axis=1)
    with np.errstate(all="ignore"):
        r = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        good = (r > 0) & np.isfinite(r)
        nrm = c / np.where(good, r, 1.0)[:, None]
        rel = p0 - np.asarray(origin, dtype=np.float64)
        e = (nrm[:, 0] * rel[:, 0] + nrm[:, 1] * rel[:, 1]) + nrm[:, 2] * rel[:, 2]
    planes = np.concatenate((nrm, e[:, None], (0.5 * r)[:, None]), axis=1)
    planes[~good] = 0.0
    return planes


def quadrics_arrays(planes, item_face, start, centres, means, origin, h, rcond):
    """vfn_cluster_quadrics on arrays -> (position[K,3], placed[K] bool, error[K], status).  A segment that is empty, decreasing or
    outside [0, items], or that names a face outside [0, m): NaN, not placed, status bit 2."""
    planes, centres, means = (np.asarray(x, dtype=np.float64) for x in (planes, centres, means))
    item_face, start = np.asarray(item_face, dtype=np.int64), np.asarray(start, dtype=np.int64)
    k, m, items = len(start) - 1, len(planes), len(item_face)
    sums = np.full((k, 10), np.nan)
    bad = np.zeros(k, dtype=bool)
    status = 0
    for q in range(k):
        b, e = int(start[q]), int(start[q + 1])
        if b < 0 or e <= b or e > items or ((item_face[b:e] < 0) | (item_face[b:e] >= m)).any():
            status |= 2
            bad[q] = True
            continue
        row = planes[item_face[b:e]]
        nrm, off, w = row[:, :3], row[:, 3], row[:, 4]
        u = centres[q] - np.asarray(origin, dtype=np.float64)
        d = ((nrm[:, 0] * u[0] + nrm[:, 1] * u[1]) + nrm[:, 2] * u[2]) - off
        wn, wd = w[:, None] * nrm, w * d
        ten = np.stack((wn[:, 0] * nrm[:, 0], wn[:, 0] * nrm[:, 1], wn[:, 0] * nrm[:, 2], wn[:, 1] * nrm[:, 1], wn[:, 1] * nrm[:, 2],
                        wn[:, 2] * nrm[:, 2], wd * nrm[:, 0], wd * nrm[:, 1], wd * nrm[:, 2], wd * d), axis=1)
        sums[q] = [CC.wave_sum(ten[:, c]) for c in range(10)]
    a00, a01, a02, a11, a12, a22, b0, b1, b2, c = sums.T
    with np.errstate(all="ignore"):
        m00, m01, m02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        m11, m12, m22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = (a00 * m00 + a01 * m01) + a02 * m02
        y = np.stack(((m00 * b0 + m01 * b1) + m02 * b2, (m01 * b0 + m11 * b1) + m12 * b2, (m02 * b0 + m12 * b1) + m22 * b2), axis=1)
        x = -(y / det[:, None])
        t = ((a00 + a11) + a22) / 3.0
        accepted = (det > rcond * ((t * t) * t)) & (np.abs(x) <= 0.5 * h).all(axis=1)
        position = np.where(accepted[:, None], centres + x, means)
        z = np.where(accepted[:, None], x, means - centres)
        p = np.stack(((a00 * z[:, 0] + a01 * z[:, 1]) + a02 * z[:, 2], (a01 * z[:, 0] + a11 * z[:, 1]) + a12 * z[:, 2],
                      (a02 * z[:, 0] + a12 * z[:, 1]) + a22 * z[:, 2]), axis=1)
        error = (((z[:, 0] * p[:, 0] + z[:, 1] * p[:, 1]) + z[:, 2] * p[:, 2]) + 2.0 * ((b0 * z[:, 0] + b1 * z[:, 1]) + b2 * z[:, 2])) + c
    position[bad], error[bad], accepted[bad] = np.nan, np.nan, False
    return position, accepted, error, status


def simplify_arrays(vertices, faces, h, contraction="average", colours=None, normals=None, rcond=1e-9):
    assert contraction in CONTRACTIONS
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
    n, m, h = len(v), len(f), float(h)
    if m == 0 or n == 0:
        return _empty(n, colours, normals)
    used = np.zeros(n, dtype=bool)
    used[f.reshape(-1)] = True
    referenced = np.nonzero(used)[0]
    vr = v[referenced]
    origin, _ = V.frame(vr, h)
    key, status = V.keys(vr, origin, h)
    assert status == 0
    perm = np.argsort(key, kind="stable")
    first = np.concatenate(([True], key[perm][1:] != key[perm][:-1]))
    start = np.concatenate((np.nonzero(first)[0], [len(vr)])).astype(np.int64)
    k_all = len(start) - 1
    cluster_of_vertex = np.full(n, -1, dtype=np.int64)
    cluster_of_vertex[referenced[perm]] = np.cumsum(first) - 1
    given = [np.asarray(x, dtype=np.float64)[referenced] for x in (colours, normals) if x is not None]
    means = V.serial_means(np.concatenate([vr] + given, axis=1)[perm], start)
    centres = np.asarray(origin) + (V.cells(vr, origin, h)[perm[start[:-1]]] + 0.5) * h
    position, placed, error = means[:, :3].copy(), np.zeros(k_all, dtype=bool), np.full(k_all, np.nan)
    counts = np.zeros(k_all, dtype=np.int64)
    if contraction == "quadric":
        face = np.arange(m, dtype=np.int64)
        both = np.unique(np.concatenate((f[:, 0] * m + face, f[:, 1] * m + face, f[:, 2] * m + face)))          # ascending (vertex, face), each once
        item_cluster = cluster_of_vertex[both // m]
        by_cluster = np.argsort(item_cluster, kind="stable")
        item_face = (both % m)[by_cluster]
        item_start = np.searchsorted(item_cluster[by_cluster], np.arange(k_all + 1)).astype(np.int64)
        counts = np.diff(item_start)
        position, placed, error, st = quadrics_arrays(planes_arrays(v, f, origin), item_face, item_start, centres, means[:, :3], origin, h, rcond)
        assert st == 0
    remapped = cluster_of_vertex[f]
    proper = np.nonzero(~((remapped[:, 0] == remapped[:, 1]) | (remapped[:, 1] == remapped[:, 2]) | (remapped[:, 2] == remapped[:, 0])))[0]
    _, where = np.unique(np.sort(remapped[proper], axis=1), axis=0, return_index=True)          # the first face of every sorted triple
    kept = proper[np.sort(where)].astype(np.int64)
    stays = np.zeros(k_all, dtype=bool)
    stays[remapped[kept].reshape(-1)] = True
    number = np.where(stays, np.cumsum(stays) - 1, -1).astype(np.int64)
    out = {"vertices": position[stays], "faces": number[remapped[kept]].reshape(-1, 3), "kept_faces": kept,
           "inverse": np.where(cluster_of_vertex >= 0, number[np.maximum(cluster_of_vertex, 0)], -1).astype(np.int64),
           "placed": placed[stays], "error": error[stays], "n_clusters": k_all, "centres": centres[stays], "items_per_cluster": counts,
           "cluster_of_vertex": cluster_of_vertex, "cluster": np.nonzero(stays)[0].astype(np.int64)}
    col = 3
    for name, x in (("colours", colours), ("normals", normals)):
        out[name] = None if x is None else means[:, col:col + 3][stays]
        col += 0 if x is None else 3
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases (tests/test_simplify_host.py and tests/test_hip_simplify.py share them): the smallest at which each thing can go wrong
# ---------------------------------------------------------------------------------------------------------------------------------
def cube(k=16):
    """The surface of [0,1]^3 at spacing 1/k, two triangles a square, wound outwards: 6 k^2 + 2 vertices, 12 k^2 faces; every
    coordinate a multiple of 1/k."""
    index, vertices, faces = {}, [], []

    def vertex(p):
        if p not in index:
            index[p] = len(vertices)
            vertices.append([c / k for c in p])
        return index[p]

    for axis in range(3):
        for side in (0, k):
            for i in range(k):
                for j in range(k):
                    corner = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side, i + di, j + dj
                        corner.append(vertex(tuple(p)))
                    a, b, c, d = corner if side else corner[::-1]
                    faces += [[a, b, c], [a, c, d]]
    return np.array(vertices, dtype=np.float64), np.array(faces, dtype=np.int64)


def golden(tag):
    fix = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_stages.npz"))
    return fix[f"{tag}.vs"].astype(np.float64), fix[f"{tag}.fs"].astype(np.int64) - 1          # the reference's faces are 1-based


def fan(k, seed=0):
    """k triangles around one vertex (an open fan over a bumpy rim, not flat): the centre is named by exactly k faces, and at the voxel
    edge ``FAN_H`` it is alone in its cell, so that its cluster holds exactly k items.  k = 1: one triangle."""
    g = np.random.default_rng(1000 + k + seed)
    theta = np.linspace(0.0, 1.5 * np.pi, k + 1)
    rim = np.stack((np.cos(theta), np.sin(theta), 0.2 * np.sin(5.0 * theta) + 0.05 * g.uniform(-1, 1, k + 1)), axis=1)
    v = np.concatenate(([[0.013, -0.007, 0.41]], rim))
    f = np.stack((np.zeros(k, dtype=np.int64), np.arange(1, k + 1), np.arange(2, k + 2)), axis=1)
    return v, f


FAN_H = 0.02
FAN_SIZES = (1, 63, 64, 65, 128, 129)
SMALL = ("no_faces", "one_face", "bow_tie", "unreferenced_vertex", "repeated_vertex")
_cases = {}


def cases():
    """{name: (vertices, faces, voxel edge)}, built once"""
    if _cases:
        return _cases
    out = {}
    # 2.0: the frame's origin is -1, so the coordinate 1 falls into cell 1 — eight clusters, the largest of 4 323 items; 4.0: ONE cluster,
    # all 9 216 incidences in one segment, and no face survives
    for h in (0.25, 0.1875, 2.0, 4.0):
        out[f"cube_{h}"] = (*cube(), h)
    for tag in ("f16", "f32"):
        for h in (0.1, 0.25):
            out[f"{tag}_{h}"] = (*golden(tag), h)
    tiny = CC._tiny()
    for name in SMALL:
        for h in (0.4, 1.5):
            out[f"{name}_{h}"] = (*tiny[name], h)
    for k in FAN_SIZES:
        out[f"fan_{k}"] = (*fan(k), FAN_H)
    _cases.update(out)
    return _cases


def attributes(n, seed=0):
    """Seeded colours and normals for n vertices (plain numbers: the means are not made unit vectors)."""
    g = np.random.default_rng(77 + seed)
    return g.uniform(0.0, 1.0, (n, 3)), g.normal(size=(n, 3))
