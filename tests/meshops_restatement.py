"""The normals unit (include/vfn.h: vfn_face_normals, vfn_vertex_normals, vfn_normal_dots), ``meshops.weld`` and the sums of
``metrics3d.normal_consistency`` restated in NumPy from their contracts, operation for operation.  NumPy does not contract or reassociate
elementwise float64 expressions, ``np.sqrt`` and ``/`` are correctly rounded, so the bits are the device's.  Ordered sums are Python loops
over the rows.  Not part of the package: tests only."""
import numpy as np

import tree_restatement as T


def unit(c, fallback):
    """c[k,3] -> (unit[k,3], overflow[k]): s = c.x c.x; s = s + c.y c.y; s = s + c.z c.z; r = sqrt(s); c / r where r > 0 and finite,
    ``fallback`` elsewhere; overflow where r is not finite."""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(all="ignore"):
        s = c[:, 0] * c[:, 0]
        s = s + c[:, 1] * c[:, 1]
        s = s + c[:, 2] * c[:, 2]
        r = np.sqrt(s)
        good = (r > 0) & np.isfinite(r)
        out = np.empty_like(c)
        out[:] = np.asarray(fallback, dtype=np.float64)
        safe = np.where(good, r, 1.0)
        for k in range(3):
            out[good, k] = (c[:, k] / safe)[good]
    return out, ~np.isfinite(r)


def face_normals(vertices, faces, normalise):
    """-> [m,3]: a = v1 - v0, b = v2 - v0, c = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x); unit(c, 0) with normalise."""
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    a, b = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    c = np.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), axis=1)
    return unit(c, (0.0, 0.0, 0.0))[0] if normalise else c


def vertex_faces(faces, n):
    """-> a list of n ascending lists: the faces of every vertex, each once."""
    rows = [set() for _ in range(n)]
    for j, face in enumerate(np.asarray(faces, dtype=np.int64)):
        for q in face:
            rows[int(q)].add(j)
    return [sorted(r) for r in rows]


def csr(rows):
    row_start = np.zeros(len(rows) + 1, dtype=np.int64)
    row_start[1:] = np.cumsum([len(r) for r in rows])
    return row_start, np.array([j for r in rows for j in r], dtype=np.int64)


def vertex_normals(vertices, faces):
    """-> [n,3]: s = fn[f_0]; s = s + fn[f_1]; ... over the vertex's faces in ascending order (fn unnormalised), unit(s, (0, 0, 1));
    (0, 0, 1) for a vertex without faces."""
    n = np.asarray(vertices).shape[0]
    fn = face_normals(vertices, faces, False)
    sums = np.zeros((n, 3))
    empty = np.zeros(n, dtype=bool)
    for i, row in enumerate(vertex_faces(faces, n)):
        if not row:
            empty[i] = True
            continue
        s = fn[row[0]].copy()
        for j in row[1:]:
            s = s + fn[j]
        sums[i] = s
    out = unit(sums, (0.0, 0.0, 1.0))[0]
    out[empty] = (0.0, 0.0, 1.0)
    return out


def normal_dots(qn, tn, index):
    """-> [n]: d = qn.x tn[j].x; d = d + qn.y tn[j].y; d = d + qn.z tn[j].z; |d| with j = index[i]."""
    qn, t = np.asarray(qn, dtype=np.float64), np.asarray(tn, dtype=np.float64)[np.asarray(index, dtype=np.int64)]
    d = qn[:, 0] * t[:, 0]
    d = d + qn[:, 1] * t[:, 1]
    d = d + qn[:, 2] * t[:, 2]
    return np.abs(d)


def weld(vertices, faces, digits):
    """-> (vertices[V',3], faces[m,3], inverse[n]): the referenced vertices in index order, keyed by their coordinates (digits None;
    -0.0 is +0.0) or by np.rint(v * 10.0**digits); a class is numbered when its first (lowest) vertex appears and keeps that vertex's
    bits; unreferenced vertices get inverse -1."""
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    used = np.zeros(v.shape[0], dtype=bool)
    used[f.reshape(-1)] = True
    inverse = np.full(v.shape[0], -1, dtype=np.int64)
    classes, keep = {}, []
    for i in np.nonzero(used)[0]:
        key = v[i] if digits is None else np.rint(v[i] * 10.0 ** digits)
        key = tuple(float(x) + 0.0 for x in key)                 # (-0.0 + 0.0 = +0.0: one key; tuples of floats compare by value)
        if key not in classes:
            classes[key] = len(keep)
            keep.append(i)
        inverse[i] = classes[key]
    out_v = v[np.array(keep, dtype=np.int64)] if keep else np.zeros((0, 3))
    return out_v, inverse[f], inverse


def tree_sum(x):
    """The first of lib.reduce_stats's four numbers: the sum of x[n] along the fixed tree, lane order "far"."""
    return float(T.two_level(np.asarray(x, dtype=np.float64).reshape(-1, 1), "far")[0])


def normal_consistency(pred_normals, ref_normals, pred_to_ref_index, ref_to_pred_index):
    """The unit normals of both sample sets and every sample's nearest sample of the other set -> the three numbers."""
    a = tree_sum(normal_dots(pred_normals, ref_normals, pred_to_ref_index)) / len(pred_normals)
    b = tree_sum(normal_dots(ref_normals, pred_normals, ref_to_pred_index)) / len(ref_normals)
    return {"pred_to_ref": a, "ref_to_pred": b, "mean": (a + b) / 2.0}
