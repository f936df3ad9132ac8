"""A CPU restatement of mesh scoring (utils/utils.py:327-367 ``get_chamfer_distance`` and the precision / recall / F-score counts that
vf_nerf_amd/metrics3d.py documents), written from the contract of include/vfn.h in numpy float64: numpy's elementwise operations
round every product and sum once, in the association written here, which is what csrc/vfn_metrics.hip does without contraction.
tests/test_metrics3d_host.py pins the brute-force distances to scipy's cKDTree (the reference's KDTree) bit for bit; the GPU tests
then hold the device to this file.  Not part of the package: tests only."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

import tree_restatement as T


def _nn_rows(q, tx, ty, tz, tile):
    best = np.full(q.shape[0], np.inf)
    qx, qy, qz = q[:, 0:1], q[:, 1:2], q[:, 2:3]
    for lo in range(0, tx.shape[0], tile):
        dx, dy, dz = qx - tx[lo:lo + tile], qy - ty[lo:lo + tile], qz - tz[lo:lo + tile]
        d = (dx * dx + dy * dy) + dz * dz
        np.minimum(best, d.min(axis=1), out=best)
    return best


def nn_sqdist(queries, targets, rows: int = 256, tile: int = 2048, workers: int = 1):
    """best[i] = min_j ((dx dx + dy dy) + dz dz), dx = q_i.x - t_j.x, ...: all pairs, in tiles (the minimum does not depend on them)."""
    q = np.ascontiguousarray(queries, dtype=np.float64)
    t = np.ascontiguousarray(targets, dtype=np.float64)
    tx, ty, tz = (np.ascontiguousarray(t[:, c]) for c in range(3))
    chunks = [q[lo:lo + rows] for lo in range(0, q.shape[0], rows)]
    if workers > 1:
        with ThreadPoolExecutor(workers) as pool:          # numpy releases the GIL inside its loops
            parts = list(pool.map(lambda c: _nn_rows(c, tx, ty, tz, tile), chunks))
    else:
        parts = [_nn_rows(c, tx, ty, tz, tile) for c in chunks]
    return np.concatenate(parts)


def nearest_distances(queries, targets, **kw):
    return np.sqrt(nn_sqdist(queries, targets, **kw))


def tri_areas(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def sample_surface(vertices, faces, cum, uniforms):
    """Area-weighted samples from an inclusive cumulative-area table and uniforms[count,3] in [0,1) -> (points, face_index)."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    cum = np.asarray(cum, dtype=np.float64)
    u = np.asarray(uniforms, dtype=np.float64)
    t = u[:, 0] * cum[-1]
    face = np.minimum(np.searchsorted(cum, t, side="right"), len(cum) - 1)        # the smallest index with cum[index] > t
    a, b = u[:, 1].copy(), u[:, 2].copy()
    fold = a + b > 1.0
    a[fold], b[fold] = 1.0 - a[fold], 1.0 - b[fold]
    v0 = v[f[face, 0]]
    e1, e2 = v[f[face, 1]] - v0, v[f[face, 2]] - v0
    return (v0 + a[:, None] * e1) + b[:, None] * e2, face.astype(np.int64)


def stats_sum(x):
    """stats[0] of vfn_reduce_stats: the sum of x[n] along the device's fixed tree (tests/tree_restatement.py, lane order "far")."""
    return float(T.two_level(np.asarray(x, dtype=np.float64)[:, None], "far")[0])


def median(x):
    """np.median's definition: the middle value, or the mean of the two middle values."""
    s = np.sort(np.asarray(x, dtype=np.float64))
    n = len(s)
    return float(s[n // 2]) if n % 2 else float((s[n // 2 - 1] + s[n // 2]) / 2.0)


def chamfer_from_distances(ref_to_pred, pred_to_ref):
    """utils.py:350-367 from the two arrays of nearest DISTANCES: statistics of their squares per direction, then the sum of the
    means, the sum of the medians, the min of the mins, the max of the maxes."""
    one, two = np.square(np.asarray(ref_to_pred, dtype=np.float64)), np.square(np.asarray(pred_to_ref, dtype=np.float64))
    return (float(np.mean(one) + np.mean(two)), median(one) + median(two), float(min(one.min(), two.min())),
            float(max(one.max(), two.max())))


def chamfer_from_points(pred_points, ref_points, **kw):
    return chamfer_from_distances(nearest_distances(ref_points, pred_points, **kw), nearest_distances(pred_points, ref_points, **kw))


def precision_recall_fscore(pred_points, ref_points, threshold, **kw):
    d_pred = nearest_distances(pred_points, ref_points, **kw)        # pred -> nearest ref
    d_ref = nearest_distances(ref_points, pred_points, **kw)         # ref -> nearest pred
    n_p, n_r = int((d_pred < threshold).sum()), int((d_ref < threshold).sum())
    p, r = n_p / len(d_pred), n_r / len(d_ref)
    return {"precision": p, "recall": r, "fscore": 2 * p * r / (p + r) if p + r > 0 else 0.0, "pred_within": n_p, "ref_within": n_r}
