"""A CPU restatement of voxel down-sampling (vf_nerf_amd/voxel.py, csrc/vfn_voxel.hip) and of the staged registration on top of it
(``icp.align_stages``), written from the contract of include/vfn.h in numpy float64 and Python floats, independently of the package's
code: numpy's elementwise operations round every difference, quotient and sum once, which is what the unit does without contraction.

* ``down_sample`` — keys by the contract's expression, ``np.argsort(kind="stable")``, serial sums in ascending position.
* ``down_sample_dict`` — a second way to the same numbers: a dictionary keyed by the voxel, filled in INPUT order, the way Open3D's hash
  map accumulates; the stable sort keeps a voxel's points in input order, so the two must agree to the bit.
* ``align_stages`` — the staged ICP from tests/icp_restatement.py's parts (imported, not edited): its search, its terms, the fixed tree
  of its sums (the device's, bit for bit), and the host's solve and composition written out here.

Not part of the package: tests only."""
from __future__ import annotations

import math

import numpy as np

import icp_restatement as R

AXIS_BITS = 21
LONG = 64               # serial_means: segments longer than this are summed one by one (speed of the restatement only)


def frame(points, h: float):
    """-> (origin[3], dims[3]) in Python floats: origin_k = min_k - 0.5 h, dims_k = floor((max_k - origin_k) / h) + 1."""
    p = np.asarray(points, dtype=np.float64)
    lo, hi = p.min(axis=0).tolist(), p.max(axis=0).tolist()
    h = float(h)
    origin = tuple(x - 0.5 * h for x in lo)
    return origin, tuple(int(math.floor((x - o) / h)) + 1 for x, o in zip(hi, origin))


def cells(points, origin, h: float) -> np.ndarray:
    """c_k = floor((p_k - origin_k) / h) as float64 [n,3]: a subtraction and a true division."""
    p = np.asarray(points, dtype=np.float64)
    return np.floor((p - np.asarray(origin, dtype=np.float64)) / np.float64(h))


def keys(points, origin, h: float):
    """-> (keys int64 [n], status): (c_0 << 42) | (c_1 << 21) | c_2; -1 and status bit 1 for a non-finite coordinate, -1 and bit 2 for a
    c_k outside [0, 2^21)."""
    p = np.asarray(points, dtype=np.float64)
    finite = np.isfinite(p).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        c = cells(np.where(finite[:, None], p, 0.0), origin, h)
    inside = ((c >= 0) & (c < float(1 << AXIS_BITS))).all(axis=1)
    ok = finite & inside
    ci = np.where(ok[:, None], c, 0.0).astype(np.int64)
    k = (ci[:, 0] << (2 * AXIS_BITS)) | (ci[:, 1] << AXIS_BITS) | ci[:, 2]
    status = (1 if (~finite).any() else 0) | (2 if (finite & ~inside).any() else 0)
    return np.where(ok, k, -1), status


def serial_means(sorted_values, start) -> np.ndarray:
    """sorted_values[n,C], start[V+1] -> [V,C]: S = x_b; S = S + x_(b+1); ...; S / count.  Serial along every segment, vectorised ACROSS
    the segments: at step r every segment that has an r-th element adds it.  A segment longer than LONG is summed on its own by
    np.cumsum, which is serial by definition (every prefix is the one before plus one element, the first prefix the first element);
    tests/test_voxel_host.py holds it to the pure-Python dictionary on a 1000-point voxel.  A segment that is empty, decreasing or
    outside [0, n] is a row of NaN."""
    x = np.asarray(sorted_values, dtype=np.float64)
    start = np.asarray(start, dtype=np.int64)
    n = x.shape[0]
    b, e = start[:-1], start[1:]
    good = (b >= 0) & (e > b) & (e <= n)
    out = np.full((len(b), x.shape[1]), np.nan)
    for v in np.nonzero(good & (e - b > LONG))[0]:
        out[v] = np.cumsum(x[b[v]:e[v]], axis=0)[-1] / np.float64(e[v] - b[v])
    idx = np.nonzero(good & (e - b <= LONG))[0]
    count = (e - b)[idx]
    by_count = idx[np.argsort(-count, kind="stable")]               # the longest segments first: the active ones are a prefix
    sorted_count = np.sort(count)                                   # ascending, to count the segments longer than r
    s = x[b[by_count]].copy()
    for r in range(1, int(count.max()) if len(count) else 0):
        active = len(count) - int(np.searchsorted(sorted_count, r, side="right"))
        s[:active] = s[:active] + x[b[by_count[:active]] + r]
    out[by_count] = s / (e - b)[by_count].astype(np.float64)[:, None]
    return out


def down_sample(points, h: float, normals=None, colours=None) -> dict:
    """The contract -> {"points", "normals", "colours", "counts", "voxel_of_point", "origin", "dims"}."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    origin, dims = frame(p, h)
    k, status = keys(p, origin, h)
    assert status == 0
    perm = np.argsort(k, kind="stable")
    sk = k[perm]
    first = np.concatenate(([True], sk[1:] != sk[:-1]))
    start = np.concatenate((np.nonzero(first)[0], [len(p)])).astype(np.int64)
    voxel_of_point = np.empty(len(p), dtype=np.int64)
    voxel_of_point[perm] = np.cumsum(first) - 1
    out = {"counts": np.diff(start), "voxel_of_point": voxel_of_point, "origin": origin, "dims": dims}
    for name, values in (("points", p), ("normals", normals), ("colours", colours)):
        out[name] = None if values is None else serial_means(np.asarray(values, dtype=np.float64)[perm], start)
    return out


def down_sample_dict(points, h: float, normals=None, colours=None) -> dict:
    """The same by a dictionary filled in input order: voxel (c_0, c_1, c_2) -> [running sums, count], every running sum started from
    the voxel's first point; the voxels then numbered in ascending (c_0, c_1, c_2)."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    origin, dims = frame(p, h)
    c = cells(p, origin, h).astype(np.int64)
    given = [np.asarray(v, dtype=np.float64) for v in (p, normals, colours) if v is not None]
    rows = np.concatenate(given, axis=1).tolist()
    acc = {}
    for cell, row in zip(map(tuple, c.tolist()), rows):
        hit = acc.get(cell)
        if hit is None:
            acc[cell] = [list(row), 1]
        else:
            hit[0] = [a + b for a, b in zip(hit[0], row)]
            hit[1] += 1
    order = sorted(acc)
    number = {cell: v for v, cell in enumerate(order)}
    means = np.array([[a / float(acc[cell][1]) for a in acc[cell][0]] for cell in order], dtype=np.float64)
    out = {"counts": np.array([acc[cell][1] for cell in order], dtype=np.int64),
           "voxel_of_point": np.array([number[cell] for cell in map(tuple, c.tolist())], dtype=np.int64), "origin": origin, "dims": dims}
    col = 0
    for name, values in (("points", p), ("normals", normals), ("colours", colours)):
        out[name] = None if values is None else means[:, col:col + 3]
        col += 0 if values is None else 3
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the staged registration
# ---------------------------------------------------------------------------------------------------------------------------------
def compose(a, b) -> np.ndarray:
    """a . b of two rigid [4,4] in Python floats: (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j, plus a_i3 in the last column."""
    out = np.eye(4)
    for i in range(3):
        for j in range(4):
            s = (float(a[i][0]) * float(b[0][j]) + float(a[i][1]) * float(b[1][j])) + float(a[i][2]) * float(b[2][j])
            out[i, j] = s + float(a[i][3]) if j == 3 else s
    return out


def host_solve(sums, anchor) -> np.ndarray:
    """The rigid update from the 17 sums as ``icp.align`` documents it (``rigid_from_sums``): means from the sums, H = sum p s^T - c
    (pbar sbar^T), its SVD, the reflection fixed by diag(1, 1, det), t = (sbar + a) - R (pbar + a).  The package calls this solve "not
    bit-pinned": what makes two evaluations of it agree to the bit is that both hand LAPACK the same H on the same machine, and H is a
    function of the sums, which ARE pinned.  So this follows the documented association exactly."""
    s, a = np.asarray(sums, dtype=np.float64), np.asarray(anchor, dtype=np.float64)
    c = s[0]
    pbar, sbar = s[2:5] / c, s[5:8] / c
    h = s[8:17].reshape(3, 3) - c * np.outer(pbar, sbar)
    u, _, vt = np.linalg.svd(h)
    d = np.diag([1.0, 1.0, float(np.sign(np.linalg.det(vt.T @ u.T)))])
    r = vt.T @ d @ u.T
    out = np.eye(4)
    out[:3, :3] = r
    out[:3, 3] = (sbar + a) - r @ (pbar + a)
    return out


def align_tree(source, targets, radius, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, workers=1) -> dict:
    """R.align from the identity with the DEVICE's sums: R's search and terms, every sum along the fixed tree (R.sums_of(..., "tree") over
    the placed rows), ``host_solve`` and numpy's 4 x 4 product for T <- U T, as the package's loop has them."""
    src, tg = np.asarray(source, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    a = R.bounding_anchor(tg)
    t_k = np.eye(4)
    history, updates, converged = [], 0, False
    while True:
        index, sqdist = R.nearest_within(src, tg, radius, t_k, workers=workers)
        s = R.sums_of(R.placed_terms(src, t_k, tg, index, sqdist, a), "tree")
        count = int(s[0])
        entry = {"transformation": t_k.copy(), "count": count, "fitness": count / len(src),
                 "inlier_rmse": math.sqrt(s[1] / count) if count else 0.0}
        history.append(entry)
        if R.stop_rule(history, relative_fitness, relative_rmse):
            converged = True
            break
        if updates >= max_iteration:
            break
        t_k = host_solve(s, a) @ t_k
        t_k[3] = [0.0, 0.0, 0.0, 1.0]
        updates += 1
    return {"transformation": t_k, "fitness": entry["fitness"], "inlier_rmse": entry["inlier_rmse"], "iterations": updates,
            "converged": converged, "history": history}


def align_stages(source, targets, stages, init=None, workers=1) -> dict:
    """Per stage (voxel or None, radius, iterations): move the source by T, down-sample both, align from the identity, T <- T_stage . T."""
    src, tg = np.asarray(source, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    t_k = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    out = []
    for size, radius, iterations in stages:
        moved = R.transform(src, t_k)
        target = tg
        if size is not None:
            moved, target = down_sample(moved, size)["points"], down_sample(tg, size)["points"]
        res = align_tree(moved, target, radius, max_iteration=iterations, workers=workers)
        t_k = compose(res["transformation"], t_k)
        out.append(dict(res, source_points=len(moved), target_points=len(target)))
    return {"transformation": t_k, "stages": out}
