"""The k-means contract of include/vfn.h (vfn_kmeans_assign / _update / _seed) and of vf_nerf_amd/cluster.py restated on the CPU, twice:
``LOOPS`` walks points, clusters and the fixed tree in Python floats, addition for addition; ``ARRAYS`` states the same array-wise, with
the tree of tests/tree_restatement.py.  Neither contracts a product into a sum (Python floats and NumPy's elementwise operations are
IEEE double operations, one rounding each), so both carry the device's bits.  Beside them: ``vfn_cumsum_f64`` (csrc/vfn_metrics.hip)
restated for the D^2 sampling, the inertia through the existing restatement of ``vfn_reduce_stats``' sum, ``meshops.simplify_to_faces``
over tests/simplify_restatement.py and ``meshops.dominant_bases`` over tests/meshops_restatement.py.  Not part of the package: tests only."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import meshops_restatement as M  # noqa: E402
import metrics3d_restatement as M3  # noqa: E402
import simplify_restatement as S  # noqa: E402
import tree_restatement as T  # noqa: E402

MAX_K = 64
FIELDS = ("centres", "labels", "counts", "sqdist", "inertia", "n_iter", "converged", "restart")
SCAN_LANES, SCAN_PER = 256, 4          # csrc/vfn_metrics.hip: a scan block is 256 lanes x 4 values
SCAN_TILE = SCAN_LANES * SCAN_PER


# ---------------------------------------------------------------------------------------------------------------------------------
# in Python loops
# ---------------------------------------------------------------------------------------------------------------------------------
def _d2(p, c):
    dx, dy, dz = p[0] - c[0], p[1] - c[1], p[2] - c[2]
    return (dx * dx + dy * dy) + dz * dz


def assign_loops(points, centres):
    """-> (label int32 [n], sqdist [n]): the least d2, the comparison strict and j ascending — a tie stays with the lower cluster."""
    p, c = np.asarray(points, dtype=np.float64).tolist(), np.asarray(centres, dtype=np.float64).tolist()
    label, sqdist = [], []
    for row in p:
        best, bj = _d2(row, c[0]), 0
        for j in range(1, len(c)):
            d = _d2(row, c[j])
            if d < best:
                best, bj = d, j
        label.append(bj)
        sqdist.append(best)
    return np.array(label, dtype=np.int32), np.array(sqdist, dtype=np.float64)


def tree_sum_loops(values):
    """A list of Python floats along THE FIXED TREE of include/vfn.h, lane order "near"."""
    n = len(values)
    partials = []
    for b in range(-(-n // T.TILE)):
        lanes = []
        for lane in range(T.LANES):
            slots = []
            for k in range(T.PER):
                i = b * T.TILE + lane + T.LANES * k
                slots.append(values[i] if i < n else 0.0)
            while len(slots) > 1:                              # slot k with slot k + 1, the lower on the left
                slots = [slots[2 * i] + slots[2 * i + 1] for i in range(len(slots) // 2)]
            lanes.append(slots[0])
        d = T.LANES // 2
        while d >= 1:
            for lane in range(d):
                lanes[lane] = lanes[lane] + lanes[lane + d]
            d //= 2
        partials.append(lanes[0])
    top = [0.0] * T.TOP
    for i, part in enumerate(partials):                        # lane l starts from partial l and adds l + 1024, l + 2048, ... serially
        top[i % T.TOP] = part if i < T.TOP else top[i % T.TOP] + part
    d = T.TOP // 2
    while d >= 1:
        for lane in range(d):
            top[lane] = top[lane] + top[lane + d]
        d //= 2
    return top[0]


def update_loops(points, label, centres):
    """-> (sums[k,3], count[k] int64, centres[k,3], status): a label outside [0, k) joins nothing (status bit 2); a cluster without
    points keeps its centre's bits."""
    p, lab = np.asarray(points, dtype=np.float64).tolist(), np.asarray(label).tolist()
    out = np.array(centres, dtype=np.float64, copy=True)
    k = len(out)
    sums, count = np.zeros((k, 3)), np.zeros(k, dtype=np.int64)
    status = 2 if any(q < 0 or q >= k for q in lab) else 0
    for j in range(k):
        count[j] = sum(1 for q in lab if q == j)
        for c in range(3):
            sums[j, c] = tree_sum_loops([row[c] if q == j else 0.0 for row, q in zip(p, lab)])
            if count[j] > 0:
                out[j, c] = sums[j, c] / float(count[j])
    return sums, count, out, status


def seed_loops(points, newest, first, mind2):
    """-> (mind2, farthest, status); ``newest`` None: mind2 is only read.  A bad index: status 2, mind2 as it was, farthest -1."""
    p = np.asarray(points, dtype=np.float64).tolist()
    out = list(np.asarray(mind2, dtype=np.float64).tolist()) if mind2 is not None else [0.0] * len(p)
    if newest is not None:
        if not 0 <= newest < len(p):
            return np.array(out), -1, 2
        for i, row in enumerate(p):
            d = _d2(row, p[newest])
            if not first:
                d = out[i] if out[i] < d else d
            out[i] = d
    best, bi = -1.0, -1
    for i, d in enumerate(out):
        if d > best:                                           # strict, i ascending: a tie stays with the lower index
            best, bi = d, i
    return np.array(out, dtype=np.float64), bi, 0


def cumsum_loops(x):
    """vfn_cumsum_f64 in Python floats: per block of 1024 a lane adds its 4 values serially, a Kogge-Stone scan over the 256 lane totals,
    one addition of the lane's exclusive prefix; the block totals scanned the same way; one addition per level on the way down."""
    x = list(np.asarray(x, dtype=np.float64).tolist())
    n = len(x)
    out, totals = [0.0] * n, []
    for b in range(-(-n // SCAN_TILE)):
        runs, lane_total = [], []
        for lane in range(SCAN_LANES):
            run, mine = 0.0, []
            for k in range(SCAN_PER):
                i = b * SCAN_TILE + lane * SCAN_PER + k
                val = x[i] if i < n else 0.0
                run = val if k == 0 else run + val
                mine.append(run)
            runs.append(mine)
            lane_total.append(run)
        d = 1
        while d < SCAN_LANES:
            lane_total = [lane_total[lane - d] + lane_total[lane] if lane >= d else lane_total[lane] for lane in range(SCAN_LANES)]
            d *= 2
        for lane in range(SCAN_LANES):
            for k in range(SCAN_PER):
                i = b * SCAN_TILE + lane * SCAN_PER + k
                if i < n:
                    out[i] = runs[lane][k] if lane == 0 else lane_total[lane - 1] + runs[lane][k]
        totals.append(lane_total[-1])
    if n > SCAN_TILE:
        prefix = cumsum_loops(totals)
        for i in range(SCAN_TILE, n):
            out[i] = prefix[i // SCAN_TILE - 1] + out[i]
    return np.array(out, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# array-wise
# ---------------------------------------------------------------------------------------------------------------------------------
def assign_arrays(points, centres):
    p, c = np.asarray(points, dtype=np.float64), np.asarray(centres, dtype=np.float64)
    best = np.full(len(p), np.inf)
    label = np.zeros(len(p), dtype=np.int32)
    for j in range(len(c)):                                    # cluster by cluster: [n] temporaries, not [n, k]
        dx, dy, dz = p[:, 0] - c[j, 0], p[:, 1] - c[j, 1], p[:, 2] - c[j, 2]
        d = (dx * dx + dy * dy) + dz * dz
        closer = d < best if j else np.ones(len(p), dtype=bool)
        best = np.where(closer, d, best)
        label[closer] = j
    return label, best


def update_arrays(points, label, centres):
    p, lab = np.asarray(points, dtype=np.float64), np.asarray(label)
    out = np.array(centres, dtype=np.float64, copy=True)
    k = len(out)
    sums, count = np.zeros((k, 3)), np.zeros(k, dtype=np.int64)
    status = 2 if ((lab < 0) | (lab >= k)).any() else 0
    for j in range(k):
        mine = lab == j
        count[j] = int(mine.sum())
        if count[j]:
            sums[j] = T.two_level(np.where(mine[:, None], p, 0.0), "near")          # (a tree of +0.0 is +0.0)
            out[j] = sums[j] / np.float64(count[j])
    return sums, count, out, status


def seed_arrays(points, newest, first, mind2):
    p = np.asarray(points, dtype=np.float64)
    out = np.array(mind2, dtype=np.float64, copy=True) if mind2 is not None else np.zeros(len(p))
    if newest is not None:
        if not 0 <= newest < len(p):
            return out, -1, 2
        dx, dy, dz = p[:, 0] - p[newest, 0], p[:, 1] - p[newest, 1], p[:, 2] - p[newest, 2]
        d = (dx * dx + dy * dy) + dz * dz
        out = d if first else np.where(out < d, out, d)
    return out, int(np.argmax(out)), 0                         # (np.argmax: the first of equal maxima)


def _scan_tiles(x):
    """One level: x[n] -> (the prefixes inside every block of 1024, the block totals)."""
    n = len(x)
    blocks = -(-n // SCAN_TILE)
    pad = np.zeros(blocks * SCAN_TILE)
    pad[:n] = x
    v = pad.reshape(blocks, SCAN_LANES, SCAN_PER)
    runs = np.empty_like(v)
    runs[:, :, 0] = v[:, :, 0]
    for k in range(1, SCAN_PER):
        runs[:, :, k] = runs[:, :, k - 1] + v[:, :, k]
    lane = runs[:, :, SCAN_PER - 1].copy()
    d = 1
    while d < SCAN_LANES:
        lane = np.concatenate((lane[:, :d], lane[:, :-d] + lane[:, d:]), axis=1)
        d *= 2
    out = runs.copy()
    out[:, 1:, :] = lane[:, :-1, None] + runs[:, 1:, :]
    return out.reshape(-1)[:n], lane[:, -1].copy()


def cumsum_arrays(x):
    x = np.asarray(x, dtype=np.float64)
    out, totals = _scan_tiles(x)
    if len(x) > SCAN_TILE:
        prefix = cumsum_arrays(totals)
        i = np.arange(SCAN_TILE, len(x))
        out[SCAN_TILE:] = prefix[i // SCAN_TILE - 1] + out[SCAN_TILE:]
    return out


class _Impl:
    def __init__(self, assign, update, seed, cumsum):
        self.assign, self.update, self.seed, self.cumsum = assign, update, seed, cumsum


LOOPS = _Impl(assign_loops, update_loops, seed_loops, cumsum_loops)
ARRAYS = _Impl(assign_arrays, update_arrays, seed_arrays, cumsum_arrays)


# ---------------------------------------------------------------------------------------------------------------------------------
# vf_nerf_amd/cluster.py
# ---------------------------------------------------------------------------------------------------------------------------------
def first_index(u, n):
    return min(int(math.floor(float(np.float64(u) * np.float64(n)))), n - 1)


def seeds_farthest(points, k, impl=ARRAYS):
    """-> the indices of the k seeds: the point farthest from the mean (``update`` with k = 1), then the farthest from the seeds so far."""
    p = np.asarray(points, dtype=np.float64)
    mean = impl.update(p, np.zeros(len(p), dtype=np.int32), np.zeros((1, 3)))[2]
    _, far = impl.assign(p, mean)
    mind2, index, _ = impl.seed(p, None, False, far)
    out = [index]
    for t in range(1, k):
        mind2, index, _ = impl.seed(p, out[-1], t == 1, mind2)
        out.append(index)
    return out


def seeds_d2(points, k, u, impl=ARRAYS):
    """-> the indices of the k seeds by plain D^2 sampling from the uniforms u[k]."""
    p = np.asarray(points, dtype=np.float64)
    n = len(p)
    out, mind2 = [first_index(u[0], n)], None
    for t in range(1, k):
        mind2 = impl.seed(p, out[-1], t == 1, mind2)[0]
        cum = np.maximum.accumulate(impl.cumsum(mind2))
        total = cum[n - 1]
        if total == 0:
            out.append(first_index(u[t], n))
        else:
            out.append(min(int(np.searchsorted(cum, np.float64(u[t]) * total, side="right")), n - 1))
    return out


def lloyd(points, centres, max_iter, impl=ARRAYS):
    p = np.asarray(points, dtype=np.float64)
    centres = np.array(centres, dtype=np.float64, copy=True)
    label, counts, t = None, None, 0
    while True:
        t += 1
        previous = label
        label, sqdist = impl.assign(p, centres)
        if t > 1 and np.array_equal(label, previous):
            return centres, label, counts, sqdist, t, True
        if t == max_iter:
            return centres, label, impl.update(p, label, centres)[1], sqdist, t, False
        _, counts, centres, _ = impl.update(p, label, centres)


def kmeans(points, k, init="farthest", n_init=1, max_iter=300, seed=None, impl=ARRAYS):
    """``cluster.kmeans`` -> {field: value}, labels int64."""
    p = np.asarray(points, dtype=np.float64)
    uniforms = np.random.default_rng(seed).random((n_init, k)) if isinstance(init, str) and init == "k-means++" else None
    best = None
    for r in range(n_init):
        if uniforms is not None:
            start = p[seeds_d2(p, k, uniforms[r], impl)]
        elif isinstance(init, str):
            start = p[seeds_farthest(p, k, impl)]
        else:
            start = np.asarray(init, dtype=np.float64)
        centres, label, counts, sqdist, n_iter, converged = lloyd(p, start, max_iter, impl)
        inertia = M3.stats_sum(sqdist)
        if best is None or inertia < best["inertia"]:
            best = dict(centres=centres, labels=label.astype(np.int64), counts=counts, sqdist=sqdist, inertia=inertia, n_iter=n_iter,
                        converged=converged, restart=r)
    return best


# ---------------------------------------------------------------------------------------------------------------------------------
# vf_nerf_amd/meshops.py: simplify_to_faces, dominant_bases
# ---------------------------------------------------------------------------------------------------------------------------------
def simplify_to_faces(vertices, faces, target_faces, contraction="quadric", steps=16):
    """-> (the restated ``Simplified`` of tests/simplify_restatement.py, the voxel edge, [(edge, faces) of every candidate])."""
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    used = np.unique(f.reshape(-1))
    lower, upper = v[used].min(axis=0).tolist(), v[used].max(axis=0).tolist()
    extent = max(hi - lo for lo, hi in zip(lower, upper))
    lo, hi = extent / 2.0 ** 20, extent
    fitting, coarsest, tried = None, None, []
    for _ in range(steps):
        h = math.sqrt(lo * hi)
        s = S.simplify_arrays(v, f, h, contraction)
        count = len(s["faces"])
        tried.append((h, count))
        if count > target_faces:
            lo = h
        else:
            hi = h
            if fitting is None or count > fitting[0]:
                fitting = (count, h, s)
        if coarsest is None or h > coarsest[1]:
            coarsest = (count, h, s)
    _, h, s = fitting if fitting is not None else coarsest
    return s, h, tried


def dominant_bases(vertices, faces, num_bases, voxel_size=None, decimation=None, unit=False, **kmeans_args):
    """``meshops.dominant_bases`` without ``orient`` -> {bases, counts, labels, inertia, n_iter, converged, n_vertices, n_faces,
    voxel_size}."""
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    h = voxel_size
    if voxel_size is not None:
        s = S.simplify_arrays(v, f, voxel_size, "quadric")
        v, f = s["vertices"], s["faces"]
    elif decimation is not None:
        s, h, _ = simplify_to_faces(v, f, max(1, math.floor(decimation * len(f))))
        v, f = s["vertices"], s["faces"]
    used = np.unique(f.reshape(-1))
    normals = np.ascontiguousarray(M.vertex_normals(v, f)[used])
    km = kmeans(normals, num_bases, **kmeans_args)
    order = np.argsort(-km["counts"], kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(num_bases)
    bases = km["centres"][order]
    if unit:
        length = np.sqrt((bases[:, 0] * bases[:, 0] + bases[:, 1] * bases[:, 1]) + bases[:, 2] * bases[:, 2])[:, None]
        bases = np.where(length > 0, bases / np.where(length > 0, length, 1.0), bases)
    return dict(bases=bases, counts=km["counts"][order], labels=rank[km["labels"]], inertia=km["inertia"], n_iter=km["n_iter"],
                converged=km["converged"], n_vertices=len(normals), n_faces=len(f), voxel_size=h)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
AXES = np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])


def blobs(n, seed, spread=0.15):
    """n seeded unit vectors around the six axis directions (what the vertex normals of a room look like)."""
    g = np.random.default_rng(seed)
    x = AXES[g.integers(0, 6, n)] + spread * g.normal(size=(n, 3))
    return x / np.linalg.norm(x, axis=1)[:, None]


def sphere(n, seed):
    """n seeded unit vectors, uniform on the sphere."""
    x = np.random.default_rng(seed).normal(size=(n, 3))
    return x / np.linalg.norm(x, axis=1)[:, None]


def labelled_ramp(n, k):
    """The input of the stand-alone ``update`` case: points that differ in every row, labels that cycle through the k clusters."""
    i = np.arange(n, dtype=np.float64)
    points = np.stack((i * 0.125 + 0.1, 1.0 - i * 1e-7, np.sin(i)), axis=1)
    return points, (np.arange(n) % k).astype(np.int32)


def flat_cube():
    """The unit cube as six separate squares (24 vertices, 12 faces, wound outwards): every vertex normal is exactly an axis direction."""
    v, f = [], []
    for axis in range(3):
        for side in (0.0, 1.0):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            corners = []
            for s, t in ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)):
                p = [0.0, 0.0, 0.0]
                p[axis], p[a], p[b] = side, s, t
                corners.append(p)
            base = len(v)
            v += corners
            quad = [(0, 1, 2), (0, 2, 3)] if side else [(0, 2, 1), (0, 3, 2)]
            f += [[base + i for i in tri] for tri in quad]
    return np.array(v), np.array(f, dtype=np.int64)
