"""Aligning one point set to another on the device (csrc/vfn_icp.hip): point-to-point ICP, the ``icp_align`` step that the reference's
``metrics_3d_no_vf`` (evaluation/methods.py:747-801) leaves to the external ``evaluate_3d_reconstruction`` package.

* ``nearest_within`` — every query's nearest target within a radius, WITH its index: exact and bit-defined (include/vfn.h:
  ``vfn_nn_radius``); ties go to the lowest target index, a query without a target in reach gets index -1 and distance +inf.  A uniform
  grid over the targets bounds the work and changes no bit of the result.
* ``align`` — the ICP loop: search, 17 sums on the device (``vfn_icp_accumulate``), ONE host read per iteration, a rigid 3 x 3 solve on
  the host in float64 (rotation + translation, no scale).
* ``transform_points`` — a point set under a 4 x 4 rigid transformation, with the arithmetic the search applies on the fly.
* ``align_stages`` — ``align`` coarse to fine on voxel-down-sampled copies (``metrics3d.voxel_down_sample``), the staged registration of
  the external package's protocol; rigid, no scale.

This is a specification, not a recording: neither Open3D nor the external package is available to compare against, and neither
publishes its arithmetic.  The defaults that imitate Open3D's ``registration_icp`` — 30 iterations, relative fitness / rmse criteria of
1e-6 — are ours and NOT verified against Open3D.  tests/icp_restatement.py restates the contract in NumPy and the device is held to it.

Inputs are numpy arrays or torch tensors on any device.  No CPU fallback: ``lib.VfnError`` when no device is visible.
"""
from __future__ import annotations

import dataclasses
import functools
import math
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import geomargs, lib
from .geomargs import LIMIT

# GRID_CAP (cells per axis at most: 128^3 + 1 int32 entries = 8 MiB however small the radius is) and GRID_MARGIN (cell edge >= radius
# (1 + 2^-20): csrc/vfn_icp.hip proves the 27 cells sufficient with it) are include/vfn.h's, read on first use (module __getattr__)
MAX_ITERATION, RELATIVE_FITNESS, RELATIVE_RMSE = 30, 1e-6, 1e-6      # ours; they imitate Open3D's defaults, not verified against it
RANK_TOLERANCE = 1e-12                 # second singular value / first below this: the correspondences are (numerically) collinear

_device = functools.partial(geomargs.device, what="point-set alignment")       # (a module attribute, so a test can stand in for the device)


def __getattr__(name: str):
    if name in ("GRID_CAP", "GRID_MARGIN"):
        return lib.icp_grid_limits()[name == "GRID_MARGIN"]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


@dataclasses.dataclass
class Grid:
    """The targets of a search, sorted by grid cell (include/vfn.h: vfn_nn_radius)."""
    targets: torch.Tensor              # [m,3] as given (original order)
    sorted_targets: torch.Tensor       # [m,3] in ascending cell key
    perm: torch.Tensor                 # [m] int64: sorted position -> original index
    cell_start: torch.Tensor           # [cells + 1] int32
    box: Tuple[float, ...]             # min[3], max[3], cell edge
    dims: Tuple[int, int, int]
    radius: float                      # 0.0: the grid of the unbounded search (metrics3d.nearest_grid), which vfn_nn_radius refuses

    @property
    def anchor(self) -> Tuple[float, float, float]:
        """The centre of the targets' bounding box: what the sums of ``align`` are taken about."""
        return tuple(0.5 * (self.box[k] + self.box[3 + k]) for k in range(3))

    def args(self):
        return self.sorted_targets, self.perm, self.cell_start, self.box, self.dims

    def nearest_args(self):
        """What ``lib.nn_nearest`` takes: the same, after the targets in their original order (its all-pairs launch reads those)."""
        return (self.targets,) + self.args()


@dataclasses.dataclass
class Result:
    transformation: np.ndarray         # host float64 [4,4]: source -> target
    fitness: float                     # correspondences / source points
    inlier_rmse: float                 # sqrt(sum d^2 / correspondences), 0 without correspondences
    iterations: int                    # updates of the transformation made
    converged: bool
    history: List[dict]                # per search: transformation (the one searched with), count, fitness, inlier_rmse


def _check_points(x, name: str) -> torch.Tensor:
    t = geomargs.as_tensor(x, name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be [n,3], got {tuple(t.shape)}")
    if not t.dtype.is_floating_point:
        raise ValueError(f"{name} must be floating point, got {t.dtype}")
    if t.shape[0] < 1:
        raise ValueError(f"{name} is empty")
    if t.shape[0] >= LIMIT:
        raise ValueError(f"{name}: {t.shape[0]} rows exceed the 2^31 limit of one call")
    return t


def _check_radius(radius, name: str = "radius") -> float:
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a real number, got {radius!r}")
    r = float(radius)
    if not math.isfinite(r) or r <= 0 or not math.isfinite(r * r) or r * r < 2.0 ** -1022:
        raise ValueError(f"{name} must be finite and > 0 with a normal square, got {radius!r}")
    return r


def _check_transform(transformation, name: str) -> Optional[np.ndarray]:
    """None, or a finite [4,4] whose last row is 0 0 0 1 -> float64 numpy (rigidity is the caller's business)."""
    if transformation is None:
        return None
    t = geomargs.as_tensor(transformation, name)
    if tuple(t.shape) != (4, 4) or not t.dtype.is_floating_point:
        raise ValueError(f"{name} must be floating point [4,4], got {t.dtype} {tuple(t.shape)}")
    m = t.to("cpu", torch.float64).numpy().copy()
    if not np.isfinite(m).all():
        raise ValueError(f"{name} has a non-finite entry")
    if not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f"{name}: the last row must be 0 0 0 1, got {m[3].tolist()}")
    return m


def _twelve(m: Optional[np.ndarray]):
    """[4,4] -> the 12 floats of include/vfn.h (rows of the rotation, then the translation); None stays None (the identity)."""
    return None if m is None else [float(x) for x in m[:3, :3].reshape(-1)] + [float(x) for x in m[:3, 3]]


def _dev_points(t: torch.Tensor, dev: torch.device) -> torch.Tensor:
    return t.to(dev, torch.float64).contiguous()


def _cells(points: torch.Tensor, box, dims, dev) -> torch.Tensor:
    """The cell key of every point in the expression of include/vfn.h, in torch on the device (a true division: the divisor is a device
    tensor, not a host scalar that torch would turn into a multiplication by its reciprocal)."""
    lo = torch.tensor(box[0:3], dtype=torch.float64, device=dev)
    hi = torch.tensor(box[3:6], dtype=torch.float64, device=dev)
    h = torch.tensor(box[6], dtype=torch.float64, device=dev)
    top = torch.tensor([d - 1 for d in dims], dtype=torch.float64, device=dev)
    c = torch.floor((torch.minimum(torch.maximum(points, lo), hi) - lo) / h)
    c = torch.minimum(torch.clamp_min(c, 0.0), top).to(torch.int64)
    return (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]


def build_grid(targets: torch.Tensor, radius: float, edge=None) -> Grid:
    """Device targets [m,3] float64 -> their ``Grid`` for searches within ``radius``.  Plumbing in torch: the bounding box (six values
    cross to the host), the cell edge, a stable sort by cell key, the table of first positions.  ``edge`` (a function of the box's three
    extents) chooses the cell edge instead: the grid of the unbounded search (``metrics3d.nearest_grid``), which has no radius.

    Cell edge h = radius (1 + 2^-20), enlarged to extent / 128 (1 + 2^-20) on the longest axis when that is larger: at most
    GRID_CAP = 128 cells an axis, so the table never exceeds 128^3 + 1 entries when the radius is tiny against the extent (the cells
    then simply hold more targets)."""
    dev = targets.device
    box = torch.cat((targets.min(dim=0).values, targets.max(dim=0).values)).cpu().tolist()
    if not all(math.isfinite(b) for b in box):
        lib.nn_check(lib.GEOM_STATUS_NONFINITE)
    extent = [box[3 + k] - box[k] for k in range(3)]
    if not all(math.isfinite(e) for e in extent):
        raise lib.VfnError("point-set alignment: the targets' bounding box overflows float64")
    cap, margin = lib.icp_grid_limits()
    if edge is None:
        h = radius * margin
        h = max([h] + [e / cap * margin for e in extent])
    else:
        h = edge(extent)
    dims = tuple(min(cap, int(math.floor(e / h)) + 1) for e in extent)
    box = tuple(box) + (h,)
    key = _cells(targets, box, dims, dev)
    sorted_key, perm = torch.sort(key, stable=True)
    cells = dims[0] * dims[1] * dims[2]
    cell_start = torch.searchsorted(sorted_key, torch.arange(cells + 1, dtype=torch.int64, device=dev)).to(torch.int32)
    return Grid(targets, targets[perm].contiguous(), perm.contiguous(), cell_start.contiguous(), box, dims, radius)


def query_order(queries: torch.Tensor, transformation: Optional[np.ndarray], grid: Grid) -> torch.Tensor:
    """A permutation of the queries by the cell they (roughly) fall in under ``transformation``, so that neighbouring lanes read
    neighbouring cells.  Only speed depends on it (its arithmetic is torch's, not the contract's)."""
    p = queries
    if transformation is not None:
        m = torch.from_numpy(transformation).to(queries.device)
        p = queries @ m[:3, :3].T + m[:3, 3]
    return torch.argsort(_cells(p, grid.box, grid.dims, queries.device)).contiguous()


def search(queries: torch.Tensor, transformation: Optional[np.ndarray], grid: Grid, order: Optional[torch.Tensor] = None,
           info: Optional[torch.Tensor] = None, check_finite: bool = True):
    """Device queries, a checked [4,4] (or None) and a ``Grid`` -> (index, sqdist) on the device."""
    return lib.nn_radius(queries, _twelve(transformation), grid.args(), grid.radius, order=order, info=info, check_finite=check_finite)


def nearest_within(queries, targets, radius, transform=None, device=None):
    """queries[n,3], targets[m,3] -> (index[n] int64, sqdist[n] float64) on the device: for every query moved by ``transform`` ([4,4],
    None = as it is) the index of, and the SQUARED distance to, its nearest target among those with squared distance <= radius^2;
    ties to the lowest index; -1 and +inf when no target is in reach.  A NaN / inf coordinate raises ``lib.VfnError``."""
    q, t = _check_points(queries, "queries"), _check_points(targets, "targets")
    radius = _check_radius(radius)
    m = _check_transform(transform, "transform")
    dev = _device(device)
    with torch.cuda.device(dev):
        q, t = _dev_points(q, dev), _dev_points(t, dev)
        grid = build_grid(t, radius)
        return search(q, m, grid, order=query_order(q, m, grid))


def transform_points(points, transformation, device=None) -> torch.Tensor:
    """points[n,3] under the [4,4] ``transformation`` -> device float64 [n,3]: ((r00 x + r01 y) + r02 z) + t0 and so on, the expression
    the search applies on the fly."""
    p = _check_points(points, "points")
    m = _check_transform(transformation, "transformation")
    if m is None:
        raise ValueError("transformation must be a [4,4] matrix, got None")
    dev = _device(device)
    with torch.cuda.device(dev):
        return lib.transform_points(_dev_points(p, dev), _twelve(m))


def rigid_from_sums(sums, anchor) -> np.ndarray:
    """The 17 sums of ``vfn_icp_accumulate`` about ``anchor`` -> the [4,4] rigid update U (rotation and translation, no scale) that
    minimises sum |U p - s|^2 over the correspondences: means from the sums, H = sum (p - a)(s - a)^T - c pbar sbar^T, its SVD with
    the reflection fixed by diag(1, 1, det), translation = sbar - R pbar with the anchor added back.  Host float64; not bit-pinned."""
    sums, a = np.asarray(sums, dtype=np.float64), np.asarray(anchor, dtype=np.float64)
    count = sums[0]
    if count < 3:
        raise lib.VfnError(f"point-set alignment: fewer than 3 correspondences ({int(count)}): no rigid transformation is determined")
    pbar, sbar = sums[2:5] / count, sums[5:8] / count
    h = sums[8:17].reshape(3, 3) - count * np.outer(pbar, sbar)
    u, sv, vt = np.linalg.svd(h)
    if not (np.isfinite(sv).all() and sv[0] > 0 and sv[1] > RANK_TOLERANCE * sv[0]):
        raise lib.VfnError("point-set alignment: rank-deficient correspondences (collinear or coincident points): no rotation is determined")
    d = np.diag([1.0, 1.0, float(np.sign(np.linalg.det(vt.T @ u.T)))])
    r = vt.T @ d @ u.T
    out = np.eye(4)
    out[:3, :3] = r
    out[:3, 3] = (sbar + a) - r @ (pbar + a)
    return out


def align(source_points, target_points, max_correspondence_distance, init=None, max_iteration: int = MAX_ITERATION,
          relative_fitness: float = RELATIVE_FITNESS, relative_rmse: float = RELATIVE_RMSE, device=None) -> Result:
    """Point-to-point ICP of ``source_points`` onto ``target_points`` -> ``Result``.  Per iteration: the nearest target within
    ``max_correspondence_distance`` of every source point under the current transformation (``init`` or the identity at first),
    the 17 sums, one host read; stop when both |fitness - previous| < relative_fitness and |rmse - previous| < relative_rmse
    (``converged``) or after ``max_iteration`` updates; otherwise solve and compose T <- U T.  The source points are never rewritten.
    The coordinates are checked for NaN / inf by the first search only (the arrays do not change), and the queries are re-sorted by
    cell under every new transformation: as the cloud moves, a stale order makes a wave's lanes read different cells (measured:
    DESIGN 6l).  The defaults imitate Open3D's and are not verified against it."""
    return _align(source_points, target_points, max_correspondence_distance, init, max_iteration, relative_fitness, relative_rmse, device,
                  reorder=True)


@dataclasses.dataclass
class StagedResult(Result):
    """``Result`` of ``align_stages``: ``transformation`` is the composed one, ``fitness`` / ``inlier_rmse`` / ``converged`` the last stage's,
    ``iterations`` the total, ``history`` every stage's searches one after the other (each entry with its "stage"; an entry's
    transformation is its stage's own, from the identity, of the source as that stage received it)."""
    stages: List[dict]                 # per stage: voxel_size, the radius, source_points / target_points after down-sampling, and
                                       # that stage's transformation, fitness, inlier_rmse, iterations, converged


def compose(a, b) -> np.ndarray:
    """The rigid [4,4] a . b in plain Python floats: every entry of the 3 x 3 block the sum of three products in ascending k,
    (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j, the translation that sum over b's translation plus a's; last row 0 0 0 1.  No BLAS enters
    the bits."""
    a, b = [[float(x) for x in row] for row in a], [[float(x) for x in row] for row in b]
    out = np.eye(4)
    for i in range(3):
        for j in range(4):
            s = (a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j]
            out[i, j] = s + a[i][3] if j == 3 else s
    return out


def _check_stages(stages) -> List[tuple]:
    from . import voxel                 # (metrics3d imports this module and voxel alike)
    if isinstance(stages, (str, bytes)) or not hasattr(stages, "__iter__"):
        raise ValueError(f"stages must be a sequence of (voxel_size or None, max_correspondence_distance, max_iteration), got {stages!r}")
    out = []
    for k, stage in enumerate(stages):
        if isinstance(stage, (str, bytes)) or not hasattr(stage, "__len__") or len(stage) != 3:
            raise ValueError(f"stages[{k}] must be (voxel_size or None, max_correspondence_distance, max_iteration), got {stage!r}")
        size, radius, iterations = stage
        size = None if size is None else voxel.check_voxel_size(size, f"stages[{k}] voxel_size")
        radius = _check_radius(radius, f"stages[{k}] max_correspondence_distance")
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or int(iterations) < 0:
            raise ValueError(f"stages[{k}] max_iteration must be a non-negative integer, got {iterations!r}")
        out.append((size, radius, int(iterations)))
    if not out:
        raise ValueError("stages is empty")
    return out


def align_stages(source_points, target_points, stages, init=None, device=None) -> StagedResult:
    """The staged registration of the ``evaluate_3d_reconstruction`` protocol: coarse to fine on voxel-down-sampled copies.  ``stages`` is
    a sequence of (voxel_size or None, max_correspondence_distance, max_iteration).  With T = ``init`` (or the identity), per stage:
    the source is moved by T (``transform_points``); the moved source and the target are down-sampled at the stage's voxel size
    (``metrics3d.voxel_down_sample``; None: taken as they are); ``align`` runs on the two from the identity; T <- T_stage . T
    (``compose``: Python floats, no BLAS).  -> ``StagedResult``.

    Rigid, with NO scale: the Tanks-and-Temples evaluation scripts that this schedule follows estimate a scale in their registration;
    this does not.  The schedule, like ``align`` and the down-sampling, is a specification of ours, not verified against Open3D or the
    external package."""
    from . import voxel
    src, tgt = _check_points(source_points, "source_points"), _check_points(target_points, "target_points")
    stages = _check_stages(stages)
    t_k = _check_transform(init, "init")
    dev = _device(device)
    with torch.cuda.device(dev):
        src, tgt = _dev_points(src, dev), _dev_points(tgt, dev)
        t_k = np.eye(4) if t_k is None else t_k
        history: List[dict] = []
        report: List[dict] = []
        targets = {None: tgt}              # the target down-sampled once per voxel size
        for k, (size, radius, iterations) in enumerate(stages):
            moved = lib.transform_points(src, _twelve(t_k))
            if size is not None:
                moved = voxel.down_sample_device(moved, size).points
                if size not in targets:
                    targets[size] = voxel.down_sample_device(tgt, size).points
            res = align(moved, targets[size], radius, max_iteration=iterations, device=dev)
            t_k = compose(res.transformation, t_k)
            history += [dict(entry, stage=k) for entry in res.history]
            report.append({"voxel_size": size, "max_correspondence_distance": radius, "source_points": int(moved.shape[0]),
                           "target_points": int(targets[size].shape[0]), "transformation": res.transformation, "fitness": res.fitness,
                           "inlier_rmse": res.inlier_rmse, "iterations": res.iterations, "converged": res.converged})
    return StagedResult(t_k, res.fitness, res.inlier_rmse, sum(s["iterations"] for s in report), res.converged, history, report)


def _align(source_points, target_points, max_correspondence_distance, init, max_iteration, relative_fitness, relative_rmse, device,
           reorder: bool) -> Result:
    """``align``; ``reorder=False`` sorts the queries once, under the initial transformation (tools/bench_icp.py measures the difference;
    no bit of the result depends on it)."""
    src, tgt = _check_points(source_points, "source_points"), _check_points(target_points, "target_points")
    radius = _check_radius(max_correspondence_distance, "max_correspondence_distance")
    t_k = _check_transform(init, "init")
    if isinstance(max_iteration, bool) or not isinstance(max_iteration, (int, np.integer)) or int(max_iteration) < 0:
        raise ValueError(f"max_iteration must be a non-negative integer, got {max_iteration!r}")
    for name, x in (("relative_fitness", relative_fitness), ("relative_rmse", relative_rmse)):
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not float(x) >= 0:
            raise ValueError(f"{name} must be a number >= 0, got {x!r}")
    dev = _device(device)
    with torch.cuda.device(dev):
        src, tgt = _dev_points(src, dev), _dev_points(tgt, dev)
        grid = build_grid(tgt, radius)
        anchor = grid.anchor
        if t_k is None:
            t_k = np.eye(4)
        order = None
        n = src.shape[0]
        history: List[dict] = []
        updates, converged = 0, False
        while True:
            info = torch.zeros(1, dtype=torch.int64, device=dev)
            twelve = _twelve(t_k)
            if order is None or reorder:
                order = query_order(src, t_k, grid)
            index, sqdist = lib.nn_radius(src, twelve, grid.args(), radius, order=order, info=info, check_finite=not history)
            sums = lib.icp_accumulate(src, twelve, tgt, index, sqdist, anchor, info=info)
            host = torch.cat((sums, info.to(torch.float64))).cpu().numpy()          # the one read of the iteration
            lib.icp_check(int(host[lib.ICP_SUMS]))
            count = int(host[0])
            fitness = count / n
            rmse = math.sqrt(host[1] / count) if count else 0.0
            history.append({"transformation": t_k.copy(), "count": count, "fitness": fitness, "inlier_rmse": rmse})
            if len(history) > 1:
                prev = history[-2]
                if abs(fitness - prev["fitness"]) < relative_fitness and abs(rmse - prev["inlier_rmse"]) < relative_rmse:
                    converged = True
                    break
            if updates >= int(max_iteration):
                break
            t_k = rigid_from_sums(host[:lib.ICP_SUMS], anchor) @ t_k
            t_k[3] = [0.0, 0.0, 0.0, 1.0]
            updates += 1
    return Result(t_k, fitness, rmse, updates, converged, history)
