"""Clustering points on the device (csrc/vfn_kmeans.hip, include/vfn.h): Lloyd's k-means over points in space, the step of
``get_dominant_bases`` (utils/utils.py:216-233) that the reference leaves to ``sklearn.cluster.KMeans`` once it has decimated a mesh and
taken its ``vertex_normals`` — ``meshops.dominant_bases`` is that function on the device.

* ``kmeans`` — seeds, then passes of ``vfn_kmeans_assign`` (the nearest centre, ties to the lowest cluster) and ``vfn_kmeans_update`` (the
  means, their sums along the fixed tree of include/vfn.h) until no label changes.  ONE 8-byte host read per pass, the number of labels
  that changed, as ``icp.align`` reads once per iteration.

A specification of ours: the plain float64 Lloyd iteration, without contraction and without floating-point atomics, so that every output
bit is a function of the data alone; tests/kmeans_restatement.py restates it in NumPy twice and the device is held to it bit for bit.
From the same seeds it agrees with scikit-learn's ``KMeans(init=seeds, n_init=1, algorithm="lloyd", tol=0)`` in every label and in the
number of iterations, and in the centres to rounding (tests/test_kmeans_host.py).  NOT verified: scikit-learn's own seeding — its greedy
k-means++ and its random stream; the seeding here is ours (``init``).

Inputs are numpy arrays or torch tensors on any device.  No CPU fallback: ``lib.VfnError`` when no device is visible.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np
import torch

from . import geomargs, lib
from .geomargs import LIMIT

INITS = ("farthest", "k-means++")
MAX_ITER = 300                         # scikit-learn's default

_device = functools.partial(geomargs.device, what="k-means")       # (a module attribute, so a test can stand in for the device)


def __getattr__(name: str):
    if name == "MAX_K":                # include/vfn.h's, read on first use
        return lib.kmeans_max_k()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class KMeans(NamedTuple):
    """What ``kmeans`` returns: device tensors, except ``n_iter``, ``converged`` and ``restart``."""
    centres: torch.Tensor                      # [k,3] float64
    labels: torch.Tensor                       # [n] int64: ``assign(points, centres)``
    counts: torch.Tensor                       # [k] int64: the points that carry each label, exact
    sqdist: torch.Tensor                       # [n] float64: every point's squared distance from its centre
    inertia: torch.Tensor                      # [] float64: the sum of ``sqdist`` along the fixed tree (``vfn_reduce_stats``)
    n_iter: int                                # passes (assignments) made
    converged: bool                            # the last pass changed no label
    restart: int                               # which of the ``n_init`` runs this is


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


def check_arguments(k, init, n_init, max_iter, seed):
    """The checks of ``kmeans`` that need neither the points nor a device -> (k, init, n_init, max_iter, seed); ``init`` is one of
    ``INITS`` or a host float64 array [k,3] of finite centres."""
    k = geomargs.positive_int(k, "k")
    if k > lib.kmeans_max_k():
        raise ValueError(f"k must be at most {lib.kmeans_max_k()}, got {k}")
    n_init, max_iter = geomargs.positive_int(n_init, "n_init"), geomargs.positive_int(max_iter, "max_iter")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or int(seed) < 0):
        raise ValueError(f"seed must be None or an integer >= 0, got {seed!r}")
    if isinstance(init, str):
        if init not in INITS:
            raise ValueError(f"init must be one of {INITS} or an array [k,3], got {init!r}")
    else:
        c = geomargs.as_tensor(init, "init")
        if tuple(c.shape) != (k, 3) or not c.dtype.is_floating_point:
            raise ValueError(f"init must be one of {INITS} or floating point [{k},3], got {c.dtype} {tuple(c.shape)}")
        init = c.to("cpu", torch.float64).numpy().copy()
        if not np.isfinite(init).all():
            raise ValueError("init: a non-finite centre")
    if n_init != 1 and not (isinstance(init, str) and init == "k-means++"):
        raise ValueError(f"n_init must be 1 unless init is 'k-means++' (the other seedings are deterministic), got {n_init}")
    return k, init, n_init, max_iter, None if seed is None else int(seed)


def first_index(u: float, n: int) -> int:
    """min(floor(u n), n - 1) in float64: the uniform draw of an index."""
    return min(int(math.floor(float(np.float64(u) * np.float64(n)))), n - 1)


class _Work:
    """The buffers of one call: allocated once, whatever the number of passes and restarts."""

    def __init__(self, p: torch.Tensor, k: int):
        n, dev = p.shape[0], p.device
        self.state = torch.zeros(3, dtype=torch.int64, device=dev)          # the changed count, the status word, a count nobody reads
        self.changed, self.info, self.ignored = self.state[0:1], self.state[1:2], self.state[2:3]
        self.update_ws = lib.kmeans_update_workspace(n, k, dev)
        self.seed_ws = lib.kmeans_seed_workspace(n, dev)
        self.mind2 = torch.empty(n, dtype=torch.float64, device=dev)
        self.index = torch.zeros(k, dtype=torch.int64, device=dev)


def _seeds_farthest(p: torch.Tensor, k: int, w: _Work) -> torch.Tensor:
    """-> centres[k,3]: the point farthest from the mean, then k - 1 times the point farthest from the seeds so far.  No host read."""
    n, dev = p.shape[0], p.device
    mean = torch.zeros(1, 3, dtype=torch.float64, device=dev)
    label = torch.zeros(n, dtype=torch.int32, device=dev)
    lib.kmeans_update(p, label, mean, info=w.info)                          # the mean is ``update`` with k = 1
    lib.kmeans_assign(p, mean, None, label, w.mind2, w.ignored, info=w.info)
    lib.kmeans_seed(p, None, False, w.mind2, w.index[0:1], info=w.info, workspace=w.seed_ws)
    for t in range(1, k):
        lib.kmeans_seed(p, w.index[t - 1:t], t == 1, w.mind2, w.index[t:t + 1], info=w.info, workspace=w.seed_ws)
    return p[w.index].contiguous()


def _seeds_d2(p: torch.Tensor, k: int, u: np.ndarray, w: _Work) -> torch.Tensor:
    """-> centres[k,3] by plain D^2 sampling from the k uniforms ``u`` of this restart.  No host read: the uniform fall-back indices are
    computed on the host beforehand and chosen on the device where the distances add up to nothing."""
    n, dev = p.shape[0], p.device
    uniform = torch.tensor([first_index(x, n) for x in u], dtype=torch.int64, device=dev)
    u_dev = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64)).to(dev)
    w.index[0:1] = uniform[0:1]
    for t in range(1, k):
        lib.kmeans_seed(p, w.index[t - 1:t], t == 1, w.mind2, None, info=w.info)
        cum = torch.cummax(lib.cumsum_f64(w.mind2), dim=0)[0]               # (the scan may step down by an ulp: the running maximum is exact)
        total = cum[n - 1]
        drawn = torch.searchsorted(cum, (u_dev[t] * total).reshape(1), right=True).clamp(max=n - 1)          # the first i with cum[i] > u total
        w.index[t:t + 1] = torch.where(total == 0, uniform[t:t + 1], drawn)
    return p[w.index].contiguous()


def _lloyd(p: torch.Tensor, centres: torch.Tensor, max_iter: int, w: _Work):
    """Device points and seeds (``centres`` is written) -> (labels int32, counts, sqdist, n_iter, converged).  One host read per pass:
    8 bytes, the changed count — the first pass reads the status word with it, so that a non-finite input ends the loop at once."""
    n, k, dev = p.shape[0], centres.shape[0], p.device
    label = torch.empty(n, dtype=torch.int32, device=dev)
    sqdist = torch.empty(n, dtype=torch.float64, device=dev)
    counts, t = None, 0
    while True:
        t += 1
        w.changed.zero_()
        lib.kmeans_assign(p, centres, None if t == 1 else label, label, sqdist, w.changed, info=w.info)
        if t == 1:
            changed, status = (int(x) for x in w.state[0:2].cpu())
            lib.kmeans_check(status)
        else:
            changed = int(w.changed.cpu())
        if t > 1 and changed == 0:
            return label, counts, sqdist, t, True
        if t == max_iter:
            # the counts of the labels returned: an update whose centres are thrown away
            _, counts = lib.kmeans_update(p, label, centres.clone(), info=w.info, workspace=w.update_ws)
            return label, counts, sqdist, t, False
        _, counts = lib.kmeans_update(p, label, centres, info=w.info, workspace=w.update_ws)


def kmeans(points, k, init="farthest", n_init: int = 1, max_iter: int = MAX_ITER, seed=None, device=None) -> KMeans:
    """points[n,3] -> ``KMeans`` on the device: k centres by Lloyd's iteration in float64 (csrc/vfn_kmeans.hip; include/vfn.h has the
    specification).  Pass t assigns every point to its nearest centre — squared distances in the association of ``vfn_nn_radius``, a
    tie going to the LOWEST cluster; if no label changed (after pass 1) the call stops with ``converged=True``; if t == ``max_iter`` it
    stops with ``converged=False``; otherwise every centre becomes the mean of its points — the sums along the fixed tree of
    include/vfn.h, lane order "near", an EMPTY cluster keeping its centre's bits (it shows in ``counts``) — and the next pass follows.
    Under both stops ``labels``, ``sqdist`` and ``inertia`` are exactly the assignment against the returned ``centres``; under
    ``converged=True`` the centres are also the update of the returned labels, bit for bit.  ``n_iter`` counts the passes, which is
    scikit-learn's ``n_iter_`` with ``tol=0``.

    ``init="farthest"`` (deterministic, no seed): the point farthest from the mean, then k - 1 times the point with the greatest squared
    distance from the seeds so far, ties to the lowest index; ``n_init`` must be 1.  ``init="k-means++"``: plain D^2 sampling from
    ``u = numpy.random.default_rng(seed).random((n_init, k))``: restart r takes the point ``min(floor(u[r,0] n), n - 1)`` first, then for
    t = 1 .. k - 1 the first i with ``cum[i] > u[r,t] cum[n-1]`` (clipped to n - 1), ``cum`` the running maximum of ``vfn_cumsum_f64`` of
    the squared distances from the seeds so far, or ``min(floor(u[r,t] n), n - 1)`` when ``cum[n-1] == 0``; the restart with the lowest
    inertia wins, ties to the lowest restart (one more host read per restart).  This is NOT scikit-learn's greedy k-means++ (which
    tries 2 + log k candidates per seed) and NOT its random stream.  ``init`` = an array [k,3]: the centres as they are, checked finite
    on the host.

    ValueError before any launch on points that are not floating point [n,3] with 1 <= n < 2^31, a k outside [1, 64], an unknown
    ``init``, ``n_init`` / ``max_iter`` < 1 and ``n_init`` > 1 without k-means++; a NaN / inf coordinate raises ``lib.VfnError``."""
    k, init, n_init, max_iter, seed = check_arguments(k, init, n_init, max_iter, seed)
    p = _check_points(points, "points")
    dev = _device(device if device is not None else (p.device if p.is_cuda else None))
    p = p.to(dev, torch.float64).contiguous()
    n = p.shape[0]
    uniforms = np.random.default_rng(seed).random((n_init, k)) if isinstance(init, str) and init == "k-means++" else None
    best = None
    with torch.cuda.device(dev):
        w = _Work(p, k)
        for r in range(n_init):
            if uniforms is not None:
                centres = _seeds_d2(p, k, uniforms[r], w)
            elif isinstance(init, str):
                centres = _seeds_farthest(p, k, w)
            else:
                centres = torch.from_numpy(init).to(dev)
            label, counts, sqdist, n_iter, converged = _lloyd(p, centres, max_iter, w)
            inertia = lib.reduce_stats(sqdist, 0.0)[0]
            if n_init > 1:                                                  # the read that ranks the restarts
                value = float(inertia.cpu())
                if best is not None and not value < best[0]:
                    continue
                best = (value, KMeans(centres, label, counts, sqdist, inertia, n_iter, converged, r))
            else:
                best = (None, KMeans(centres, label, counts, sqdist, inertia, n_iter, converged, r))
        lib.kmeans_check(int(w.info.cpu()))                                 # the final status word
        out = best[1]
        return out._replace(labels=out.labels.to(torch.int64))
