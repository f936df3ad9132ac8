#!/usr/bin/env python3
"""Device time of mesh scoring (vf_nerf_amd.metrics3d): the all-pairs nearest-neighbour search at n = m = 2^17, 10^6 and 2.5 x 10^6
(metrics_3d's and get_chamfer_distance's default point counts), the surface sampling of 10^6 points and the statistics
(lib.reduce_stats: sum, min, max, count) of 2.5 x 10^6 seeded values shaped like squared distances, on a mesh that
mesh.extract_mesh makes from the trained-weight scene of bench.py (the random-weight scene when the fixture is absent).  The two point
sets of a search are surface samples of that mesh and of a copy scaled by 1.01: what the scorer itself searches.

HIP events around each call, one warm-up call, --reps timed calls, the median reported (all repeats are listed).  Beside each search:

    pairs_per_s                    n x m / seconds
    fraction_of_fp64_vector_peak   9 fp64 lane-instructions per pair (3 subtracts, 3 multiplies, 2 adds, 1 min) against 39.3e12 per
                                   second: AMD's PUBLISHED 78.6 TFLOP/s of vector fp64 for the MI355X counted as FMAs (2 flops per
                                   lane-instruction).  It is the data-sheet figure, not a rate measured on this machine.
    ckdtree_build_s / _query_s     scipy.spatial.cKDTree(targets) and .query(queries, workers=16) on the same inputs on the same host,
                                   host clock; equal_to_ckdtree says whether the device's distances equal the tree's bit for bit.

--search grid (or both) adds, for every size and in the same process on the same two point sets, the grid search
(metrics3d.nearest: the timed interval is the grid build, the query order and both launches with the host read between them), whether
its distances equal the all-pairs kernel's bit for bit, the share of leftovers at the default max_rings, the number of queries that
stop after ring 0, 1, ... (ring passes alone, max_rings = 0 .. 8) and the three phases timed apart; and once, at the smallest size, a
DISJOINT pair (the queries moved 100 box widths away), where every query is a leftover and the all-pairs launch does all the work.

    python tools/bench_metrics3d.py [--sizes 131072 1000000 2500000] [--reps 3] [--search all_pairs|grid|both]
                                    [--out profiles/r08/bench_metrics3d.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PEAK_LANE_INSTRUCTIONS = 39.3e12     # published: 78.6e12 fp64 vector flop/s / 2 flops per FMA lane-instruction
INSTRUCTIONS_PER_PAIR = 9


def timed(fn, reps):
    """One warm-up call, then `reps` calls between HIP events -> (median seconds, all seconds, last result)."""
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return statistics.median(times), times, out


def ring_pass_leftovers(q, grid, max_rings, order):
    """The ring launch alone (no all-pairs launch) -> the number of queries that have not stopped after ring ``max_rings``."""
    import ctypes as C
    from vf_nerf_amd import lib
    n, m = q.shape[0], grid.sorted_targets.shape[0]
    index = torch.empty(n, dtype=torch.int64, device=q.device)
    sqdist = torch.empty(n, dtype=torch.float64, device=q.device)
    leftover = torch.empty(n, dtype=torch.int64, device=q.device)
    state = torch.zeros(2, dtype=torch.int64, device=q.device)
    lib._check(lib.load().vfn_nn_nearest(lib._ptr(q, "queries", torch.float64), n, lib._ptr(grid.sorted_targets, "sorted_targets", torch.float64),
                                         lib._ptr(grid.perm, "perm", torch.int64), m, lib._ptr(grid.cell_start, "cell_start", torch.int32),
                                         (C.c_double * 7)(*grid.box), grid.dims[0], grid.dims[1], grid.dims[2], max_rings,
                                         lib._ptr(order, "order", torch.int64), 0, lib._ptr(index, "index", torch.int64),
                                         lib._ptr(sqdist, "sqdist", torch.float64), lib._ptr(leftover, "leftover", torch.int64),
                                         lib._ptr(state[0:1], "leftover_count", torch.int64), lib._ptr(state[1:2], "info", torch.int64),
                                         lib._stream()), "vfn_nn_nearest")
    return int(state[0].cpu())


def grid_leg(q, tg, all_pairs_dist, all_pairs_seconds, reps):
    """One size of the --search grid leg (see the module docstring) -> its line."""
    from vf_nerf_amd import icp, lib, metrics3d
    n = q.shape[0]
    t, all_t, (index, dist) = timed(lambda: metrics3d.nearest(q, tg), reps)
    line = {"n": n, "m": tg.shape[0], "search": "grid", "seconds": round(t, 6), "all_seconds": [round(x, 6) for x in all_t],
            "includes": "grid build (one host read of the box), query order, ring launch, host read of the count, all-pairs launch over the leftovers",
            "max_rings": metrics3d.MAX_RINGS}
    if all_pairs_dist is not None:
        line.update({"all_pairs_seconds": round(all_pairs_seconds, 6), "speedup_over_all_pairs": round(all_pairs_seconds / t, 2),
                     "equal_to_all_pairs": bool(torch.equal(dist.view(torch.int64), all_pairs_dist.view(torch.int64)))})
    t_grid, _, grid = timed(lambda: metrics3d.nearest_grid(tg), reps)
    t_order, _, order = timed(lambda: icp.query_order(q, None, grid), reps)
    t_search, _, found = timed(lambda: lib.nn_nearest(q, grid.nearest_args(), metrics3d.MAX_RINGS, order=order), reps)
    left = [ring_pass_leftovers(q, grid, r, order) for r in range(metrics3d.MAX_RINGS + 1)]
    stops = [n - left[0]] + [left[r - 1] - left[r] for r in range(1, len(left))]
    line.update({"dims": list(grid.dims), "cell_edge": grid.box[6], "leftovers": found[2], "leftover_share": round(found[2] / n, 6),
                 "stopped_after_ring": stops, "phases_seconds": {"grid_build": round(t_grid, 6), "query_order": round(t_order, 6),
                                                                 "both_launches": round(t_search, 6)},
                 "index_min": int(index.min().cpu()), "index_max": int(index.max().cpu())})
    return line


def statistics_input(n, dev):
    """n seeded values in [0, 0.3), most of them small: 0.3 u^3 for uniform u."""
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    return torch.rand(n, dtype=torch.float64, device=dev, generator=g) ** 3 * 0.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1 << 17, 1000000, 2500000])
    ap.add_argument("--sample-count", type=int, default=1000000)
    ap.add_argument("--statistics-count", type=int, default=2500000)
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-ckdtree", action="store_true")
    ap.add_argument("--search", choices=("all_pairs", "grid", "both"), default="all_pairs",
                    help="grid / both: add the grid search beside the all-pairs kernel (both is grid's synonym: all pairs is always timed)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics3d: no GPU visible (nothing here can be measured on a CPU)")
    import bench
    from vf_nerf_amd import lib, mesh, metrics3d
    dev = torch.device("cuda:0")
    trained = bench.build_trained_scene(dev, 64, 32, 32, 0)
    scene, model = ("trained", trained[0]) if trained is not None else ("random", bench.build_scene(dev, 64, 32, 32, 0)[0])
    m = mesh.extract_mesh(model.vector_field_network, args.res)
    other = (m.vertices_scaled * 1.01, m.faces)
    result = {"device": torch.cuda.get_device_name(0), "scene": scene, "mesh_res": args.res, "mesh_faces": int(m.faces.shape[0]),
              "reps": args.reps, "timing": "HIP events, one warm-up call, median of reps",
              "peak_lane_instructions_per_s": PEAK_LANE_INSTRUCTIONS,
              "peak_note": "published 78.6 TFLOP/s vector fp64 / 2 (not measured here); 9 fp64 lane-instructions per pair",
              "nearest_distances": [], "sample_surface": None, "statistics": None}
    if args.search != "all_pairs":
        result.update({"nearest_grid": [], "nearest_grid_disjoint": None})
    x = statistics_input(args.statistics_count, dev)
    t, all_t, _ = timed(lambda: lib.reduce_stats(x, 0.05), args.reps)
    result["statistics"] = {"count": args.statistics_count, "seconds": round(t, 6), "all_seconds": [round(v, 6) for v in all_t],
                            "values_per_s": round(args.statistics_count / t, 1)}
    print(json.dumps(result["statistics"]), flush=True)
    del x
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    t, all_t, _ = timed(lambda: metrics3d.sample_surface(m.vertices_scaled, m.faces, args.sample_count, generator=g), args.reps)
    result["sample_surface"] = {"count": args.sample_count, "seconds": round(t, 6), "all_seconds": [round(x, 6) for x in all_t],
                                "points_per_s": round(args.sample_count / t, 1),
                                "includes": "areas, the scan, one host read of the total area, torch.rand, the sampling kernel"}
    print(json.dumps(result["sample_surface"]), flush=True)
    for n in args.sizes:
        g.manual_seed(n)
        q, _ = metrics3d.sample_surface(m.vertices_scaled, m.faces, n, generator=g)
        tg, _ = metrics3d.sample_surface(*other, n, generator=g)
        t, all_t, dist = timed(lambda: metrics3d.nearest_distances(q, tg), args.reps)
        pairs = float(n) * float(n)
        line = {"n": n, "m": n, "seconds": round(t, 6), "all_seconds": [round(x, 6) for x in all_t], "pairs_per_s": round(pairs / t, 1),
                "fraction_of_fp64_vector_peak": round(pairs * INSTRUCTIONS_PER_PAIR / t / PEAK_LANE_INSTRUCTIONS, 4)}
        if not args.no_ckdtree:
            from scipy.spatial import cKDTree
            qh, th = q.cpu().numpy(), tg.cpu().numpy()
            t0 = time.perf_counter()
            tree = cKDTree(th)
            t1 = time.perf_counter()
            ref = tree.query(qh, workers=args.workers)[0]
            t2 = time.perf_counter()
            line.update({"ckdtree_build_s": round(t1 - t0, 4), "ckdtree_query_s": round(t2 - t1, 4), "ckdtree_workers": args.workers,
                         "equal_to_ckdtree": bool(np.array_equal(ref.view(np.uint64), dist.cpu().numpy().view(np.uint64)))})
        print(json.dumps(line), flush=True)
        result["nearest_distances"].append(line)
        if args.search != "all_pairs":
            grid_line = grid_leg(q, tg, dist, t, args.reps)
            print(json.dumps(grid_line), flush=True)
            result["nearest_grid"].append(grid_line)
            if n == min(args.sizes):
                width = float((tg.max(dim=0).values - tg.min(dim=0).values).max().cpu())
                away = q + torch.tensor([100.0 * width, 0.0, 0.0], dtype=torch.float64, device=dev)
                t_far, _, far = timed(lambda: metrics3d.nearest_distances(away, tg), args.reps)
                far_line = grid_leg(away, tg, far, t_far, args.reps)
                far_line["queries"] = "the same, moved 100 box widths along x: every query a leftover"
                print(json.dumps(far_line), flush=True)
                result["nearest_grid_disjoint"] = far_line
        del q, tg, dist
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
