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

    python tools/bench_metrics3d.py [--sizes 131072 1000000 2500000] [--reps 3] [--out profiles/r08/bench_metrics3d.json]
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
        del q, tg, dist
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
