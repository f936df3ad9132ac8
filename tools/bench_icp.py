#!/usr/bin/env python3
"""Device time of point-set alignment (vf_nerf_amd.icp) at 10^5 and 10^6 surface samples of one mesh against a moved copy: the mesh that
mesh.extract_mesh makes from the trained-weight scene of bench.py (the random-weight scene when the fixture is absent); the targets
are samples of it, the source is another sampling moved by 5 degrees about (1, 2, 3) and 0.01 of the bounding-box diagonal; the
correspondence radius is 0.05 of the diagonal.

Per size, HIP events around each call, one warm-up call, --reps timed calls, the median reported (all repeats are listed):

    nearest_within_with_grid    one radius-bounded search as the public call runs it: grid build (bounding box read, sort, cell table),
                                query ordering, the search kernel
    nearest_within_search_only  the search kernel alone on a grid and a query order built before
    grid_build / query_order    the two pieces of plumbing on their own
    nn_sqdist                   the all-pairs search of vf_nerf_amd.metrics3d on the same sets (no index, no radius)
    accumulate                  the 17 sums over the search's result
    align                       a whole icp.align (its iterations and whether it converged are recorded): the queries re-sorted by
                                cell under every new transformation, the coordinates checked for NaN / inf by the first search only
    align_order_once            the same with the queries sorted once, under the initial transformation
    search_at_result_*          one search under align's final transformation with the order made under the initial one (stale), with
                                a fresh order, and the fresh one with the NaN / inf pass skipped: what a late iteration's search costs

Every size runs in a child process of its own under a time limit (--limit seconds); the parent never opens the device and stops at the
first child that fails.

    python tools/bench_icp.py [--sizes 100000 1000000] [--reps 3] [--out profiles/r11/bench_icp.json]
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps):
    """One warm-up call, then `reps` calls between HIP events -> (median seconds, all seconds, last result)."""
    import torch
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


def one_size(n, res, reps):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_icp: no GPU visible (nothing here can be measured on a CPU)")
    import bench
    from vf_nerf_amd import icp, lib, mesh, metrics3d
    dev = torch.device("cuda:0")
    trained = bench.build_trained_scene(dev, 64, 32, 32, 0)
    scene, model = ("trained", trained[0]) if trained is not None else ("random", bench.build_scene(dev, 64, 32, 32, 0)[0])
    m = mesh.extract_mesh(model.vector_field_network, res)
    v = m.vertices_scaled
    diagonal = float((v.max(dim=0).values - v.min(dim=0).values).norm())
    g = torch.Generator(device=dev)
    g.manual_seed(n)
    targets, _ = metrics3d.sample_surface(v, m.faces, n, generator=g)
    sampled, _ = metrics3d.sample_surface(v, m.faces, n, generator=g)
    axis = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    k = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    th = math.radians(5.0)
    move = np.eye(4)
    move[:3, :3] = np.eye(3) + math.sin(th) * k + (1.0 - math.cos(th)) * (k @ k)
    move[:3, 3] = 0.01 * diagonal * np.array([1.0, -0.5, 0.7])
    source = icp.transform_points(sampled, move)
    radius = 0.05 * diagonal
    line = {"n": n, "m": n, "scene": scene, "mesh_res": res, "mesh_faces": int(m.faces.shape[0]), "diagonal": round(diagonal, 6),
            "radius": round(radius, 6), "device": torch.cuda.get_device_name(0)}

    def put(name, result):
        t, all_t, out = result
        line[name] = {"seconds": round(t, 6), "all_seconds": [round(x, 6) for x in all_t]}
        return out

    put("nearest_within_with_grid", timed(lambda: icp.nearest_within(source, targets, radius), reps))
    grid = put("grid_build", timed(lambda: icp.build_grid(targets, radius), reps))
    order = put("query_order", timed(lambda: icp.query_order(source, None, grid), reps))
    index, sqdist = put("nearest_within_search_only", timed(lambda: icp.search(source, None, grid, order=order), reps))
    put("nearest_within_search_unordered", timed(lambda: icp.search(source, None, grid), reps))
    line["grid_dims"] = list(grid.dims)
    line["found"] = int((index >= 0).sum())
    best = put("nn_sqdist", timed(lambda: lib.nn_sqdist(source, targets), reps))
    line["sqdist_equal_to_nn_sqdist_where_found"] = bool(torch.equal(best[index >= 0].view(torch.int64), sqdist[index >= 0].view(torch.int64)))
    put("accumulate", timed(lambda: lib.icp_accumulate(source, None, targets, index, sqdist, grid.anchor), reps))
    res_align = put("align", timed(lambda: icp.align(source, targets, radius), reps))
    line["align"].update({"iterations": res_align.iterations, "converged": res_align.converged, "fitness": res_align.fitness,
                          "inlier_rmse": res_align.inlier_rmse,
                          "max_abs_T_M_minus_I": float(np.abs(res_align.transformation @ move - np.eye(4)).max())})
    once = put("align_order_once", timed(lambda: icp._align(source, targets, radius, None, icp.MAX_ITERATION, icp.RELATIVE_FITNESS,
                                                            icp.RELATIVE_RMSE, None, reorder=False), reps))
    line["align_order_once"].update({"iterations": once.iterations,
                                     "same_transformation": bool(np.array_equal(once.transformation, res_align.transformation))})
    final = res_align.transformation
    fresh = icp.query_order(source, final, grid)
    put("search_at_result_stale_order", timed(lambda: icp.search(source, final, grid, order=order), reps))
    put("search_at_result_fresh_order", timed(lambda: icp.search(source, final, grid, order=fresh), reps))
    put("search_at_result_fresh_order_no_finite_pass", timed(lambda: icp.search(source, final, grid, order=fresh, check_finite=False), reps))
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a size's child process may take")
    ap.add_argument("--one", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.one is not None:
        one_size(args.one, args.res, args.reps)
        return
    result = {"reps": args.reps, "timing": "HIP events, one warm-up call, median of reps; one child process per size", "sizes": []}
    for n in args.sizes:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", str(n), "--res", str(args.res), "--reps", str(args.reps)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"bench_icp: n = {n} exceeded {args.limit} s; stopping")
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            raise SystemExit(f"bench_icp: n = {n} ended with status {done.returncode}; stopping")
        line = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps(line), flush=True)
        result["sizes"].append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
