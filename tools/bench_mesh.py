#!/usr/bin/env python3
"""Per-stage device time of the mesh pipeline (evaluation/methods.py:140-322 as vf_nerf_amd.mesh runs it) at res 128 / 256 / 512, on
the random-weight scene and the trained-weight scene of bench.py (built by import).  HIP events around each stage:

    queries      lattice regeneration + the vector-field queries (grid.DEVICE_CHUNK points per launch)
    divergence   grid.extract_divergence
    norms        norms + normalised field (vfn_mesh_field_norms)
    sides        side bytes (vfn_grid_unify_direction_sides, no int64 table)
    triangulate  count + scan, emit, dedup + scan, number (lib.mesh_triangulate, two small read-backs inside)

For the new kernels, algorithmic bytes per cell (what a perfect kernel must move) against 8 TB/s.  One JSON line per (scene, res).

    python tools/bench_mesh.py [--res 128 256 512] [--reps 3]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_BPS = 8e12


def timed(fn, reps):
    best, out = None, None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b) / 1e3
        best = t if best is None else min(best, t)
    return best, out


def run(scene, dec, res, reps):
    from vf_nerf_amd import grid, lib, mesh
    dev = torch.device("cuda:0")
    n = res ** 3
    axes = tuple(a.to(dev) for a in mesh.lattice_axes(res))
    pred = torch.empty(n, 3, device=dev)

    def queries():
        for lo in range(0, n, grid.DEVICE_CHUNK):
            cnt = min(grid.DEVICE_CHUNK, n - lo)
            pred[lo:lo + cnt] = dec(lib.grid_lattice_points(axes, res, lo, cnt), vector_only=True)
        return pred
    t = {}
    with torch.no_grad():
        t["queries"], _ = timed(queries, reps)
        t["divergence"], div = timed(lambda: grid.extract_divergence(pred, res), reps)
        t["norms"], (norms, unit) = timed(lambda: lib.mesh_field_norms(pred), reps)
        t["sides"], (sides, _) = timed(lambda: lib.grid_unify_direction_sides(div.reshape(-1), unit, res, want_table=False), reps)
        t["triangulate"], (v, f) = timed(lambda: lib.mesh_triangulate(lib.MESH_FUSED, n, res, 2.0, 0.0, sides=sides, norms=norms), reps)
    cells = int(((sides != 0) & (sides != 255)).sum())
    tri, verts = f.shape[0], v.shape[0]
    # algorithmic bytes: count (1 B side + 4 B norm read, 4 B count write; 32 B of corner norms per surface cell), scan (8 B), emit (4 B count;
    # 72 B per triangle out), dedup (24 B key + 8 B table/owner + 4 B bucket per slot, 8 B table init per slot x 2), flag + scan (12 B per
    # slot), number (12 B read + 8 B face per slot, 24 B per vertex)
    slots = 3 * tri
    tri_bytes = n * (9 + 8 + 4) + cells * 32 + tri * 72 + slots * (24 + 8 + 4 + 16 + 12 + 20) + verts * 24
    norm_bytes = n * (12 + 4 + 12)
    after = t["divergence"] + t["norms"] + t["sides"] + t["triangulate"]
    return {"scene": scene, "res": res, "seconds": {k: round(x, 6) for k, x in t.items()}, "after_queries_s": round(after, 6),
            "after_queries_over_queries": round(after / t["queries"], 3), "target_met": after < t["queries"],
            "cells_triangulated": cells, "triangles": tri, "unique_vertices": verts,
            "algorithmic_bytes_per_cell": {"triangulate": round(tri_bytes / n, 2), "norms": round(norm_bytes / n, 2)},
            "fraction_of_8TBps": {"triangulate": round(tri_bytes / t["triangulate"] / HBM_BPS, 3),
                                  "norms": round(norm_bytes / t["norms"] / HBM_BPS, 3)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    dev = torch.device("cuda:0")
    scenes = [("random", bench.build_scene(dev, 64, 32, 32, 0)[0])]
    trained = bench.build_trained_scene(dev, 64, 32, 32, 0)
    if trained is not None:
        scenes.append(("trained", trained[0]))
    lines = []
    for name, model in scenes:
        for res in args.res:
            line = run(name, model.vector_field_network, res, args.reps)
            print(json.dumps(line), flush=True)
            lines.append(line)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(lines, fh, indent=1)


if __name__ == "__main__":
    main()
