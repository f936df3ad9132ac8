#!/usr/bin/env python3
"""Device time and quality of quadric edge-collapse decimation (vf_nerf_amd.decimate.simplify_edge_collapse, csrc/vfn_collapse.hip) on the
mesh tools/bench_simplify.py uses: the room scene fused at --res^3 (512) from --views (100) analytic depth maps of --height x --width
(680 x 1200).  At the targets faces / --divisors (4 and 10) it reports

    collapse           the whole public call on the device mesh: seconds, rounds, edges collapsed, faces out, seconds a round
    first_round        the stages of the FIRST round (the largest) timed apart: planes (vfn_face_planes), edges (the stable sort of the 3m
                       keys and unique_consecutive: torch), boundary (vfn_boundary_planes), items (the sort of the item keys and
                       searchsorted: torch), quadrics (vfn_vertex_quadrics), candidates (vfn_edge_collapse_candidates), select
                       (vfn_collapse_select, five launches), budget (nonzero, the stable sort of the costs, cumsum, searchsorted: torch);
                       the share of torch's sorts in the round
    clustering         meshops.simplify_to_faces at the same target (its 16 vertex clusterings), in the same process
    chamfer            metrics3d.chamfer_distance (grid search) between --samples (10^6) samples of the original and of each simplified mesh,
                       from one seed: collapse against clustering at about equal face count
    surface_deviation  metrics3d.surface_deviation beside it: the one-sided mean / rms / max / median distance from --samples samples of each
                       simplified mesh to the SURFACE of the original (the closest point on its faces, not on samples of it)

HIP events around each call, one warm-up call, --reps timed calls, the median reported (all repeats are listed).  No test asserts a time.

    python tools/bench_collapse.py [--res 512] [--reps 5] [--out profiles/r23/bench_collapse.json]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_refuse import fused_room, rounded  # noqa: E402
from bench_tsdf import room_views, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--divisors", type=float, nargs="+", default=[4.0, 10.0])
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-clustering", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_collapse: no GPU visible (nothing here can be measured on a CPU)")
    import tsdf_restatement as T
    from vf_nerf_amd import decimate, lib, meshops, metrics3d, voxel
    dev = torch.device("cuda:0")
    h, w = args.height, args.width
    (verts, faces), _, extraction_voxel, _ = fused_room(args.res, room_views(args.views), T.pinhole(h, w, 0.6 * w), h, w, dev)
    verts, faces = verts.to(torch.float64).contiguous(), faces.to(torch.int64).contiguous()
    n, m = int(verts.shape[0]), int(faces.shape[0])
    result = {"device": torch.cuda.get_device_name(0), "res": args.res, "views": args.views, "map": [h, w], "vertices": n, "faces": m,
              "extraction_voxel": extraction_voxel, "reps": args.reps, "samples": args.samples,
              "timing": "HIP events, one warm-up call, median of reps; host reads inside a call are part of it", "targets": []}

    # ---- the stages of the first round, apart
    origin = voxel.bounding_box(verts)[0]
    zero = lambda: torch.zeros(1, dtype=torch.int64, device=dev)          # noqa: E731
    stages = {}
    t, all_t, planes = timed(lambda: lib.face_planes(verts, faces, origin, info=zero()), args.reps)
    stages["planes"] = rounded(t, all_t)

    def edges():
        a, b = torch.cat((faces[:, 0], faces[:, 1], faces[:, 2])), torch.cat((faces[:, 1], faces[:, 2], faces[:, 0]))
        keys, order = torch.sort(torch.minimum(a, b) * n + torch.maximum(a, b), stable=True)
        key, run = torch.unique_consecutive(keys, return_counts=True)
        return a, b, order, key, run

    t, all_t, (a, b, order, key, run) = timed(edges, args.reps)
    stages["edges"] = dict(rounded(t, all_t), edges=int(key.shape[0]), torch_sort=True)
    r = decimate.collapse_round(verts, faces, origin, target_faces=int(m / args.divisors[0]))
    n_boundary = int((r.run == 1).sum())
    if n_boundary:
        boundary = torch.nonzero(run == 1).reshape(-1)
        pair = order[(torch.cumsum(run, dim=0) - run)[boundary]]
        bf, ba, bb = (pair % m).contiguous(), a[pair].contiguous(), b[pair].contiguous()
        t, all_t, _ = timed(lambda: lib.boundary_planes(verts, planes, bf, ba, bb, origin, 1.0, info=zero()), args.reps)
        stages["boundary"] = dict(rounded(t, all_t), boundary_edges=n_boundary)
    rows = m + n_boundary

    def items():
        face = torch.arange(m, dtype=torch.int64, device=dev)
        keys = [faces[:, 0] * rows + face, faces[:, 1] * rows + face, faces[:, 2] * rows + face]
        item_key = torch.sort(torch.cat(keys))[0]
        vertex = torch.div(item_key, rows, rounding_mode="floor")
        return item_key - vertex * rows, torch.searchsorted(vertex, torch.arange(n + 1, dtype=torch.int64, device=dev))

    t, all_t, _ = timed(items, args.reps)
    stages["items"] = dict(rounded(t, all_t), items=int(r.item_row.shape[0]), torch_sort=True, note="the face incidences only (the boundary's few keys left out)")
    t, all_t, _ = timed(lambda: lib.vertex_quadrics(r.planes, r.item_row, r.start, info=zero()), args.reps)
    stages["quadrics"] = rounded(t, all_t)
    t, all_t, _ = timed(lambda: lib.edge_collapse_candidates(verts, faces, r.quadrics, r.item_row, r.start, rows, r.edge_a, r.edge_b, r.run, origin, 1e-9, 2.0,
                                                             float("inf"), info=zero()), args.reps)
    stages["candidates"] = rounded(t, all_t)
    t, all_t, _ = timed(lambda: lib.collapse_select(r.cost, r.flags, r.edge_a, r.edge_b, faces, n, info=zero()), args.reps)
    stages["select"] = rounded(t, all_t)

    def budget():
        stays = torch.nonzero(r.proposed & ~r.withdrawn).reshape(-1)
        stays = stays[torch.sort(r.cost[stays], stable=True)[1]]
        return torch.searchsorted(torch.cumsum(r.run[stays], dim=0), torch.full((1,), m // 2, dtype=torch.int64, device=dev))

    t, all_t, _ = timed(budget, args.reps)
    stages["budget"] = dict(rounded(t, all_t), torch_sort=True)
    t, all_t, _ = timed(lambda: decimate.collapse_round(verts, faces, origin, target_faces=int(m / args.divisors[0])), args.reps)
    stages["round"] = dict(rounded(t, all_t), note="decimate.collapse_round, the whole first round with its one read", candidates=int((r.flags & 1).sum()),
                           proposed=int(r.proposed.sum()), withdrawn=int(r.withdrawn.sum()), taken=r.n_taken)
    total = sum(s["seconds"] for k, s in stages.items() if k != "round")
    stages["share_of_torch_sorts"] = round(sum(s["seconds"] for s in stages.values() if isinstance(s, dict) and s.get("torch_sort")) / total, 4)
    stages["share_of_kernels"] = round(sum(stages[k]["seconds"] for k in ("planes", "boundary", "quadrics", "candidates", "select") if k in stages) / total, 4)
    result["first_round"] = stages
    print(json.dumps({"first_round": stages}), flush=True)

    # ---- the whole calls, against the bisection over vertex clusterings, with the chamfer distance to the original
    def chamfer(mesh):
        g = torch.Generator(device=dev)
        g.manual_seed(23)
        return list(metrics3d.chamfer_distance(mesh, (verts, faces), num_points=args.samples, generator=g, search="grid"))

    def deviation(mesh):
        g = torch.Generator(device=dev)
        g.manual_seed(23)
        return metrics3d.surface_deviation(mesh, (verts, faces), num_points=args.samples, generator=g)

    for divisor in args.divisors:
        target = max(1, int(m / divisor))
        line = {"divisor": divisor, "target_faces": target}
        t, all_t, c = timed(lambda: decimate.simplify_edge_collapse((verts, faces), target_faces=target), args.reps)
        line["collapse"] = dict(rounded(t, all_t), faces_out=int(c.faces.shape[0]), vertices_out=int(c.vertices.shape[0]), rounds=c.rounds,
                                collapsed=c.collapsed, reached=c.reached, seconds_per_round=round(t / max(c.rounds, 1), 6),
                                largest_absorbed_cost=float(c.cost.max().cpu()) if c.cost.shape[0] else 0.0,
                                chamfer_mean_median_min_max=chamfer((c.vertices, c.faces)), surface_deviation=deviation((c.vertices, c.faces)))
        if not args.no_clustering:
            t, all_t, (s, size) = timed(lambda: meshops.simplify_to_faces((verts, faces), target), args.reps)
            line["clustering"] = dict(rounded(t, all_t), faces_out=int(s.faces.shape[0]), vertices_out=int(s.vertices.shape[0]), voxel_size=size,
                                      chamfer_mean_median_min_max=chamfer((s.vertices, s.faces)), surface_deviation=deviation((s.vertices, s.faces)))
            line["collapse_over_clustering_seconds"] = round(line["collapse"]["seconds"] / line["clustering"]["seconds"], 3)
        result["targets"].append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
