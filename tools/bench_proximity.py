"""What the closest-point search costs on one MI355X (csrc/vfn_proximity.hip through vf_nerf_amd/metrics3d.py), on the mesh
tools/bench_tsdf.py fuses: the room scene at --res^3 (512) from --views (100) analytic depth maps of --height x --width.  The queries are
--samples (10^6) area-weighted surface samples of a SECOND copy of the mesh whose vertices are moved by seeded normal noise of
--noise (0.5) extraction voxels: near the surface, not on it.

    grid build, by stage   ranges (vfn_tri_cell_ranges: the packed [F, 9] table, cell ranges, counts), pairs (torch's cumsum, the one host
                           read, vfn_tri_cell_pairs), sort (torch's stable sort by key, the gather, searchsorted); and the whole
                           metrics3d.triangle_grid call.  Reported with it: pairs per face, the share of large faces, the grid's dims.
    closest_point          the search on the built grid (the ordering of the queries and the leftovers' all-pairs pass included), the
                           leftover count at the default max_rings, and the number of queries each ring settles: the ring launch alone
                           with max_rings = 0, 1, ..., --rings (8), the differences of its leftover counts.
    --big-face-cells       the build's pair count and the search at each listed value beside the default (what the default of 64 rests on)
    baseline (a)           vfn_tri_nearest_list over EVERYTHING for the first --list-queries (2048) queries: all pairs, the pair rate
    baseline (b)           metrics3d.nearest (the point search, grid) of the same queries against --samples samples of the mesh itself:
                           what a direction of a sampled score costs
    baseline (c)           metrics3d.score_mesh of the perturbed copy against the mesh with surface="mesh" and with surface="samples"
                           (search="grid"), the same seed: both dictionaries' chamfer means and F-scores beside the two times

HIP events around each call, one warm-up call, --reps timed calls; the median is reported with every repeat listed, so the spread is on
the page.  Nothing from any other tree is read.  No test asserts a time.

    python tools/bench_proximity.py [--res 512] [--reps 5] [--out profiles/r24/bench_proximity.json]
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
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--noise", type=float, default=0.5, help="standard deviation of the second copy's vertex noise, in extraction voxels")
    ap.add_argument("--list-queries", type=int, default=2048)
    ap.add_argument("--rings", type=int, default=8)
    ap.add_argument("--big-face-cells", type=int, nargs="*", default=[8, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-score", action="store_true", help="skip baseline (c)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_proximity: no GPU visible (nothing here can be measured on a CPU)")
    import tsdf_restatement as T
    from vf_nerf_amd import icp, lib, metrics3d
    dev = torch.device("cuda:0")
    h, w = args.height, args.width
    (verts, faces), _, voxel_length, _ = fused_room(args.res, room_views(args.views), T.pinhole(h, w, 0.6 * w), h, w, dev)
    verts, faces = verts.to(torch.float64).contiguous(), faces.to(torch.int64).contiguous()
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    g = torch.Generator(device=dev)
    g.manual_seed(24)
    moved = (verts + args.noise * voxel_length * torch.randn(nv, 3, dtype=torch.float64, device=dev, generator=g)).contiguous()
    queries, _ = metrics3d.sample_surface(moved, faces, args.samples, generator=g, device=dev)
    n = int(queries.shape[0])
    result = {"device": torch.cuda.get_device_name(0), "res": args.res, "views": args.views, "map": [h, w], "vertices": nv, "faces": nf,
              "extraction_voxel": voxel_length, "queries": n, "noise_voxels": args.noise, "reps": args.reps,
              "timing": "HIP events, one warm-up call, median of reps with every repeat listed; host reads inside a call are part of it"}

    def say(key, value):
        result[key] = value
        print(json.dumps({key: value}), flush=True)

    # ---- the grid build, by stage
    zero = lambda: torch.zeros(1, dtype=torch.int64, device=dev)          # noqa: E731
    whole = metrics3d.triangle_grid((verts, faces), device=dev)
    box, dims, big = whole.box, whole.dims, whole.big_face_cells
    stages = {}
    t, all_t, (tri, cell_lo, cell_hi, ncells) = timed(lambda: lib.tri_cell_ranges(verts, faces, box, dims, zero()), args.reps)
    stages["ranges"] = rounded(t, all_t)

    def pairs():
        count = ncells.to(torch.int64)
        small = torch.where(count > big, torch.zeros_like(count), count)
        inclusive = torch.cumsum(small, dim=0)
        n_pairs = int(inclusive[-1].cpu())
        return lib.tri_cell_pairs(cell_lo, cell_hi, ncells, (inclusive - small).contiguous(), big, dims, n_pairs, zero())

    t, all_t, (key, face) = timed(pairs, args.reps)
    stages["pairs"] = dict(rounded(t, all_t), note="torch's cumsum, the host read of the pair count, vfn_tri_cell_pairs")

    def sort():
        sorted_key, perm = torch.sort(key, stable=True)
        cells = torch.arange(dims[0] * dims[1] * dims[2] + 1, dtype=torch.int32, device=dev)
        return face[perm].contiguous(), torch.searchsorted(sorted_key, cells).to(torch.int32)

    t, all_t, _ = timed(sort, args.reps)
    stages["sort"] = dict(rounded(t, all_t), torch_sort=True)
    t, all_t, grid = timed(lambda: metrics3d.triangle_grid((verts, faces), device=dev), args.reps)
    stages["triangle_grid"] = dict(rounded(t, all_t), note="the whole call: the box over the named vertices and its host read included")
    say("build", dict(stages, dims=list(grid.dims), cell_edge=grid.box[6], n_pairs=grid.n_pairs, n_large=grid.n_large, big_face_cells=big,
                      pairs_per_face=round(grid.n_pairs / nf, 4), large_share=round(grid.n_large / nf, 6),
                      table_bytes=int(grid.tri.numel() * 8)))

    # ---- the search on the built grid
    def search_leg(gr):
        t, all_t, out = timed(lambda: metrics3d._closest(queries, gr, metrics3d.MAX_RINGS), args.reps)
        return dict(rounded(t, all_t), leftovers=int(out[3]), queries_per_second=round(n / t, 1)), out

    leg, (found_face, _, found_sq, _) = search_leg(grid)
    order = torch.argsort(icp._cells(queries, grid.box, grid.dims, dev)).contiguous()
    left = [lib.tri_nearest(queries, grid.args(), r, nv, order=order, serve_leftovers=False)[3] for r in range(args.rings + 1)]
    settled = [n - left[0]] + [left[r - 1] - left[r] for r in range(1, args.rings + 1)]
    t, all_t, _ = timed(lambda: lib.tri_nearest(queries, grid.args(), metrics3d.MAX_RINGS, nv, order=order, serve_leftovers=False), args.reps)
    say("closest_point", dict(leg, ring_launch_alone=rounded(t, all_t), settled_by_ring=settled, unsettled_after_last_ring=left[-1],
                              mean_distance=float(torch.sqrt(found_sq).mean().cpu())))
    others = {}
    for value in args.big_face_cells:
        t, all_t, gr = timed(lambda: metrics3d.triangle_grid((verts, faces), big_face_cells=value, device=dev), args.reps)
        others[str(value)] = {"build": rounded(t, all_t), "n_pairs": gr.n_pairs, "n_large": gr.n_large, "search": search_leg(gr)[0]}
        del gr
    say("big_face_cells", others)

    # ---- (a) all pairs, at a query count that finishes
    few = queries[:max(1, min(args.list_queries, n))].contiguous()
    t, all_t, listed = timed(lambda: metrics3d._closest(few, grid, None), args.reps)
    same = bool(torch.equal(listed[0], found_face[:few.shape[0]]) and torch.equal(listed[2], found_sq[:few.shape[0]]))
    say("all_pairs", dict(rounded(t, all_t), queries=int(few.shape[0]), pairs_per_second=round(few.shape[0] * nf / t, 1),
                          seconds_for_all_queries_at_that_rate=round(t * n / few.shape[0], 3), equals_the_grid_search=same))

    # ---- (b) the point search against samples of the same mesh
    targets, _ = metrics3d.sample_surface(verts, faces, args.samples, generator=g, device=dev)
    t, all_t, point_grid = timed(lambda: metrics3d.nearest_grid(targets, device=dev), args.reps)
    build_b = rounded(t, all_t)
    t, all_t, (_, point_distance) = timed(lambda: metrics3d.nearest(queries, point_grid), args.reps)
    say("nearest_on_samples", dict(rounded(t, all_t), grid_build=build_b, targets=int(targets.shape[0]),
                                   mean_distance=float(point_distance.mean().cpu())))

    # ---- (c) a whole score, through the meshes and through the samples
    if not args.no_score:
        scores = {}
        for surface in ("mesh", "samples"):
            def score():
                gen = torch.Generator(device=dev)
                gen.manual_seed(25)
                return metrics3d.score_mesh((moved, faces), (verts, faces), num_points=args.samples, distance_thresh=voxel_length, generator=gen,
                                            device=dev, search="grid", surface=surface)
            t, all_t, entry = timed(score, args.reps)
            scores[surface] = dict(rounded(t, all_t), chamfer_mean=entry["chamfer distance"]["mean"], precision=entry["precision"],
                                   recall=entry["recall"], fscore=entry["fscore"])
        scores["mesh_over_samples_seconds"] = round(scores["mesh"]["seconds"] / scores["samples"]["seconds"], 3)
        say("score_mesh", scores)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
        print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
