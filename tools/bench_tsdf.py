#!/usr/bin/env python3
"""Device time of TSDF fusion (vf_nerf_amd.tsdf, csrc/vfn_tsdf.hip): a --res^3 volume (512) over the room scene of the tests — cameras
inside an axis-aligned box [-0.6, 0.6]^3 looking at its walls, analytic plane depth — fused from --views (100) depth maps of
--height x --width (680 x 1200).  Recorded:

    batched            ONE vfn_tsdf_integrate call over all views: the volume is read and written once.
    view_by_view       the same kernel called once per view (the baseline: the volume moves --views times).
    traffic_floor_s    16 B per voxel (tsdf + weight, read + written) at the 6.29 TB/s a device-to-device copy reaches on one MI355X.
    extract            count + scan + emit + merge + numbering of the fused volume, with the two host reads that size the outputs.
    cpu                the NumPy restatement (tests/tsdf_restatement.py) on a --cpu-res^3 volume (128) with the same views, the volume cut
                       into slabs along x for --workers (16) threads; host clock.  A slab restates the contract with its own origin:
                       a timing, not a bit-for-bit reference.

HIP events around each call, one warm-up call, --reps timed calls, the median reported (all repeats are listed).

    python tools/bench_tsdf.py [--res 512] [--views 100] [--height 680] [--width 1200] [--reps 3] [--out profiles/r09/bench_tsdf.json]

--colour measures, INSTEAD of the rows above and in one process, alternating over --reps (plain, rgb, plain extract, coloured extract,
plain, rgb, ...), on the same scene with pattern images (tests/tsdf_colour_restatement.py):

    plain              the batched colourless integration (the `batched` row above: the same call).
    rgb                ONE vfn_tsdf_integrate_rgb call over all views (colour[res^3, 3] next to tsdf and weight).
    extract / extract_coloured   extract_mesh and extract_coloured_mesh of the fused volume.
    bytes              the algorithmic traffic of both integrations: 16 B against 40 B per voxel (each array read and written once),
                       and the image gathers: 4 B (depth) against 4 + 3 B (depth + rgb) per voxel-view that reaches the image.

    python tools/bench_tsdf.py --colour [--reps 5] [--parent profiles/r09/bench_tsdf.json] [--out profiles/r13/bench_tsdf_colour.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

COPY_RATE = 6.29e12          # B/s: the rate of a large device-to-device copy on one MI355X
HALF = 0.6                   # the room


def timed(fn, reps, before=None):
    """One warm-up call, then `reps` calls between HIP events -> (median seconds, all seconds, last result)."""
    if before:
        before()
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return statistics.median(times), times, out


def room_views(n, seed=0):
    """n camera-to-world poses inside the room: eyes in [-0.3, 0.3]^3, each looking at a point of a wall."""
    import tsdf_restatement as R
    g = np.random.default_rng(seed)
    poses = []
    for i in range(n):
        eye = g.uniform(-0.3, 0.3, 3)
        target = g.uniform(-HALF, HALF, 3)
        target[i % 3] = HALF if (i // 3) % 2 == 0 else -HALF
        poses.append(R.look_at(eye, target))
    return np.stack(poses)


def room_depths(poses, k4, h, w, dev):
    """Analytic z-depth of every pixel against the inside of the room, float64 geometry on the device -> float32 [V,h,w]."""
    out = torch.empty(len(poses), h, w, dtype=torch.float32, device=dev)
    v, u = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing="ij")
    cam = torch.stack([(u - float(k4[2])) / float(k4[0]), (v - float(k4[3])) / float(k4[1]), torch.ones_like(u)], dim=-1)
    for i, p in enumerate(poses):
        p = torch.from_numpy(p).to(dev)
        d = cam @ p[:3, :3].T
        t = (HALF * torch.sign(d) - p[:3, 3]) / d                       # the wall each axis' component runs towards
        t = torch.where(torch.isfinite(t) & (t > 0), t, torch.full_like(t, float("inf"))).min(dim=-1).values
        out[i] = t.to(torch.float32)
    return out


def cpu_baseline(res, vl, trunc, depths, k4s, e12s, workers):
    import tsdf_restatement as R
    edges = np.linspace(0, res, workers + 1).astype(int)

    def slab(j):
        lo, hi = edges[j], edges[j + 1]
        if hi == lo:
            return 0
        origin = (-0.7 + lo * vl, -0.7, -0.7)
        t, w = R.fused((hi - lo, res, res), origin, vl, trunc, depths, k4s, e12s)
        return int((w > 0).sum())

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=workers) as pool:
        observed = sum(pool.map(slab, range(workers)))
    return time.perf_counter() - t0, observed


def event_time(fn, before=None):
    """One call between HIP events -> (seconds, result)."""
    if before:
        before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3, out


def colour_rows(args, dev, vl, trunc, poses, depths, k, e):
    import tsdf_colour_restatement as C
    from vf_nerf_amd import lib, tsdf
    res, nv, h, w = args.res, args.views, args.height, args.width
    rgb = torch.from_numpy(C.pattern_images(nv, h, w)).to(dev)
    dims = (res, res, res)
    plain_vol = tsdf.TSDFVolume((-0.7, -0.7, -0.7), dims, voxel_length=vl, sdf_trunc=trunc, device=dev)
    rgb_vol = tsdf.TSDFVolume((-0.7, -0.7, -0.7), dims, voxel_length=vl, sdf_trunc=trunc, device=dev, colour=True)
    box = (plain_vol.origin, plain_vol.voxel_length, plain_vol.sdf_trunc)
    calls = {"plain": (lambda: lib.tsdf_integrate(plain_vol.tsdf, plain_vol.weight, *box, depths, k, e), plain_vol.reset),
             "rgb": (lambda: lib.tsdf_integrate_rgb(rgb_vol.tsdf, rgb_vol.weight, rgb_vol.colour, *box, depths, rgb, k, e), rgb_vol.reset),
             "extract": (plain_vol.extract_mesh, None), "extract_coloured": (rgb_vol.extract_coloured_mesh, None)}
    times = {name: [] for name in calls}
    meshes = {}
    for rep in range(args.reps + 1):                     # round 0 is the warm-up; every round runs the four calls in the same order
        for name, (fn, before) in calls.items():
            t, out = event_time(fn, before)
            if rep:
                times[name].append(t)
            if out is not None:
                meshes[name] = out
    same = torch.equal(plain_vol.tsdf.view(torch.int32), rgb_vol.tsdf.view(torch.int32)) and torch.equal(plain_vol.weight, rgb_vol.weight)
    same_mesh = torch.equal(meshes["extract"][0], meshes["extract_coloured"][0]) and torch.equal(meshes["extract"][1], meshes["extract_coloured"][1])
    voxels = res ** 3
    voxel_views = float(rgb_vol.weight.sum())            # updates applied; the gathers also serve the voxel-views a test then rejects
    rows = {name: {"seconds": round(statistics.median(ts), 6), "all_seconds": [round(x, 6) for x in ts],
                   "spread": round((max(ts) - min(ts)) / statistics.median(ts), 4)} for name, ts in times.items()}
    result = {"device": torch.cuda.get_device_name(0), "res": res, "views": nv, "map": [h, w], "voxel_length": vl, "sdf_trunc": trunc,
              "reps": args.reps,
              "timing": "HIP events per call; one warm-up round, then --reps rounds of plain, rgb, extract, extract_coloured in that order "
                        "in one process; the volume is zeroed before every integration (untimed); median, all repeats, (max - min) / median",
              **rows,
              "rgb_over_plain": round(rows["rgb"]["seconds"] / rows["plain"]["seconds"], 3),
              "extract_coloured_over_extract": round(rows["extract_coloured"]["seconds"] / rows["extract"]["seconds"], 3),
              "tsdf_weight_bits_equal": bool(same), "mesh_bits_equal": bool(same_mesh),
              "vertices": int(meshes["extract_coloured"][0].shape[0]), "faces": int(meshes["extract_coloured"][1].shape[0]),
              "bytes": {"plain_volume": 16 * voxels, "rgb_volume": 40 * voxels, "per_voxel": [16, 40],
                        "updates_applied": voxel_views, "plain_gather_at_least": 4 * voxel_views, "rgb_gather_at_least": 7 * voxel_views,
                        "note": "volume: every array read and written once (tsdf + weight; + 3 colour floats); gathers: 4 B of depth, and 3 B "
                                "of rgb more, per update applied — a lower bound: the depth (and, issued with it, the rgb) is also read for "
                                "voxel-views that the d > 0 or the truncation test then rejects",
                        "plain_floor_s": round(16 * voxels / COPY_RATE, 6), "rgb_floor_s": round(40 * voxels / COPY_RATE, 6)}}
    if args.parent:
        with open(args.parent) as fh:
            parent = json.load(fh)["batched"]
        result["parent"] = {"file": args.parent, "batched_seconds": parent["seconds"], "batched_all_seconds": parent["all_seconds"],
                            "plain_over_parent": round(rows["plain"]["seconds"] / parent["seconds"], 4)}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-res", type=int, default=128)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-extract", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--colour", action="store_true", help="plain / rgb integration and plain / coloured extraction, alternating, in one process")
    ap.add_argument("--parent", default=None, help="--colour: an earlier bench_tsdf.json whose `batched` time the plain one is compared with")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf: no GPU visible (nothing here can be measured on a CPU)")
    import tsdf_restatement as R
    from vf_nerf_amd import lib, tsdf
    dev = torch.device("cuda:0")
    res, nv, h, w = args.res, args.views, args.height, args.width
    vl = 1.4 / res
    trunc = 5.12 * vl                                   # the reference's 0.04 m at 4 / 512 m voxels
    poses = room_views(nv)
    k4 = R.pinhole(h, w, 0.6 * w)
    depths = room_depths(poses, k4, h, w, dev)
    k = torch.from_numpy(np.tile(k4, (nv, 1))).to(dev)
    e = tsdf.extrinsics_from_poses(poses, nv).to(dev)
    if args.colour:
        return colour_rows(args, dev, vl, trunc, poses, depths, k, e)
    vol = tsdf.TSDFVolume((-0.7, -0.7, -0.7), (res, res, res), voxel_length=vl, sdf_trunc=trunc, device=dev)
    args_vol = (vol.tsdf, vol.weight, vol.origin, vol.voxel_length, vol.sdf_trunc)

    def batched():
        lib.tsdf_integrate(*args_vol, depths, k, e)

    def view_by_view():
        for i in range(nv):
            lib.tsdf_integrate(*args_vol, depths[i:i + 1], k[i:i + 1], e[i:i + 1])

    voxels = res ** 3
    floor = 16.0 * voxels / COPY_RATE
    result = {"device": torch.cuda.get_device_name(0), "res": res, "views": nv, "map": [h, w], "voxel_length": vl, "sdf_trunc": trunc,
              "reps": args.reps, "timing": "HIP events, one warm-up call, median of reps; the volume is zeroed before every call (untimed)",
              "traffic_floor_s": round(floor, 6), "traffic_floor_note": "16 B per voxel at 6.29 TB/s (device-to-device copy rate)"}
    t, all_t, _ = timed(view_by_view, args.reps, before=vol.reset)
    by_view = (vol.tsdf.clone(), vol.weight.clone())
    result["view_by_view"] = {"seconds": round(t, 6), "all_seconds": [round(x, 6) for x in all_t], "per_view_s": round(t / nv, 6),
                              "floor_multiple": round(t / (nv * floor), 2)}
    print(json.dumps({"view_by_view": result["view_by_view"]}), flush=True)
    t, all_t, _ = timed(batched, args.reps, before=vol.reset)
    same = torch.equal(vol.tsdf.view(torch.int32), by_view[0].view(torch.int32)) and torch.equal(vol.weight, by_view[1])
    observed = int((vol.weight > 0).sum())
    result["batched"] = {"seconds": round(t, 6), "all_seconds": [round(x, 6) for x in all_t], "floor_multiple": round(t / floor, 2),
                         "voxel_views_per_s": round(voxels * nv / t, 1), "speedup_over_view_by_view": round(result["view_by_view"]["seconds"] / t, 2),
                         "bits_equal_view_by_view": bool(same), "observed_voxels": observed,
                         "mean_views_per_observed_voxel": round(float(vol.weight.sum()) / max(observed, 1), 2)}
    print(json.dumps({"batched": result["batched"]}), flush=True)
    del by_view
    if not args.no_extract:
        t, all_t, m = timed(vol.extract_mesh, args.reps)
        result["extract"] = {"seconds": round(t, 6), "all_seconds": [round(x, 6) for x in all_t], "vertices": int(m[0].shape[0]),
                             "faces": int(m[1].shape[0]), "cells_per_s": round((res - 1) ** 3 / t, 1)}
        print(json.dumps({"extract": result["extract"]}), flush=True)
    if not args.no_cpu:
        cres = args.cpu_res
        cvl = 1.4 / cres
        secs, obs = cpu_baseline(cres, cvl, 5.12 * cvl, depths.cpu().numpy(), np.tile(k4, (nv, 1)), e.cpu().numpy(), args.workers)
        result["cpu"] = {"res": cres, "workers": args.workers, "seconds": round(secs, 3), "voxel_views_per_s": round(cres ** 3 * nv / secs, 1),
                         "observed_voxels": obs, "what": "tests/tsdf_restatement.py (NumPy), x-slabs on a thread pool, host clock"}
        print(json.dumps({"cpu": result["cpu"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
