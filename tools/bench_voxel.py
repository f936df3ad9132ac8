#!/usr/bin/env python3
"""Device time of voxel down-sampling (vf_nerf_amd.voxel, csrc/vfn_voxel.hip) on --samples (10^6) surface samples of the mesh
tools/bench_refuse.py builds: the room scene fused at --res^3 (512) from --views (100) analytic depth maps of --height x --width
(680 x 1200).  At every --voxels size (0.025 and 0.005: half of the reference's two distance thresholds) it reports

    down_sample        metrics3d.voxel_down_sample of the samples already on the device, V, points per voxel, and its parts timed apart:
                       box (the bounding box and its host read), keys (vfn_voxel_keys and one status read), sort (torch.sort,
                       stable), table (run flags, cumsum, ONE host read, searchsorted, the inverse scatter), gather (values[perm]),
                       means (vfn_voxel_means and one status read) — the two kernels with their algorithmic bytes against the
                       6.29 TB/s float4 copy rate, each also as 20 launches in a row without the read (a single launch and its
                       status read outweigh a kernel of this size; 20 in a row are bounded by the rate the binding issues them at)
    score_mesh         metrics3d.score_mesh(search="grid") against a shifted copy with and without voxel_size, alternating
    host               what a user had to do without it, in the same process: download both clouds, the same keys and np.unique-based
                       means on the host (numpy; the per-channel sums on --workers threads at most), upload — host clock around all of
                       it — and whether the host's voxels and counts are the device's (its sums are np.bincount's, not the contract's
                       serial ones, so the means are compared within 1e-12)

HIP events around each call, one warm-up call, --reps timed calls, the median reported (all repeats are listed).  No test asserts a time.

    python tools/bench_voxel.py [--samples 1000000] [--voxels 0.025 0.005] [--reps 5] [--out profiles/r18/bench_voxel.json]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_refuse import fused_room, rounded  # noqa: E402
from bench_tsdf import room_views, timed  # noqa: E402

HBM_COPY_RATE = 6.29e12            # bytes / s: the measured float4 copy
BURST = 20                         # launches in a row of the kernel-only timings: at 10^6 points one launch and its status read outweigh the kernel


def with_rate(t, all_t, nbytes):
    return dict(rounded(t, all_t), algorithmic_bytes=int(nbytes), bytes_per_s=round(nbytes / t, 1), share_of_hbm_copy_rate=round(nbytes / t / HBM_COPY_RATE, 4))


def host_down_sample(points: np.ndarray, h: float, workers: int):
    """np.unique-based voxel means on the host -> (means[V,3], counts[V], inverse[n]): the contract's keys, then a sum per channel by
    np.bincount over the inverse (numpy's order of summation, not the contract's)."""
    origin = points.min(axis=0) - 0.5 * h
    c = np.floor((points - origin) / h).astype(np.int64)
    keys = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    with ThreadPoolExecutor(min(workers, 3)) as pool:
        sums = list(pool.map(lambda k: np.bincount(inverse, weights=points[:, k], minlength=len(counts)), range(3)))
    return np.stack(sums, axis=1) / counts[:, None], counts, inverse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--voxels", type=float, nargs="+", default=[0.025, 0.005])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_voxel: no GPU visible (nothing here can be measured on a CPU)")
    import tsdf_restatement as R
    from vf_nerf_amd import lib, metrics3d, voxel
    dev = torch.device("cuda:0")
    h, w = args.height, args.width
    (verts, faces), _, vl, _ = fused_room(args.res, room_views(args.views), R.pinhole(h, w, 0.6 * w), h, w, dev)
    other = (verts * 1.002 + 0.5 * vl, faces)
    n = args.samples
    u = torch.rand(n, 3, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(18))
    pred, _ = metrics3d.sample_surface(verts, faces, n, uniforms=u)
    ref, _ = metrics3d.sample_surface(*other, n, uniforms=u)
    result = {"device": torch.cuda.get_device_name(0), "res": args.res, "views": args.views, "map": [h, w], "vertices": int(verts.shape[0]),
              "faces": int(faces.shape[0]), "samples": n, "reps": args.reps, "hbm_copy_rate_bytes_per_s": HBM_COPY_RATE,
              "timing": "HIP events, one warm-up call, median of reps; host reads inside a call are part of it", "voxels": []}
    zero = lambda: torch.zeros(1, dtype=torch.int64, device=dev)          # noqa: E731
    for size in args.voxels:
        t, all_t, sample = timed(lambda: metrics3d.voxel_down_sample(pred, size), args.reps)
        v = int(sample.points.shape[0])
        line = {"voxel_size": size, "V": v, "points_per_voxel": round(n / v, 3), "largest_voxel": int(sample.counts.max().cpu()),
                "dims": list(sample.dims), "down_sample": dict(rounded(t, all_t), points_per_s=round(n / t, 1),
                                                              note="the public call on device points: box read, keys, sort, table with its read, gather, means")}
        origin = sample.origin
        t, all_t, _ = timed(lambda: voxel.bounding_box(pred), args.reps)
        parts = {"box": dict(rounded(t, all_t), note="voxel.bounding_box: minima and maxima in two steps, ONE host read")}
        t, all_t, keys = timed(lambda: lib.voxel_keys(pred, origin, size), args.reps)
        parts["keys"] = dict(with_rate(t, all_t, 32 * n), note="vfn_voxel_keys and one status read; 24 B read and 8 B written a point")
        shared = zero()
        t, all_t, _ = timed(lambda: [lib.voxel_keys(pred, origin, size, info=shared) for _ in range(BURST)], args.reps)
        parts["keys"]["kernel_only"] = dict(with_rate(t / BURST, [x / BURST for x in all_t], 32 * n), note=f"{BURST} launches in a row, no read: seconds per launch")
        t, all_t, (sorted_key, perm) = timed(lambda: torch.sort(keys, stable=True), args.reps)
        parts["sort"] = dict(rounded(t, all_t), note="torch.sort(keys, stable=True): int64 keys and the permutation")
        t, all_t, (perm, start, _, _) = timed(lambda: voxel.table(keys, zero()), args.reps)
        parts["table_with_sort"] = dict(rounded(t, all_t), note="voxel.table: the sort again, run flags, cumsum, ONE host read, searchsorted, inverse scatter")
        t, all_t, gathered = timed(lambda: pred[perm].contiguous(), args.reps)
        parts["gather"] = dict(with_rate(t, all_t, (8 + 24 + 24) * n), note="values[perm]: 8 B of index, 24 B gathered and 24 B written a point")
        t, all_t, means = timed(lambda: lib.voxel_means(gathered, start), args.reps)
        parts["means"] = dict(with_rate(t, all_t, 24 * n + (16 + 24) * v),
                              note="vfn_voxel_means (C = 3) and one status read; 24 B a point, 16 B of bounds and 24 B written a voxel")
        t, all_t, _ = timed(lambda: [lib.voxel_means(gathered, start, info=shared) for _ in range(BURST)], args.reps)
        parts["means"]["kernel_only"] = dict(with_rate(t / BURST, [x / BURST for x in all_t], 24 * n + (16 + 24) * v),
                                             note=f"{BURST} launches in a row, no read: seconds per launch")
        line["parts"] = parts
        line["parts_equal_the_call"] = bool(torch.equal(means.view(torch.int64), sample.points.view(torch.int64)))
        print(json.dumps(line), flush=True)

        score = lambda **kw: metrics3d.score_mesh((verts, faces), other, num_points=n, distance_thresh=2 * size, uniforms=u, search="grid", **kw)      # noqa: E731
        score(voxel_size=size)
        score()
        torch.cuda.synchronize()
        with_v, without = [], []
        for _ in range(args.reps):                                   # alternating: the two share whatever else the machine is doing
            tv, _, entry = timed(lambda: score(voxel_size=size), 1)
            tp, _, plain = timed(lambda: score(), 1)
            with_v.append(tv)
            without.append(tp)
        med = lambda x: float(np.median(x))                          # noqa: E731
        line["score_mesh"] = {"distance_thresh": 2 * size, "with_voxel_size": rounded(med(with_v), with_v), "without": rounded(med(without), without),
                              "voxel": entry["voxel"], "scores": {k: (plain[k], entry[k]) for k in ("precision", "recall", "fscore")},
                              "note": "search=\"grid\"; each timing is the second of two calls; (without, with) in scores"}
        print(json.dumps({"score_mesh": line["score_mesh"]}), flush=True)

        if not args.no_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ph, rh = pred.cpu().numpy(), ref.cpu().numpy()
            t1 = time.perf_counter()
            (pm, pc, pi), (rm, _, _) = host_down_sample(ph, size, args.workers), host_down_sample(rh, size, args.workers)
            t2 = time.perf_counter()
            up = torch.from_numpy(pm).to(dev), torch.from_numpy(rm).to(dev)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            td, _, _ = timed(lambda: (metrics3d.voxel_down_sample(pred, size), metrics3d.voxel_down_sample(ref, size)), args.reps)
            line["host"] = {"download_s": round(t1 - t0, 4), "unique_means_s": round(t2 - t1, 4), "upload_s": round(t3 - t2, 4),
                            "total_s": round(t3 - t0, 4), "device_both_clouds_s": round(td, 6), "speedup": round((t3 - t0) / td, 1),
                            "workers": min(args.workers, 3),
                            "same_voxels_and_counts": bool(np.array_equal(pc, sample.counts.cpu().numpy())
                                                           and np.array_equal(pi, sample.voxel_of_point.cpu().numpy())),
                            "largest_mean_difference": float(np.abs(pm - sample.points.cpu().numpy()).max()) if len(pm) == v else None,
                            "note": "both clouds; numpy on the host clock, np.unique and np.bincount (one thread each, three channels at a time)"}
            del up
            print(json.dumps({"host": line["host"]}), flush=True)
        result["voxels"].append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
