#!/usr/bin/env python3
"""Device time of k-means (vf_nerf_amd.cluster.kmeans, csrc/vfn_kmeans.hip) on what meshops.dominant_bases clusters: the vertex normals of
the mesh tools/bench_simplify.py uses — the room scene fused at --res^3 (512) from --views (100) analytic depth maps of --height x --width
(680 x 1200) — as it is and after a vertex-clustering simplification at --factor (2) times the extraction's voxel.  For k in --ks
(3, 6, 16) it reports

    kmeans             the whole public call on the device normals (farthest-point seeding, Lloyd's passes with one 8-byte read each):
                       passes, convergence, counts
    seeding            the farthest-point seeds alone (a mean, k launches of vfn_kmeans_seed, a gather; no read)
    assign / update    one pass of each kernel pair, as --burst (20) launches in a row without a read: seconds per launch, with the
                       algorithmic bytes against the 6.29 TB/s float4 copy rate
    host               what a user had to do without it, in the same process: download the normals, sklearn.cluster.KMeans from the
                       SAME seeds (n_init=1, algorithm="lloyd", tol=0, the threads the box allows), upload centres and labels — host clock
                       around all of it — and whether its labels and iteration count are the device's

HIP events around each call, one warm-up call, --reps timed calls, the median reported (all repeats are listed).  No test asserts a time.

    python tools/bench_kmeans.py [--res 512] [--reps 5] [--out profiles/r22/bench_kmeans.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_refuse import fused_room, rounded  # noqa: E402
from bench_tsdf import room_views, timed  # noqa: E402

HBM_COPY_RATE = 6.29e12            # bytes / s: the measured float4 copy
THREADS = 16                       # what a command may use on the box


def with_rate(t, all_t, nbytes):
    return dict(rounded(t, all_t), algorithmic_bytes=int(nbytes), bytes_per_s=round(nbytes / t, 1), share_of_hbm_copy_rate=round(nbytes / t / HBM_COPY_RATE, 4))


def referenced_normals(meshops, v, f):
    used = torch.zeros(v.shape[0], dtype=torch.bool, device=v.device)
    used[f.reshape(-1)] = True
    return meshops.vertex_normals((v, f))[used].contiguous()


def host_alternative(normals, seeds, k, max_iter, device_result):
    try:
        from sklearn.cluster import KMeans
    except Exception as e:          # the comparison is optional: the tool still reports the device
        return {"unavailable": f"{type(e).__name__}: {e}"}
    try:
        from threadpoolctl import threadpool_limits
    except Exception:
        threadpool_limits = None
    dev = normals.device
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x, init = normals.cpu().numpy(), seeds.cpu().numpy()
    t1 = time.perf_counter()
    model = KMeans(n_clusters=k, init=init, n_init=1, algorithm="lloyd", tol=0, max_iter=max_iter)
    if threadpool_limits is not None:
        with threadpool_limits(limits=THREADS):
            model.fit(x)
    else:
        model.fit(x)
    t2 = time.perf_counter()
    up = [torch.from_numpy(model.cluster_centers_).to(dev), torch.from_numpy(model.labels_.astype(np.int64)).to(dev)]
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    del up
    return {"download_s": round(t1 - t0, 4), "fit_s": round(t2 - t1, 4), "upload_s": round(t3 - t2, 4), "total_s": round(t3 - t0, 4),
            "n_iter": int(model.n_iter_), "fit_s_per_pass": round((t2 - t1) / max(int(model.n_iter_), 1), 6),
            "labels_equal": bool(np.array_equal(model.labels_, device_result.labels.cpu().numpy())),
            "n_iter_equal": int(model.n_iter_) == device_result.n_iter,
            "largest_centre_difference": float(np.abs(model.cluster_centers_ - device_result.centres.cpu().numpy()).max()),
            "threads": THREADS if threadpool_limits is not None else os.environ.get("OMP_NUM_THREADS", "unset"),
            "note": "sklearn.cluster.KMeans(init=the device's farthest-point seeds, n_init=1, algorithm='lloyd', tol=0) on the host clock"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--factor", type=float, default=2.0)
    ap.add_argument("--ks", type=int, nargs="+", default=[3, 6, 16])
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans: no GPU visible (nothing here can be measured on a CPU)")
    import tsdf_restatement as R
    from vf_nerf_amd import cluster, lib, meshops
    dev = torch.device("cuda:0")
    h, w = args.height, args.width
    (verts, faces), _, extraction_voxel, _ = fused_room(args.res, room_views(args.views), R.pinhole(h, w, 0.6 * w), h, w, dev)
    verts, faces = verts.to(torch.float64).contiguous(), faces.to(torch.int64).contiguous()
    simplified = meshops.simplify_vertex_clustering((verts, faces), args.factor * extraction_voxel, "quadric")
    sets = {"as_fused": referenced_normals(meshops, verts, faces), f"simplified_{args.factor:g}x": referenced_normals(meshops, simplified.vertices, simplified.faces)}
    result = {"device": torch.cuda.get_device_name(0), "res": args.res, "views": args.views, "map": [h, w], "vertices": int(verts.shape[0]),
              "faces": int(faces.shape[0]), "extraction_voxel": extraction_voxel, "simplification_voxel": args.factor * extraction_voxel,
              "reps": args.reps, "burst": args.burst, "max_iter": args.max_iter, "hbm_copy_rate_bytes_per_s": HBM_COPY_RATE,
              "timing": "HIP events, one warm-up call, median of reps; host reads inside a call are part of it", "sets": []}
    for name, normals in sets.items():
        n = int(normals.shape[0])
        for k in args.ks:
            line = {"set": name, "normals": n, "k": k}
            t, all_t, r = timed(lambda: cluster.kmeans(normals, k, max_iter=args.max_iter), args.reps)
            line["kmeans"] = dict(rounded(t, all_t), passes=r.n_iter, converged=r.converged, seconds_per_pass=round(t / r.n_iter, 7),
                                  counts=r.counts.cpu().tolist(), inertia=float(r.inertia.cpu()),
                                  note="the public call on device normals: seeding, passes of assign + update with one 8-byte read each, the inertia")
            work = cluster._Work(normals, k)
            t, all_t, seeds = timed(lambda: cluster._seeds_farthest(normals, k, work), args.reps)
            line["seeding"] = dict(rounded(t, all_t), note="update with k = 1, assign, k launches of vfn_kmeans_seed, the gather: no read")
            label = torch.empty(n, dtype=torch.int32, device=dev)
            sqdist = torch.empty(n, dtype=torch.float64, device=dev)
            centres = r.centres.clone()
            lib.kmeans_assign(normals, centres, None, label, sqdist, work.changed, info=work.info)
            burst = lambda fn: [fn() for _ in range(args.burst)]          # noqa: E731
            t, all_t, _ = timed(lambda: burst(lambda: lib.kmeans_assign(normals, centres, label, label, sqdist, work.changed, info=work.info)), args.reps)
            line["assign"] = dict(with_rate(t / args.burst, [x / args.burst for x in all_t], 40 * n),
                                  note=f"{args.burst} launches in a row, no read: seconds per launch; 24 B of point and 4 B of label read, 4 + 8 B written a point")
            t, all_t, _ = timed(lambda: burst(lambda: lib.kmeans_update(normals, label, centres, info=work.info, workspace=work.update_ws)), args.reps)
            line["update"] = dict(with_rate(t / args.burst, [x / args.burst for x in all_t], 28 * n),
                                  note=f"{args.burst} launches in a row (two kernels each), no read: seconds per launch; 24 B of point and 4 B of label read a point")
            pass_s = line["assign"]["seconds"] + line["update"]["seconds"]
            line["kernels_share_of_a_pass"] = round(pass_s / (line["kmeans"]["seconds"] / r.n_iter), 4)
            if not args.no_host:
                line["host"] = host_alternative(normals, seeds, k, args.max_iter, r)
                if "total_s" in line["host"]:
                    line["host"]["device_s"] = line["kmeans"]["seconds"]
                    line["host"]["ratio"] = round(line["host"]["total_s"] / line["kmeans"]["seconds"], 1)
            print(json.dumps(line), flush=True)
            result["sets"].append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
