#!/usr/bin/env python3
"""Device time of refuse (vf_nerf_amd.refuse, csrc/vfn_raster.hip) on the workload of tools/bench_tsdf.py: the room scene — cameras inside
the box [-0.6, 0.6]^3 — fused at --res^3 (512) from --views (100) analytic depth maps of --height x --width (680 x 1200), and the mesh
that gives then refused with the same cameras.  Recorded:

    raster_batched       ONE vfn_raster_depth call over all views: faces and vertices are read once.
    raster_view_by_view  the same kernel called once per view (the baseline).
    counters             fragments (kept (face, pixel) candidates), atomics sent, (face, view) pairs walked by a whole wave.
    smooth               10 Jacobi steps of Laplacian smoothing, with and without building the adjacency (torch unique).
    refuse               the whole chain: rasterise, truncate, fuse into a fresh volume, extract.
    cpu                  the NumPy restatement (tests/raster_restatement.py) of the rasteriser on a reduced size: the mesh of a
                         --cpu-res^3 (64) volume, --cpu-views (16) views of a quarter of the size, one view per thread on --workers
                         (16) threads; host clock.

HIP events around each call, one warm-up call, --reps timed calls, the median reported (all repeats are listed).

    python tools/bench_refuse.py [--res 512] [--views 100] [--height 680] [--width 1200] [--reps 3] [--out profiles/r10/bench_refuse.json]
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

from bench_tsdf import room_depths, room_views, timed  # noqa: E402


def fused_room(res, poses, k4, h, w, dev):
    """The room fused at res^3 from the analytic depth maps of the given views -> (mesh, bounds, voxel length, truncation)."""
    from vf_nerf_amd import tsdf
    vl = 1.4 / res
    trunc = 5.12 * vl
    depths = room_depths(poses, k4, h, w, dev)
    vol = tsdf.TSDFVolume((-0.7, -0.7, -0.7), (res, res, res), voxel_length=vl, sdf_trunc=trunc, device=dev)
    vol.integrate(depths, matrices(k4, len(poses)), poses)
    del depths
    return vol.extract_mesh(), ((-0.7, -0.7, -0.7), (0.7, 0.7, 0.7)), vl, trunc


def matrices(k4, n):
    k = np.tile(np.eye(3, dtype=np.float32), (n, 1, 1))
    k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2] = k4
    return k


def rounded(t, all_t):
    return {"seconds": round(t, 6), "all_seconds": [round(x, 6) for x in all_t]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-res", type=int, default=64)
    ap.add_argument("--cpu-views", type=int, default=16)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-view-by-view", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refuse: no GPU visible (nothing here can be measured on a CPU)")
    import raster_restatement as RR
    import tsdf_restatement as R
    from vf_nerf_amd import lib, raster, refuse, tsdf
    dev = torch.device("cuda:0")
    res, nv, h, w = args.res, args.views, args.height, args.width
    poses = room_views(nv)
    k4 = R.pinhole(h, w, 0.6 * w)
    mesh, bounds, vl, trunc = fused_room(res, poses, k4, h, w, dev)
    verts, faces = mesh
    k = torch.from_numpy(np.tile(k4, (nv, 1))).to(dev)
    e = tsdf.extrinsics_from_poses(poses, nv).to(dev)
    ras = (h, w, raster.NEAR, raster.FAR, raster.PIXEL_CENTRE)
    result = {"device": torch.cuda.get_device_name(0), "res": res, "views": nv, "map": [h, w], "voxel_length": vl, "sdf_trunc": trunc,
              "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "reps": args.reps,
              "near_far_pixel_centre": [raster.NEAR, raster.FAR, raster.PIXEL_CENTRE],
              "timing": "HIP events, one warm-up call, median of reps; every call fills and finishes its own depth maps"}
    print(json.dumps({"mesh": [result["vertices"], result["faces"]]}), flush=True)

    t, all_t, out = timed(lambda: lib.raster_depth(verts, faces, k, e, *ras), args.reps)
    batched, counters = out
    pairs = faces.shape[0] * nv
    result["raster_batched"] = dict(rounded(t, all_t), face_views_per_s=round(pairs / t, 1), fragments_per_s=round(counters["fragments"] / t, 1),
                                    atomics_per_s=round(counters["atomics"] / t, 1), pixels_hit=int((batched > 0).sum()),
                                    note="includes the fill and finish passes over the depth maps and one 32-byte status read")
    result["counters"] = dict(counters, face_view_pairs=pairs, fragments_per_pair=round(counters["fragments"] / pairs, 4),
                              atomics_per_fragment=round(counters["atomics"] / max(counters["fragments"], 1), 4))
    print(json.dumps({"raster_batched": result["raster_batched"], "counters": result["counters"]}), flush=True)

    if not args.no_view_by_view:
        def view_by_view():
            return torch.cat([lib.raster_depth(verts, faces, k[i:i + 1], e[i:i + 1], *ras)[0] for i in range(nv)])
        t, all_t, single = timed(view_by_view, args.reps)
        result["raster_view_by_view"] = dict(rounded(t, all_t), per_view_s=round(t / nv, 6),
                                             batched_speedup=round(t / result["raster_batched"]["seconds"], 2),
                                             bits_equal_batched=bool(torch.equal(single.view(torch.int32), batched.view(torch.int32))))
        del single
        print(json.dumps({"raster_view_by_view": result["raster_view_by_view"]}), flush=True)
    del batched

    t, all_t, _ = timed(lambda: refuse.smooth_laplacian(mesh), args.reps)
    row_start, nb = refuse.vertex_adjacency(faces, verts.shape[0])
    t2, all_t2, _ = timed(lambda: lib.smooth_laplacian(verts, row_start, nb, refuse.ITERATIONS, refuse.LAM), args.reps)
    result["smooth"] = dict(rounded(t, all_t), iterations=refuse.ITERATIONS, kernel_only=rounded(t2, all_t2), neighbours=int(nb.shape[0]))
    del row_start, nb
    print(json.dumps({"smooth": result["smooth"]}), flush=True)

    km = matrices(k4, nv)
    t, all_t, refused = timed(lambda: refuse.refuse(mesh, km, poses, h, w, bounds=bounds, voxel_length=vl, sdf_trunc=trunc), args.reps)
    result["refuse"] = dict(rounded(t, all_t), vertices=int(refused[0].shape[0]), faces=int(refused[1].shape[0]),
                            note="rasterise + truncate + fresh volume + integrate + extract, host reads included")
    print(json.dumps({"refuse": result["refuse"]}), flush=True)
    del refused

    if not args.no_cpu:
        ch, cw, cv = h // 4, w // 4, args.cpu_views
        ck4 = R.pinhole(ch, cw, 0.6 * cw)
        cmesh = fused_room(args.cpu_res, poses[:cv], ck4, ch, cw, dev)[0]
        cverts, cfaces = cmesh[0].cpu().numpy(), cmesh[1].cpu().numpy()
        ce = [R.extrinsic(p) for p in poses[:cv]]
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=args.workers) as pool:
            maps = list(pool.map(lambda i: RR.rasterize_view(cverts, cfaces, ck4, ce[i], ch, cw), range(cv)))
        secs = time.perf_counter() - t0
        got = lib.raster_depth(cmesh[0], cmesh[1], torch.from_numpy(np.tile(ck4, (cv, 1))).to(dev),
                               tsdf.extrinsics_from_poses(poses[:cv], cv).to(dev), ch, cw, raster.NEAR, raster.FAR, raster.PIXEL_CENTRE)[0]
        t, all_t, _ = timed(lambda: lib.raster_depth(cmesh[0], cmesh[1], torch.from_numpy(np.tile(ck4, (cv, 1))).to(dev),
                                                     tsdf.extrinsics_from_poses(poses[:cv], cv).to(dev), ch, cw, *ras[2:]), args.reps)
        result["cpu"] = {"res": args.cpu_res, "views": cv, "map": [ch, cw], "faces": int(cfaces.shape[0]), "workers": args.workers,
                         "seconds": round(secs, 3), "face_views_per_s": round(cfaces.shape[0] * cv / secs, 1),
                         "device_same_size": rounded(t, all_t),
                         "device_bits_equal": bool(np.array_equal(got.cpu().numpy().view(np.uint32), np.stack(maps).view(np.uint32))),
                         "what": "tests/raster_restatement.py (NumPy), one view per thread, host clock"}
        print(json.dumps({"cpu": result["cpu"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
