#!/usr/bin/env python3
"""Device time of vertex-clustering simplification (vf_nerf_amd.meshops.simplify_vertex_clustering, csrc/vfn_simplify.hip) on the mesh
tools/bench_refuse.py builds: the room scene fused at --res^3 (512) from --views (100) analytic depth maps of --height x --width
(680 x 1200).  At the voxel edges --factors (2 and 4) times the extraction's it reports, for both contractions,

    simplify           the whole public call on the device mesh with its colours: faces in and out, clusters, the share placed by the quadric
    parts              the same steps timed apart: clusters (the referenced vertices, the bounding box, vfn_voxel_keys and the table with its
                       sort: torch and the voxel unit), means (the gather and vfn_voxel_means), planes (vfn_face_planes), items (the
                       incidences and their stable sort by cluster: torch), quadrics (vfn_cluster_quadrics), faces (the remap, the two
                       cleaning steps and the compaction: torch) — the two new kernels with their algorithmic bytes against the 6.29 TB/s
                       float4 copy rate, each also as 20 launches in a row without the status read
    host               what a user had to do without it, in the same process: download the mesh, the NumPy restatement of the same
                       contract (tests/simplify_restatement.py: simplify_arrays), upload the result — host clock around all of it — and
                       whether the host's bits are the device's (--host-factors: by default the largest voxel only)

HIP events around each call, one warm-up call, --reps timed calls, the median reported (all repeats are listed).  No test asserts a time.

    python tools/bench_simplify.py [--res 512] [--reps 5] [--out profiles/r21/bench_simplify.json]
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
BURST = 20                         # launches in a row of the kernel-only timings


def with_rate(t, all_t, nbytes):
    return dict(rounded(t, all_t), algorithmic_bytes=int(nbytes), bytes_per_s=round(nbytes / t, 1), share_of_hbm_copy_rate=round(nbytes / t / HBM_COPY_RATE, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--factors", type=float, nargs="+", default=[2.0, 4.0])
    ap.add_argument("--host-factors", type=float, nargs="*", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_simplify: no GPU visible (nothing here can be measured on a CPU)")
    import simplify_restatement as S
    import tsdf_restatement as R
    from vf_nerf_amd import lib, meshops, voxel
    host_factors = [max(args.factors)] if args.host_factors is None else args.host_factors
    dev = torch.device("cuda:0")
    h, w = args.height, args.width
    (verts, faces), _, extraction_voxel, _ = fused_room(args.res, room_views(args.views), R.pinhole(h, w, 0.6 * w), h, w, dev)
    verts, faces = verts.to(torch.float64).contiguous(), faces.to(torch.int64).contiguous()
    n, m = int(verts.shape[0]), int(faces.shape[0])
    colours = ((verts - verts.amin(dim=0)) / (verts.amax(dim=0) - verts.amin(dim=0))).contiguous()          # a colour per vertex: its place in the box
    result = {"device": torch.cuda.get_device_name(0), "res": args.res, "views": args.views, "map": [h, w], "vertices": n, "faces": m,
              "extraction_voxel": extraction_voxel, "reps": args.reps, "hbm_copy_rate_bytes_per_s": HBM_COPY_RATE,
              "timing": "HIP events, one warm-up call, median of reps; host reads inside a call are part of it", "voxels": []}
    zero = lambda: torch.zeros(1, dtype=torch.int64, device=dev)          # noqa: E731
    for factor in args.factors:
        size = factor * extraction_voxel
        line = {"factor": factor, "voxel_size": size}
        for contraction in meshops.CONTRACTIONS:
            t, all_t, s = timed(lambda: meshops.simplify_vertex_clustering((verts, faces), size, contraction=contraction, colours=colours), args.reps)
            line[contraction] = dict(rounded(t, all_t), faces_in=m, faces_out=int(s.faces.shape[0]), vertices_out=int(s.vertices.shape[0]),
                                     clusters=s.n_clusters, placed=int(s.placed.sum().cpu()),
                                     placed_share=round(float(s.placed.double().mean().cpu()), 4) if s.placed.shape[0] else 0.0,
                                     faces_per_s=round(m / t, 1),
                                     note="the public call on a device mesh with colours: index check, clusters, means, (planes, items, quadrics,) "
                                          "faces; three host reads of its own")
        quadric = s

        def clusters():
            used = torch.zeros(n, dtype=torch.bool, device=dev)
            used[faces.reshape(-1)] = True
            referenced = torch.nonzero(used).reshape(-1)
            vr = verts[referenced].contiguous()
            origin, _ = voxel.frame(*voxel.bounding_box(vr), size)
            info = zero()
            keys = lib.voxel_keys(vr, origin, size, info=info)
            return (referenced, vr, origin, keys) + voxel.table(keys, info)

        t, all_t, (referenced, vr, origin, keys, perm, start, cluster_of_referenced, _) = timed(clusters, args.reps)
        k = int(start.shape[0]) - 1
        parts = {"clusters": dict(rounded(t, all_t), clusters=k, note="referenced vertices (nonzero), the bounding box, vfn_voxel_keys, the stable sort "
                                                                      "of the keys and the table: two host reads")}
        values = torch.cat((vr, colours[referenced]), dim=1)
        t, all_t, means = timed(lambda: lib.voxel_means(values[perm].contiguous(), start, info=zero()), args.reps)
        parts["means"] = dict(rounded(t, all_t), note="the gather into sorted order and vfn_voxel_means over six channels, no read")
        plane_bytes = (24 + 72 + 40) * m
        t, all_t, planes = timed(lambda: lib.face_planes(verts, faces, origin), args.reps)
        parts["planes"] = dict(with_rate(t, all_t, plane_bytes), note="vfn_face_planes and one status read; 24 B of indices, 72 B gathered, 40 B written a face")
        shared = zero()
        t, all_t, _ = timed(lambda: [lib.face_planes(verts, faces, origin, info=shared) for _ in range(BURST)], args.reps)
        parts["planes"]["kernel_only"] = dict(with_rate(t / BURST, [x / BURST for x in all_t], plane_bytes), note=f"{BURST} launches in a row, no read: seconds per launch")
        cluster_of_vertex = torch.full((n,), -1, dtype=torch.int64, device=dev)
        cluster_of_vertex[referenced] = cluster_of_referenced
        t, all_t, (item_face, item_start) = timed(lambda: meshops._cluster_items(faces, cluster_of_vertex, k), args.reps)
        items = int(item_face.shape[0])
        parts["items"] = dict(rounded(t, all_t), items=items, items_per_cluster=round(items / k, 2), largest_cluster=int((item_start[1:] - item_start[:-1]).max().cpu()),
                              note="torch.unique of the 3m incidence keys, the stable sort by cluster, searchsorted: no read")
        key = keys[perm[start[:-1]]]
        cells = torch.stack((key >> 42, (key >> 21) & ((1 << 21) - 1), key & ((1 << 21) - 1)), dim=1).to(torch.float64)
        centres = ((cells + 0.5) * size + torch.tensor(origin, dtype=torch.float64, device=dev)).contiguous()
        mean_points = means[:, 0:3].contiguous()
        quadric_bytes = (8 + 40) * items + (16 + 24 + 24 + 24 + 8 + 1) * k
        call = lambda info=None: lib.cluster_quadrics(planes, item_face, item_start, centres, mean_points, origin, size, 1e-9, info=info)          # noqa: E731
        t, all_t, (position, placed, error) = timed(call, args.reps)
        parts["quadrics"] = dict(with_rate(t, all_t, quadric_bytes),
                                 note="vfn_cluster_quadrics and one status read; 8 B of the table and a gathered plane of 40 B an item, 16 B of bounds, "
                                      "72 B of centre / mean / position and 9 B of error and flag a cluster")
        t, all_t, _ = timed(lambda: [call(shared) for _ in range(BURST)], args.reps)
        parts["quadrics"]["kernel_only"] = dict(with_rate(t / BURST, [x / BURST for x in all_t], quadric_bytes), note=f"{BURST} launches in a row, no read: seconds per launch")

        def clean():
            remapped = cluster_of_vertex[faces]
            proper, kept = meshops._without_degenerate(position, remapped)
            kept = kept[meshops._without_duplicates(proper)[1]]
            face_keep = torch.zeros(m, dtype=torch.bool, device=dev)
            face_keep[kept] = True
            return meshops._select_faces(position, remapped, face_keep)

        t, all_t, cleaned = timed(clean, args.reps)
        parts["faces"] = dict(rounded(t, all_t), note="the remap, the degenerate faces, the duplicate triples (unique over sorted rows), the compaction: torch")
        line["parts"] = parts
        line["parts_equal_the_call"] = bool(torch.equal(cleaned[1], quadric.faces) and torch.equal(cleaned[0].view(torch.int64), quadric.vertices.view(torch.int64)))
        print(json.dumps(line), flush=True)

        if factor in host_factors:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vh, fh, ch = verts.cpu().numpy(), faces.cpu().numpy(), colours.cpu().numpy()
            t1 = time.perf_counter()
            ref = S.simplify_arrays(vh, fh, size, "quadric", ch)
            t2 = time.perf_counter()
            up = [torch.from_numpy(np.ascontiguousarray(ref[name])).to(dev) for name in ("vertices", "faces", "colours")]
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            td = line["quadric"]["seconds"]
            same = bool(np.array_equal(ref["vertices"].view(np.uint64), quadric.vertices.cpu().numpy().view(np.uint64)) and
                        np.array_equal(ref["faces"], quadric.faces.cpu().numpy()) and np.array_equal(ref["placed"], quadric.placed.cpu().numpy()))
            line["host"] = {"download_s": round(t1 - t0, 4), "restatement_s": round(t2 - t1, 4), "upload_s": round(t3 - t2, 4), "total_s": round(t3 - t0, 4),
                            "device_s": td, "ratio": round((t3 - t0) / td, 1), "same_bits": same,
                            "note": "numpy on the host clock, one thread; the restatement adds every cluster's ten sums lane by lane in Python"}
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
