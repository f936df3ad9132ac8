#!/usr/bin/env python3
"""Device time of connected components (vf_nerf_amd.meshops, csrc/vfn_cc.hip) on the mesh tools/bench_refuse.py builds: the room scene
fused at --res^3 (512) from --views (100) analytic depth maps of --height x --width (680 x 1200).  For both connectivities it reports

    components         meshops.connected_components of the mesh already on the device (K, the largest component), and its parts timed apart:
                       items (the half-edge keys or vertex incidences and their sort: torch), union (the identity forest and
                       vfn_cc_union_runs), flatten (vfn_cc_flatten), unique (torch.unique with the inverse: the read for K), labels
                       (vertex labels and counts: torch), areas (vfn_tri_areas, the stable sort by label, the gather and
                       vfn_cc_segment_sums) — the three kernels with their algorithmic bytes against the 6.29 TB/s float4 copy rate, each
                       also as 20 launches in a row without the status read
    filter             meshops.filter_components(min_faces=--min-faces), the whole call
    host               what a user had to do without it, in the same process: download the faces, the face adjacency by a numpy sort of
                       the same keys, scipy.sparse.csgraph.connected_components, upload the labels — host clock around all of it — and
                       whether the host's partition is the device's

HIP events around each call, one warm-up call, --reps timed calls, the median reported (all repeats are listed).  No test asserts a time.

    python tools/bench_components.py [--res 512] [--reps 5] [--out profiles/r19/bench_components.json]
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


def by_lowest(labels: np.ndarray) -> np.ndarray:
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inverse.reshape(-1)]


def host_components(faces: np.ndarray, n_vertices: int, connectivity: str):
    """-> (labels[m], seconds of the adjacency, seconds of scipy): faces that hold one key joined along the sorted key list."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    m = len(faces)
    face = np.arange(m, dtype=np.int64)
    if connectivity == "edge":
        a = np.concatenate((faces[:, 0], faces[:, 1], faces[:, 2]))
        b = np.concatenate((faces[:, 1], faces[:, 2], faces[:, 0]))
        keys, nodes = np.minimum(a, b) * n_vertices + np.maximum(a, b), np.concatenate((face, face, face))
        keys[a == b] = -1
    else:
        keys, nodes = faces.T.reshape(-1), np.concatenate((face, face, face))
    order = np.argsort(keys, kind="stable")
    keys, nodes = keys[order], nodes[order]
    same = (keys[1:] == keys[:-1]) & (keys[1:] >= 0)
    graph = coo_matrix((np.ones(int(same.sum()), dtype=np.int8), (nodes[:-1][same], nodes[1:][same])), shape=(m, m)).tocsr()
    t1 = time.perf_counter()
    _, labels = connected_components(graph, directed=False)
    return labels, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--min-faces", type=int, default=51)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_components: no GPU visible (nothing here can be measured on a CPU)")
    import tsdf_restatement as R
    from vf_nerf_amd import lib, meshops
    if not args.no_host:
        import scipy.sparse.csgraph  # noqa: F401  (loaded before the host route is timed)
    dev = torch.device("cuda:0")
    h, w = args.height, args.width
    (verts, faces), _, _, _ = fused_room(args.res, room_views(args.views), R.pinhole(h, w, 0.6 * w), h, w, dev)
    verts, faces = verts.to(torch.float64).contiguous(), faces.to(torch.int64).contiguous()
    n, m = int(verts.shape[0]), int(faces.shape[0])
    result = {"device": torch.cuda.get_device_name(0), "res": args.res, "views": args.views, "map": [h, w], "vertices": n, "faces": m,
              "reps": args.reps, "hbm_copy_rate_bytes_per_s": HBM_COPY_RATE,
              "timing": "HIP events, one warm-up call, median of reps; host reads inside a call are part of it", "connectivities": []}
    zero = lambda: torch.zeros(1, dtype=torch.int64, device=dev)          # noqa: E731
    forest = lambda: torch.arange(m, dtype=torch.int32, device=dev)       # noqa: E731
    for connectivity in meshops.CONNECTIVITIES:
        t, all_t, c = timed(lambda: meshops.connected_components((verts, faces), connectivity=connectivity), args.reps)
        line = {"connectivity": connectivity, "K": c.n_components, "largest_component": int(c.face_count.max().cpu()),
                "components": dict(rounded(t, all_t), faces_per_s=round(m / t, 1),
                                   note="the public call on a device mesh: index check, items, unions, flatten, unique, labels, areas, ONE status read")}
        t, all_t, _ = timed(lambda: meshops.connected_components((verts, faces), connectivity=connectivity, areas=False), args.reps)
        line["components_without_areas"] = rounded(t, all_t)
        t, all_t, (keys, nodes) = timed(lambda: meshops.component_items(faces, n, connectivity), args.reps)
        items = int(keys.shape[0])
        parts = {"items": dict(rounded(t, all_t), items=items, note="edge: 3m keys and torch.sort(stable); vertex: torch.unique of the 3m incidence keys")}
        union_bytes = 16 * items + 8 * m
        t, all_t, parent = timed(lambda: lib.cc_union_runs(keys, nodes, forest()), args.reps)
        parts["union"] = dict(with_rate(t, all_t, union_bytes),
                              note="the identity forest, vfn_cc_union_runs and one status read; 16 B an item streamed, a forest word read and written a node — "
                                   "the finds' gathered words are not counted: the kernel waits for dependent loads and compare-and-swaps")
        shared = zero()
        t, all_t, _ = timed(lambda: [lib.cc_union_runs(keys, nodes, forest(), info=shared) for _ in range(BURST)], args.reps)
        parts["union"]["kernel_only"] = dict(with_rate(t / BURST, [x / BURST for x in all_t], union_bytes),
                                             note=f"{BURST} launches in a row (each with its fresh forest), no read: seconds per launch")
        t, all_t, _ = timed(lambda: [forest() for _ in range(BURST)], args.reps)
        parts["union"]["forest_only"] = dict(rounded(t / BURST, [x / BURST for x in all_t]), note="torch.arange(m, int32) alone, the same way")
        t, all_t, root = timed(lambda: lib.cc_flatten(parent), args.reps)
        parts["flatten"] = dict(with_rate(t, all_t, 12 * m), note="vfn_cc_flatten and one status read; 4 B read and 8 B written a node, chains on top")
        t, all_t, _ = timed(lambda: [lib.cc_flatten(parent, info=shared) for _ in range(BURST)], args.reps)
        parts["flatten"]["kernel_only"] = dict(with_rate(t / BURST, [x / BURST for x in all_t], 12 * m), note=f"{BURST} launches in a row, no read")
        depth = parent.to(torch.int64)
        hops = 0
        while not bool((depth[depth] == depth).all()) and hops < 64:
            depth, hops = depth[depth], hops + 1
        parts["flatten"]["forest_depth_at_most"] = 2 ** hops
        t, all_t, (first_face, face_label) = timed(lambda: torch.unique(root, return_inverse=True), args.reps)
        parts["unique"] = dict(rounded(t, all_t), note="torch.unique(root, return_inverse=True): the numbering and the read for K")
        k = int(first_face.shape[0])

        def labels():
            vl = torch.full((n,), k, dtype=torch.int64, device=dev).scatter_reduce(0, faces.reshape(-1), face_label.repeat_interleave(3), reduce="amin")
            return torch.where(vl == k, torch.full_like(vl, -1), vl), torch.bincount(face_label, minlength=k)

        t, all_t, (_, face_count) = timed(labels, args.reps)
        parts["labels"] = dict(rounded(t, all_t), note="vertex labels (scatter amin) and face counts (bincount): torch")
        t, all_t, per_face = timed(lambda: lib.tri_areas(verts, faces), args.reps)
        parts["tri_areas"] = dict(with_rate(t, all_t, (24 + 72 + 8) * m), note="vfn_tri_areas and one status read; 24 B of indices, 72 B gathered, 8 B written a face")

        def sort_gather():
            order = torch.sort(face_label, stable=True)[1]
            return per_face[order].contiguous(), torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(face_count, dim=0))).contiguous()

        t, all_t, (sorted_areas, start) = timed(sort_gather, args.reps)
        parts["area_sort"] = dict(rounded(t, all_t), note="torch.sort(face_label, stable=True), the gather of the areas, the cumsum of the counts")
        sum_bytes = 8 * m + 24 * k
        t, all_t, area = timed(lambda: lib.cc_segment_sums(sorted_areas, start), args.reps)
        parts["segment_sums"] = dict(with_rate(t, all_t, sum_bytes), note="vfn_cc_segment_sums and one status read; 8 B a value, 16 B of bounds and 8 B written a segment")
        t, all_t, _ = timed(lambda: [lib.cc_segment_sums(sorted_areas, start, info=shared) for _ in range(BURST)], args.reps)
        parts["segment_sums"]["kernel_only"] = dict(with_rate(t / BURST, [x / BURST for x in all_t], sum_bytes), note=f"{BURST} launches in a row, no read")
        line["parts"] = parts
        line["parts_equal_the_call"] = bool(torch.equal(face_label, c.face_label) and torch.equal(area.view(torch.int64), c.area.view(torch.int64)))
        t, all_t, kept = timed(lambda: meshops.filter_components((verts, faces), min_faces=args.min_faces, connectivity=connectivity), args.reps)
        line["filter"] = dict(rounded(t, all_t), min_faces=args.min_faces, faces_kept=int(kept[1].shape[0]), vertices_kept=int(kept[0].shape[0]),
                              note="meshops.filter_components, the whole call: the components without areas, the masks, the compaction")
        print(json.dumps(line), flush=True)

        if not args.no_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fh = faces.cpu().numpy()
            t1 = time.perf_counter()
            labels_host, t_adjacency, t_scipy = host_components(fh, n, connectivity)
            t2 = time.perf_counter()
            up = torch.from_numpy(labels_host).to(dev)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            td = line["components_without_areas"]["seconds"]
            line["host"] = {"download_s": round(t1 - t0, 4), "adjacency_s": round(t_adjacency, 4), "connected_components_s": round(t_scipy, 4),
                            "upload_s": round(t3 - t2, 4), "total_s": round(t3 - t0, 4), "device_without_areas_s": td,
                            "ratio": round((t3 - t0) / td, 1),
                            "same_partition": bool(np.array_equal(by_lowest(labels_host), c.face_label.cpu().numpy())),
                            "note": "numpy and scipy on the host clock, one thread; the labels alone (no counts, no areas)"}
            del up
            print(json.dumps({"host": line["host"]}), flush=True)
        result["connectivities"].append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
