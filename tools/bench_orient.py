#!/usr/bin/env python3
"""Device time of mesh orientation (vf_nerf_amd.meshops.orient, csrc/vfn_orient.hip) on the mesh tools/bench_refuse.py builds: the room
scene fused at --res^3 (512) from --views (100) analytic depth maps of --height x --width (680 x 1200) — wound consistently by
construction, so a seeded --flip fraction (0.1) of its faces is rewound first.  It reports

    orient             meshops.orient of the mesh already on the device, per reference ("first", "majority", "volume", "viewpoints" with
                       the --views camera centres), and whether the result has no inconsistent edge left
    parts              the stages timed apart: key sort (the half-edge keys with their direction bytes: torch), union (the x << 1 forest and
                       vfn_orient_union_runs), flatten (vfn_orient_flatten), numbering (torch.unique with the inverse: the read for K, and
                       the counts), conflicts (the manifold mask over all adjacent items and the per-component test: torch, no host read), votes (vfn_orient_votes, the stable
                       sort by label, the gather and vfn_cc_segment_sums), swap (the column swap: torch) — the kernels also as 20
                       launches in a row without the status read
    yardstick          meshops.connected_components(connectivity="edge", areas=False) and vfn_cc_union_runs alone, the same way, in the
                       same process: the union-find this one adds a bit to
    host               what a user had to do without it, in the same process: download the faces, the breadth-first two-colouring of
                       tests/orient_restatement.py (pure Python), upload the flips — host clock around all of it — and whether the host's
                       flips are the device's

HIP events around each call, one warm-up call, --reps timed calls, the median reported (all repeats are listed).  No test asserts a time.

    python tools/bench_orient.py [--res 512] [--reps 5] [--out profiles/r20/bench_orient.json]
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

BURST = 20                         # launches in a row of the kernel-only timings


def spread(all_t):
    return round((max(all_t) - min(all_t)) / min(all_t), 4)


def entry(t, all_t, **more):
    return dict(rounded(t, all_t), spread_over_repeats=spread(all_t), **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--flip", type=float, default=0.1)
    ap.add_argument("--seed", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_orient: no GPU visible (nothing here can be measured on a CPU)")
    import orient_restatement as OR
    import tsdf_restatement as R
    from vf_nerf_amd import lib, meshops
    dev = torch.device("cuda:0")
    h, w = args.height, args.width
    poses = room_views(args.views)
    (verts, faces), _, _, _ = fused_room(args.res, poses, R.pinhole(h, w, 0.6 * w), h, w, dev)
    verts, faces = verts.to(torch.float64).contiguous(), faces.to(torch.int64).contiguous()
    n, m = int(verts.shape[0]), int(faces.shape[0])
    as_fused = meshops.inconsistent_edges((verts, faces))
    which = torch.from_numpy(np.random.default_rng(args.seed).uniform(0, 1, m) < args.flip).to(dev)
    faces = meshops._rewind(faces, which)
    eyes = torch.from_numpy(np.ascontiguousarray(poses[:, :3, 3], dtype=np.float64)).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "res": args.res, "views": args.views, "map": [h, w], "vertices": n, "faces": m,
              "flipped_fraction": args.flip, "faces_flipped": int(which.sum().cpu()), "inconsistent_edges_as_fused": as_fused,
              "inconsistent_edges": meshops.inconsistent_edges((verts, faces)), "reps": args.reps,
              "timing": "HIP events, one warm-up call, median of reps; host reads inside a call are part of it; spread = (max - min) / min"}

    # the whole call, per reference
    result["orient"] = {}
    for reference in meshops.REFERENCES:
        views = eyes if reference == "viewpoints" else None
        t, all_t, (_, rewound, o) = timed(lambda: meshops.orient((verts, faces), reference=reference, viewpoints=views), args.reps)
        result["orient"][reference] = entry(t, all_t, faces_per_s=round(m / t, 1), K=o.n_components, not_orientable=int((~o.orientable).sum().cpu()),
                                            faces_rewound=int(o.flip.sum().cpu()), inconsistent_edges_after=meshops.inconsistent_edges((verts, rewound)))
        print(json.dumps({reference: result["orient"][reference]}), flush=True)

    # the stages
    zero = lambda: torch.zeros(1, dtype=torch.int64, device=dev)                          # noqa: E731
    forest = lambda: torch.arange(0, 2 * m, 2, dtype=torch.int32, device=dev)             # noqa: E731
    parts = {}
    t, all_t, (keys, nodes, dirs) = timed(lambda: meshops.orient_items(faces, n), args.reps)
    items = int(keys.shape[0])
    parts["key_sort"] = entry(t, all_t, items=items, note="3m keys with their direction bytes and torch.sort(stable)")
    t, all_t, words = timed(lambda: lib.orient_union_runs(keys, nodes, dirs, forest()), args.reps)
    parts["union"] = entry(t, all_t, note="the x << 1 forest, vfn_orient_union_runs and one status read")
    shared = zero()
    t, all_t, _ = timed(lambda: [lib.orient_union_runs(keys, nodes, dirs, forest(), info=shared) for _ in range(BURST)], args.reps)
    parts["union"]["kernel_only"] = entry(t / BURST, [x / BURST for x in all_t], note=f"{BURST} launches in a row (each with its fresh forest), no read: seconds per launch")
    t, all_t, _ = timed(lambda: [forest() for _ in range(BURST)], args.reps)
    parts["union"]["forest_only"] = entry(t / BURST, [x / BURST for x in all_t], note="torch.arange(0, 2m, 2, int32) alone, the same way")
    t, all_t, (root, parity) = timed(lambda: lib.orient_flatten(words), args.reps)
    parts["flatten"] = entry(t, all_t, note="vfn_orient_flatten and one status read; 4 B read, 9 B written a node, chains on top")
    t, all_t, _ = timed(lambda: [lib.orient_flatten(words, info=shared) for _ in range(BURST)], args.reps)
    parts["flatten"]["kernel_only"] = entry(t / BURST, [x / BURST for x in all_t], note=f"{BURST} launches in a row, no read")

    def numbering():
        return torch.unique(root, return_inverse=True, return_counts=True)

    t, all_t, (first_face, face_label, face_count) = timed(numbering, args.reps)
    k = int(first_face.shape[0])
    parts["numbering"] = entry(t, all_t, K=k, note="torch.unique(root, return_inverse=True, return_counts=True): the numbering, the counts, the read for K")

    def conflicts():
        manifold, want = meshops.manifold_mask(keys, nodes, dirs)
        a, b = nodes[:-1], nodes[1:]
        wrong = manifold & (((parity[a] ^ parity[b]) != 0) != want)
        return meshops._count_by_label(face_label[a], wrong, k) == 0, (manifold & want).sum()

    t, all_t, (orientable, _) = timed(conflicts, args.reps)
    t2, all_t2, _ = timed(lambda: meshops._count_by_label(face_label, parity, k), args.reps)
    parts["count_by_label"] = entry(t2, all_t2, note="one exact per-component count (scatter_add of int64 flags; used for the majority and for flipped_count)")
    parts["conflicts"] = entry(t, all_t, note="the manifold mask over all adjacent items, the test of every pair, the count per component: torch, nothing compacted, no host read")
    for mode, name, views in ((lib.ORIENT_VOLUME, "votes_volume", None), (lib.ORIENT_VIEWPOINTS, "votes_viewpoints", eyes)):
        t, all_t, per_face = timed(lambda: lib.orient_votes(verts, faces, parity, mode, views), args.reps)
        parts[name] = entry(t, all_t, note="vfn_orient_votes and one status read" + ("" if views is None else f"; every lane walks {args.views} viewpoints"))
        t, all_t, _ = timed(lambda: [lib.orient_votes(verts, faces, parity, mode, views, info=shared) for _ in range(BURST)], args.reps)
        parts[name]["kernel_only"] = entry(t / BURST, [x / BURST for x in all_t], note=f"{BURST} launches in a row, no read")

    def vote_sums():
        order = torch.sort(face_label, stable=True)[1]
        start = torch.cat((torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(face_count, dim=0))).contiguous()
        return lib.cc_segment_sums(per_face[order].contiguous(), start)

    t, all_t, sums = timed(vote_sums, args.reps)
    parts["vote_sums"] = entry(t, all_t, note="torch.sort(face_label, stable=True), the gather, the cumsum, vfn_cc_segment_sums and one status read")
    flip = (parity != 0) ^ ((sums < 0) & orientable)[face_label]
    t, all_t, _ = timed(lambda: meshops._rewind(faces, flip), args.reps)
    parts["swap"] = entry(t, all_t, note="the column swap of the flipped faces: torch.where and torch.stack")
    result["parts"] = parts
    print(json.dumps({"parts": parts}), flush=True)

    # the yardstick: the components' union-find on the same mesh, in the same process
    t, all_t, c = timed(lambda: meshops.connected_components((verts, faces), connectivity="edge", areas=False), args.reps)
    yard = {"connected_components_edge_without_areas": entry(t, all_t, K=c.n_components)}
    ck, cn = meshops.component_items(faces, n, "edge")
    identity = lambda: torch.arange(m, dtype=torch.int32, device=dev)                     # noqa: E731
    t, all_t, _ = timed(lambda: lib.cc_union_runs(ck, cn, identity()), args.reps)
    yard["cc_union"] = entry(t, all_t, note="the identity forest, vfn_cc_union_runs and one status read")
    t, all_t, _ = timed(lambda: [lib.cc_union_runs(ck, cn, identity(), info=shared) for _ in range(BURST)], args.reps)
    yard["cc_union"]["kernel_only"] = entry(t / BURST, [x / BURST for x in all_t], note=f"{BURST} launches in a row, no read")
    yard["orient_union_over_cc_union_kernel_only"] = round(parts["union"]["kernel_only"]["seconds"] / yard["cc_union"]["kernel_only"]["seconds"], 3)
    yard["orient_first_over_components"] = round(result["orient"]["first"]["seconds"] / yard["connected_components_edge_without_areas"]["seconds"], 3)
    result["yardstick"] = yard
    print(json.dumps({"yardstick": yard}), flush=True)

    if not args.no_host:
        _, _, o = meshops.orient((verts, faces), reference="first")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fh = faces.cpu().numpy()
        t1 = time.perf_counter()
        host_root, host_parity, host_conflict = OR.parity_colouring(fh, n)
        t2 = time.perf_counter()
        up = torch.from_numpy(host_parity).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        td = result["orient"]["first"]["seconds"]
        result["host"] = {"download_s": round(t1 - t0, 4), "two_colouring_s": round(t2 - t1, 4), "upload_s": round(t3 - t2, 4), "total_s": round(t3 - t0, 4),
                          "device_orient_first_s": td, "ratio": round((t3 - t0) / td, 1),
                          "same_flips": bool(not host_conflict.any() and torch.equal(up != 0, o.flip)),
                          "note": "the breadth-first restatement of tests/orient_restatement.py: pure Python on the host clock, one thread; parities alone"}
        print(json.dumps({"host": result["host"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
