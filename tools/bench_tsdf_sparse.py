#!/usr/bin/env python3
"""Device time and memory of the block-sparse TSDF volume (tsdf.SparseTSDFVolume, csrc/vfn_tsdf.hip: vfn_tsdf_sparse_*) against the dense
one, on the scene of tools/bench_tsdf.py — the room [-0.6, 0.6]^3 seen from --views (100) cameras inside it, analytic depth maps of
--height x --width (680 x 1200), pattern images — in ONE process:

    (a) the --res^3 lattice (512) over the box [-0.7, 0.7]^3:
          dense    integrate and extract, without and with colour (the rows of bench_tsdf.py --colour);
          sparse   mark (vfn_tsdf_sparse_mark alone), allocate (mark + the torch plumbing that numbers the blocks and grows the arrays;
                   table_update = allocate - mark), integrate and extract, without and with colour; blocks opened and memory_bytes
                   against the dense bytes; whether the meshes are the same triangles.
    (b) the same box at --fine-res^3 (2048), which the dense volume refuses: the sparse rows alone.

The truncation is 5.12 voxels in both (the reference's 0.04 m at 4 / 512 m voxels).  HIP events around each call; one warm-up round, then
--reps rounds of all calls in the same order; the voxel arrays are zeroed before every integration (untimed); median, all repeats.

    python tools/bench_tsdf_sparse.py [--res 512] [--fine-res 2048] [--reps 3] [--out profiles/r17/bench_tsdf_sparse.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_tsdf import event_time, room_depths, room_views  # noqa: E402

ORIGIN = (-0.7, -0.7, -0.7)


def rounds(calls, reps):
    """calls = {name: (fn, before)} -> ({name: row}, {name: last result}); round 0 is the warm-up."""
    times, last = {name: [] for name in calls}, {}
    for rep in range(reps + 1):
        for name, (fn, before) in calls.items():
            t, out = event_time(fn, before)
            if rep:
                times[name].append(t)
            last[name] = out
    rows = {name: {"seconds": round(statistics.median(ts), 6), "all_seconds": [round(x, 6) for x in ts],
                   "spread": round((max(ts) - min(ts)) / statistics.median(ts), 4)} for name, ts in times.items()}
    return rows, last


def triangle_keys(mesh):
    """The triangles of a mesh as sorted rows of vertex bits (the numbering drops out), on the device."""
    v, f = mesh[:2]
    rows = v.view(torch.int64)[f].reshape(f.shape[0], 9)
    return torch.unique(rows, dim=0)


def sparse_rows(tsdf, lib, res, vl, trunc, depths, rgb, k, e, reps, dev):
    dims = (res, res, res)
    out = {}
    meshes = {}
    for colour in (False, True):
        vol = tsdf.SparseTSDFVolume(ORIGIN, dims, voxel_length=vl, sdf_trunc=trunc, device=dev, colour=colour)
        cams = tsdf.mark_cameras(k.cpu(), e.cpu()).to(dev)
        marks = torch.zeros(vol.block_dims, dtype=torch.uint8, device=dev)

        def zero():
            vol.tsdf.zero_()
            vol.weight.zero_()
            if colour:
                vol.colour.zero_()

        def allocate():
            vol.reset()
            return vol._allocate(depths, k.cpu(), e.cpu())

        calls = {"mark": (lambda: lib.tsdf_sparse_mark(marks, vol.origin, vol.voxel_length, vol.sdf_trunc, depths, cams), marks.zero_),
                 "allocate": (allocate, None),
                 "integrate": (lambda: lib.tsdf_sparse_integrate(vol.tsdf, vol.weight, vol.colour, vol.block_coords, vol.dims, vol.origin,
                                                                 vol.voxel_length, vol.sdf_trunc, depths, rgb if colour else None, k, e), zero),
                 "extract": (vol.extract_coloured_mesh if colour else vol.extract_mesh, None)}
        rows, last = rounds(calls, reps)
        rows["table_update"] = {"seconds": round(rows["allocate"]["seconds"] - rows["mark"]["seconds"], 6),
                                "note": "allocate - mark: zeroed marks, nonzero (one host read), the table scatter and the torch.cat of the arrays"}
        rows["total_seconds"] = round(rows["allocate"]["seconds"] + rows["integrate"]["seconds"] + rows["extract"]["seconds"], 6)
        rows.update({"blocks": vol.n_blocks, "block_lattice": int(vol.block_of.numel()), "memory_bytes": vol.memory_bytes,
                     "voxels_held": vol.n_blocks * 512, "observed_voxels": int((vol.weight > 0).sum()),
                     "mark_bytes_per_pixel_at_1.2_m": round(float((2 * (trunc + 0.5 * (1.2 + trunc) * float(cams[0, 16]) + 2 * vl) / (8 * vl) + 1) ** 3), 1),
                     "vertices": int(last["extract"][0].shape[0]), "faces": int(last["extract"][1].shape[0])})
        out["colour" if colour else "plain"] = rows
        meshes[colour] = last["extract"]
        del vol, marks, last
        torch.cuda.empty_cache()
    return out, meshes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--fine-res", type=int, default=2048)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_sparse: no GPU visible (nothing here can be measured on a CPU)")
    import tsdf_colour_restatement as C
    import tsdf_restatement as R
    from vf_nerf_amd import lib, tsdf
    dev = torch.device("cuda:0")
    nv, h, w = args.views, args.height, args.width
    poses = room_views(nv)
    k4 = R.pinhole(h, w, 0.6 * w)
    depths = room_depths(poses, k4, h, w, dev)
    k = torch.from_numpy(np.tile(k4, (nv, 1))).to(dev)
    e = tsdf.extrinsics_from_poses(poses, nv).to(dev)
    rgb = torch.from_numpy(C.pattern_images(nv, h, w)).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "views": nv, "map": [h, w], "reps": args.reps,
              "timing": "HIP events per call; one warm-up round, then --reps rounds of all calls of a volume in the same order, in one process; "
                        "voxel arrays zeroed before every integration (untimed); median, all repeats, (max - min) / median"}

    # (a) the lattice both volumes can hold
    res = args.res
    vl = 1.4 / res
    trunc = 5.12 * vl
    dims = (res, res, res)
    dense = {}
    dense_meshes = {}
    for colour in (False, True):
        vol = tsdf.TSDFVolume(ORIGIN, dims, voxel_length=vl, sdf_trunc=trunc, device=dev, colour=colour)
        box = (vol.origin, vol.voxel_length, vol.sdf_trunc)
        integrate = (lambda: lib.tsdf_integrate_rgb(vol.tsdf, vol.weight, vol.colour, *box, depths, rgb, k, e)) if colour else \
            (lambda: lib.tsdf_integrate(vol.tsdf, vol.weight, *box, depths, k, e))
        rows, last = rounds({"integrate": (integrate, vol.reset), "extract": (vol.extract_coloured_mesh if colour else vol.extract_mesh, None)},
                            args.reps)
        rows["total_seconds"] = round(rows["integrate"]["seconds"] + rows["extract"]["seconds"], 6)
        rows.update({"memory_bytes": res ** 3 * (20 if colour else 8), "observed_voxels": int((vol.weight > 0).sum()),
                     "vertices": int(last["extract"][0].shape[0]), "faces": int(last["extract"][1].shape[0])})
        dense["colour" if colour else "plain"] = rows
        dense_meshes[colour] = last["extract"]
        del vol, last
        torch.cuda.empty_cache()
    sparse, sparse_meshes = sparse_rows(tsdf, lib, res, vl, trunc, depths, rgb, k, e, args.reps, dev)
    same = {name: bool(torch.equal(triangle_keys(dense_meshes[c]), triangle_keys(sparse_meshes[c]))) for name, c in (("plain", False), ("colour", True))}
    result["a"] = {"res": res, "voxel_length": vl, "sdf_trunc": trunc, "dense": dense, "sparse": sparse, "same_triangles_as_dense": same,
                   "sparse_over_dense_seconds": {n: round(sparse[n]["total_seconds"] / dense[n]["total_seconds"], 3) for n in ("plain", "colour")},
                   "sparse_over_dense_bytes": {n: round(sparse[n]["memory_bytes"] / dense[n]["memory_bytes"], 4) for n in ("plain", "colour")}}
    print(json.dumps({"a": result["a"]}), flush=True)
    del dense_meshes, sparse_meshes
    torch.cuda.empty_cache()

    # (b) the same box, finer: beyond the dense volume
    res = args.fine_res
    vl = 1.4 / res
    trunc = 5.12 * vl
    try:
        tsdf.TSDFVolume(ORIGIN, (res, res, res), voxel_length=vl, sdf_trunc=trunc, device=dev)
        refused = None
    except ValueError as err:
        refused = str(err)
    sparse, _ = sparse_rows(tsdf, lib, res, vl, trunc, depths, rgb, k, e, args.reps, dev)
    result["b"] = {"res": res, "voxel_length": vl, "sdf_trunc": trunc, "dense_refusal": refused, "sparse": sparse,
                   "dense_bytes_if_it_existed": {"plain": res ** 3 * 8, "colour": res ** 3 * 20}}
    print(json.dumps({"b": result["b"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
