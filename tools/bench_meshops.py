#!/usr/bin/env python3
"""Device time of the mesh normals unit (vf_nerf_amd.meshops, csrc/vfn_normals.hip) and of normal consistency (vf_nerf_amd.metrics3d) on the
mesh tools/bench_refuse.py builds: the room scene fused at --res^3 (512) from --views (100) analytic depth maps of --height x --width
(680 x 1200).  Recorded:

    vertex_faces       the incidence CSR (torch: unique of the keys vertex * m + face).
    face_normals       vfn_face_normals, unit normals; algorithmic bytes 120 per face (24 of indices, 72 of vertex rows, 24 written).
    vertex_normals     the public call (raw face normals + CSR + vfn_vertex_normals + one status read) and the kernel alone; algorithmic
                       bytes per vertex 16 (row bounds) + 32 per incident face (8 of index, 24 of normal) + 24 written.
    weld               meshops.weld(digits=8) of the mesh with its vertices duplicated per face (3 m vertices).
    score_mesh         metrics3d.score_mesh against a shifted copy at --samples (10^6): normals=True against normals=False with
                       search="grid" (the same two searches), alternating, and vfn_normal_dots alone (64 bytes per sample).
    cpu                the NumPy restatement (tests/meshops_restatement.py) on the host, host clock, the only baseline there is: the mesh of a
                       --cpu-res^3 (128) volume for the normals, the CSR and the weld, with the device's time at the same size beside it
                       and the bits compared; normal consistency at --samples from the device's samples and neighbour indices.

The share of HBM rate is the algorithmic bytes over the kernel's time over the copy rate the microarchitecture notes give (6.29 TB/s): a
lower bound on what the kernel moves, since a 24-byte row touches more than 24 bytes of a line when its neighbours are not read with it.
HIP events around each call, one warm-up call, --reps timed calls, the median reported (all repeats are listed).

    python tools/bench_meshops.py [--res 512] [--views 100] [--reps 5] [--samples 1000000] [--out profiles/r16/bench_meshops.json]
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


def with_rate(t, all_t, nbytes):
    return dict(rounded(t, all_t), algorithmic_bytes=int(nbytes), bytes_per_s=round(nbytes / t, 1), share_of_hbm_copy_rate=round(nbytes / t / HBM_COPY_RATE, 4))


def host_clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def same_bits(dev_tensor, array):
    return bool(np.array_equal(dev_tensor.cpu().numpy().view(np.int64), np.ascontiguousarray(array).view(np.int64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--height", type=int, default=680)
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--cpu-res", type=int, default=128)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshops: no GPU visible (nothing here can be measured on a CPU)")
    import meshops_restatement as M
    import tsdf_restatement as R
    from vf_nerf_amd import lib, meshops, metrics3d
    dev = torch.device("cuda:0")
    h, w = args.height, args.width
    poses = room_views(args.views)
    k4 = R.pinhole(h, w, 0.6 * w)
    (verts, faces), _, vl, _ = fused_room(args.res, poses, k4, h, w, dev)
    n, m = int(verts.shape[0]), int(faces.shape[0])
    result = {"device": torch.cuda.get_device_name(0), "res": args.res, "views": args.views, "map": [h, w], "vertices": n, "faces": m,
              "reps": args.reps, "hbm_copy_rate_bytes_per_s": HBM_COPY_RATE,
              "timing": "HIP events, one warm-up call, median of reps; host reads inside a call are part of it"}
    print(json.dumps({"mesh": [n, m]}), flush=True)

    t, all_t, (row_start, incident) = timed(lambda: meshops.vertex_faces(faces, n), args.reps)
    nnz = int(incident.shape[0])
    result["vertex_faces"] = dict(rounded(t, all_t), incident=nnz, faces_per_vertex=round(nnz / n, 3), note="torch plumbing; includes the host's range check of the indices")
    print(json.dumps({"vertex_faces": result["vertex_faces"]}), flush=True)

    t, all_t, _ = timed(lambda: lib.face_normals(verts, faces, True), args.reps)
    result["face_normals"] = dict(with_rate(t, all_t, 120 * m), faces_per_s=round(m / t, 1), note="vfn_face_normals and one status read")
    t, all_t, _ = timed(lambda: meshops.face_normals((verts, faces)), args.reps)
    result["face_normals"]["public_call"] = rounded(t, all_t)
    print(json.dumps({"face_normals": result["face_normals"]}), flush=True)

    raw = lib.face_normals(verts, faces, False)
    t, all_t, _ = timed(lambda: lib.vertex_normals(raw, row_start, incident), args.reps)
    result["vertex_normals"] = {"kernel_only": dict(with_rate(t, all_t, 40 * n + 32 * nnz), vertices_per_s=round(n / t, 1),
                                                    note="vfn_vertex_normals and one status read")}
    t, all_t, _ = timed(lambda: meshops.vertex_normals((verts, faces)), args.reps)
    result["vertex_normals"].update(rounded(t, all_t), note="the public call: raw face normals, the CSR, the kernel, one status read")
    print(json.dumps({"vertex_normals": result["vertex_normals"]}), flush=True)
    del raw, row_start, incident

    soup_v = verts[faces.reshape(-1)].contiguous()
    soup_f = torch.arange(3 * m, dtype=torch.int64, device=dev).reshape(m, 3)
    t, all_t, welded = timed(lambda: meshops.weld((soup_v, soup_f), digits=8), args.reps)
    result["weld"] = dict(rounded(t, all_t), vertices_in=3 * m, vertices_out=int(welded[0].shape[0]), vertices_in_per_s=round(3 * m / t, 1),
                          recovers_the_indexed_mesh=bool(welded[0].shape[0] == n and torch.equal(welded[0][welded[1]], verts[faces])))
    print(json.dumps({"weld": result["weld"]}), flush=True)
    del soup_v, soup_f, welded

    other = (verts * 1.002 + 0.5 * vl, faces)
    u = torch.rand(args.samples, 3, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(16))
    score = lambda **kw: metrics3d.score_mesh((verts, faces), other, num_points=args.samples, distance_thresh=0.01, uniforms=u, **kw)      # noqa: E731
    score(normals=True)
    score(search="grid")
    torch.cuda.synchronize()
    with_n, without = [], []
    for _ in range(args.reps):                                   # alternating: the two share whatever else the machine is doing
        tn, _, entry = timed(lambda: score(normals=True), 1)
        tp, _, plain = timed(lambda: score(search="grid"), 1)
        with_n.append(tn)
        without.append(tp)
    med = lambda x: float(np.median(x))                          # noqa: E731
    result["score_mesh"] = {"samples": args.samples, "normals": rounded(med(with_n), with_n), "grid_without_normals": rounded(med(without), without),
                            "added_seconds": round(med(with_n) - med(without), 6), "normal_consistency": entry["normal consistency"],
                            "other_keys_equal": bool({k: v for k, v in entry.items() if k != "normal consistency"} == plain),
                            "note": "each timing is the second of two calls (timed()'s warm-up, then the timed one)"}
    pp, pf = metrics3d.sample_surface(verts, faces, args.samples, uniforms=u)
    rp, rf = metrics3d.sample_surface(*other, args.samples, uniforms=u)
    pn, rn = meshops.face_normals((verts, faces))[pf].contiguous(), meshops.face_normals(other)[rf].contiguous()
    to_ref, to_pred = metrics3d.nearest(pp, rp)[0], metrics3d.nearest(rp, pp)[0]
    t, all_t, _ = timed(lambda: lib.normal_dots(pn, rn, to_ref), args.reps)
    result["score_mesh"]["normal_dots"] = dict(with_rate(t, all_t, 64 * args.samples), note="vfn_normal_dots and one status read")
    print(json.dumps({"score_mesh": result["score_mesh"]}), flush=True)

    if not args.no_cpu:
        secs, want = host_clock(lambda: M.normal_consistency(pn.cpu().numpy(), rn.cpu().numpy(), to_ref.cpu().numpy(), to_pred.cpu().numpy()))
        cpu = {"normal_consistency": {"samples": args.samples, "seconds": round(secs, 3), "equals_device": bool(want == entry["normal consistency"]),
                                      "what": "the dots and the fixed tree in NumPy from the device's normals and neighbour indices (no search)"}}
        ch, cw = h // 4, w // 4
        (cv, cf), _, _, _ = fused_room(args.cpu_res, poses, R.pinhole(ch, cw, 0.6 * cw), ch, cw, dev)
        hv, hf = cv.cpu().numpy(), cf.cpu().numpy()
        cpu.update(res=args.cpu_res, vertices=int(hv.shape[0]), faces=int(hf.shape[0]), what="tests/meshops_restatement.py (NumPy, Python loops for the ordered sums), one thread, host clock")
        for name, host_fn, dev_fn, same in (
                ("vertex_faces", lambda: M.csr(M.vertex_faces(hf, hv.shape[0])), lambda: meshops.vertex_faces(cf, hv.shape[0]),
                 lambda a, b: bool(np.array_equal(a[0].cpu().numpy(), b[0]) and np.array_equal(a[1].cpu().numpy(), b[1]))),
                ("face_normals", lambda: M.face_normals(hv, hf, True), lambda: meshops.face_normals((cv, cf)), same_bits),
                ("vertex_normals", lambda: M.vertex_normals(hv, hf), lambda: meshops.vertex_normals((cv, cf)), same_bits),
                ("weld", lambda: M.weld(hv[hf.reshape(-1)], np.arange(hf.size).reshape(-1, 3), 8),
                 lambda: meshops.weld((cv[cf.reshape(-1)].contiguous(), torch.arange(cf.numel(), device=dev).reshape(-1, 3)), digits=8),
                 lambda a, b: bool(same_bits(a[0], b[0]) and np.array_equal(a[1].cpu().numpy(), b[1])))):
            secs, want = host_clock(host_fn)
            t, all_t, got = timed(dev_fn, args.reps)
            cpu[name] = {"seconds": round(secs, 3), "device_same_size": rounded(t, all_t), "device_bits_equal": same(got, want)}
            print(json.dumps({"cpu " + name: cpu[name]}), flush=True)
        result["cpu"] = cpu
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
