#!/usr/bin/env python3
"""Device time of the image scores (vf_nerf_amd.metrics2d, csrc/vfn_image.hip) on --views views of 680 x 1200 x 3 resident on the device
(byte predictions, float32 targets: what evaluator.metrics scores), seeded random content:

    one_call            all views in one vfn_image_scores call            (PSNR + SSIM, and PSNR only)
    view_by_view        one call per view, back to back on one stream      (PSNR + SSIM, and PSNR only)
    public_one_call     metrics2d.image_scores on the resident tensors: the launches plus its one read-back and the Python around them
    quantize            vfn_image_quantize8 over all views of a float32 prediction
    restatement_cpu     tests/metrics2d_restatement.py on ONE view, host clock (what the same arithmetic costs in NumPy)

HIP events around each variant, three warm-up calls, --reps timed calls, the median reported (all repeats are listed).  Beside each time
stands the roofline of DESIGN 6m, computed here from the shapes: bytes over the measured copy bandwidth, fp64 operations over the
published fp64 vector rate counted without FMA (the unit is compiled without contraction), and the achieved share of the larger.

    python tools/bench_metrics2d.py [--views 100] [--reps 20] [--out profiles/r12/bench_metrics2d.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

H, W, C = 680, 1200, 3
HBM_BYTES_PER_S = 6.29e12          # measured float4 copy
FP64_OPS_PER_S = 39.3e12           # the published 78.6 TFLOP/s counts an FMA as two
# per element, from the kernel's loops (16 x 16 tile, 26 x 26 staged): horizontal 26 x 16 sites / 256 lanes x (11 x 3 products +
# 10 x 5 additions), vertical 5 x 10 additions, the formula 16, the squared difference 2, the sums 3; a division counted as ONE operation
OPS_SSIM = (26 * 16 / 256) * (11 * 3 + 10 * 5) + 5 * 10 + 16 + 2 + 3
DIVS_SSIM = 6
OPS_PSNR = 2 + 3
BYTES = 1 + 4                      # a byte of the prediction, a float32 of the target: each read from HBM once (the halo comes from L2)


WARMUP = 3


def timed(fn, reps):
    import torch
    for _ in range(WARMUP):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 1e3)
    return statistics.median(times), times, out


def roofline(elements, ssim):
    ops = (OPS_SSIM + DIVS_SSIM) if ssim else OPS_PSNR
    t_ops, t_bytes = elements * ops / FP64_OPS_PER_S, elements * BYTES / HBM_BYTES_PER_S
    return {"fp64_operations_per_element": round(ops, 2), "bytes_per_element": BYTES, "seconds_fp64": t_ops, "seconds_bytes": t_bytes,
            "binds": "fp64" if t_ops > t_bytes else "bytes", "seconds": max(t_ops, t_bytes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics2d: no GPU visible (nothing here can be measured on a CPU)")
    from vf_nerf_amd import lib, metrics2d
    import metrics2d_restatement as R
    dev = torch.device("cuda:0")
    v = args.views
    g = torch.Generator(device=dev)
    g.manual_seed(12)
    target = torch.rand(v, H, W, C, device=dev, generator=g)
    pred_f = (target + 0.05 * torch.randn(v, H, W, C, device=dev, generator=g)).clamp_(0.0, 1.0)
    info = torch.zeros(1, dtype=torch.int64, device=dev)
    pred = lib.image_quantize8(pred_f, info)
    elements = v * H * W * C
    result = {"views": v, "height": H, "width": W, "channels": C, "reps": args.reps, "device": torch.cuda.get_device_name(0),
              "timing": f"HIP events, {WARMUP} warm-up calls, median of reps", "tile": lib.image_tile()}

    def put(name, res, ssim=None):
        t, all_t, out = res
        result[name] = {"seconds": round(t, 6), "all_seconds": [round(x, 6) for x in all_t], "views_per_second": round(v / t, 1)}
        if ssim is not None:
            roof = roofline(elements, ssim)
            result[name]["roofline"] = roof
            result[name]["share_of_roofline"] = round(roof["seconds"] / t, 4)
        return out

    one = put("one_call_psnr_ssim", timed(lambda: lib.image_scores(pred, target, True, info), args.reps), True)
    one_p = put("one_call_psnr", timed(lambda: lib.image_scores(pred, target, False, info), args.reps), False)
    by = put("view_by_view_psnr_ssim", timed(lambda: torch.cat([lib.image_scores(pred[i:i + 1], target[i:i + 1], True, info) for i in range(v)]),
                                             args.reps), True)
    put("view_by_view_psnr", timed(lambda: torch.cat([lib.image_scores(pred[i:i + 1], target[i:i + 1], False, info) for i in range(v)]),
                                   args.reps), False)
    scores = put("public_one_call_psnr_ssim", timed(lambda: metrics2d.image_scores(pred, target), args.reps))
    put("quantize", timed(lambda: lib.image_quantize8(pred_f, info), args.reps))
    result["one_call_equals_view_by_view_bits"] = bool(torch.equal(one.view(torch.int64), by.view(torch.int64)))
    result["psnr_sums_equal_with_and_without_ssim"] = bool(torch.equal(one[:, 0].view(torch.int64), one_p[:, 0].view(torch.int64)))
    result["info"] = int(info.cpu())
    result["mean_psnr"] = sum(s["psnr"] for s in scores) / v
    result["mean_ssim"] = sum(s["ssim"] for s in scores) / v
    p0, t0 = pred[0].cpu().numpy(), target[0].cpu().numpy()
    start = time.perf_counter()
    want = R.scores_sums(p0[None], t0[None])
    result["restatement_cpu_one_view"] = {"seconds": round(time.perf_counter() - start, 3), "clock": "host, one run"}
    result["view_0_equals_restatement_bits"] = bool(np.array_equal(one[0].cpu().numpy().view(np.uint64), want[0].view(np.uint64)))
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
