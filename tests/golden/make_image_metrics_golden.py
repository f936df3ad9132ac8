#!/usr/bin/env python3
"""Golden vectors for the image scores by running the REFERENCE's own functions: utils/utils.py get_psnr (:235-245), get_ssim (:248-289)
and get_l1_cm (:312-325), twice — in float32 as shipped (what evaluation/methods.py feeds them: load_rgb's byte / 255 as float32 against
a float32 target) and with ``torch.set_default_dtype(torch.float64)`` on float64 inputs (the same formulas, the window included, in
double).  Build container only (needs /root/reference, read-only); the fixture holds inputs and recorded outputs, nothing of the
reference's source.

utils/utils.py imports cv2, imageio, open3d, skimage, lpips, trimesh and torchvision at module level for functions these three do not
call; whichever is not installed is stubbed in ``sys.modules`` for the run.

    python tests/golden/make_image_metrics_golden.py            # writes tests/golden/image_metrics.npz

Predictions are bytes (what a PNG holds), targets lie on a 1/1024 lattice and depths on a 1/256 lattice, so that the file compresses.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")


class _Stub(types.ModuleType):
    """A module whose every attribute exists: annotations such as ``trimesh.Trimesh`` and ``o3d.geometry.TriangleMesh`` resolve."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub(f"{self.__name__}.{name}")


for _name in ("cv2", "imageio", "open3d", "skimage", "lpips", "trimesh", "torchvision", "torchvision.transforms"):
    try:
        importlib.import_module(_name)
    except Exception:
        sys.modules[_name] = _Stub(_name)
from utils import utils  # noqa: E402


def lattice(x, steps):
    return (np.round(np.clip(x, 0.0, 1.0) * steps) / steps).astype(np.float32)


def noise_case(h, w, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (h, w, 3), dtype=np.uint8), lattice(g.random((h, w, 3)), 1024)


def smooth_case(h, w, seed):
    g = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w]
    base = np.stack([0.5 + 0.4 * np.sin(x / 9.0) * np.cos(y / 13.0), 0.3 + 0.3 * (x / w) + 0.2 * (y / h),
                     0.5 + 0.45 * np.cos((x + 2 * y) / 17.0)], axis=-1)
    target = lattice(base, 1024)
    pred = np.clip(np.trunc((base + 0.02 * g.standard_normal(base.shape)).clip(0, 1) * 255), 0, 255).astype(np.uint8)
    return pred, target


def cases():
    out = {"noise_1x1": noise_case(1, 1, 1), "noise_7x5": noise_case(7, 5, 2), "noise_5x40": noise_case(5, 40, 3),
           "noise_11x11": noise_case(11, 11, 4), "noise_33x47": noise_case(33, 47, 5), "smooth_120x160": smooth_case(120, 160, 6)}
    g = np.random.default_rng(7)
    out["const_target_120x160"] = (g.integers(0, 256, (120, 160, 3), dtype=np.uint8), np.full((120, 160, 3), 0.5, dtype=np.float32))
    pred, _ = smooth_case(40, 56, 8)
    out["equal_40x56"] = (pred, None)                      # the target IS the prediction (byte / 255): recorded as a uint8 target
    return out


def depth_pair(h, w, seed):
    g = np.random.default_rng(seed)
    target = (np.round((1.0 + 3.0 * g.random((h, w))) * 256) / 256).astype(np.float32)
    pred = (np.round((target + 0.05 * g.standard_normal((h, w))) * 256) / 256).astype(np.float32)
    return pred, target


def run(pred, target, pred_depth, target_depth, dtype):
    """The three functions on tensors of ``dtype`` with that default dtype (get_ssim builds its window with torch.ones)."""
    torch.set_default_dtype(dtype)
    try:
        p, t = torch.from_numpy(pred).to(dtype), torch.from_numpy(target).to(dtype)
        return (utils.get_psnr(p, t), utils.get_ssim(p, t),
                utils.get_l1_cm(torch.from_numpy(pred_depth).to(dtype), torch.from_numpy(target_depth).to(dtype)))
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    out = {}
    names = []
    for i, (name, (pred_u8, target)) in enumerate(cases().items()):
        h, w = pred_u8.shape[:2]
        pd, td = depth_pair(h, w, 100 + i)
        # float32 as shipped: load_rgb hands byte / 255 over as float32; float64: the same byte / 255 in double
        pred32 = pred_u8.astype(np.float32) / np.float32(255.0)
        pred64 = pred_u8.astype(np.float64) / 255.0
        t32 = pred32 if target is None else target
        t64 = pred64 if target is None else target.astype(np.float64)
        r32 = run(pred32, t32, pd, td, torch.float32)
        r64 = run(pred64, t64, pd.astype(np.float64), td.astype(np.float64), torch.float64)
        names.append(name)
        out[f"{name}/pred_u8"] = pred_u8
        if target is not None:
            out[f"{name}/target"] = target
        out[f"{name}/pred_depth"], out[f"{name}/target_depth"] = pd, td
        out[f"{name}/ref32"] = np.array(r32, dtype=np.float64)          # psnr, ssim, l1_cm
        out[f"{name}/ref64"] = np.array(r64, dtype=np.float64)
        print(f"{name:24s} ref32 {r32}  ref64 {r64}")
    out["names"] = np.array(names)
    path = os.path.join(HERE, "image_metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
