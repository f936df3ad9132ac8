"""Scoring rendered views on the device (csrc/vfn_image.hip): the image scores of evaluation/methods.py:549-610 (``metrics``) —
``utils.get_psnr`` (utils/utils.py:235-245), ``utils.get_ssim`` (:248-289), ``utils.get_l1_cm`` (:312-325) — and the byte quantisation of
the ``save_rgb`` -> PNG -> ``load_rgb`` round trip (:73-108), without copying an image to the host.

* ``quantize_rgb8`` — ``(image * 255).astype(uint8)`` as ``save_rgb`` writes it; a value that cast is undefined for is refused.
* ``image_scores`` — PSNR, SSIM and the depth L1 (in cm) of one view or of ``V`` views of one size in one launch.
* ``score_views`` — the reference's ``metrics.json`` dictionary for any number of views; views of one size go in one launch.

The arithmetic is a float64 specification of the reference's formulas (include/vfn.h, restated in tests/metrics2d_restatement.py): the
reference evaluates them in float32.  Inputs are numpy arrays or torch tensors on any device.  No CPU fallback: ``lib.VfnError`` when no
device is visible.

Out of scope: LPIPS, depth validity masks (the reference has none), a Gaussian SSIM window (the reference's is the 11 x 11 box), PNG
encoding and decoding.
"""
from __future__ import annotations

import functools
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import geomargs, lib
from .geomargs import LIMIT

_device = functools.partial(geomargs.device, what="image scoring")       # (a module attribute, so a test can stand in for the device)

SIDE_LIMIT = 1 << 15         # H, W of one view (include/vfn.h)
L1_SCALE_CM = 100.0          # get_l1_cm: metres -> centimetres


def _check_images(x, name: str, dtypes, channels) -> torch.Tensor:
    """[H,W,C] or [V,H,W,C] with C in ``channels`` and a dtype in ``dtypes`` -> the tensor as given (any device).  Host checks only."""
    t = geomargs.as_tensor(x, name)
    if t.dim() not in (3, 4):
        raise ValueError(f"{name} must be [H,W,C] or [V,H,W,C], got {tuple(t.shape)}")
    if t.dtype not in dtypes:
        raise ValueError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if t.shape[-1] not in channels:
        raise ValueError(f"{name} must have {' or '.join(str(c) for c in channels)} channels, got {tuple(t.shape)}")
    if min(t.shape) < 1:
        raise ValueError(f"{name} is empty: {tuple(t.shape)}")
    h, w = t.shape[-3], t.shape[-2]
    if h >= SIDE_LIMIT or w >= SIDE_LIMIT:
        raise ValueError(f"{name}: {h} x {w} pixels exceed the 2^15 limit per side")
    if math.prod(t.shape) >= LIMIT:
        raise ValueError(f"{name}: {math.prod(t.shape)} values exceed the 2^31 limit of one call")
    return t


def _check_flag(x, name: str) -> bool:
    if not isinstance(x, (bool, np.bool_)):
        raise ValueError(f"{name} must be a bool, got {x!r}")
    return bool(x)


def _check_depth(x, name: str, views_shape) -> torch.Tensor:
    """A depth map per view: [H,W] / [H,W,1] for one view, [V,H,W] / [V,H,W,1] for V -> [V,H,W] (a view of the input)."""
    t = geomargs.as_tensor(x, name)
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be torch.float32, got {t.dtype}")
    want = tuple(views_shape[:3])
    if tuple(t.shape) in (want[1:], want[1:] + (1,), want, want + (1,)):
        return t.reshape(want)
    raise ValueError(f"{name} must be [H,W], [H,W,1], [V,H,W] or [V,H,W,1] matching the images' {want}, got {tuple(t.shape)}")


def _raise_on(status: int, what: str) -> None:
    if status & lib.GEOM_STATUS_NONFINITE:
        raise lib.VfnError(f"{what}: a non-finite value")
    if status & lib.IMAGE_STATUS_RANGE:
        raise lib.VfnError(f"{what}: a value below 0 or at least 256/255 — the cast to a byte is undefined there (clip the image first)")


def quantize_rgb8(rgb, device=None) -> torch.Tensor:
    """float32 image(s) of any shape -> uint8 on the device: ``trunc(float64(x) * 255)``, the bytes ``utils.save_rgb`` writes for the
    image (and ``load_rgb`` reads back as ``byte / 255``).  ``lib.VfnError`` on a NaN / inf and on a value outside [0, 256/255): numpy's
    cast is undefined there and wraps on most hosts."""
    t = geomargs.as_tensor(rgb, "rgb")
    if t.dtype != torch.float32:
        raise ValueError(f"rgb must be torch.float32, got {t.dtype}")
    if t.numel() < 1:
        raise ValueError(f"rgb is empty: {tuple(t.shape)}")
    if t.numel() >= LIMIT:
        raise ValueError(f"rgb: {t.numel()} values exceed the 2^31 limit of one call")
    dev = _device(device)
    info = torch.zeros(1, dtype=torch.int64, device=dev)
    u = lib.image_quantize8(t.to(dev).contiguous(), info)
    _raise_on(int(info.cpu()), "quantize_rgb8")
    return u


def _scores(pred, target, quantize, ssim, pred_depth, target_depth, device):
    """The checks and launches of ``image_scores`` -> (list of per-view dicts, whether the input had a leading V)."""
    p = _check_images(pred, "pred", (torch.float32, torch.uint8), (1, 3))
    t = _check_images(target, "target", (torch.float32, torch.uint8), (1, 3))
    if p.shape != t.shape:
        raise ValueError(f"pred {tuple(p.shape)} and target {tuple(t.shape)} differ in shape")
    quantize, ssim = _check_flag(quantize, "quantize"), _check_flag(ssim, "ssim")
    if (pred_depth is None) != (target_depth is None):
        raise ValueError("pred_depth and target_depth go together: one of them is missing")
    batched = p.dim() == 4
    shape = tuple(p.shape) if batched else (1,) + tuple(p.shape)
    v, h, w, c = shape
    dp = dt = None
    if pred_depth is not None:
        dp, dt = _check_depth(pred_depth, "pred_depth", shape), _check_depth(target_depth, "target_depth", shape)
    dev = _device(device)
    info = torch.zeros(1, dtype=torch.int64, device=dev)
    p, t = p.to(dev).reshape(shape).contiguous(), t.to(dev).reshape(shape).contiguous()
    if quantize and p.dtype == torch.float32:
        p = lib.image_quantize8(p, info)
    parts = [lib.image_scores(p, t, ssim, info).reshape(-1)]
    if dp is not None:
        parts.append(lib.image_abs_err(dp.to(dev).contiguous(), dt.to(dev).contiguous(), L1_SCALE_CM, info))
    host = torch.cat(parts + [info.to(torch.float64)]).cpu().numpy()          # the one read-back
    _raise_on(int(host[-1]), "image_scores")
    sums = host[:3 * v].reshape(v, 3)
    out = []
    for i in range(v):
        s0 = float(sums[i, 0])
        row = {"psnr": math.inf if s0 == 0.0 else -10.0 * math.log10(s0 / (h * w * c))}
        if ssim:
            row["ssim"] = float(sums[i, 1]) / (h * w * c)
        if dp is not None:
            row["depth_l1_cm"] = float(host[3 * v + i]) / (h * w)
        out.append(row)
    return out, batched


def image_scores(pred, target, *, quantize: bool = True, ssim: bool = True, pred_depth=None, target_depth=None, device=None):
    """``pred`` against ``target`` ([H,W,C] or [V,H,W,C], C = 3 or 1; float32 or uint8, a byte b standing for b / 255) ->
    {"psnr", "ssim", "depth_l1_cm"} as Python floats — only the requested keys — or a list of V such dictionaries.

    * ``quantize=True`` sends a float32 prediction through ``quantize_rgb8`` first: what ``methods.metrics`` scores, after the PNG round
      trip.  ``quantize=False`` scores the float image itself.  A uint8 prediction is taken as it is.
    * psnr = -10 log10(S0 / (H W C)) with S0 = the sum of squared differences, ``inf`` when S0 == 0 (``get_psnr``).
    * ssim = the mean over all H W C elements of ``get_ssim``'s map (11 x 11 box window, zero padding, C1 = 1e-4, C2 = 9e-4).
    * depth_l1_cm (with ``pred_depth`` and ``target_depth``, float32 metres, [H,W] or [V,H,W], a trailing 1 allowed) = the mean of
      |100 a - 100 b| (``get_l1_cm``).
    The sums are float64 on the device in a fixed order; one read-back of 3 V (+ V) + 1 numbers."""
    rows, batched = _scores(pred, target, quantize, ssim, pred_depth, target_depth, device)
    return rows if batched else rows[0]


def _mean(values: Sequence[float]) -> float:
    total = 0.0
    for x in values:                 # serially, in index order, in float64
        total += x
    return total / len(values)


def score_views(preds, targets, *, quantize: bool = True, ssim: bool = False, pred_depths=None, target_depths=None, device=None) -> dict:
    """The reference's ``metrics.json`` dictionary (methods.py:587-610) for views ``preds[i]`` against ``targets[i]`` (sequences of
    [H,W,3] images, or [V,H,W,3] arrays): {"image-0": {"psnr": ..}, ..., "mean_psnr": ..}.  ``ssim=True`` adds "ssim" to every entry and
    "mean_ssim" after "mean_psnr"; depth maps add "depth_l1_cm" and "mean_depth_l1_cm".  The means are taken serially in index order in
    float64 (the reference averages a float32 tensor).  Views of one size and dtype are scored in one launch."""
    n = len(preds)
    if n < 1 or len(targets) != n:
        raise ValueError(f"{n} predictions against {len(targets)} targets")
    if (pred_depths is None) != (target_depths is None):
        raise ValueError("pred_depths and target_depths go together: one of them is missing")
    if pred_depths is not None and (len(pred_depths) != n or len(target_depths) != n):
        raise ValueError(f"{n} views need {n} depth maps each, got {len(pred_depths)} and {len(target_depths)}")
    quantize, ssim = _check_flag(quantize, "quantize"), _check_flag(ssim, "ssim")
    P = [_check_images(preds[i], f"preds[{i}]", (torch.float32, torch.uint8), (1, 3)) for i in range(n)]
    T = [_check_images(targets[i], f"targets[{i}]", (torch.float32, torch.uint8), (1, 3)) for i in range(n)]
    groups: dict = {}
    for i in range(n):
        if P[i].dim() != 3 or P[i].shape != T[i].shape:
            raise ValueError(f"view {i}: pred {tuple(P[i].shape)} and target {tuple(T[i].shape)} must be two [H,W,C] images of one shape")
        groups.setdefault((tuple(P[i].shape), P[i].dtype, T[i].dtype), []).append(i)
    if pred_depths is not None:
        D = [(_check_depth(pred_depths[i], f"pred_depths[{i}]", (1,) + tuple(P[i].shape)),
              _check_depth(target_depths[i], f"target_depths[{i}]", (1,) + tuple(P[i].shape))) for i in range(n)]
    dev = _device(device)
    rows: list = [None] * n
    for idx in groups.values():
        kw = {}
        if pred_depths is not None:
            kw = {"pred_depth": torch.cat([D[i][0].to(dev) for i in idx]), "target_depth": torch.cat([D[i][1].to(dev) for i in idx])}
        got, _ = _scores(torch.stack([P[i].to(dev) for i in idx]), torch.stack([T[i].to(dev) for i in idx]), quantize, ssim,
                         kw.get("pred_depth"), kw.get("target_depth"), dev)
        for i, row in zip(idx, got):
            rows[i] = row
    return views_dictionary(rows)


def views_dictionary(rows: Sequence[dict]) -> dict:
    """Per-view score dictionaries, in view order -> the ``metrics.json`` dictionary: "image-{i}" entries, then the "mean_*" keys."""
    out = {f"image-{i}": row for i, row in enumerate(rows)}
    for key in ("psnr", "ssim", "depth_l1_cm"):
        if rows and key in rows[0]:
            out[f"mean_{key}"] = _mean([r[key] for r in rows])
    return out
