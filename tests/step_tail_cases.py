"""Inputs, float64 references and scoring for the scalar tail of the training step (tests/test_step_tail_host.py,
tests/test_hip_step_tail.py): the fused loss (csrc/vfn_loss.hip), the flat gradient clip and Adam (csrc/vfn_adam.hip) and the sample
selection of the sparse colour branch (vfn_select_samples, csrc/vfn_rays.hip).  No device is used here.

References.  Nothing is restated where the package or torch states it:
  loss       vf_nerf_amd.loss.VFLoss with fused = False and supervision.get_center_indices_and_gt on CPU tensors, in float64 by promoting
             the float32 inputs the kernel gets (weights, clamp, radius and centroid are the float32 values of vfn_loss_params); the ball rows
             are concatenated behind segment 0, as the reference trainer does; gradients by torch.autograd.  An empty operand (no rays, no
             normals) is a mean over nothing, NaN in torch and 0 by the kernel's contract: the reference is then handed one row whose terms
             are exactly 0 (rgb = rgb_gt = 0, depth = depth_gt = 0, the normal (1, 0, 0)), which leaves the weighted total as VFLoss adds it.
  clip/Adam  torch.nn.utils.clip_grad_norm_(foreach=False) and torch.optim.Adam(foreach=False) on the CPU in float64 over a parameter list
             built from the regions of the flat buffer (region_list): one tensor per region, listed twice for multiplicity 2, elements outside
             every region not listed.
  selection  select_reference: a NumPy restatement of the contract in csrc/vfn_rays.hip / include/vfn.h.  The weights are an input: the
             oracle's volsdf_weights in float32 on the host, never the device's.
The yardstick of a float64 comparison is the same formulation in float32 on the host (host_*), pooled over the cases of one unit.

Decision margins.  An item (loss), a gradient (clip) or a ray (selection) is drawn again from the same generator while it sits on a
discontinuity of the float64 evaluation; nothing is skipped when scoring.  At most REDRAW_SHARE of the items or rays of a case may be
redrawn and none more than MAX_REDRAWS times (asserted by make_* and again by the host test).
  loss       | |p - c| - radius | < 1e-4 radius;  |e| < 1e-6 for rgb and depth;  | |e| - clamp | < 1e-6;  |n| < 1e-6 unless planted
  clip       |total - max_norm| < 1e-4 max_norm (by construction never: max_norm is total / 20 or 2 total)
  selection  a sample with sigma > 0, delta > 0 and 95 < before < 125 (the kernel's fp64 scan adds in another order, and its constant 110
             over-estimates float's 103.98 on purpose)
Planted exact cases sit beside the random ones and are never redrawn (LossInputs.planted, SelCase.planted_ray).
"""
from __future__ import annotations

import functools
import hashlib
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from oracle import vfnerf_oracle as O
from vf_nerf_amd import loss as vloss
from vf_nerf_amd import supervision

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24
MARGIN_FACTOR = 8.0
MAX_REDRAWS = 10
REDRAW_SHARE = 0.05
YARDSTICK_CAP = 1e-3


def _f32(x: float) -> float:
    return float(np.float32(x))


def _seed(tag: str) -> int:
    return int.from_bytes(hashlib.sha256(tag.encode()).digest()[:4], "little")


def rel_score(x: torch.Tensor, ref: torch.Tensor) -> float:
    """max |x - ref| / max |ref| over one tensor; a reference that is all zero scores 0 where x is exactly zero and infinity otherwise.
    Entries that are NaN on both sides count as equal; NaN on one side only is infinity."""
    x, ref = x.detach().to("cpu", F64).reshape(-1), ref.detach().to("cpu", F64).reshape(-1)
    if x.numel() == 0:
        return 0.0
    nx, nr = torch.isnan(x), torch.isnan(ref)
    if not torch.equal(nx, nr):
        return float("inf")
    x, ref = torch.where(nx, torch.zeros_like(x), x), torch.where(nr, torch.zeros_like(ref), ref)
    scale = float(ref.abs().max())
    if scale == 0.0:
        return 0.0 if bool((x == 0).all()) else float("inf")
    return float((x - ref).abs().max()) / scale


# ================================================================================================
# loss
# ================================================================================================
W_RGB, W_DEPTH, W_UNIT, W_SUP, W_SMALL = (_f32(v) for v in (2.0, 0.5, 0.1, 1.0, 0.1))
CLAMP = _f32(0.5)
RADIUS = _f32(0.15)
CENTROID = tuple(_f32(v) for v in (0.0, 0.0, 0.55))
LOSS_TERMS = ("rgb_loss", "depth_loss", "unit_norm_loss", "supervision_loss", "norm_smaller_than_one_loss")
LOSS_GRADS = ("d_rgb", "d_depth", "d_normals", "d_sup0", "d_sup1", "d_sup2")


@dataclass(frozen=True)
class LossCase:
    n_rays: int
    n_normals: int
    sup: Tuple[int, int, int]
    has_depth: int = 1
    smaller_on: int = 1
    ball: str = "on"                   # "on": about 6 % of the points inside; "off"; "empty": on, with every point outside (R = segments only)
    grad_out: Optional[float] = 0.6    # None: a NULL pointer (1)
    nan: str = ""                      # "depth", "normal", "rgb": one NaN planted there

    @property
    def items(self) -> int:
        return self.n_rays + self.n_normals + sum(self.sup)

    @property
    def planted(self) -> bool:
        return self.n_rays >= 3 and self.n_normals >= 2 and not self.nan

    @property
    def id(self) -> str:
        tag = f"{self.n_rays}-{self.n_normals}-{'.'.join(map(str, self.sup))}-d{self.has_depth}s{self.smaller_on}-ball_{self.ball}"
        tag += "-gNULL" if self.grad_out is None else f"-g{self.grad_out:g}"
        return tag + (f"-nan_{self.nan}" if self.nan else "")


LOSS_SHAPES = ((1, 0, (0, 0, 0)), (0, 1, (0, 0, 0)), (3, 250, (5, 0, 7)), (37, 37 * 13, (37, 0, 0)), (255, 769, (0, 0, 1)))
LOSS_CAPPED = (4096, 1_100_000, (40_000, 3, 65_537))          # 1 209 636 items: reduce grid 1024, backward grid 4096, 5 items per thread


def _loss_case_list():
    c = [LossCase(*s) for s in LOSS_SHAPES]
    c += [LossCase(0, 1, (0, 0, 0), ball="empty")]                                           # R = 0 with the ball on
    c += [LossCase(37, 37 * 13, (0, 0, 0), ball="empty"), LossCase(37, 37 * 13, (0, 0, 0), ball="empty", grad_out=None)]
    for s in LOSS_SHAPES[2:4]:
        c += [LossCase(*s, has_depth=0), LossCase(*s, smaller_on=0), LossCase(*s, ball="off"), LossCase(*s, grad_out=None),
              LossCase(*s, has_depth=0, smaller_on=0, ball="off", grad_out=None)]
    c += [LossCase(*LOSS_CAPPED), LossCase(*LOSS_CAPPED, has_depth=0, smaller_on=0, grad_out=None)]
    return tuple(c)


LOSS_CASES = _loss_case_list()
LOSS_NAN_CASES = tuple(LossCase(*LOSS_SHAPES[2], nan=k) for k in ("depth", "normal", "rgb")) + \
    (LossCase(*LOSS_SHAPES[2], smaller_on=0, ball="off", nan="normal"),)


@dataclass(frozen=True, eq=False)
class LossInputs:
    case: LossCase
    rgb: torch.Tensor          # [N,3] float32
    rgb_gt: torch.Tensor
    depth: torch.Tensor        # [N]
    depth_gt: torch.Tensor
    normals: torch.Tensor      # [M,3]
    points: torch.Tensor       # [M,3]
    sup_pred: Tuple[torch.Tensor, ...]     # three [n_sup[k],3]
    sup_gt: Tuple[torch.Tensor, ...]
    redraws: Dict[str, int]    # rays / normals drawn again, and the largest number of draws of one item
    planted: Dict[str, int]    # name -> row


def _ray_margin(rgb, rgb_gt, depth, depth_gt, has_depth):
    e = (rgb.double() - rgb_gt.double()).abs()
    bad = (e < 1e-6).any(dim=1)
    if has_depth:
        d = (depth.double() - depth_gt.double()).abs()
        bad |= (d < 1e-6) | ((d - CLAMP).abs() < 1e-6)
    return bad


def _normal_margin(normals, points, ball_on):
    bad = torch.linalg.vector_norm(normals.double(), dim=1) < 1e-6
    if ball_on:
        d = torch.linalg.vector_norm(points.double() - torch.tensor(CENTROID, dtype=F64), dim=1)
        bad |= (d - RADIUS).abs() < 1e-4 * RADIUS
    return bad


@functools.lru_cache(maxsize=None)
def make_loss_inputs(case: LossCase) -> LossInputs:
    g = torch.Generator().manual_seed(_seed("loss-" + case.id))
    n, m = case.n_rays, case.n_normals

    def rays(k):
        return (torch.rand(k, 3, generator=g), torch.rand(k, 3, generator=g), 1.5 * torch.rand(k, generator=g), 1.5 * torch.rand(k, generator=g))

    def normal_rows(k):
        nrm = 0.8 * torch.randn(k, 3, generator=g)
        pts = 0.6 * torch.rand(k, 3, generator=g) + torch.tensor([-0.3, -0.3, 0.25])
        if case.ball == "empty":
            pts = pts + torch.tensor([0.0, 0.0, 1.0])            # the whole box a full unit above the ball
        return nrm, pts

    rgb, rgb_gt, depth, depth_gt = rays(n)
    normals, points = normal_rows(m)
    stats = dict(rays=0, normals=0, most=0)
    for kind in ("rays", "normals"):
        count = torch.zeros(n if kind == "rays" else m, dtype=torch.long)
        while True:
            bad = _ray_margin(rgb, rgb_gt, depth, depth_gt, case.has_depth) if kind == "rays" else _normal_margin(normals, points, case.ball != "off")
            idx = torch.nonzero(bad).reshape(-1)
            if idx.numel() == 0:
                break
            count[idx] += 1
            assert int(count.max()) < MAX_REDRAWS, f"{case.id}: a {kind[:-1]} drawn {MAX_REDRAWS} times without clearing the margins"
            if kind == "rays":
                a, b, c, d = rays(idx.numel())
                rgb[idx], rgb_gt[idx], depth[idx], depth_gt[idx] = a, b, c, d
            else:
                a, b = normal_rows(idx.numel())
                normals[idx], points[idx] = a, b
        stats[kind] = int((count > 0).sum())
        stats["most"] = max(stats["most"], int(count.max()) if count.numel() else 0)
        assert stats[kind] <= REDRAW_SHARE * max(count.numel(), 1), f"{case.id}: {stats[kind]} of {count.numel()} {kind} redrawn"
    sup_pred = tuple(0.8 * torch.randn(k, 3, generator=g) for k in case.sup)
    sup_gt = tuple(torch.nn.functional.normalize(torch.randn(k, 3, generator=g), dim=1) for k in case.sup)
    planted = {}
    if case.planted:
        rgb[0, 0] = rgb_gt[0, 0]                                 # |e| = 0: gradient 0
        depth[1], depth_gt[1] = 1.0, 0.5                         # |e| = clamp, a tie: the gradient passes
        depth[2], depth_gt[2] = 0.5, 1.0625                      # |e| > clamp: gradient 0
        normals[0] = 0.0                                         # |n| = 0
        planted = dict(rgb_equal=0, depth_tie=1, depth_clamped=2, zero_normal=0)
        if case.ball == "on":
            points[1] = torch.tensor(CENTROID)                   # F.normalize's 1e-12
            planted["at_centroid"] = 1
    if case.nan == "depth":
        depth[1] = float("nan")
    elif case.nan == "rgb":
        rgb[1, 2] = float("nan")
    elif case.nan == "normal":
        normals[3, 1] = float("nan")
    return LossInputs(case, rgb, rgb_gt, depth, depth_gt, normals, points, sup_pred, sup_gt, stats, planted)


def loss_eval(inp: LossInputs, dtype) -> Dict[str, torch.Tensor]:
    """VFLoss (tensor-op formulation) + the trainer's centre-ball compaction in ``dtype`` -> out8 [8] (the kernel's out_terms) and
    d_rgb, d_depth, d_normals, d_sup0..2 (zeros where torch gives no gradient), times grad_out."""
    case = inp.case
    cfg = SimpleNamespace(depth_loss_clamp=CLAMP, norm_smaller_than_one_start=0 if case.smaller_on else 10 ** 9, directional_derivatives_start=10 ** 9)
    w = SimpleNamespace(rgb=W_RGB, depth=W_DEPTH, unit_norm=W_UNIT, supervision=W_SUP, norm_smaller_than_one=W_SMALL, directional_derivatives=0.0)
    crit = vloss.VFLoss(cfg, w)
    crit.fused = False
    def leaf(t):
        return t.detach().to(dtype).clone().requires_grad_(True)        # (a copy: .to() of the same dtype would mark the shared input)

    leaves = dict(d_rgb=leaf(inp.rgb), d_depth=leaf(inp.depth), d_normals=leaf(inp.normals))
    for k in range(3):
        leaves[f"d_sup{k}"] = leaf(inp.sup_pred[k])
    one = torch.zeros(1, 3, dtype=dtype)
    rgb, rgb_gt = (leaves["d_rgb"], inp.rgb_gt.to(dtype)) if case.n_rays else (one, one)
    depth, depth_gt = (leaves["d_depth"], inp.depth_gt.to(dtype)) if case.n_rays else (one[:, 0], one[:, 0])
    normals = leaves["d_normals"] if case.n_normals else torch.tensor([[1.0, 0.0, 0.0]], dtype=dtype)
    ball_n, ball_gt = torch.empty(0, 3, dtype=dtype), torch.empty(0, 3, dtype=dtype)
    if case.ball != "off" and case.n_normals:
        ball_n, ball_gt = supervision.get_center_indices_and_gt(inp.points.to(dtype).reshape(-1, 1, 3), leaves["d_normals"],
                                                                torch.tensor(CENTROID, dtype=dtype), RADIUS)
    preds = [leaves["d_sup0"], ball_n, leaves["d_sup1"], leaves["d_sup2"]]
    gts = [inp.sup_gt[0].to(dtype), ball_gt, inp.sup_gt[1].to(dtype), inp.sup_gt[2].to(dtype)]
    pred = {"rgb": rgb, "depth": depth, "normals": normals, "supervised_normals": torch.cat(preds), "directional_derivatives": None}
    gt = {"rgb": rgb_gt, "depth": depth_gt if case.has_depth else torch.empty(0, dtype=dtype), "supervised_normals": torch.cat(gts)}
    total, logs = crit(pred, gt, 1)
    rows = pred["supervised_normals"].shape[0]
    terms = [float(logs.get(k)) for k in LOSS_TERMS]
    out = dict(out8=torch.tensor(terms + [0.0, float(total.detach()), float(rows)], dtype=dtype))
    if total.requires_grad:
        got = torch.autograd.grad(total * (1.0 if case.grad_out is None else _f32(case.grad_out)), list(leaves.values()), allow_unused=True)
    else:
        got = [None] * len(leaves)
    for (k, x), y in zip(leaves.items(), got):
        out[k] = torch.zeros_like(x) if y is None else y.detach()
    return out


@functools.lru_cache(maxsize=None)
def loss_reference(case: LossCase):
    return loss_eval(make_loss_inputs(case), F64)


@functools.lru_cache(maxsize=None)
def loss_host_fp32(case: LossCase):
    return loss_eval(make_loss_inputs(case), F32)


def loss_scores(case: LossCase, run: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """Every term and the total on its own scale, every gradient tensor on its own; 'rows' is 0 where out[7] equals the float64 row
    count exactly and infinity otherwise; out[5] likewise against 0."""
    ref = loss_reference(case)
    out = {}
    for i, name in enumerate(LOSS_TERMS + ("dd", "total", "rows")):
        if name in ("dd", "rows"):
            out[name] = 0.0 if float(run["out8"][i]) == float(ref["out8"][i]) else float("inf")
        else:
            out[name] = rel_score(run["out8"][i], ref["out8"][i])
    for k in LOSS_GRADS:
        if k in run and run[k] is not None:
            out[k] = rel_score(run[k], ref[k])
    return out


def _pooled(cases, host, scores) -> Dict[str, float]:
    pool: Dict[str, float] = {}
    for case in cases:
        for k, v in scores(case, host(case)).items():
            pool[k] = max(pool.get(k, 0.0), v)
    return pool


@functools.lru_cache(maxsize=None)
def loss_pool(case: LossCase) -> str:
    """The cases of one item apart: (|n| - 1)^2 of a single normal cancels to 1e-6 of itself in float32, which a mean over hundreds
    never does, and the bound of every other case should not inherit that."""
    return "one item" if case.items <= 1 else "many"


@functools.lru_cache(maxsize=None)
def loss_yardsticks() -> Dict[str, Dict[str, float]]:
    return {key: _pooled([c for c in LOSS_CASES if loss_pool(c) == key], loss_host_fp32, loss_scores) for key in ("one item", "many")}


def loss_yardstick(case: LossCase) -> Dict[str, float]:
    """{quantity: float32 host against float64}, the maximum over the LOSS_CASES of the case's pool (the NaN cases are held to the
    figures of the clean ones)."""
    return loss_yardsticks()[loss_pool(case)]


def failures(scores: Dict[str, float], yard: Dict[str, float], what: str) -> List[str]:
    """The quantities of ``scores`` beyond MARGIN_FACTOR x their yardstick."""
    return [f"{what} {k}: {v:.3e} against {yard[k]:.3e} float32 on the host (x {MARGIN_FACTOR:g} allowed)"
            for k, v in scores.items() if not v <= MARGIN_FACTOR * yard[k]]


def loss_planted_failures(case: LossCase, run: Dict[str, torch.Tensor]) -> List[str]:
    """The planted items, exactly: gradient 0 at an rgb element equal to its ground truth and beyond the clamp, the float64 sign times
    the same float32 factor at the tie, the zero normal's gradient equal to its ball part alone."""
    inp, ref, bad = make_loss_inputs(case), loss_reference(case), []
    if not inp.planted:
        return bad
    if run.get("d_rgb") is not None and float(run["d_rgb"][0, 0]) != 0.0:
        bad.append("d_rgb at rgb == rgb_gt is not 0")
    if run.get("d_depth") is not None:
        d = run["d_depth"].detach().cpu().double()
        if float(d[2]) != 0.0:
            bad.append("d_depth beyond the clamp is not 0")
        if case.has_depth:
            assert float(ref["d_depth"][1]) > 0.0 and float(ref["d_depth"][2]) == 0.0        # (torch: clamp(max=) passes at the tie)
            if not float(d[1]) > 0.0:
                bad.append("d_depth at |e| == clamp does not pass the gradient")
        elif float(d.abs().max()) != 0.0:
            bad.append("d_depth without depth ground truth is not 0")
    if run.get("d_normals") is not None:
        z = run["d_normals"][0].detach().cpu().double()
        inside = case.ball == "on" and float(torch.linalg.vector_norm(inp.points[0].double() - torch.tensor(CENTROID, dtype=F64))) < RADIUS
        if not inside and float(z.abs().max()) != 0.0:
            bad.append("d_normals of the zero normal is not 0")
        if not bool(torch.isfinite(z).all()):
            bad.append("d_normals of the zero normal is not finite")
    return bad


# ================================================================================================
# clip and Adam
# ================================================================================================
def region_sets(n: int):
    """{name: [(start, end, mult)]} for a flat buffer of n elements: two regions meeting at 63, 64 and 65; four regions with a gap, a
    zero-length region and a tail outside every region."""
    if n == 1:
        return {"one-x2": [(0, 1, 2)], "one-x1": [(0, 1, 1)]}
    sets = {f"edge{e}": [(0, e, 2), (e, n, 1)] for e in (63, 64, 65) if e < n}
    a, b, c = n // 4 - 1, n // 4 + 6, (3 * n) // 4 + 1
    sets["four"] = [(0, a, 2), (a, a, 1), (b, c, 1), (c, n - 7, 2)]
    return sets


def region_list(flat: torch.Tensor, regions):
    """The parameter list a flat buffer stands for -> (unique tensors, one per region, views of nothing: clones; the list with the
    tensors of multiplicity 2 named twice, in optim.FlatAdam._layout's order of the regions)."""
    uniq = [flat[s:e].clone() for s, e, _ in regions]
    return uniq, [t for t, (_, _, m) in zip(uniq, regions) for _ in range(m)]


def mult_vector(n: int, regions) -> torch.Tensor:
    m = torch.zeros(n, dtype=torch.long)
    for s, e, k in regions:
        m[s:e] = k
    return m


@dataclass(frozen=True)
class ClipCase:
    n: int
    regions_name: str
    mode: str                      # "clipped" (total = 20 max_norm), "unclipped" (total = max_norm / 2), "zero"
    plant: str = ""                # "nan" / "inf": in one element of a multiplicity-1 region
    scale: float = 1.0             # of every gradient: 1e-6 puts the total where the + 1e-6 of the coefficient counts

    @property
    def regions(self):
        return region_sets(self.n)[self.regions_name]

    @property
    def id(self) -> str:
        return f"n{self.n}-{self.regions_name}-{self.mode}" + (f"-{self.plant}" if self.plant else "") + (f"-x{self.scale:g}" if self.scale != 1.0 else "")


CLIP_BIG = 262_144 + 256 + 77
CLIP_MODES = ("clipped", "unclipped", "zero")


def _clip_groups():
    """[(n, regions_name)]: every group runs its three modes in turn on ONE workspace (the kernel resets its own counter)."""
    g = [(1, "one-x2"), (1, "one-x1")]
    g += [(n, f"edge{e}") for n, e in ((255, 63), (256, 64), (257, 65), (257, 63), (255, 65), (256, 63))]
    g += [(257, "four"), (CLIP_BIG, "edge65"), (CLIP_BIG, "four")]
    return tuple(g)


CLIP_GROUPS = _clip_groups()
CLIP_CASES = tuple(ClipCase(n, r, mode) for n, r in CLIP_GROUPS for mode in CLIP_MODES) + \
    (ClipCase(255, "edge63", "clipped", scale=1e-6), ClipCase(257, "four", "clipped", scale=1e-6))
CLIP_PLANT_CASES = tuple(ClipCase(n, r, "clipped", plant=p) for n, r in ((257, "four"), (CLIP_BIG, "edge65")) for p in ("nan", "inf"))


@dataclass(frozen=True, eq=False)
class ClipInputs:
    case: ClipCase
    grad: torch.Tensor             # [n] float32
    max_norm: float                # a float32 value
    plant_at: int


@functools.lru_cache(maxsize=None)
def make_clip_inputs(case: ClipCase) -> ClipInputs:
    g = torch.Generator().manual_seed(_seed("clip-" + case.id))
    n = case.n
    mag = 10.0 ** (-12.0 + 13.0 * torch.rand(n, generator=g, dtype=F64))              # log-uniform 1e-12 .. 10
    grad = (mag * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0) * case.scale).float()
    if case.mode == "zero":
        grad.zero_()
    plant_at = -1
    if case.plant:
        s, e = next((s, e) for s, e, m in case.regions if m == 1 and e > s)
        plant_at = s + (e - s) // 3
        grad[plant_at] = float("nan") if case.plant == "nan" else float("inf")
    total = float(torch.sqrt((mult_vector(n, case.regions).double() * torch.nan_to_num(grad.double(), nan=0.0, posinf=0.0) ** 2).sum()))
    max_norm = 1.0 if case.mode == "zero" else _f32(total / 20.0 if case.mode == "clipped" else 2.0 * total)
    if max_norm == 0.0:           # (a single element outside every region cannot happen: the sets of n = 1 cover it)
        max_norm = 1.0
    assert case.mode == "zero" or abs(total - max_norm) >= 1e-4 * max_norm
    return ClipInputs(case, grad, max_norm, plant_at)


def clip_eval(inp: ClipInputs, dtype):
    """torch.nn.utils.clip_grad_norm_(foreach=False) over the region list in ``dtype`` -> total norm (0-dim), scaled flat gradient [n]
    (elements outside every region as they were)."""
    regions = inp.case.regions
    flat = inp.grad.to(dtype).clone()
    uniq, plist = region_list(flat, regions)
    params = {id(t): torch.nn.Parameter(torch.zeros_like(t)) for t in uniq}
    for t in uniq:
        params[id(t)].grad = t
    total = torch.nn.utils.clip_grad_norm_([params[id(t)] for t in plist], inp.max_norm, foreach=False)
    for t, (s, e, _) in zip(uniq, regions):
        flat[s:e] = params[id(t)].grad
    return total.detach(), flat


@functools.lru_cache(maxsize=None)
def clip_reference(case: ClipCase):
    return clip_eval(make_clip_inputs(case), F64)


def _ulp32(x: float) -> float:
    return float(np.spacing(np.float32(abs(x))))


def clip_failures(case: ClipCase, out2: torch.Tensor, grad: torch.Tensor) -> List[str]:
    """The derived bounds (u = 2^-24): out2[0] within one float32 ulp of the float64 norm; out2[1] within 4 u of max_norm /
    (total64 + 1e-6), exactly 1.0 where that is at least 1; every gradient element within 5 mult u of its float64 value, the same bits
    where unclipped and outside every region.  A planted NaN: NaN, NaN and NaN inside the regions; a planted +inf: inf, 0, the infinite
    element NaN and every other listed element 0 — both as float64 torch gives them."""
    inp = make_clip_inputs(case)
    total64, want = clip_reference(case)
    out2, grad = out2.detach().cpu(), grad.detach().cpu()
    mult = mult_vector(case.n, case.regions)
    bad = []
    outside = mult == 0
    if not torch.equal(grad[outside].view(torch.int32), inp.grad[outside].view(torch.int32)):
        bad.append("elements outside every region changed")
    if case.plant:
        t, c = float(out2[0]), float(out2[1])
        if case.plant == "nan":
            assert bool(torch.isnan(total64)) and bool(torch.isnan(want[~outside]).all())
            if not (t != t and c != c):
                bad.append(f"NaN gradient: out2 = ({t}, {c}), expected NaN, NaN")
            if not bool(torch.isnan(grad[~outside]).all()):
                bad.append("NaN total: gradients inside the regions are not all NaN")
        else:
            assert float(total64) == float("inf")
            if not (t == float("inf") and c == 0.0):
                bad.append(f"infinite gradient: out2 = ({t}, {c}), expected inf, 0")
            inside = grad[~outside].double()
            if not torch.equal(torch.isnan(inside), torch.isnan(want[~outside])) or float(torch.nan_to_num(inside, nan=0.0).abs().max()) != 0.0:
                bad.append("infinite total: expected NaN at the infinite element and 0 elsewhere")
        return bad
    t64 = float(total64)
    if abs(float(out2[0]) - t64) > _ulp32(t64):
        bad.append(f"total norm {float(out2[0]):.9e} against {t64:.9e}: more than one float32 ulp")
    coef64 = inp.max_norm / (t64 + 1e-6)
    if coef64 >= 1.0:
        if float(out2[1]) != 1.0:
            bad.append(f"coefficient {float(out2[1])!r} where nothing is clipped, expected exactly 1.0")
        if not torch.equal(grad.view(torch.int32), inp.grad.view(torch.int32)):
            bad.append("an unclipped gradient changed its bits")
        return bad
    if abs(float(out2[1]) - coef64) > 4 * U * coef64:
        bad.append(f"coefficient {float(out2[1]):.9e} against {coef64:.9e}: more than 4 u")
    err = (grad.double() - want).abs()
    room = 5.0 * mult.double() * U * want.abs()
    if not bool((err <= room).all()):
        i = int(torch.argmax(err - room))
        bad.append(f"scaled gradient [{i}] (mult {int(mult[i])}): {float(grad[i]):.9e} against {float(want[i]):.9e}")
    return bad


@dataclass(frozen=True)
class AdamCase:
    n: int
    regions_name: str
    t0: Tuple[int, ...]            # the step count of every region before the first step
    weight_decay: float = 0.0
    steps: int = 3

    @property
    def regions(self):
        return region_sets(self.n)[self.regions_name]

    @property
    def id(self) -> str:
        return f"n{self.n}-{self.regions_name}-t{'.'.join(map(str, self.t0))}-wd{self.weight_decay:g}"


ADAM_BIG = 524_288 + 256 + 77
ADAM_LR, ADAM_BETAS, ADAM_EPS = 3e-3, (0.9, 0.999), 1e-8
ADAM_CASES = tuple(AdamCase(n, r, t0, wd) for wd in (0.0, 1e-2) for n, r, t0 in (
    (1, "one-x2", (0,)), (1, "one-x2", (1,)), (1, "one-x1", (999,)), (257, "edge65", (0, 1)), (257, "edge63", (1, 999)), (257, "four", (999, 0, 0, 1)),
    (ADAM_BIG, "edge65", (1, 0)), (ADAM_BIG, "four", (0, 1, 999, 1))))
ADAM_STATE = ("p", "m", "v")


@dataclass(frozen=True, eq=False)
class AdamInputs:
    case: AdamCase
    p: torch.Tensor
    m: torch.Tensor
    v: torch.Tensor
    grads: Tuple[torch.Tensor, ...]        # one per step


@functools.lru_cache(maxsize=None)
def make_adam_inputs(case: AdamCase) -> AdamInputs:
    g = torch.Generator().manual_seed(_seed("adam-" + case.id))
    n = case.n
    p = 0.1 * torch.randn(n, generator=g)
    m, v = 1e-2 * torch.randn(n, generator=g), (1e-2 * torch.randn(n, generator=g)) ** 2       # carried from a previous step ...
    for (s, e, _), t0 in zip(case.regions, case.t0):
        if t0 == 0:                                                                             # ... or zero, before the first
            m[s:e], v[s:e] = 0.0, 0.0
    grads = tuple((10.0 ** (-9.0 + 9.0 * torch.rand(n, generator=g, dtype=F64)) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).float()
                  for _ in range(case.steps))
    return AdamInputs(case, p, m, v, grads)


def adam_scalars(case: AdamCase, step: int):
    """step_size[2 per region], bc2_sqrt[2 per region] of step number ``step`` (0-based) of the case, in double precision as
    optim.FlatAdam.step_scalars evaluates them for its (at most two) regions: update k of a region is its t0 + mult step + k + 1 th."""
    b1, b2 = ADAM_BETAS
    ss, bc = [], []
    for (_, _, mult), t0 in zip(case.regions, case.t0):
        for k in range(2):
            t = t0 + mult * step + k + 1
            ss.append(ADAM_LR / (1 - b1 ** t))
            bc.append((1 - b2 ** t) ** 0.5)
    return ss, bc


def adam_eval(inp: AdamInputs, dtype) -> List[Dict[str, torch.Tensor]]:
    """torch.optim.Adam(foreach=False) over the region list in ``dtype`` -> after every step the flat p, m, v (elements outside every
    region as they were)."""
    case = inp.case
    flat = {k: getattr(inp, k).to(dtype).clone() for k in ADAM_STATE}
    uniq, plist = region_list(flat["p"], case.regions)
    params = {id(t): torch.nn.Parameter(t) for t in uniq}
    opt = torch.optim.Adam([params[id(t)] for t in plist], lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=case.weight_decay, foreach=False)
    for t, (s, e, _), t0 in zip(uniq, case.regions, case.t0):
        opt.state[params[id(t)]] = {"step": torch.tensor(float(t0)), "exp_avg": flat["m"][s:e].clone(), "exp_avg_sq": flat["v"][s:e].clone()}
    out = []
    for grad in inp.grads:
        for t, (s, e, _) in zip(uniq, case.regions):
            params[id(t)].grad = grad[s:e].to(dtype).clone()
        opt.step()
        now = {k: v.clone() for k, v in flat.items()}
        for t, (s, e, _) in zip(uniq, case.regions):
            st = opt.state[params[id(t)]]
            now["p"][s:e], now["m"][s:e], now["v"][s:e] = params[id(t)].detach(), st["exp_avg"], st["exp_avg_sq"]
        out.append(now)
    for t, (s, e, mult), t0 in zip(uniq, case.regions, case.t0):
        assert float(opt.state[params[id(t)]]["step"]) == t0 + mult * case.steps
    return out


@functools.lru_cache(maxsize=None)
def adam_reference(case: AdamCase):
    return adam_eval(make_adam_inputs(case), F64)


@functools.lru_cache(maxsize=None)
def adam_host_fp32(case: AdamCase):
    return adam_eval(make_adam_inputs(case), F32)


def adam_scores(case: AdamCase, run: List[Dict[str, torch.Tensor]]) -> Dict[str, float]:
    """{p, m, v, update}: the worst region and step, each region on its own scale; 'outside' is 0 where the elements outside every
    region keep the bits of p, m and v and infinity otherwise.  update = p_new - p_old, the step from the run's own previous state."""
    inp, ref = make_adam_inputs(case), adam_reference(case)
    out = dict(p=0.0, m=0.0, v=0.0, update=0.0, outside=0.0)
    outside = mult_vector(case.n, case.regions) == 0
    for step, (got, want) in enumerate(zip(run, ref)):
        got = {k: v.detach().cpu() for k, v in got.items()}
        prev_got = (run[step - 1]["p"].detach().cpu() if step else inp.p).double()
        prev_want = ref[step - 1]["p"] if step else inp.p.double()
        for s, e, _ in case.regions:
            if e == s:
                continue
            for k in ADAM_STATE:
                out[k] = max(out[k], rel_score(got[k][s:e], want[k][s:e]))
            out["update"] = max(out["update"], rel_score(got["p"][s:e].double() - prev_got[s:e], want["p"][s:e] - prev_want[s:e]))
        for k in ADAM_STATE:
            if not torch.equal(got[k][outside].float().view(torch.int32), getattr(inp, k)[outside].view(torch.int32)):
                out["outside"] = float("inf")
    return out


@functools.lru_cache(maxsize=None)
def adam_yardstick() -> Dict[int, Dict[str, float]]:
    """{n: {quantity: float32 host against float64}}: pooled over the cases of one buffer size (a single element's update can cancel
    to 1e-4 of itself in float32; the bound of 5e5 elements should not inherit that)."""
    return {n: _pooled([c for c in ADAM_CASES if c.n == n], adam_host_fp32, adam_scores) for n in sorted({c.n for c in ADAM_CASES})}


# the optim.FlatAdam + optim.clip_grad_norm_ leg: a duplicated list of 524 982 elements, step counters 6 (listed twice) and 3
FLAT_SHAPES = ((512, 600), (77,), (700, 311), (5,))
FLAT_TWICE = 2                      # the first two are listed twice
FLAT_STEPS0 = (6.0, 3.0)
FLAT_MAX_NORM = 0.5


def flat_leg_inputs():
    g = torch.Generator().manual_seed(_seed("flat-leg"))
    p = [0.1 * torch.randn(*s, generator=g) for s in FLAT_SHAPES]
    m = [1e-2 * torch.randn(*s, generator=g) for s in FLAT_SHAPES]
    v = [(1e-2 * torch.randn(*s, generator=g)) ** 2 for s in FLAT_SHAPES]
    grads = [[(10.0 ** (-9.0 + 9.0 * torch.rand(*s, generator=g, dtype=F64)) * torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0)).float()
              for s in FLAT_SHAPES] for _ in range(3)]
    return p, m, v, grads


def flat_leg_run(make_optimizer, clip, device, dtype):
    """Three clipped steps of the duplicated list -> [(total norm, [p], [m], [v]) per step] on the CPU.  ``make_optimizer(plist)`` and
    ``clip(plist, max_norm)``: torch's sequential ones for the reference, optim.FlatAdam and optim.clip_grad_norm_ on the device."""
    p0, m0, v0, grads = flat_leg_inputs()
    ps = [torch.nn.Parameter(t.to(device, dtype)) for t in p0]
    plist = ps + ps[:FLAT_TWICE]
    opt = make_optimizer(plist)
    for i, p in enumerate(ps):
        opt.state[p] = {"step": torch.tensor(FLAT_STEPS0[0] if i < FLAT_TWICE else FLAT_STEPS0[1]), "exp_avg": m0[i].to(device, dtype).clone(),
                        "exp_avg_sq": v0[i].to(device, dtype).clone()}
    out = []
    for gs in grads:
        opt.zero_grad()
        for p, gg in zip(ps, gs):
            if p.grad is None:
                p.grad = gg.to(device, dtype).clone()
            else:
                p.grad.add_(gg.to(device, dtype))
        total = clip(plist, FLAT_MAX_NORM)
        opt.step()
        out.append((float(total), [p.detach().cpu().clone() for p in ps], [opt.state[p]["exp_avg"].detach().cpu().clone() for p in ps],
                    [opt.state[p]["exp_avg_sq"].detach().cpu().clone() for p in ps]))
    steps = [float(opt.state[p]["step"]) for p in ps]
    assert steps == [FLAT_STEPS0[0] + 6.0] * FLAT_TWICE + [FLAT_STEPS0[1] + 3.0] * (len(ps) - FLAT_TWICE), steps
    return out


def flat_leg_torch(dtype):
    return flat_leg_run(lambda pl: torch.optim.Adam(pl, lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, foreach=False),
                        lambda pl, mx: torch.nn.utils.clip_grad_norm_(pl, mx, foreach=False), "cpu", dtype)


def flat_leg_scores(run, ref) -> Dict[str, float]:
    """p, m, v per parameter and step on the parameter's own scale (worst), and the total norm in float32 ulps of the reference."""
    out = dict(p=0.0, m=0.0, v=0.0, norm_ulps=0.0)
    for (tn, p, m, v), (tn64, p64, m64, v64) in zip(run, ref):
        out["norm_ulps"] = max(out["norm_ulps"], abs(tn - tn64) / _ulp32(tn64))
        for k, got, want in (("p", p, p64), ("m", m, m64), ("v", v, v64)):
            out[k] = max([out[k]] + [rel_score(a, b) for a, b in zip(got, want)])
    return out


# ================================================================================================
# selection
# ================================================================================================
SEL_FAMILIES = ("sparse", "dense", "tiny", "opaque", "all", "none")
SEL_S = (1, 2, 63, 64, 65, 128, 200, 512)
SEL_N = (1, 5, 255, 256, 257, 1030)
SENTINEL = -7


@dataclass(frozen=True)
class SelCase:
    n_rays: int
    s: int
    family: str

    @property
    def id(self) -> str:
        return f"{self.family}-N{self.n_rays}-S{self.s}"

    @property
    def planted_ray(self) -> bool:
        """ray 0 holds a sample with delta = 0 (duplicate depths) and sigma > 0, in front of everything opaque"""
        return self.s >= 3 and self.family in ("sparse", "dense", "tiny")


def _sel_case_list():
    shapes = [(257, s) for s in SEL_S] + [(n, 200) for n in SEL_N if n != 257]
    c = [SelCase(n, s, f) for f in ("sparse", "dense", "tiny", "opaque") for n, s in shapes]
    c += [SelCase(n, s, f) for f in ("all", "none") for n, s in ((257, 1), (257, 65), (257, 200), (1030, 200), (5, 512))]
    return tuple(c)


SEL_CASES = _sel_case_list()


@dataclass(frozen=True, eq=False)
class SelInputs:
    case: SelCase
    weights: np.ndarray        # [N,S] float32
    sigma: np.ndarray
    z: np.ndarray
    points: np.ndarray         # [N,S,3]
    dirs: np.ndarray           # [N,3]
    redrawn: int               # rays drawn again
    most: int                  # the largest number of draws of one ray


def _sel_draw(rng: np.random.Generator, case: SelCase, k: int, first: bool):
    """k rays -> sigma [k,S], z [k,S] float32; ``first``: row 0 is the case's ray 0 (the planted one)."""
    s = case.s

    def logu(lo, hi, *shape):
        return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), shape)

    if case.family == "all":
        gaps = rng.uniform(1e-3, 2e-3, (k, max(s - 1, 0)))
    else:
        # a ray of about unit length whatever S: spacings log-uniform over a decade below 3 / S.  (Spacings independent of S would let the
        # exponent sum wander through the band 95 .. 125 on one ray in ten at S = 512, past the redraw cap.)
        gaps = logu(0.3 / s, 3.0 / s, k, max(s - 1, 0))
    z = (0.5 + rng.uniform(0, 1, (k, 1)) + np.concatenate([np.zeros((k, 1)), np.cumsum(gaps, axis=1)], axis=1)).astype(np.float32)
    z = np.maximum.accumulate(z, axis=1)
    if case.family == "sparse" or case.family == "opaque":
        sigma = np.where(rng.uniform(0, 1, (k, s)) < 0.05, logu(1e-9, 1e4, k, s), 0.0)
        if case.family == "opaque":
            sigma[np.arange(k), rng.integers(0, min(2, s), k)] = 1e6
    elif case.family == "dense":
        sigma = logu(1e-9, 1e3, k, s)
    elif case.family == "tiny":
        sigma = np.where(rng.uniform(0, 1, (k, s)) < 0.3, logu(1e-8, 1e-5, k, s), 0.0)
    elif case.family == "all":
        sigma = np.ones((k, s))
    else:
        sigma = np.zeros((k, s))
    if first and case.planted_ray:
        z[0, 1] = z[0, 0]                      # delta_0 = 0 ...
        sigma[0, 0] = 1.0                      # ... under a positive sigma: not selected by the training clause
        sigma[0, 1] = min(sigma[0, 1], 1e-3)
    return sigma.astype(np.float32), z


def sel_parts(sigma: np.ndarray, z: np.ndarray):
    """delta [N,S] float32 (the last one float32(1e10)), e = float32(sigma delta), before = the float64 sum of e_i over i < j."""
    n, s = sigma.shape
    delta = np.concatenate([z[:, 1:] - z[:, :-1], np.full((n, 1), np.float32(1e10), dtype=np.float32)], axis=1).astype(np.float32)
    e = (sigma * delta).astype(np.float32)
    before = np.concatenate([np.zeros((n, 1)), np.cumsum(e[:, :-1].astype(np.float64), axis=1)], axis=1)
    return delta, e, before


def sel_in_band(sigma, z) -> np.ndarray:
    delta, _, before = sel_parts(sigma, z)
    return ((sigma > 0) & (delta > 0) & (before > 95.0) & (before < 125.0)).any(axis=1)


@functools.lru_cache(maxsize=None)
def make_sel_inputs(case: SelCase) -> SelInputs:
    rng = np.random.default_rng(_seed("sel-" + case.id))
    n, s = case.n_rays, case.s
    sigma, z = _sel_draw(rng, case, n, True)
    count = np.zeros(n, dtype=np.int64)
    while True:
        idx = np.nonzero(sel_in_band(sigma, z))[0]
        if idx.size == 0:
            break
        count[idx] += 1
        assert count.max() < MAX_REDRAWS, f"{case.id}: a ray drawn {MAX_REDRAWS} times without leaving the band"
        for i in idx:
            sg, zz = _sel_draw(rng, case, 1, i == 0)
            sigma[i], z[i] = sg[0], zz[0]
    redrawn = int((count > 0).sum())
    assert redrawn <= max(REDRAW_SHARE * n, 0.0) or n < 20 and redrawn <= 1, f"{case.id}: {redrawn} of {n} rays redrawn"
    weights = O.volsdf_weights(torch.from_numpy(z), torch.from_numpy(sigma), False).numpy().astype(np.float32)
    dirs = rng.standard_normal((n, 3)).astype(np.float32)
    points = (rng.standard_normal((n, 1, 3)).astype(np.float32) + z[:, :, None] * dirs[:, None, :]).astype(np.float32)
    return SelInputs(case, weights, sigma, z, points, dirs, redrawn, int(count.max()))


def select_reference(weights, sigma, z, points, dirs, training: bool):
    """-> (index [K] int32 ascending in ray S + j, points_sel [K,3], dirs_sel [K,3]).  Forward: w > 0.  Training: w > 0 or
    (sigma > 0 and delta > 0 and before < 110)."""
    n, s = weights.shape
    sel = weights > 0
    if training:
        delta, _, before = sel_parts(sigma, z)
        sel = sel | ((sigma > 0) & (delta > 0) & (before < 110.0))
    index = np.nonzero(sel.reshape(-1))[0].astype(np.int32)
    return index, points.reshape(-1, 3)[index], dirs[index // s]


def sel_failures(case: SelCase, training: bool, count: int, index: np.ndarray, points_sel: np.ndarray, dirs_sel: np.ndarray) -> List[str]:
    """``index``: the whole [N S] buffer, which held SENTINEL everywhere before the call; points_sel / dirs_sel: at least ``count`` rows."""
    inp = make_sel_inputs(case)
    want, wp, wd = select_reference(inp.weights, inp.sigma, inp.z, inp.points, inp.dirs, training)
    bad = []
    if count != want.size:
        bad.append(f"count {count}, expected {want.size}")
    k = min(max(count, 0), index.size)
    if not np.array_equal(index[:k], want[:k]) or k != want.size:
        bad.append("the selected indices differ")
    if not bool((index[want.size:] == SENTINEL).all()):
        bad.append("entries past the count were written")
    if k == want.size and not (np.array_equal(points_sel[:k], wp) and np.array_equal(dirs_sel[:k], wd)):
        bad.append("the gathered points / directions differ")
    return bad


def sel_training_only(case: SelCase) -> int:
    """How many samples the training clause alone selects (what a too narrow predicate would lose)."""
    inp = make_sel_inputs(case)
    a = select_reference(inp.weights, inp.sigma, inp.z, inp.points, inp.dirs, True)[0]
    b = select_reference(inp.weights, inp.sigma, inp.z, inp.points, inp.dirs, False)[0]
    return int(a.size - b.size)
