"""Float64 margins for the dense-grid stages (csrc/vfn_grid.hip) and the smoothed meshes: a restatement in float64 of the quantities the
kernels DECIDE on, fed with the fp32 inputs widened exactly, so that every difference to it is the arithmetic's and not the data's.

A thresholded / argmax'ed output of an fp32 kernel may differ from the float64 decision only where the deciding quantity lies within
the rounding of the fp32 expression of the boundary; the ``explain_*`` functions assert exactly that, cell by cell, instead of counting
mismatches.  Written from the expressions of oracle/vfnerf_oracle.py (grid_divergence, grid_unify_direction, smooth_field) and the
kernel comments; plain torch, on whatever device the inputs live (the host tests run it on the CPU, the GPU tests may keep res^3
float64 temporaries on the device).  Not part of the package: tests only (a helper like mesh_restatement.py).

Tolerances (derivations in DESIGN.md, "Grid-stage tolerances"):
  TAU_DIV  = 2^-17   the flux: eight terms x|x| sqrt(3)/4 with |x| <= 1, about 12 fp32 roundings each, 9 on the sum, |value| <= 7.4
  TAU_PAIR = 2^-19   a pair distance 1 - <a, b>: five roundings on values <= 2; a difference of two of them
  TAU_SIDE = 2^-19   d1 - d2 of two corner distances, each the sqrt of three squares of values <= 2
  c_k = 3 (k + 2)    smoothing: per pass a k-term sum of non-negative weights is within (k + 1) 2^-24 of sum w |x|, plus one rounding of
                     each fp32 weight; three passes.  A single pass: (k + 2).
Caps on the share of cells that may sit inside a band at all (a kernel must not hide behind ambiguity): see CAP_*."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

TAU_DIV = 2.0 ** -17
TAU_PAIR = 2.0 ** -19
TAU_SIDE = 2.0 ** -19
CAP_DIV_BAND = 1e-3          # of the surface cells
CAP_SIDES_AMBIGUOUS = 1e-2   # of the surface cells
CAP_SNAP_BAND = 1e-2         # of the cut edges
U32 = 2.0 ** -24             # unit roundoff of fp32
# The reference's smoothing is ONE dense conv3d: k^3 products in a single fp32 accumulation, not three k-term passes, so c_k (derived for
# separable passes) does not cover it: on the host test fields it lies up to 1.37 c_9 from float64 (k = 9; inside c_k for k = 3, 5).
# Wherever the comparand is the reference's conv3d (the oracle's smooth_field, the recorded norms of smoothed fields) the bound is
# widened by that factor times 2.  The kernels sum separably and are held to c_k itself.
CONV3D_WIDEN = 2.8

CORNERS = ((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1), (1, 0, 1))   # the selection-filter order


@dataclass
class Report:
    ok: bool
    what: str
    cells: int = 0               # cells looked at
    surface: int = 0             # surface cells among them
    differing: int = 0           # cells where the output differs from the float64 decision
    worst_margin: float = 0.0    # largest margin of a differing cell
    band: int = 0                # cells inside the band (divergence) / ambiguous cells (sides)
    unexplained: int = 0
    examples: List[str] = field(default_factory=list)

    @property
    def band_share(self) -> float:
        return self.band / max(1, self.surface)

    def __str__(self) -> str:
        return (f"{self.what}: {'ok' if self.ok else 'FAILED'}; {self.cells} cells, {self.surface} surface, {self.differing} differ from float64 "
                f"(worst margin {self.worst_margin:.3e}), {self.band} in the band (share {self.band_share:.2e}), {self.unexplained} unexplained"
                + ("; " + "; ".join(self.examples) if self.examples else ""))


# ------------------------------------------------------------------------------------------------------------------------
# divergence
# ------------------------------------------------------------------------------------------------------------------------
def flux_block(v: torch.Tensor) -> torch.Tensor:
    """v[A,B,C,3] (fp32 field, any block of the grid) -> float64 [A-1,B-1,C-1]: the flux of the normalised field through the eight
    corners of every cell whose corners all lie in the block: sum_c x_c |x_c| (sqrt(3)/4) / (sqrt(2)/3), x_c = <u, outward diagonal>."""
    v = v.double()
    u = v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    a_, b_, c_ = (s - 1 for s in v.shape[:3])
    s = torch.zeros(a_, b_, c_, dtype=torch.float64, device=v.device)
    r3 = 1.0 / math.sqrt(3.0)
    for c in range(8):
        a, b, cc = c >> 2, (c >> 1) & 1, c & 1
        blk = u[a:a + a_, b:b + b_, cc:cc + c_]
        x = (blk[..., 0] * (2 * a - 1) + blk[..., 1] * (2 * b - 1) + blk[..., 2] * (2 * cc - 1)) * r3
        s += x * x.abs()
    return s * (math.sqrt(3.0) / 4.0) / (math.sqrt(2.0) / 3.0)


def divergence_value(pred: torch.Tensor, n: int) -> torch.Tensor:
    """pred[n^3,3] fp32 -> float64 [n,n,n]: the flux per cell before thresholding; the last planes (no cell there) are 0."""
    out = torch.zeros(n, n, n, dtype=torch.float64, device=pred.device)
    if n > 1:
        out[:-1, :-1, :-1] = flux_block(pred.reshape(n, n, n, 3))
    return out


def explain_divergence(mask: torch.Tensor, pred: Optional[torch.Tensor], n: int, tau: float = TAU_DIV, threshold: float = -0.5,
                       value: Optional[torch.Tensor] = None, what: str = "divergence") -> Report:
    """mask: the kernel's 0 / 1 output; passes iff every cell where it differs from ``value64 <= threshold`` has |value64 - threshold| <= tau
    and every entry is exactly 0.0 or 1.0.  ``value`` (float64, same shape as mask) replaces divergence_value(pred, n) for blocks."""
    if value is None:
        value = divergence_value(pred, n)
    mask = mask.reshape(value.shape).to(value.device)
    want = value <= threshold
    binary = bool(((mask == 0) | (mask == 1)).all())
    diff = (mask == 1) != want
    margin = (value - threshold).abs()
    worst = float(margin[diff].max()) if bool(diff.any()) else 0.0
    rep = Report(ok=binary and worst <= tau, what=what, cells=value.numel(), surface=int(want.sum()), differing=int(diff.sum()),
                 worst_margin=worst, band=int((margin <= tau).sum()), unexplained=int((diff & (margin > tau)).sum()))
    if not binary:
        rep.examples.append("entries other than 0.0 / 1.0")
    for idx in torch.nonzero(diff & (margin > tau))[:4].tolist():
        rep.examples.append(f"cell {tuple(idx)}: value64 {float(value[tuple(idx)]):.9f}, mask {float(mask[tuple(idx)])}")
    return rep


# ------------------------------------------------------------------------------------------------------------------------
# sides
# ------------------------------------------------------------------------------------------------------------------------
def as_side_bytes(sides_or_choice: torch.Tensor) -> torch.Tensor:
    """uint8 side bytes [M], or the int64 [M,8] table (entries must be 0 / 1) -> int64 [M] with bit q = corner q's side."""
    t = sides_or_choice
    if t.dim() == 2:
        if t.shape[1] != 8 or not bool(((t == 0) | (t == 1)).all()):
            raise AssertionError("the choice table must be [M,8] with entries 0 / 1")
        return (t.long() << torch.arange(8, device=t.device)).sum(dim=1)
    return t.long()


def pad_unit(unit: torch.Tensor, n: int) -> torch.Tensor:
    """unit[n^3,3] -> [n+1,n+1,n+1,3]: zero beyond the grid, as the reference's zero padding."""
    out = torch.zeros(n + 1, n + 1, n + 1, 3, dtype=unit.dtype, device=unit.device)
    out[:n, :n, :n] = unit.reshape(n, n, n, 3)
    return out


def _side_bits(sv: torch.Tensor, f: torch.Tensor, s: torch.Tensor):
    """sv[m,8,3] float64, anchors f, s [m] -> (d1 - d2 [m,8], bit [m,8]: 1 where the corner is strictly nearer to the second anchor)."""
    ar = torch.arange(sv.shape[0], device=sv.device)
    d1 = (sv[ar, f][:, None, :] - sv).norm(dim=-1)
    d2 = (sv[ar, s][:, None, :] - sv).norm(dim=-1)
    return d1 - d2, (d2 < d1).long()


def float64_sides(sv: torch.Tensor):
    """sv[m,8,3] -> (dist[m,64] float64 pair distances in a-major order, first[m] index of the first maximum, delta[m,8], bits[m,8])."""
    sv = sv.double()
    a, b = sv[:, :, None, :], sv[:, None, :, :]
    dist = (1.0 - ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])).reshape(-1, 64)
    top = dist.max(dim=1, keepdim=True)[0]
    idx = torch.arange(64, device=sv.device).expand_as(dist)
    first = torch.where(dist == top, idx, torch.full_like(idx, 64)).min(dim=1)[0]       # the FIRST maximum, whatever argmax does on ties
    delta, bits = _side_bits(sv, first // 8, first % 8)
    return dist, first, delta, bits


def explain_sides_block(bits: torch.Tensor, div: torch.Tensor, unit_padded: torch.Tensor, tau_pair: float = TAU_PAIR,
                        tau_side: float = TAU_SIDE, what: str = "sides") -> Report:
    """bits[A,B,C] (side byte per cell), div[A,B,C] (the mask the kernel was given), unit_padded[A+1,B+1,C+1,3] (the normalised fp32 field
    the kernel was given, with the next plane in every direction, zeros beyond the grid).  See explain_sides."""
    a_, b_, c_ = div.shape
    bits = bits.reshape(div.shape).long()
    sel = div == 1
    stray = int((bits[~sel] != 0).sum())
    cells = torch.nonzero(sel)
    m = cells.shape[0]
    rep = Report(ok=stray == 0, what=what, cells=div.numel(), surface=m)
    if stray:
        rep.examples.append(f"{stray} non-surface cells with side bits")
    if m == 0:
        return rep
    sv = torch.stack([unit_padded[cells[:, 0] + a, cells[:, 1] + b, cells[:, 2] + c] for a, b, c in CORNERS], dim=1).double()   # [m,8,3]
    got = (bits[sel][:, None] >> torch.arange(8, device=bits.device)) & 1                                                        # [m,8]
    dist, first, delta, want = float64_sides(sv)
    top = dist.max(dim=1, keepdim=True)[0]
    gap = top - dist
    ambiguous = ((gap > 0) & (gap <= tau_pair)).any(dim=1) | ((delta != 0) & (delta.abs() <= tau_side)).any(dim=1)
    differs = (got != want).any(dim=1)
    rep.differing, rep.band = int(differs.sum()), int(ambiguous.sum())
    bad = differs & ~ambiguous                                     # an unambiguous cell equals the float64 decision bit for bit
    # an ambiguous cell must still be explainable: some candidate pair inside the band (the first of its group of exactly equal
    # distances: exact ties resolve by order, not by rounding) for which every corner outside its own band has the kernel's bit
    amb = torch.nonzero(ambiguous & differs).reshape(-1)
    if amb.numel():
        sva, gota, dista, gapa = sv[amb], got[amb], dist[amb], gap[amb]
        explained = torch.zeros(amb.numel(), dtype=torch.bool, device=sv.device)
        for p in range(64):
            cand = gapa[:, p] <= tau_pair
            if p:
                cand &= ~(dista[:, :p] == dista[:, p:p + 1]).any(dim=1)
            if not bool(cand.any()):
                continue
            full = torch.full((amb.numel(),), p, device=sv.device)
            d, w = _side_bits(sva, full // 8, full % 8)
            in_band = (d != 0) & (d.abs() <= tau_side)
            explained |= cand & (in_band | (w == gota)).all(dim=1)
        bad[amb[~explained]] = True
    if bool(differs.any()):
        # the margin of a differing cell: what separates the kernel's decision from the float64 one (the smaller of the pair gap to the
        # nearest other candidate and the smallest |d1 - d2| among the corners that differ)
        dd = torch.where(got != want, delta.abs(), torch.full_like(delta, float("inf"))).min(dim=1)[0]
        g2 = torch.where(gap > 0, gap, torch.full_like(gap, float("inf"))).min(dim=1)[0]
        rep.worst_margin = float(torch.minimum(dd, g2)[differs].max())
    rep.unexplained = int(bad.sum())
    rep.ok = rep.ok and rep.unexplained == 0
    for r in torch.nonzero(bad).reshape(-1)[:4].tolist():
        rep.examples.append(f"cell {tuple(cells[r].tolist())}: bits {int(bits[sel][r]):08b}, float64 "
                            f"{int((want[r] << torch.arange(8, device=want.device)).sum()):08b}, first maximum pair {int(first[r]) // 8},{int(first[r]) % 8}")
    return rep


def explain_sides(sides_or_choice: torch.Tensor, div: torch.Tensor, unit: torch.Tensor, n: int, tau: float = TAU_PAIR,
                  tau_side: Optional[float] = None, what: str = "sides") -> Report:
    """Per surface cell (div == 1), in float64: the 64 pair distances 1 - ((a0 b0 + a1 b1) + a2 b2) of its eight corner vectors, their first
    maximum (a-major), and per corner d1 - d2 to the two anchors.  A cell is AMBIGUOUS iff some pair lies within (0, tau] below the maximum
    or some corner has 0 < |d1 - d2| <= tau_side.  Exact float64 ties are not ambiguous: they resolve by the reference's rules (first
    maximum, first anchor).  Unambiguous cells must equal the float64 decision bit for bit; an ambiguous cell must be explainable by a
    candidate pair inside the band; non-surface cells must be 0.  ``unit``: the normalised fp32 field [n^3,3] the kernel was given."""
    bits = as_side_bytes(sides_or_choice).reshape(n, n, n)
    return explain_sides_block(bits, div.reshape(n, n, n).to(bits.device), pad_unit(unit, n).to(bits.device), tau,
                               tau if tau_side is None else tau_side, what)


# ------------------------------------------------------------------------------------------------------------------------
# smoothing
# ------------------------------------------------------------------------------------------------------------------------
def gaussian_weights64(k: int, sigma: float) -> List[float]:
    """The 1-D factor of the reference's kernel: exp(-((x - mean) / (2 sigma))^2), normalised to sum 1 (guassian_smoothing.py:81-97)."""
    mean = (k - 1) / 2.0
    w = [math.exp(-(((i - mean) / (2.0 * sigma)) ** 2)) for i in range(k)]
    tot = math.fsum(w)
    return [x / tot for x in w]


def smooth_pass64(x: torch.Tensor, weights: Sequence[float], axis: int, lo: int = 0, n: Optional[int] = None,
                  out: Optional[Sequence[int]] = None) -> torch.Tensor:
    """One pass along ``axis`` in float64 with replicate padding.  ``x`` holds positions [lo, lo + x.shape[axis]) of an axis of length
    ``n`` (default: the whole axis); ``out``: the positions to produce (default: all of them) — every clamped tap must lie in the block."""
    size = x.shape[axis]
    n = size if n is None else n
    pos = torch.arange(lo, lo + size) if out is None else torch.as_tensor(list(out))
    k, h = len(weights), len(weights) // 2
    x = x.double()
    acc = None
    for t in range(k):
        q = (pos + (t - h)).clamp(0, n - 1) - lo
        assert int(q.min()) >= 0 and int(q.max()) < size, "a tap outside the block"
        term = x.index_select(axis, q.to(x.device)) * float(weights[t])
        acc = term if acc is None else acc + term
    return acc


def smooth64(vf: torch.Tensor, k: int, sigma: float, axis: Optional[int] = None, weights: Optional[Sequence[float]] = None) -> torch.Tensor:
    """vf[n,n,n,3] fp32 -> float64: three separable passes (``axis=None``) or the single pass along ``axis``, replicate padding, with
    the float64 Gaussian weights of (k, sigma) or the given ``weights``."""
    w = gaussian_weights64(k, sigma) if weights is None else list(weights)
    x = vf.double()
    for ax in ((0, 1, 2) if axis is None else (axis,)):
        x = smooth_pass64(x, w, ax)
    return x


def smooth_constant(k: int, passes: int = 3) -> float:
    return passes * (k + 2)


def smooth_bound(vf: torch.Tensor, k: int, sigma: float, axis: Optional[int] = None, weights: Optional[Sequence[float]] = None) -> torch.Tensor:
    """Elementwise bound on |fp32 smoothing - smooth64|: c 2^-24 smooth64(|vf|) with c = 3 (k + 2) for the three passes, (k + 2) for one.
    Scaled by the local smoothed MAGNITUDE: says as much at 1e-3 and at the zero crossing of the field as at 1."""
    w = gaussian_weights64(k, sigma) if weights is None else [abs(float(x)) for x in weights]
    return smooth_constant(len(w), 3 if axis is None else 1) * U32 * smooth64(vf.abs(), k, sigma, axis, w)


def smooth_ratio(got: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor) -> float:
    """max |got - want64| / bound over the elements (0 / 0 counts as 0, x / 0 as inf): passes iff <= 1."""
    err = (got.double().to(want64.device) - want64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------------
# meshes
# ------------------------------------------------------------------------------------------------------------------------
def triangle_corners(v, f):
    """vertices [V,3], faces [F,3] (0-based) -> [F,3,3]: the three corner positions of every triangle."""
    return v[f]


def edge_snap_margin(sides, norms, res: int, eps_norm: float, edge_vertex):
    """The ``|v1 - v2| > 1e-5`` switch of vertex_interpolate on the cut edges of the fused triangulation (side bytes + norms): corner value
    = +-norm (minus on the side of corner 0), an edge is cut when exactly one of its corner values is < 0.
    -> (cut: number of cut edges, band: those with ||v1 - v2| - 1e-5| <= 2 eps_norm max(|v1|, |v2|), segments [band,2,3]: their end points
    as grid indices).  numpy in, numpy out."""
    import numpy as np
    sides = np.asarray(sides).reshape(res, res, res).astype(np.int64)
    npad = np.zeros((res + 1, res + 1, res + 1), dtype=np.float64)
    npad[:res, :res, :res] = np.asarray(norms, dtype=np.float32).reshape(res, res, res)
    cells = np.argwhere((sides != 0) & (sides != 255))
    bits = sides[cells[:, 0], cells[:, 1], cells[:, 2]]
    b0 = bits & 1
    val = np.stack([np.where(((bits >> q) & 1) != b0, 1.0, -1.0) * npad[cells[:, 0] + a, cells[:, 1] + b, cells[:, 2] + c]
                    for q, (a, b, c) in enumerate(CORNERS)], axis=1)                       # [M,8]
    cut_n, segs = 0, []
    for e1, e2 in np.asarray(edge_vertex).tolist():
        v1, v2 = val[:, e1], val[:, e2]
        cut = (v1 < 0) != (v2 < 0)
        cut_n += int(cut.sum())
        band = cut & (np.abs(np.abs(v1 - v2) - 1e-5) <= 2.0 * eps_norm * np.maximum(np.abs(v1), np.abs(v2)))
        if band.any():
            c = cells[band]
            segs.append(np.stack([c + np.array(CORNERS[e1]), c + np.array(CORNERS[e2])], axis=1))
    segments = np.concatenate(segs) if segs else np.zeros((0, 2, 3), dtype=np.int64)
    return cut_n, len(segments), segments


def corners_on_segments(corners, segments, res: int, size: float = 2.0):
    """corners [F,3,3] positions, segments [B,2,3] grid indices -> bool [F,3]: the corner lies on one of the grid edges (to 1e-9)."""
    import numpy as np
    out = np.zeros(corners.shape[:2], dtype=bool)
    for seg in np.asarray(segments, dtype=np.float64) / res * size - size / 2:
        p, q = seg
        d = q - p
        t = np.clip(((corners - p) @ d) / (d @ d), 0.0, 1.0)
        out |= np.linalg.norm(corners - (p + t[..., None] * d), axis=-1) < 1e-9
    return out


def smoothed_norm_reference(pred, res: int, smooth_after: bool, smooth_all: bool):
    """The norms evaluation/methods.py:212-226 takes of a smoothed field, in float64, and how far an fp32 evaluation may be from them.
    pred[res^3,3] fp32 -> (norm64 [res^3], tol [res^3] for separable fp32 passes, tol_conv3d [res^3] for the
    reference's dense conv3d, see CONV3D_WIDEN).  Smoothing: k = 3, sigma 1 first if smooth_all, then k = 9, sigma 2; each fp32
    smoothing is within its smooth_bound B of the float64 one (componentwise), the bounds of a chain add up on the smoothed magnitudes:
    B = (c_3 + c_9) 2^-24 S9(S3 |x|), or c_9 2^-24 S9 |x|.  | |a| - |b| | <= |a - b|_2 <= |B|_2, and the fp32 norm itself (three squares,
    two additions, a square root) adds 4 x 2^-24 relative."""
    x = pred.reshape(res, res, res, 3)
    mag, val, c = x.abs().double(), x.double(), 0.0
    if smooth_all:
        val, mag, c = smooth64(val, 3, 1.0), smooth64(mag, 3, 1.0), c + smooth_constant(3)
    if smooth_after or smooth_all:
        val, mag, c = smooth64(val, 9, 2.0), smooth64(mag, 9, 2.0), c + smooth_constant(9)
    norm64 = val.norm(dim=-1).reshape(-1)
    smoothing, rounding = c * U32 * mag.norm(dim=-1).reshape(-1), 4.0 * U32 * norm64
    return norm64, smoothing + rounding, CONV3D_WIDEN * smoothing + rounding


# ------------------------------------------------------------------------------------------------------------------------
# vertex deduplication on chosen keys
# ------------------------------------------------------------------------------------------------------------------------
def dedup_reference(rows, fold_zero: bool = True):
    """rows [S,3] float64 (numpy) -> (vertices [V,3], ids [S]): a Python dict over tuple(row) — float equality, so -0.0 and +0.0 are one
    key — ids in order of first appearance, the first occurrence's raw bits kept.  ``fold_zero=False`` keys on the raw bits instead: the
    defect of a table without the canon() fold (host tests only)."""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 3)
    keys = rows.tolist() if fold_zero else rows.view(np.uint64).tolist()
    ids, first, out = {}, [], []
    for s, key in enumerate(map(tuple, keys)):
        i = ids.get(key)
        if i is None:
            i = ids[key] = len(first)
            first.append(s)
        out.append(i)
    return rows[np.array(first, dtype=np.int64)].reshape(-1, 3), np.array(out, dtype=np.int64)


def dedup_cases(big: bool = True):
    """(name, rows [S,3] float64) of the hand-made slot lists (no non-finite keys: refusing those is the count kernel's job)."""
    import numpy as np
    rng = np.random.default_rng(20240817)
    cases = [("empty", np.zeros((0, 3))), ("three", np.array([[0.5, -0.25, 1.0], [0.5, -0.25, 1.0], [1.0, 0.5, -0.25]]))]
    # signed zeros: in each coordinate alone and in all three; one key each, the FIRST one's sign bits stored
    z = []
    for c in range(3):
        for i, first in enumerate((-0.0, 0.0)):
            a = [1.5 + c + 0.25 * i] * 3
            b = list(a)
            a[c], b[c] = first, -first
            z += [a, b, a, b]
    z += [[-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [0.0, -0.0, 0.0], [-0.0, 0.0, -0.0], [0.0, 0.0, -0.0]]
    cases.append(("signed_zeros", np.array(z)))
    # the lowest mantissa bit of one coordinate: distinct keys
    base = np.array([0.1, -0.7, 3.0])
    low = [base.copy()]
    for c in range(3):
        for nxt in (np.inf, -np.inf):
            r = base.copy()
            r[c] = np.nextafter(r[c], nxt)
            low.append(r)
    low = np.array(low)
    cases.append(("low_bit", np.concatenate([low, low[::-1], low])))
    tiny, huge = 5e-324, 1.8e308
    ext = np.array([[tiny, 0.0, 0.0], [-tiny, 0.0, 0.0], [0.0, tiny, -tiny], [2 * tiny, tiny, tiny], [2.2250738585072014e-308, tiny, 0.0],
                    [huge, -huge, huge], [-huge, huge, -huge], [huge, huge, np.nextafter(huge, 0.0)], [tiny, -0.0, 0.0], [huge, -huge, huge]])
    cases.append(("denormals_and_extremes", np.concatenate([ext, ext[::-1]])))
    # a few thousand keys, each repeated 1-64 times, shuffled
    keys = rng.standard_normal((3000, 3))
    rep = np.repeat(np.arange(3000), rng.integers(1, 65, size=3000))
    rng.shuffle(rep)
    cases.append(("repeats_shuffled", keys[rep]))
    if big:
        cases.append(("one_key_everywhere", np.tile(np.array([[0.25, -0.0, 1e-300]]), (3 << 20, 1))))
        # all keys distinct: S = 2^20 is a load factor of exactly 0.5 (the bound vfn_mesh_dedup accepts), one under, one over (next table)
        for name, s in (("distinct_under_half", (1 << 20) - 1), ("distinct_at_half", 1 << 20), ("distinct_over_half", (1 << 20) + 1)):
            d = rng.standard_normal((s, 3))
            d[:, 0] = np.arange(s)                                # distinct by construction
            cases.append((name, d))
    return cases
