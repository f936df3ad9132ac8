"""The dense-grid kernels (csrc/vfn_grid.hip) and the vertex deduplication (csrc/vfn_mesh.hip) on the MI355X against the float64 margin
checker of tests/grid_margins.py: every decision the kernels take either equals the float64 decision or sits within the rounding of its
fp32 expression of the boundary, cell by cell; smoothing is held elementwise to a bound scaled by the local smoothed magnitude; the hash
table is driven with hand-made keys.  tests/test_grid_margins_host.py shows on the CPU that the checker fails on the kernel defects
these sizes are chosen for.  The float64 side of the res^3 comparisons is plain torch float64 on the device (the checker is device
agnostic); the 512^3 test computes it on the CPU from the planes its slabs depend on.  Every test prints the figures it asserts on
(pytest -s; recorded in profiles/r08/grid_margins.md)."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vf_nerf_amd import grid, lib  # noqa: E402
import grid_margins as GM  # noqa: E402
from helpers import divergence_seg_len, per_point_scale, smooth_seg_len, surface_field  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# 8 x 64 footprints whole (64, 72 in j), one past (65), partial in j and in k (9, 63, 131, 258); one and several march segments
SIZES = (2, 3, 9, 63, 64, 65, 72, 131, 258)
CAPS_FROM = 63
SMOOTH_SIZES = (1, 2, 3, 4, 8, 10, 64, 65, 70, 131, 258)     # N < k (all taps clamped); 3 N divisible by 4 and not; one and several segments
SMOOTH_KS = ((3, 1.0), (9, 2.0), (5, 1.5), (15, 3.0))         # register window / LDS rows (3, 9), the generic per-voxel kernel (5, 15)


def field(n, scaled):
    pred = surface_field(n)
    if scaled:
        pred = pred * per_point_scale(n ** 3, n)                  # every vector 10^U(-6, 3) times itself; zero vectors stay in
    return pred.to(DEV)


@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "scaled"])
@pytest.mark.parametrize("n", SIZES)
def test_divergence_margins(n, scaled):
    dp = field(n, scaled)
    keep = dp.clone()
    mask = grid.extract_divergence(dp, n)
    assert mask.shape == (n, n, n) and torch.equal(dp, keep)
    rep = GM.explain_divergence(mask, dp, n, what=f"divergence n={n} {'scaled' if scaled else 'unit'} seg_len={divergence_seg_len(n)}")
    print(rep)
    assert rep.ok, str(rep)
    assert float(mask[-1].abs().max()) == 0 and float(mask[:, -1].abs().max()) == 0 and float(mask[:, :, -1].abs().max()) == 0
    if n >= CAPS_FROM:
        assert rep.surface > 0.005 * n ** 3 and rep.band_share <= GM.CAP_DIV_BAND, str(rep)
    if scaled:
        # the mask depends on directions only: outside the band it is the mask of the unscaled field, bit for bit
        plain = surface_field(n).to(DEV)
        value = GM.divergence_value(plain, n)
        # the scaling rounds every component once (2^-24 relative): a direction moves by <= 2 sqrt(3) 2^-24 = 2.1e-7, the flux (eight
        # terms of slope 2 |x| (sqrt(3)/4) / (sqrt(2)/3) <= 1.84 each) by <= 3.1e-6, on top of the arithmetic's TAU_DIV: 2 TAU_DIV in all
        rep2 = GM.explain_divergence(mask, None, n, tau=2 * GM.TAU_DIV, value=value, what=f"divergence n={n} scaled, against the unscaled field's float64")
        print(rep2)
        assert rep2.ok, str(rep2)


@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "scaled"])
@pytest.mark.parametrize("n", SIZES)
def test_sides_margins(n, scaled):
    dp = field(n, scaled)
    mask = grid.extract_divergence(dp, n)                                     # the device's own mask
    unit = torch.nn.functional.normalize(dp, dim=1).contiguous()
    choice = grid.unify_direction(mask, unit.reshape(n, n, n, 3).permute(3, 0, 1, 2), N=n)
    assert choice.shape == (n ** 3, 8) and choice.dtype == torch.int64
    sides, none = lib.grid_unify_direction_sides(mask.reshape(-1), unit, n, want_table=False)
    assert none is None and sides.dtype == torch.uint8
    sides2, table = lib.grid_unify_direction_sides(mask.reshape(-1), unit, n, want_table=True)
    assert torch.equal(sides2, sides) and torch.equal(table, choice)
    assert torch.equal(GM.as_side_bytes(table), sides.long()), "byte == table"
    del table, sides2
    tag = f"n={n} {'scaled' if scaled else 'unit'}"
    rep = GM.explain_sides(choice, mask, unit, n, what=f"sides (unify_direction) {tag}")
    print(rep)
    assert rep.ok, str(rep)
    rep_b = GM.explain_sides(sides, mask, unit, n, what=f"sides (bytes, no table) {tag}")
    assert rep_b.ok and (rep_b.differing, rep_b.band) == (rep.differing, rep.band), str(rep_b)
    if n >= CAPS_FROM:
        assert rep.surface > 0.005 * n ** 3 and rep.band_share <= GM.CAP_SIDES_AMBIGUOUS, str(rep)


def smoothing_fields(n):
    """(name, [n,n,n,3] fp32 on the device) at scales 1e-3, 1, 1e3 and with a per-point scale over nine decades."""
    base = surface_field(n)
    base[0] = torch.tensor([0.3, -0.7, 1.1])                      # (n = 1 would otherwise be the all-zero field)
    out = [("1e-3", base * 1e-3), ("1", base), ("1e3", base * 1e3), ("per-point", base * per_point_scale(n ** 3, 31 * n + 1))]
    return [(name, x.reshape(n, n, n, 3).contiguous().to(DEV)) for name, x in out]


@pytest.mark.parametrize("k,sigma", SMOOTH_KS, ids=[f"k{k}" for k, _ in SMOOTH_KS])
@pytest.mark.parametrize("n", SMOOTH_SIZES)
def test_smoothing_margins(n, k, sigma):
    gauss = grid.gaussian_weights(k, sigma)
    asym = [(t + 1.0) ** 2 for t in range(k)]                     # asymmetric: a reversed or rotated tap ring shows
    asym = [a / sum(asym) for a in asym]
    worst = {}
    for name, x in smoothing_fields(n):
        keep = x.clone()
        flat = x.reshape(-1, 3)
        for axis in range(3):
            for wname, w in (("gauss", gauss), ("asym", asym)):
                out = torch.full_like(flat, float("nan"))
                lib.grid_smooth_axis(flat, out, n, axis, w)
                ratio = GM.smooth_ratio(out.reshape(n, n, n, 3), GM.smooth64(x, k, sigma, axis, w), GM.smooth_bound(x, k, sigma, axis, w))
                worst[(axis, wname)] = max(worst.get((axis, wname), 0.0), ratio)
                assert ratio <= 1.0, (name, axis, wname, ratio)
        sm = grid.smooth_vf(x, k=k, sigma=sigma)
        assert sm.shape == (n, n, n, 3) and sm.data_ptr() != x.data_ptr()
        ratio = GM.smooth_ratio(sm, GM.smooth64(x, k, sigma), GM.smooth_bound(x, k, sigma))
        worst["three passes"] = max(worst.get("three passes", 0.0), ratio)
        assert ratio <= 1.0, (name, "three passes", ratio)
        assert torch.equal(x, keep), "smoothing must not write into its input"
    print(f"smoothing n={n} k={k}: worst err / bound (single pass c = {GM.smooth_constant(k, 1)}, three passes c = {GM.smooth_constant(k)}): "
          + ", ".join(f"{key}: {v:.3f}" for key, v in worst.items()))
    with pytest.raises(lib.VfnError):
        lib.grid_smooth_axis(flat, flat, n, 0, gauss)              # in == out is refused


# ------------------------------------------------------------------------------------------------------------------------
# the evaluator's shipped 512^3, on slabs
# ------------------------------------------------------------------------------------------------------------------------
def planes_of(t, axis, planes):
    """Planes ``planes`` of a device tensor along ``axis`` -> CPU."""
    return t.index_select(axis, torch.as_tensor(planes, device=t.device)).cpu()


def slab_groups(n, boundary):
    """Three groups of consecutive planes: the first, one straddling ``boundary``, the last."""
    return [list(range(0, 3)), list(range(boundary - 2, boundary + 2)), list(range(n - 3, n))]


SHIPPED_N = 512      # the evaluator's resolution


def test_shipped_size_on_slabs():
    n = SHIPPED_N
    dp = surface_field(n, device=DEV)                                        # 1.6 GB, built on the device (its generator)
    x4 = dp.reshape(n, n, n, 3)
    mask = grid.extract_divergence(dp, n)
    unit = torch.nn.functional.normalize(dp, dim=1).contiguous()
    sides, _ = lib.grid_unify_direction_sides(mask.reshape(-1), unit, n, want_table=False)
    choice = grid.unify_direction(mask, unit.reshape(n, n, n, 3).permute(3, 0, 1, 2), N=n)
    assert torch.equal(GM.as_side_bytes(choice), sides.long())
    del choice
    assert float(mask[-1].abs().max()) == 0 and float(mask[:, -1].abs().max()) == 0 and float(mask[:, :, -1].abs().max()) == 0
    sides3, unit4 = sides.reshape(n, n, n), unit.reshape(n, n, n, 3)
    total = GM.Report(ok=True, what="512^3 divergence slabs")
    total_s = GM.Report(ok=True, what="512^3 sides slabs")
    for axis in range(3):
        boundary = (divergence_seg_len(n), 8 * (n // 16), 64 * (n // 128) or n // 2)[axis]      # a march segment (i), a footprint edge in j, in k
        for planes in slab_groups(n, boundary):
            more = planes + ([planes[-1] + 1] if planes[-1] + 1 < n else [])  # the next plane holds the far corners
            blk = planes_of(x4, axis, more)
            shape = [n, n, n]
            shape[axis] = len(planes)
            value = torch.zeros(shape, dtype=torch.float64)
            fl = GM.flux_block(blk)
            value[tuple(slice(0, s) for s in fl.shape)] = fl
            rep = GM.explain_divergence(planes_of(mask, axis, planes), None, n, value=value, what=f"512^3 divergence axis {axis} planes {planes[0]}..{planes[-1]}")
            print(rep)
            assert rep.ok, str(rep)
            up = torch.zeros([s + 1 for s in shape] + [3])
            ub = planes_of(unit4, axis, more)
            up[tuple(slice(0, s) for s in ub.shape[:3])] = ub
            rep_s = GM.explain_sides_block(planes_of(sides3, axis, planes), planes_of(mask, axis, planes), up,
                                           what=f"512^3 sides axis {axis} planes {planes[0]}..{planes[-1]}")
            print(rep_s)
            assert rep_s.ok, str(rep_s)
            for t, r in ((total, rep), (total_s, rep_s)):
                t.cells, t.surface, t.differing, t.band = t.cells + r.cells, t.surface + r.surface, t.differing + r.differing, t.band + r.band
                t.worst_margin = max(t.worst_margin, r.worst_margin)
    print(total, total_s, sep="\n")
    assert total.surface > 1000 and total.band_share <= GM.CAP_DIV_BAND, str(total)
    assert total_s.band_share <= GM.CAP_SIDES_AMBIGUOUS, str(total_s)
    del mask, unit, sides, sides3, unit4
    for k, sigma in ((9, 2.0), (3, 1.0)):
        sm = grid.smooth_vf(x4, k=k, sigma=sigma)
        w, h = GM.gaussian_weights64(k, sigma), k // 2
        worst = 0.0
        for axis in range(3):
            seg = smooth_seg_len(n, k, axis) if axis < 2 else n
            for planes in slab_groups(n, seg if seg < n else n // 2):
                need = list(range(max(0, planes[0] - h), min(n, planes[-1] + h + 1)))     # k = 9: 4 planes either side
                blk = planes_of(x4, axis, need)
                ref, mag = blk.double(), blk.abs().double()
                for ax in range(3):
                    kw = dict(lo=need[0], n=n, out=planes) if ax == axis else {}
                    ref, mag = GM.smooth_pass64(ref, w, ax, **kw), GM.smooth_pass64(mag, w, ax, **kw)
                ratio = GM.smooth_ratio(planes_of(sm, axis, planes), ref, GM.smooth_constant(k) * GM.U32 * mag)
                print(f"512^3 smooth_vf k={k} axis {axis} planes {planes[0]}..{planes[-1]}: worst err / bound {ratio:.3f}")
                worst = max(worst, ratio)
        assert worst <= 1.0, (k, worst)
        del sm
    assert float(x4[0, 0, 0].abs().sum()) == 0                                 # (every 997th vector is zero; the field is untouched)


# ------------------------------------------------------------------------------------------------------------------------
# vertex deduplication on chosen keys
# ------------------------------------------------------------------------------------------------------------------------
CASES = GM.dedup_cases()


@pytest.mark.parametrize("name,rows", CASES, ids=[c[0] for c in CASES])
def test_dedup_on_chosen_keys(name, rows):
    want_v, want_ids = GM.dedup_reference(rows)
    d = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 3)).to(DEV)
    v, ids = lib.mesh_dedup(d)
    v2, ids2 = lib.mesh_dedup(d)                                              # the owner must not depend on the arrival order
    assert v.dtype == torch.float64 and ids.dtype == torch.int64 and v.shape == (len(want_v), 3) and ids.shape == (len(rows),)
    assert torch.equal(v.view(torch.int64), v2.view(torch.int64)) and torch.equal(ids, ids2)
    assert np.array_equal(v.cpu().numpy().view(np.uint64), want_v.view(np.uint64)), "vertices: the first occurrence's bits, in order of first appearance"
    assert np.array_equal(ids.cpu().numpy(), want_ids)
    slots = len(rows)
    print(f"dedup {name}: {slots} slots -> {len(want_v)} vertices, table {1 << max(6, (2 * slots - 1).bit_length())}"
          f" (load factor {len(want_v) / (1 << max(6, (2 * slots - 1).bit_length())):.4f})")
