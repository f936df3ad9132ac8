"""The float64 margin checker (tests/grid_margins.py) has teeth: the fp32 oracle passes every check — which is what proves the margins wide
enough for the reference's own arithmetic — and each mutation of the oracle's output that stands for a kernel defect fails it.  CPU only.

Mutation -> the defect it stands for -> the GPU test of tests/test_hip_grid_margins.py that would trip on the real one:
  footprint index off by one   a wrong (j, k) -> LDS index inside one 8 x 64 footprint     test_divergence_margins
  a lost segment plane         the last plane of a march segment not written / not staged  test_divergence_margins
  a wrong side bit             a corner compared against the wrong anchor                  test_sides_margins
  a wrong tie-break            the wave reduction keeping the LAST maximum                 test_sides_margins
  zero instead of replicate    the clamped window fill reading zeros beyond a face         test_smoothing_margins
  a rotated tap ring           the register ring / weight index running backwards          test_smoothing_margins (asymmetric weights)
  a missing canon() fold       -0.0 and +0.0 hashed as two keys                            test_dedup_on_chosen_keys"""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import vfnerf_oracle as O  # noqa: E402
import grid_margins as GM  # noqa: E402
from helpers import divergence_seg_len, per_point_scale, surface_field, synthetic_field  # noqa: E402

FIELDS = {"surface70": (70, lambda: surface_field(70)), "synthetic64": (64, lambda: synthetic_field(64, 64))}
_cache = {}


def stages(name):
    """(n, pred, oracle mask, unit field, oracle side table) of a field, computed once."""
    if name not in _cache:
        n, make = FIELDS[name]
        pred = make()
        div = O.grid_divergence(pred, n)
        unit = torch.nn.functional.normalize(pred, dim=1)
        choice = O.grid_unify_direction(div, unit.reshape(n, n, n, 3).permute(3, 0, 1, 2), n)
        _cache[name] = (n, pred, div, unit, choice)
    return _cache[name]


@pytest.mark.parametrize("name", list(FIELDS))
def test_oracle_divergence_passes_and_the_band_is_thin(name):
    n, pred, div, _, _ = stages(name)
    rep = GM.explain_divergence(div, pred, n)
    print(rep)
    assert rep.ok, str(rep)
    assert rep.surface > 0.005 * n ** 3 and rep.band_share <= GM.CAP_DIV_BAND, str(rep)
    assert float((GM.divergence_value(pred, n)[:-1, :-1, :-1]).abs().max()) <= 7.4
    # the mask depends on directions only: a per-point rescaling over nine decades leaves the oracle inside the same margins
    rep2 = GM.explain_divergence(O.grid_divergence(pred * per_point_scale(n ** 3, n), n), pred, n)
    assert rep2.ok, str(rep2)


@pytest.mark.parametrize("name", list(FIELDS))
def test_oracle_sides_pass_and_few_cells_are_ambiguous(name):
    n, pred, div, unit, choice = stages(name)
    rep = GM.explain_sides(choice, div, unit, n)
    print(rep)
    assert rep.ok, str(rep)
    assert rep.band_share <= GM.CAP_SIDES_AMBIGUOUS, str(rep)
    sides = GM.as_side_bytes(choice).to(torch.uint8)
    assert GM.explain_sides(sides, div, unit, n).ok                      # the byte form reads the same


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("k,sigma", [(3, 1.0), (9, 2.0), (5, 1.5)])
def test_oracle_smoothing_is_inside_the_bound(name, k, sigma):
    n, pred, _, _, _ = stages(name)
    worst = 0.0
    for scale in (1.0, 1e-3, None):
        x = (pred * (per_point_scale(n ** 3, 7) if scale is None else scale)).reshape(n, n, n, 3)
        ratio = GM.smooth_ratio(O.smooth_field(x, k, sigma), GM.smooth64(x, k, sigma), GM.smooth_bound(x, k, sigma))
        print(f"{name} k={k} scale={scale}: conv3d oracle err / bound = {ratio:.3f} (c_k = {GM.smooth_constant(k)})")
        worst = max(worst, ratio)
    # conv3d is one dense k^3-term accumulation: up to 1.37 c_9 here (the per-point-scaled field), inside c_k for k = 3 and 5; the allowance is that factor times 2.
    # (the separable fp32 arithmetic the kernels restate is held to c_k itself: test_fp32_separable_passes_are_inside_the_bound)
    assert worst <= GM.CONV3D_WIDEN and (k == 9 or worst <= 1.0), (k, worst)


def fp32_pass(x, w, axis):
    """One separable pass as the kernels sum it: fp32 weights, fp32 products and additions, taps in ascending order."""
    n, h = x.shape[axis], len(w) // 2
    acc = torch.zeros_like(x)
    for t, wt in enumerate(w):
        q = (torch.arange(n) + t - h).clamp(0, n - 1)
        acc = acc + torch.tensor(wt, dtype=torch.float32) * x.index_select(axis, q)
    return acc


@pytest.mark.parametrize("n", [2, 10, 24])
@pytest.mark.parametrize("k,sigma", [(3, 1.0), (9, 2.0), (5, 1.5), (15, 3.0)])
def test_fp32_separable_passes_are_inside_the_bound(n, k, sigma):
    """The arithmetic the kernels restate (not the kernels): single passes with an asymmetric weight vector and the three-pass Gaussian."""
    x = (surface_field(n) * per_point_scale(n ** 3, k)).reshape(n, n, n, 3)
    asym = [(t + 1.0) ** 2 for t in range(k)]
    asym = [a / sum(asym) for a in asym]
    for axis in range(3):
        got = fp32_pass(x, asym, axis)
        assert GM.smooth_ratio(got, GM.smooth64(x, k, sigma, axis, asym), GM.smooth_bound(x, k, sigma, axis, asym)) <= 1.0
    w = GM.gaussian_weights64(k, sigma)
    got = fp32_pass(fp32_pass(fp32_pass(x, w, 0), w, 1), w, 2)
    assert GM.smooth_ratio(got, GM.smooth64(x, k, sigma), GM.smooth_bound(x, k, sigma)) <= 1.0


def test_weights_agree_with_the_package():
    from vf_nerf_amd import grid
    for k, sigma in ((3, 1.0), (9, 2.0), (5, 1.5), (15, 3.0)):
        assert np.allclose(grid.gaussian_weights(k, sigma), GM.gaussian_weights64(k, sigma), rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------------------------------------
# mutations: every one must FAIL the checker
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIELDS))
def test_mutation_footprint_index_off_by_one_fails(name):
    n, pred, div, _, _ = stages(name)
    # the 8 x 64 footprint (rows j0..j0+7, columns 0..63) with the most surface cells, its mask shifted by one cell along k
    per_block = div[:, : n // 8 * 8, :64].reshape(n, n // 8, 8, 64).sum(dim=(0, 2, 3))
    j0 = int(per_block.argmax()) * 8
    bad = div.clone()
    bad[:, j0:j0 + 8, :64] = torch.roll(div[:, j0:j0 + 8, :64], 1, dims=2)
    assert not torch.equal(bad, div)
    rep = GM.explain_divergence(bad, pred, n)
    assert not rep.ok and rep.unexplained > 0, str(rep)


@pytest.mark.parametrize("name", list(FIELDS))
def test_mutation_lost_segment_plane_fails(name):
    n, pred, div, _, _ = stages(name)
    plane = divergence_seg_len(n) - 1
    assert 0 < plane < n - 1 and float(div[plane].sum()) > 0, "the plane must hold surface cells"
    bad = div.clone()
    bad[plane] = 0
    rep = GM.explain_divergence(bad, pred, n)
    assert not rep.ok and rep.unexplained > 0, str(rep)


def unambiguous_cells(n, div, unit):
    """Flat indices of surface cells no pair / corner of which lies inside a band, and the float64 decision of every surface cell."""
    sel = torch.nonzero(div.reshape(-1) == 1).reshape(-1)
    cells = torch.nonzero(div == 1)
    up = GM.pad_unit(unit, n)
    sv = torch.stack([up[cells[:, 0] + a, cells[:, 1] + b, cells[:, 2] + c] for a, b, c in GM.CORNERS], dim=1).double()
    dist, first, delta, bits = GM.float64_sides(sv)
    gap = dist.max(dim=1, keepdim=True)[0] - dist
    amb = ((gap > 0) & (gap <= GM.TAU_PAIR)).any(dim=1) | ((delta != 0) & (delta.abs() <= GM.TAU_SIDE)).any(dim=1)
    return sel, ~amb, sv, first, bits


@pytest.mark.parametrize("name", list(FIELDS))
def test_mutation_wrong_side_bit_fails(name):
    n, pred, div, unit, choice = stages(name)
    sel, clear, _, _, _ = unambiguous_cells(n, div, unit)
    for pick, corner in ((0, 0), (len(sel) // 2, 5), (-1, 7)):
        cell = int(sel[clear][pick])
        bad = choice.clone()
        bad[cell, corner] ^= 1
        rep = GM.explain_sides(bad, div, unit, n)
        assert not rep.ok and rep.unexplained == 1, str(rep)
    stray = choice.clone()
    stray[int(torch.nonzero(div.reshape(-1) != 1)[3]), 2] = 1            # a side bit on a non-surface cell
    assert not GM.explain_sides(stray, div, unit, n).ok


@pytest.mark.parametrize("name", list(FIELDS))
def test_mutation_wrong_tie_break_fails(name):
    """A cell with an exactly-zero vector among its corners, resolved to the LAST maximum of its pair distances (the mirror pair (b, a) of the
    first maximum (a, b) is an exact tie in any arithmetic): every decided corner flips.  Ties are not ambiguity."""
    n, pred, div, unit, choice = stages(name)
    sel, clear, sv, first, bits = unambiguous_cells(n, div, unit)
    has_zero = (sv == 0).all(dim=2).any(dim=1)
    rows = torch.nonzero(clear & has_zero).reshape(-1)
    assert rows.numel() > 0, "the field must hold surface cells with a zero corner vector"
    for r in rows.tolist():
        dist = GM.float64_sides(sv[r:r + 1])[0][0]
        last = int(torch.nonzero(dist == dist.max()).max())
        _, flipped = GM._side_bits(sv[r:r + 1], torch.tensor([last // 8]), torch.tensor([last % 8]))
        if last != int(first[r]) and not torch.equal(flipped[0], bits[r]):
            break
    else:
        raise AssertionError("no cell whose last maximum decides differently")
    bad = choice.clone()
    bad[int(sel[r])] = flipped[0]
    rep = GM.explain_sides(bad, div, unit, n)
    assert not rep.ok and rep.unexplained == 1, str(rep)
    # ... and the oracle itself resolved that cell by the rule
    assert torch.equal(choice[int(sel[r])], bits[r])


@pytest.mark.parametrize("k,sigma", [(3, 1.0), (9, 2.0)])
def test_mutation_zero_instead_of_replicate_padding_fails(k, sigma):
    n, pred, _, _, _ = stages("surface70")
    x = pred.reshape(n, n, n, 3)
    want, bound = GM.smooth64(x, k, sigma), GM.smooth_bound(x, k, sigma)
    good = O.smooth_field(x, k, sigma)
    assert GM.smooth_ratio(good, want, bound) <= GM.CONV3D_WIDEN
    # the same smoothing with zeros beyond the face j = 0 only
    h = k // 2
    padded = torch.nn.functional.pad(x.permute(3, 0, 1, 2).unsqueeze(0), (h,) * 6, mode="replicate")
    padded[:, :, :, :h, :] = 0
    ax = torch.arange(k, dtype=torch.float32)
    g = torch.exp(-(((ax - (k - 1) / 2.0) / (2 * sigma)) ** 2))
    kern = g[:, None, None] * g[None, :, None] * g[None, None, :]
    w = (kern / kern.sum()).view(1, 1, k, k, k).repeat(3, 1, 1, 1, 1)
    bad = torch.nn.functional.conv3d(padded, w, groups=3).squeeze(0).permute(1, 2, 3, 0)
    assert GM.smooth_ratio(bad[:, h:], want[:, h:], bound[:, h:]) <= GM.CONV3D_WIDEN       # only the face differs
    assert GM.smooth_ratio(bad, want, bound) > 1000.0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_mutation_rotated_tap_ring_fails(axis):
    """Reversed taps are invisible to a symmetric (Gaussian) weight vector and plain with an asymmetric one."""
    n, pred, _, _, _ = stages("synthetic64")
    x = pred.reshape(n, n, n, 3)[:24, :24, :24].contiguous()
    w = [0.1, 0.2, 0.7]
    want, bound = GM.smooth64(x, 3, 1.0, axis, w), GM.smooth_bound(x, 3, 1.0, axis, w)
    assert GM.smooth_ratio(fp32_pass(x, w, axis), want, bound) <= 1.0
    assert GM.smooth_ratio(fp32_pass(x, w[::-1], axis), want, bound) > 1.0
    assert GM.smooth_ratio(fp32_pass(x, [0.7, 0.1, 0.2], axis), want, bound) > 1.0          # rotated by one
    g = GM.gaussian_weights64(3, 1.0)
    assert GM.smooth_ratio(fp32_pass(x, g[::-1], axis), GM.smooth64(x, 3, 1.0, axis), GM.smooth_bound(x, 3, 1.0, axis)) <= 1.0   # hidden


def test_mutation_missing_canon_fold_fails():
    """The dict-side mutation of the dedup reference: keyed on raw bits (no -0.0 -> +0.0 fold) it disagrees with the reference on the
    signed-zero keys the GPU test drives the table with — and on nothing else."""
    for name, rows in GM.dedup_cases(big=False):
        v, ids = GM.dedup_reference(rows)
        v2, ids2 = GM.dedup_reference(rows, fold_zero=False)
        same = v.shape == v2.shape and np.array_equal(ids, ids2)
        if name in ("signed_zeros", "denormals_and_extremes"):
            assert not same, name
        else:
            assert same and np.array_equal(v.view(np.uint64), v2.view(np.uint64)), name
    rows = dict(GM.dedup_cases(big=False))["signed_zeros"]
    v, ids = GM.dedup_reference(rows)
    assert np.signbit(v[0, 0]) and not np.signbit(v[1, 0]) and len(v) == 7          # the first occurrence's sign bits are the ones stored
    assert np.array_equal(v[ids], rows)                                              # float equality: -0.0 == 0.0


# ------------------------------------------------------------------------------------------------------------------------
# smoothed meshes: the recorded (reference) norms lie inside the tolerance the device is held to
# ------------------------------------------------------------------------------------------------------------------------
def test_recorded_smoothed_norms_are_inside_the_norm_tolerance():
    from test_mesh_host import FIX, TABLES, field_inputs
    seen = 0
    for tag in (str(t) for t in FIX["index.fields"]):
        after, all_ = tag.endswith(".after"), tag.endswith(".all")
        if not (after or all_):
            continue
        res, sides, norms = field_inputs(tag)
        norm64, _, tol = GM.smoothed_norm_reference(torch.from_numpy(FIX[f"f{res}.pred"]), res, after, all_)
        err = (torch.from_numpy(np.asarray(norms)).double() - norm64).abs()
        print(f"{tag}: conv3d norms err / tol = {float((err / tol).max()):.3f}, smallest norm {float(norm64.min()):.4f}")
        assert bool((err <= tol).all()), tag
        cut, band, _ = GM.edge_snap_margin(sides, norms, res, float((2 * tol / norm64).max()), TABLES[1])
        assert cut > 100 and band == 0, (tag, cut, band)
        seen += 1
    assert seen >= 2
