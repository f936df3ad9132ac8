"""vfn_ray_density_weights, vfn_ray_density_weights_bwd and vfn_ray_density_sigma_bwd against the oracle in float64, ray by ray.

Inputs, reference and scoring: tests/density_cases.py (checked on the host by tests/test_density_host.py).  Every error below is a
per-ray one, max |x - x64| / max |x64| over the ray's entries (scalar gradients: |x - x64| / sum_rays |ray's float64 contribution|);
a ray, or a scalar gradient, that is exactly zero in float64 must be exactly zero on the device.  No ray and no sample is skipped:
the inputs keep 1e-4 away from every discontinuity.

Bounds: 8 x the same oracle in float32 on the host against float64, computed here at run time on the very inputs of each case and
pooled over the cases of one family under one setting of the density scalars (DC.bound).  The factor covers what the host's float32
does not have: the device's expf / division / sqrtf, 64-lane tree sums against sequential ones, atomics in no fixed order.

Measured on an MI355X, worst ray of each pool: device | host-float32 yardstick (both against float64; the bound is 8 x the second
figure; "depth." and so on: that upstream gradient alone; "sigma.": the sigma entry point).  The device never measured more than
4.9 x its yardstick (d_scale with d_rgb alone, crossing under mean 1.2: 3.3e-07 against 6.8e-08).

  pool                  sigma               weights             rgb                 depth
  noise S<=3, shipped   8.8e-05 | 8.8e-05   1.7e-04 | 1.7e-04   1.7e-04 | 1.7e-04   1.7e-04 | 1.7e-04
  noise, shipped        2.8e-07 | 2.8e-07   3.4e-06 | 3.4e-06   1.4e-06 | 1.0e-06   1.8e-07 | 2.5e-07
  crossing, shipped     1.2e-06 | 1.2e-06   1.0e-05 | 7.0e-06   8.8e-06 | 4.8e-06   2.4e-06 | 2.4e-06
  empty, shipped        4.5e-06 | 4.5e-06   1.4e-04 | 1.5e-04   8.8e-05 | 8.8e-05   8.8e-05 | 8.8e-05
  crossing, mean 0.5    8.0e-07 | 8.0e-07   5.0e-06 | 5.0e-06   1.7e-06 | 1.7e-06   5.0e-07 | 6.0e-07
  crossing, mean 1.2    1.0e-06 | 1.1e-06   4.8e-06 | 2.2e-06   2.7e-06 | 1.4e-06   3.7e-07 | 3.5e-07
  crossing, scale -100  1.2e-06 | 1.2e-06   3.7e-06 | 3.6e-06   2.5e-06 | 2.5e-06   2.6e-06 | 1.9e-06
  crossing, scale 0.5   1.1e-06 | 1.1e-06   1.4e-04 | 1.4e-04   5.3e-05 | 5.3e-05   1.9e-05 | 1.0e-05
  noise, beta 0.05      2.2e-06 | 1.5e-06   1.1e-05 | 8.6e-06   9.8e-06 | 6.4e-06   4.1e-07 | 8.3e-07
  noise, beta 5e-05     9.9e-04 | 9.9e-04   3.5e-04 | 3.5e-04   1.1e-04 | 1.1e-04   5.3e-05 | 5.3e-05

  pool                  d_normals           d_colors            d_beta              d_mean              d_scale
  noise S<=3, shipped   2.9e-03 | 2.4e-03   1.7e-04 | 1.7e-04   3.7e-04 | 3.7e-04   3.4e-04 | 3.4e-04   3.4e-04 | 3.4e-04
  noise, shipped        6.4e-06 | 5.9e-06   3.4e-06 | 3.4e-06   8.3e-07 | 9.5e-07   1.5e-06 | 4.5e-06   4.2e-06 | 2.3e-06
  crossing, shipped     1.7e-04 | 3.7e-04   1.0e-05 | 7.0e-06   2.3e-06 | 7.4e-07   2.1e-06 | 7.8e-07   2.0e-06 | 9.2e-07
  empty, shipped        1.2e-03 | 1.0e-03   1.4e-04 | 1.5e-04   9.7e-05 | 5.4e-05   1.1e-04 | 5.6e-05   1.1e-04 | 5.6e-05
  crossing, mean 0.5    1.3e-04 | 5.7e-05   5.0e-06 | 5.0e-06   3.7e-07 | 2.8e-07   0 | 0               3.5e-07 | 2.2e-07
  crossing, mean 1.2    2.3e-05 | 1.0e-04   4.8e-06 | 2.2e-06   1.1e-07 | 4.1e-08   0 | 0               2.7e-07 | 3.5e-07
  crossing, scale -100  1.6e-05 | 2.1e-05   3.7e-06 | 3.6e-06   6.3e-07 | 3.8e-07   5.4e-07 | 3.5e-07   1.3e-06 | 1.3e-06
  crossing, scale 0.5   1.0e-03 | 1.0e-03   1.4e-04 | 1.4e-04   2.2e-05 | 2.1e-05   6.0e-05 | 6.4e-05   0 | 0
  noise, beta 0.05      1.8e-04 | 1.8e-04   1.1e-05 | 8.6e-06   7.2e-06 | 6.9e-06   3.0e-06 | 7.2e-06   9.7e-06 | 1.8e-05
  noise, beta 5e-05     1.8e-03 | 1.9e-03   3.5e-04 | 3.5e-04   0 | 0               2.2e-04 | 2.4e-04   1.5e-06 | 1.3e-05

  pool                  depth.d_normals     depth.d_beta        weights.d_normals   rgb.d_normals
  noise S<=3, shipped   2.7e-03 | 2.9e-03   4.5e-04 | 4.5e-04   2.9e-03 | 2.9e-03   1.9e-03 | 4.8e-03
  noise, shipped        1.0e-04 | 1.1e-04   6.7e-06 | 3.5e-06   4.0e-06 | 3.9e-06   6.4e-06 | 6.6e-06
  crossing, shipped     3.8e-03 | 3.8e-03   1.0e-06 | 1.4e-06   1.6e-04 | 1.7e-04   2.1e-04 | 5.6e-04
  empty, shipped        7.4e-04 | 7.4e-04   1.1e-04 | 1.2e-04   7.4e-04 | 7.4e-04   7.4e-04 | 7.4e-04
  crossing, mean 0.5    1.0e-03 | 5.2e-03   3.4e-07 | 4.5e-07   6.0e-05 | 6.0e-05   5.0e-05 | 4.6e-05
  crossing, mean 1.2    2.2e-04 | 2.7e-03   2.7e-07 | 3.3e-07   1.0e-05 | 1.2e-05   1.3e-05 | 5.5e-05
  crossing, scale -100  6.5e-04 | 2.3e-03   7.3e-07 | 1.0e-06   1.4e-05 | 1.2e-05   1.1e-05 | 1.1e-05
  crossing, scale 0.5   1.8e-03 | 2.1e-03   7.5e-05 | 2.6e-05   2.1e-03 | 1.7e-03   8.6e-04 | 8.5e-04
  noise, beta 0.05      2.9e-04 | 1.4e-04   1.8e-06 | 3.3e-06   2.0e-04 | 1.5e-04   9.2e-04 | 9.2e-04
  noise, beta 5e-05     1.8e-03 | 2.0e-03   0 | 0               1.7e-03 | 2.3e-03   3.1e-03 | 1.9e-03

  pool                  sigma.d_normals     sigma.d_beta        sigma.d_mean        sigma.d_scale
  noise S<=3, shipped   4.2e-07 | 9.0e-07   1.2e-07 | 7.0e-08   4.3e-08 | 5.7e-08   4.6e-08 | 1.9e-08
  noise, shipped        5.1e-07 | 7.2e-07   2.4e-07 | 1.5e-07   5.8e-08 | 5.8e-08   1.8e-07 | 3.9e-07
  crossing, shipped     1.5e-06 | 1.2e-06   1.5e-07 | 1.5e-07   1.5e-07 | 1.1e-07   3.2e-07 | 3.2e-07
  empty, shipped        4.3e-07 | 6.3e-07   1.6e-07 | 2.0e-07   1.6e-07 | 1.4e-07   3.9e-07 | 3.9e-07
  crossing, mean 0.5    7.6e-07 | 8.9e-07   5.2e-08 | 1.7e-08   0 | 0               6.0e-08 | 9.0e-08
  crossing, mean 1.2    6.7e-07 | 6.7e-07   3.5e-08 | 2.4e-08   0 | 0               8.9e-08 | 2.5e-08
  crossing, scale -100  7.5e-07 | 6.7e-07   6.7e-08 | 1.9e-08   4.9e-08 | 2.4e-08   2.8e-08 | 3.4e-08
  crossing, scale 0.5   9.1e-07 | 6.5e-07   5.4e-08 | 7.3e-08   4.2e-08 | 3.0e-08   0 | 0
  noise, beta 0.05      6.3e-05 | 6.3e-05   1.0e-06 | 9.7e-07   2.8e-07 | 1.6e-07   2.1e-08 | 5.1e-08
  noise, beta 5e-05     1.5e-03 | 1.5e-03   0 | 0               3.3e-04 | 2.8e-04   2.0e-05 | 1.5e-05

  zero normal, the zeroed sample on its own scale: d_normals 1.4e-06 | 1.2e-06, with d_depth alone 1.3e-05 | 4.1e-05, sigma entry 3.5e-07 | 6.5e-07
  the three one-upstream d_normals against the combined run: at most 3.1e-03 of the ray (noise, S = 2)
"""
import functools

import pytest
import torch

import density_cases as DC
from vf_nerf_amd import lib

pytestmark = pytest.mark.gpu

BACKWARD_CASES = [c for c in DC.ALL_CASES if c.backward]
ids = lambda c: c.id      # noqa: E731


def dev():
    return torch.device("cuda:0")


def params(case):
    return lib.DensityParams(0, 0, case.w, case.normalize, case.th, DC.BOUNDS["beta_bounds"][0], DC.BOUNDS["beta_bounds"][1],
                             DC.BOUNDS["mean_bounds"][0], DC.BOUNDS["mean_bounds"][1], DC.BOUNDS["scale_min"], DC.CUTOFF)


@functools.lru_cache(maxsize=None)
def on_device(case):
    inp = DC.make_inputs(case)
    g = {k: getattr(inp, k).to(dev()).contiguous() for k in ("normals", "z", "ray_dirs", "colors", "a", "b", "cw", "gs")}
    g["scalars"] = torch.tensor(case.scalars, dtype=torch.float32, device=dev())
    return g


def forward(case, colors=True, want_sigma=True):
    g = on_device(case)
    sigma, w, imax, rgb, depth = lib.ray_density_weights(params(case), g["normals"], g["ray_dirs"], g["z"], g["scalars"],
                                                         colors=g["colors"] if colors else None, want_sigma=want_sigma, want_argmax=True)
    return dict(sigma=sigma, weights=w, argmax=imax, rgb=rgb, depth=depth)


def backward(case, upstream=DC.FULL, d_normals=None, d_scalars=None, d_colors=None):
    """One launch of the composite backward with the upstream gradients named; buffers start from zeros unless given."""
    g = on_device(case)
    n, s = case.n, case.s
    with_colors = "rgb" in upstream
    out = dict(d_normals=torch.zeros(n, s, 3, device=dev()) if d_normals is None else d_normals,
               d_scalars=torch.zeros(3, device=dev()) if d_scalars is None else d_scalars)
    if with_colors:
        out["d_colors"] = torch.zeros(n, s, 3, device=dev()) if d_colors is None else d_colors
    lib.ray_density_weights_bwd(params(case), g["normals"], g["ray_dirs"], g["z"], g["scalars"], g["colors"] if with_colors else None,
                                g["a"] if with_colors else None, g["b"] if "depth" in upstream else None,
                                g["cw"] if "weights" in upstream else None, out["d_normals"], out.get("d_colors"), out["d_scalars"])
    return out


def sigma_backward(case, d_normals=None, d_scalars=None):
    g = on_device(case)
    out = dict(d_normals=torch.zeros(case.n, case.s, 3, device=dev()) if d_normals is None else d_normals,
               d_scalars=torch.zeros(3, device=dev()) if d_scalars is None else d_scalars)
    lib.ray_density_sigma_bwd(params(case), g["normals"], g["ray_dirs"], g["z"], g["scalars"], g["gs"], out["d_normals"], out["d_scalars"])
    return out


def held(case, run, upstream=DC.FULL, prefix="", what=""):
    """Scores ``run`` against float64, prints every figure beside its yardstick (``prefix``: the yardstick of one upstream term
    alone), asserts 8 x."""
    scores = DC.case_scores(case, run, upstream)
    rows = {k: (v, DC.bound(case, prefix + k) / DC.MARGIN_FACTOR) for k, v in scores.items()}
    print(f"{case.id} {what}: " + "  ".join(f"{k} {v:.2e} | {y:.2e}" for k, (v, y) in rows.items()))
    for k, (v, y) in rows.items():
        assert v <= DC.MARGIN_FACTOR * y, f"{case.id} {what} {k}: {v:.3e} on the device, {y:.3e} float32 on the host (x {DC.MARGIN_FACTOR:g} allowed)"
    return scores


@pytest.mark.parametrize("case", DC.ALL_CASES, ids=ids)
def test_forward(case):
    """sigma, weights, rgb and depth per ray; argmax equal to the float64 argmax on every ray (the two largest weights of a ray differ
    by 1e-4 of the larger at least); without colours, or without sigma, the remaining outputs are the same bits."""
    lib.load()
    ref, full = DC.reference(case), forward(case)
    held(case, full, what="forward")
    assert full["depth"].shape == (case.n, 1)
    assert torch.equal(full["argmax"].cpu(), ref["argmax"]), "argmax differs from float64"
    bare, quiet = forward(case, colors=False), forward(case, want_sigma=False)
    assert bare["rgb"] is None and bare["depth"] is None and quiet["sigma"] is None
    for k in ("sigma", "weights", "argmax"):
        assert torch.equal(bare[k], full[k]), k
    for k in ("weights", "argmax", "rgb", "depth"):
        assert torch.equal(quiet[k], full[k]), k


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=ids)
def test_backward_full_path(case):
    """d_rgb, d_depth and d_weights together into zeroed buffers: d_normals and d_colors per ray, the three scalar gradients on
    sum_rays |contribution|.  A scalar outside its clamp (beta < beta_min, mean outside [0.6, 1], |scale| < scale_min) has a
    gradient of exactly 0; a negative scale flips the sign of its own."""
    ref, got = DC.reference(case), backward(case)
    held(case, got, what="backward")
    b, m, sc = case.scalars
    clamped = [i for i, out in enumerate((b < 1e-4, not 0.6 <= m <= 1.0, abs(sc) < 1.0)) if out]
    assert float(ref["d_scalars"][clamped].abs().sum()) == 0.0
    assert torch.equal(got["d_scalars"][clamped], torch.zeros(len(clamped), device=dev()))


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=ids)
def test_backward_one_upstream_at_a_time(case):
    """Only d_depth (no colours, no d_colors), only d_weights, only d_rgb: each against the float64 gradient of its own term and
    8 x the host's float32 on that term (d_depth alone is the worst conditioned gradient here: dL/dw_j = b z_j is nearly the same
    for the few samples that carry weight, and the normalisation subtracts their weighted mean).  The three d_normals add up to
    the combined run's within the bound of the combined d_normals."""
    parts = {}
    for upstream in (("depth",), ("weights",), ("rgb",)):
        parts[upstream] = backward(case, upstream)
        held(case, parts[upstream], upstream, prefix=upstream[0] + ".", what=f"backward, d_{upstream[0]} alone")
    combined = backward(case)["d_normals"]
    total = sum(p["d_normals"].double() for p in parts.values())
    zero = DC.zero_normal_mask(DC.make_inputs(case)).to(dev()) if case.zero_normal else torch.zeros(case.n, case.s, 1, dtype=torch.bool, device=dev())
    err = max(float(DC.per_ray_error(total, combined, (~zero).expand_as(combined).cpu()).max()),
              float(DC.per_ray_error(total, combined, zero.expand_as(combined).cpu()).max()))
    print(f"{case.id}: sum of the three d_normals against the combined run {err:.2e}")
    assert err <= DC.bound(case, "d_normals")


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=ids)
def test_sigma_backward(case):
    """vfn_ray_density_sigma_bwd against the float64 gradient of sum gs sigma."""
    held(case, sigma_backward(case), ("sigma",), prefix="sigma.", what="sigma backward")


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=ids)
def test_accumulation(case):
    """d_normals is added to and d_scalars is added to atomically: from a random tensor r and from (1, 2, 3) the results are r + g and
    (1, 2, 3) + g, g being the run from zeros, to the rounding of those additions (d_normals: the one float32 addition per entry;
    scalars: one addition per workgroup in any order, each within half an ulp of |start| + sum_rays |contribution|).  d_colors is
    written, not added to: started from NaN it comes back the same bits as from zeros."""
    eps = 2.0 ** -23
    blocks = -(-case.n // 4) + 1                      # at most: 4 rays per workgroup at S > 160
    for run, upstream in ((backward, DC.FULL), (sigma_backward, ("sigma",))):
        g = run(case)
        gen = torch.Generator().manual_seed(case.s * 31 + case.w)
        r = torch.randn(case.n, case.s, 3, generator=gen).to(dev())
        start = torch.tensor([1.0, 2.0, 3.0], device=dev())
        kw = dict(d_normals=r.clone(), d_scalars=start.clone())
        if run is backward:
            kw["d_colors"] = torch.full((case.n, case.s, 3), float("nan"), device=dev())
        acc = run(case, **kw)
        diff = (acc["d_normals"].double() - (r.double() + g["d_normals"].double())).abs()
        room = eps * torch.maximum(r.abs(), g["d_normals"].abs()).double()
        assert bool((diff <= room).all()), f"d_normals += : off by {float((diff - room).max()):.3e} beyond one rounding"
        mag = start.double().cpu() + DC.reference(case, upstream)["scalar_parts"].abs().sum(dim=0)
        sdiff = (acc["d_scalars"].double() - (start.double() + g["d_scalars"].double())).abs().cpu()
        print(f"{case.id} {run.__name__}: accumulated scalars off by {[f'{float(x):.1e}' for x in sdiff]}, room {[f'{float(x):.1e}' for x in blocks * eps * mag]}")
        assert bool((sdiff <= blocks * eps * mag).all())
        if run is backward:
            assert torch.equal(acc["d_colors"], g["d_colors"]), "d_colors must be overwritten, whatever it held"


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=ids)
def test_inputs_untouched(case):
    """normals, colours, depths, ray directions and scalars hold the same bits after the forward and both backward launches (the
    forward kernel can write into normals / colours, but only for vfn_render_fwd's composite pass, which hands it a row map)."""
    g = on_device(case)
    before = {k: v.clone() for k, v in g.items()}
    forward(case)
    backward(case)
    sigma_backward(case)
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(g[k], v), k


def test_zero_normal():
    """One sample per ray with a normal of exactly (0, 0, 0).  Forward: u = 0 / 1e-8 = 0, so every cosine it takes part in is 0 and
    nothing is NaN.  Backward: the kernel's rule dn = du / 1e-8 is what the float64 autograd of the oracle gives there
    (test_density_host.py checks that against a difference quotient), so the sample is compared against it, on its own scale — it is
    1e8 times its neighbours' — and the rest of the ray on the ray's scale without it."""
    case = DC.ZERO_NORMAL_CASE
    zero = DC.zero_normal_mask(DC.make_inputs(case))
    out, grads, sg = forward(case), backward(case), sigma_backward(case)
    for t in list(out.values()) + list(grads.values()) + list(sg.values()):
        assert bool(torch.isfinite(t.float()).all())
    ref = DC.reference(case)
    j = torch.nonzero(zero[:, :-1, 0])
    assert float(ref["c"][j[:, 0], j[:, 1]].abs().max()) == 0.0          # (float64: the cosine of the zero sample with anything is 0)
    held(case, out, what="zero normal, forward")
    scores = held(case, grads, what="zero normal, backward")
    assert "d_normals.zero" in scores
    at_zero = (grads["d_normals"].cpu().abs() * zero).amax(dim=(1, 2))
    others = grads["d_normals"].cpu().masked_fill(zero, 0.0).abs().amax(dim=(1, 2))
    assert float((at_zero / others).median()) > 1e6
    held(case, sg, ("sigma",), prefix="sigma.", what="zero normal, sigma backward")
