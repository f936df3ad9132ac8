"""The scalar tail of the training step on the device against float64: vfn_vf_loss_fwd / _bwd (csrc/vfn_loss.hip), vfn_flat_clip_grad_norm
and vfn_flat_adam_step (csrc/vfn_adam.hip) and vfn_select_samples (csrc/vfn_rays.hip).

Inputs, references and scoring: tests/step_tail_cases.py (checked on the host, with mutants, by tests/test_step_tail_host.py).
  loss       every term, the total and every gradient tensor: max |x - x64| / max |x64| over the tensor, at most 8 x the same formulation in
             float32 on the host (pooled over the loss cases); out[7] equal to the float64 row count; a quantity that is exactly 0 in
             float64 exactly 0 here; the planted items exactly; NaN inputs give the NaN pattern of float64 torch
  clip       derived bounds, u = 2^-24: the norm within one float32 ulp, the coefficient within 4 u, every scaled element within 5 mult u,
             exactly 1.0 and the same bits where nothing is clipped, the same bits outside every region
  Adam       p, m, v and the update p_new - p_old per region, at most 8 x torch.optim.Adam(foreach=False) in float32 on the host (pooled
             over the cases of one buffer size); the same bits outside every region
  selection  indices, count, gathered points and directions equal to the NumPy restatement; the sentinel kept past the count

Measured on an MI355X, worst case of each pool: device | host-float32 yardstick (both against float64; the bound is 8 x the second
figure).  The device never measured more than 2.0 x its yardstick (norm_smaller_than_one_loss, 1.07e-07 against 5.5e-08); most figures
are the host's own, the same IEEE operations in the same order.  121 tests, 4.9 s of wall time on the device machine.

  loss, many items   rgb 7.8e-08 | 1.0e-07   depth 8.0e-08 | 1.1e-07   unit_norm 9.4e-08 | 9.4e-08   supervision 8.7e-08 | 1.2e-07
                     smaller 1.1e-07 | 5.5e-08   total 6.1e-08 | 8.0e-08   d_rgb 3.0e-08 | 3.0e-08   d_depth 3.0e-08 | 3.0e-08
                     d_normals 1.2e-07 | 1.2e-07   d_sup0 9.6e-08 | 9.6e-08   d_sup1 4.1e-08 | 4.1e-08   d_sup2 9.4e-08 | 9.4e-08
  loss, one item     rgb 2.5e-08 | 2.5e-08   unit_norm, smaller 1.6e-06 | 1.6e-06   total 1.7e-06 | 1.7e-06   d_rgb 2.5e-08 | 2.5e-08
                     d_normals 8.2e-07 | 7.5e-07   (everything else exactly 0 on both sides)
  Adam, n = 1        p 1.2e-07 | 1.2e-07   m 1.0e-07 | 1.0e-07   v 1.0e-07 | 1.0e-07   update 9.5e-05 | 9.5e-05
  Adam, n = 257      p 1.4e-07 | 1.4e-07   m 1.2e-07 | 1.2e-07   v 1.8e-07 | 1.8e-07   update 4.5e-06 | 4.5e-06
  Adam, n = 524 621  p 2.0e-07 | 1.8e-07   m 9.5e-08 | 9.5e-08   v 2.3e-07 | 2.3e-07   update 1.8e-05 | 1.8e-05
  FlatAdam leg       p 1.3e-07 | 7.0e-07   m 1.5e-07 | 1.6e-07   v 1.6e-07 | 1.6e-07   total norm 0.41 float32 ulp (float32 torch: 59)
  clip               every norm within one float32 ulp, every coefficient within 4 u, every element within 5 mult u (asserted, not scored)

Redraws (host, deterministic): selection 61 of 3603 rays (sparse), 31 of 3603 (dense), none in the other families, no ray more than
twice; loss at most 42 of 1 100 000 normals, no ray; clip none.
"""
import functools

import numpy as np
import pytest
import torch

import step_tail_cases as SC
from vf_nerf_amd import lib, optim

pytestmark = pytest.mark.gpu

ids = lambda c: c.id      # noqa: E731
WORST = {}                # (unit, quantity) -> (device, yardstick) with the largest ratio, for the report at the end


def dev():
    return torch.device("cuda:0")


def held(unit, case, scores, yard):
    """Prints every figure beside its yardstick, remembers the worst ratio, asserts MARGIN_FACTOR x."""
    print(f"{unit} {case.id}: " + "  ".join(f"{k} {v:.2e} | {yard[k]:.2e}" for k, v in scores.items()))
    for k, v in scores.items():
        old = WORST.get((unit, k), (0.0, 0.0))
        if v > old[0]:
            WORST[(unit, k)] = (v, yard[k])
    bad = SC.failures(scores, yard, f"{unit} {case.id}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------
def loss_params(case):
    lp = lib.LossParams()
    lp.n_rays, lp.n_normals = case.n_rays, case.n_normals
    for k in range(3):
        lp.n_sup[k] = case.sup[k]
    lp.has_depth, lp.smaller_on, lp.ray_center = case.has_depth, case.smaller_on, int(case.ball != "off")
    lp.w_rgb, lp.w_depth, lp.w_unit, lp.w_sup, lp.w_smaller = SC.W_RGB, SC.W_DEPTH, SC.W_UNIT, SC.W_SUP, SC.W_SMALL
    lp.depth_clamp, lp.radius = SC.CLAMP, SC.RADIUS
    for i in range(3):
        lp.centroid[i] = SC.CENTROID[i]
    return lp


def loss_on_device(case, skip=()):
    """Forward and backward through lib.vf_loss_fwd / vf_loss_bwd -> the dict loss_scores takes.  Operands of extent 0 are NULL; the
    outputs named in ``skip`` are NULL; every output buffer holds NaN before the launch.  Asserts that no input was written."""
    inp = SC.make_loss_inputs(case)

    def up(t):
        return t.to(dev()).contiguous() if t.numel() else None

    g = dict(rgb=up(inp.rgb), rgb_gt=up(inp.rgb_gt), depth=up(inp.depth), depth_gt=up(inp.depth_gt), normals=up(inp.normals),
             points=up(inp.points) if case.ball != "off" else None)
    sp, sg = [up(t) for t in inp.sup_pred], [up(t) for t in inp.sup_gt]
    before = [None if t is None else t.clone() for t in list(g.values()) + sp + sg]
    lp, ws = loss_params(case), lib.vf_loss_workspace(dev())
    args = (lp, g["rgb"], g["rgb_gt"], g["depth"], g["depth_gt"], g["normals"], g["points"], sp, sg, ws)
    out = dict(out8=lib.vf_loss_fwd(*args))

    def buf(name, like):
        return None if (like is None or name in skip) else torch.full_like(like, float("nan"))

    d = dict(d_rgb=buf("d_rgb", g["rgb"]), d_depth=buf("d_depth", g["depth"]), d_normals=buf("d_normals", g["normals"]))
    d_sup = [buf(f"d_sup{k}", sp[k]) for k in range(3)]
    grad_out = None if case.grad_out is None else torch.tensor([case.grad_out], dtype=torch.float32, device=dev())
    lib.vf_loss_bwd(*args, grad_out, d["d_rgb"], d["d_depth"], d["d_normals"], d_sup)
    torch.cuda.synchronize()
    for a, b in zip(list(g.values()) + sp + sg, before):
        assert a is None or torch.equal(a.view(torch.int32), b.view(torch.int32)), "an input was written"
    for k in range(3):
        d[f"d_sup{k}"] = d_sup[k]
    for k, t in d.items():
        out[k] = t.cpu() if t is not None else (None if k in skip else torch.zeros(SC.loss_reference(case)[k].shape))
    out["out8"] = out["out8"].cpu()
    return out


@pytest.mark.parametrize("case", SC.LOSS_CASES, ids=ids)
def test_loss(case):
    lib.load()
    run, ref = loss_on_device(case), SC.loss_reference(case)
    assert float(run["out8"][7]) == float(ref["out8"][7]) and float(run["out8"][5]) == 0.0
    held(f"loss, {SC.loss_pool(case)}", case, SC.loss_scores(case, run), SC.loss_yardstick(case))
    for k in SC.LOSS_GRADS:
        assert bool(torch.isfinite(run[k]).all()), f"{k}: not every element written, or not finite"
    bad = SC.loss_planted_failures(case, run)
    assert not bad, bad
    if case.ball == "empty" and sum(case.sup) == 0:
        assert float(run["out8"][3]) == 0.0 and float(run["out8"][7]) == 0.0
    if not case.has_depth:
        assert float(run["out8"][1]) == 0.0 and float(run["d_depth"].abs().sum()) == 0.0


@pytest.mark.parametrize("case", [SC.LOSS_CASES[2], SC.LOSS_CASES[3]], ids=ids)
def test_loss_null_outputs(case):
    """Each of d_rgb, d_depth, d_normals and d_sup[k] NULL in turn: the others are the same bits."""
    full = loss_on_device(case)
    for name in SC.LOSS_GRADS:
        if full[name].numel() == 0:
            continue
        part = loss_on_device(case, skip=(name,))
        assert part[name] is None
        for k in SC.LOSS_GRADS:
            if k != name:
                assert torch.equal(part[k].view(torch.int32), full[k].view(torch.int32)), (name, k)
        assert torch.equal(part["out8"], full["out8"])


@pytest.mark.parametrize("case", SC.LOSS_NAN_CASES, ids=ids)
def test_loss_nan_inputs(case):
    """A NaN depth, normal component or rgb element: the eight outputs and every gradient have the NaN pattern of the float64
    formulation (rel_score is infinite where the patterns differ), the rest within the bounds of the clean cases."""
    run, ref = loss_on_device(case), SC.loss_reference(case)
    assert torch.equal(torch.isnan(run["out8"]), torch.isnan(ref["out8"])), (run["out8"], ref["out8"])
    for k in SC.LOSS_GRADS:
        assert torch.equal(torch.isnan(run[k]), torch.isnan(ref[k])), k
    held(f"loss, {SC.loss_pool(case)}", case, SC.loss_scores(case, run), SC.loss_yardstick(case))


# ------------------------------------------------------------------------------------------------
# clip
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", SC.CLIP_GROUPS, ids=lambda g: f"n{g[0]}-{g[1]}")
def test_clip(group):
    """Clipped, unclipped and all zero, one after the other on ONE workspace (the kernel resets its own counter)."""
    lib.load()
    ws, out2 = lib.flat_clip_workspace(dev()), torch.full((2,), float("nan"), device=dev())
    for case in [c for c in SC.CLIP_CASES if (c.n, c.regions_name) == group]:
        inp = SC.make_clip_inputs(case)
        grad = inp.grad.to(dev())
        lib.flat_clip_grad_norm(grad, case.regions, inp.max_norm, ws, out2)
        bad = SC.clip_failures(case, out2, grad)
        t64 = float(SC.clip_reference(case)[0])
        print(f"clip {case.id}: norm {float(out2[0]):.9e} | {t64:.9e}  coefficient {float(out2[1]):.9e}")
        assert not bad, bad


@pytest.mark.parametrize("case", SC.CLIP_PLANT_CASES, ids=ids)
def test_clip_nan_and_inf(case):
    """A NaN gradient element: out2 = NaN, NaN and every gradient inside the regions NaN, as torch.nn.utils.clip_grad_norm_.  A +inf
    one: inf, 0, the infinite element NaN, the rest 0.  Elements outside every region keep their bits."""
    inp = SC.make_clip_inputs(case)
    ws, out2, grad = lib.flat_clip_workspace(dev()), torch.zeros(2, device=dev()), inp.grad.to(dev())
    lib.flat_clip_grad_norm(grad, case.regions, inp.max_norm, ws, out2)
    bad = SC.clip_failures(case, out2, grad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.ADAM_CASES, ids=ids)
def test_adam(case):
    lib.load()
    inp = SC.make_adam_inputs(case)
    p, m, v = (getattr(inp, k).to(dev()) for k in SC.ADAM_STATE)
    run = []
    for step, grad in enumerate(inp.grads):
        ss, bc = SC.adam_scalars(case, step)
        g = grad.to(dev())
        lib.flat_adam_step(p, g, m, v, case.regions, ss, bc, SC.ADAM_BETAS[0], SC.ADAM_BETAS[1], SC.ADAM_EPS, case.weight_decay)
        assert torch.equal(g.cpu().view(torch.int32), grad.view(torch.int32)), "the gradient was written"
        run.append(dict(p=p.cpu(), m=m.cpu(), v=v.cpu()))
    scores = SC.adam_scores(case, run)
    assert scores["outside"] == 0.0, "elements outside every region changed"
    held(f"adam n={case.n}", case, scores, SC.adam_yardstick()[case.n])


def test_flat_adam_and_clip_through_the_optimizer():
    """optim.FlatAdam + optim.clip_grad_norm_ over a duplicated list of 524 982 elements, three clipped steps from step counters 6 and
    3, against torch's sequential optimizer and clip in float64: step_scalars and the Python-to-kernel hand-over at a size where every
    stride loop runs.  p, m, v per parameter within 8 x the same in float32 on the host; the total norm within one float32 ulp."""
    ref, host = SC.flat_leg_torch(SC.F64), SC.flat_leg_torch(SC.F32)
    yard = SC.flat_leg_scores(host, ref)
    assert all(yard[k] <= SC.YARDSTICK_CAP for k in ("p", "m", "v"))
    run = SC.flat_leg_run(lambda pl: optim.FlatAdam(pl, lr=SC.ADAM_LR, betas=SC.ADAM_BETAS, eps=SC.ADAM_EPS), optim.clip_grad_norm_, dev(), torch.float32)
    scores = SC.flat_leg_scores(run, ref)
    print("FlatAdam leg: " + "  ".join(f"{k} {scores[k]:.2e} | {yard[k]:.2e}" for k in scores))
    assert scores["norm_ulps"] <= 1.0
    for k in ("p", "m", "v"):
        WORST[("flat leg", k)] = (scores[k], yard[k])
        assert scores[k] <= SC.MARGIN_FACTOR * yard[k], k


# ------------------------------------------------------------------------------------------------
# selection
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.SEL_CASES, ids=ids)
def test_selection(case):
    lib.load()
    inp = SC.make_sel_inputs(case)
    w, sigma, z, pts, dirs = (torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in (inp.weights, inp.sigma, inp.z, inp.points, inp.dirs))
    for training in (False, True):
        count, index, ps, ds = lib.select_samples(w, pts, dirs, sigma if training else None, z if training else None, return_all=True,
                                                  index_fill=SC.SENTINEL)
        bad = SC.sel_failures(case, training, count, index.cpu().numpy(), ps.cpu().numpy(), ds.cpu().numpy())
        assert not bad, (training, bad)
    for a, b in ((w, inp.weights), (sigma, inp.sigma), (z, inp.z), (pts, inp.points), (dirs, inp.dirs)):
        assert np.array_equal(a.cpu().numpy().view(np.int32), np.ascontiguousarray(b).view(np.int32)), "an input was written"
    if case.family in ("none", "all"):
        assert count == (0 if case.family == "none" else case.n_rays * case.s)
    # the wrapper's list form is the same selection
    if case.n_rays * case.s <= 20_000:
        assert lib.select_samples(w, pts, dirs, sigma, z) == index[:count].tolist()


def test_zz_report():
    """The worst device figure of every pool beside its yardstick (what the module docstring quotes)."""
    worst = 0.0
    for (unit, k), (v, y) in sorted(WORST.items()):
        print(f"  {unit:14s} {k:28s} {v:.1e} | {y:.1e}")
        if y > 0:
            worst = max(worst, v / y)
    print(f"  worst ratio {worst:.2f}")
