"""Host checks under tests/test_hip_step_tail.py: the float32 yardsticks of tests/step_tail_cases.py stay under their cap, the redraw
caps hold, the selection restatement equals a plain loop, the region-to-list construction is optim.FlatAdam's layout read backwards, and
the scoring functions the device test uses can fail: float32 stand-ins of the three units (the kernels' arithmetic, restated here in
NumPy / torch on the host), each with one defect, must be refused by them, and without a defect accepted.  No device is needed."""
import numpy as np
import pytest
import torch

import step_tail_cases as SC
from vf_nerf_amd import optim

f32 = np.float32


# ------------------------------------------------------------------------------------------------
# yardsticks, redraw caps, restatements
# ------------------------------------------------------------------------------------------------
def test_float32_yardsticks_stay_under_their_cap():
    for loss in SC.loss_yardsticks().values():
        assert set(loss) >= set(SC.LOSS_TERMS) | {"total", "rows", "d_rgb", "d_depth", "d_normals", "d_sup0", "d_sup1", "d_sup2"}
        assert loss["rows"] == 0.0 and loss["dd"] == 0.0
        assert all(v <= SC.YARDSTICK_CAP for v in loss.values()), loss
    loss = SC.loss_yardsticks()
    for n, pool in SC.adam_yardstick().items():
        assert pool["outside"] == 0.0 and all(v <= SC.YARDSTICK_CAP for v in pool.values()), (n, pool)
    print("loss", {n: {k: f"{v:.1e}" for k, v in p.items()} for n, p in loss.items()})
    print("adam", {n: {k: f"{v:.1e}" for k, v in p.items()} for n, p in SC.adam_yardstick().items()})


def test_flat_leg_yardstick():
    ref, host = SC.flat_leg_torch(SC.F64), SC.flat_leg_torch(SC.F32)
    y = SC.flat_leg_scores(host, ref)
    assert all(y[k] <= SC.YARDSTICK_CAP for k in ("p", "m", "v")), y
    assert sum(int(np.prod(s)) for s in SC.FLAT_SHAPES) > 524_288


def test_nan_cases_of_the_loss_reference():
    """What float64 torch gives for a NaN input, the pattern the kernels are held to: the term and the total NaN; gradient 0 at an rgb or
    depth element whose error is NaN; all three components NaN at a normal with one NaN component."""
    for case in SC.LOSS_NAN_CASES:
        ref = SC.loss_reference(case)
        out = ref["out8"]
        assert bool(torch.isnan(out[6]))
        if case.nan == "depth":
            assert bool(torch.isnan(out[1])) and int(torch.isnan(out).sum()) == 2 and float(ref["d_depth"][1]) == 0.0
            assert not any(bool(torch.isnan(ref[k]).any()) for k in SC.LOSS_GRADS)
        elif case.nan == "rgb":
            assert bool(torch.isnan(out[0])) and int(torch.isnan(out).sum()) == 2 and float(ref["d_rgb"][1, 2]) == 0.0
        else:
            assert bool(torch.isnan(out[2])) and bool(torch.isnan(out[4])) == bool(case.smaller_on)
            assert bool(torch.isnan(ref["d_normals"][3]).all()) and int(torch.isnan(ref["d_normals"]).sum()) == 3
        assert SC.failures(SC.loss_scores(case, SC.loss_host_fp32(case)), SC.loss_yardstick(case), case.id) == []


def test_redraw_caps():
    """At most 5 % of the items or rays of a case drawn again, none ten times (make_* assert it; here for every case, with the counts)."""
    for case in SC.LOSS_CASES + SC.LOSS_NAN_CASES:
        inp = SC.make_loss_inputs(case)
        assert inp.redraws["rays"] <= SC.REDRAW_SHARE * max(case.n_rays, 1) and inp.redraws["normals"] <= SC.REDRAW_SHARE * max(case.n_normals, 1)
        assert inp.redraws["most"] < SC.MAX_REDRAWS
    per_family = {}
    for case in SC.SEL_CASES:
        inp = SC.make_sel_inputs(case)
        assert inp.redrawn <= SC.REDRAW_SHARE * case.n_rays and inp.most < SC.MAX_REDRAWS, (case.id, inp.redrawn, inp.most)
        assert not bool(SC.sel_in_band(inp.sigma, inp.z).any())
        a, b = per_family.get(case.family, (0, 0))
        per_family[case.family] = (a + inp.redrawn, b + case.n_rays)
    print("selection rays redrawn / drawn:", per_family)
    for case in SC.CLIP_CASES:
        inp = SC.make_clip_inputs(case)
        total = float(SC.clip_reference(case)[0])
        assert case.mode == "zero" or abs(total - inp.max_norm) >= 1e-4 * inp.max_norm


def test_selection_cases_have_something_to_lose():
    for case in SC.SEL_CASES:
        only = SC.sel_training_only(case)
        if case.family in ("sparse", "dense", "tiny") and case.n_rays >= 255 and case.s >= 63:
            assert only >= 150, (case.id, only)
        if case.family == "none":
            inp = SC.make_sel_inputs(case)
            assert SC.select_reference(inp.weights, inp.sigma, inp.z, inp.points, inp.dirs, True)[0].size == 0
        if case.family == "all":
            inp = SC.make_sel_inputs(case)
            assert SC.select_reference(inp.weights, inp.sigma, inp.z, inp.points, inp.dirs, False)[0].size == case.n_rays * case.s


@pytest.mark.parametrize("case", [SC.SelCase(5, 200, "sparse"), SC.SelCase(5, 200, "opaque"), SC.SelCase(1, 200, "tiny")], ids=lambda c: c.id)
def test_selection_restatement_equals_a_plain_loop(case):
    inp = SC.make_sel_inputs(case)
    for training in (False, True):
        want = []
        for r in range(case.n_rays):
            before = 0.0
            for j in range(case.s):
                delta = f32(inp.z[r, j + 1] - inp.z[r, j]) if j < case.s - 1 else f32(1e10)
                ok = inp.weights[r, j] > 0
                if training and inp.sigma[r, j] > 0 and delta > 0 and before < 110.0:
                    ok = True
                if ok:
                    want.append(r * case.s + j)
                before += float(f32(inp.sigma[r, j] * delta))
        got, pts, dirs = SC.select_reference(inp.weights, inp.sigma, inp.z, inp.points, inp.dirs, training)
        assert got.tolist() == want
        assert np.array_equal(pts, inp.points.reshape(-1, 3)[want]) and np.array_equal(dirs, inp.dirs[[i // case.s for i in want]])
    if case.planted_ray:
        assert 0 not in SC.select_reference(inp.weights, inp.sigma, inp.z, inp.points, inp.dirs, True)[0].tolist()      # delta = 0, sigma > 0


def test_region_list_is_flat_adams_layout_read_backwards():
    n = 257
    for regions in ([(0, 65, 2), (65, n, 1)], [(0, n, 2)], [(0, n, 1)]):
        flat = torch.arange(n, dtype=torch.float32)
        uniq, plist = SC.region_list(flat, regions)
        params = {id(t): torch.nn.Parameter(t) for t in uniq}
        opt = optim.FlatAdam([params[id(t)] for t in plist], lr=1e-3)
        entries, got, total = opt._layout()
        assert got == [tuple(r) for r in regions] and total == n
        assert [(off, k, m) for _, off, k, m in entries] == [(s, e - s, m) for s, e, m in regions]
        assert all(torch.equal(p.detach(), flat[off:off + k]) for p, off, k, _ in entries)
    # several tensors of one multiplicity merge into one region, the ones listed twice first (the reference's list: ps + ps[:2])
    ps = [torch.nn.Parameter(torch.zeros(k)) for k in (7, 5, 9, 4)]
    assert optim.FlatAdam(ps + ps[:2], lr=1e-3)._layout()[1] == [(0, 12, 2), (12, 25, 1)]


# ------------------------------------------------------------------------------------------------
# stand-ins: the kernels' float32 arithmetic on the host, with one defect each
# ------------------------------------------------------------------------------------------------
def loss_standin(case, defect=None):
    """csrc/vfn_loss.hip in float32 torch: sums, the finish, the elementwise backward."""
    inp = SC.make_loss_inputs(case)
    n, m = case.n_rays, case.n_normals
    g = torch.tensor(1.0 if case.grad_out is None else case.grad_out, dtype=torch.float32)
    e_rgb = inp.rgb - inp.rgb_gt
    e_d = inp.depth - inp.depth_gt
    nrm = torch.linalg.vector_norm(inp.normals, dim=1)
    diff = inp.points - torch.tensor(SC.CENTROID)
    dist = torch.linalg.vector_norm(diff, dim=1)
    inside = (dist < SC.RADIUS) if case.ball != "off" else torch.zeros(m, dtype=torch.bool)
    e_ball = inp.normals - diff / dist.clamp_min(1e-12).unsqueeze(1)
    e_sup = [a - b for a, b in zip(inp.sup_pred, inp.sup_gt)]
    rows = sum(case.sup) + (0 if defect == "no_ball_rows" else int(inside.sum()))
    rgb = float(e_rgb.abs().double().sum()) / (3.0 * n) if n else 0.0
    depth = float(e_d.abs().clamp(max=SC.CLAMP).double().sum()) / n if (n and case.has_depth) else 0.0
    unit = float(((nrm - 1) ** 2).double().sum()) / m if m else 0.0
    small = float((torch.relu(nrm - 1) ** 2).double().sum()) / m if (m and case.smaller_on) else 0.0
    sup_sum = float((e_ball[inside] ** 2).double().sum()) + sum(float((e ** 2).double().sum()) for e in e_sup)
    sup = sup_sum / (3.0 * rows) if rows else 0.0
    total = SC.W_RGB * rgb + SC.W_DEPTH * depth + SC.W_UNIT * unit + SC.W_SUP * sup + SC.W_SMALL * small
    out = dict(out8=torch.tensor([rgb, depth, unit, sup, small, 0.0, total, float(rows)], dtype=torch.float32))
    k_rows = rows + 17 if defect == "stale_rows" else rows
    k_sup = g * SC.W_SUP * 2.0 * (torch.tensor(1.0 / (3.0 * k_rows), dtype=torch.float32) if k_rows else 0.0)
    k_rgb, k_depth = (g * SC.W_RGB / (3.0 * n), g * SC.W_DEPTH / n) if n else (0.0, 0.0)
    k_unit, k_small = (g * SC.W_UNIT * 2.0 / m, g * SC.W_SMALL * 2.0 / m) if m else (0.0, 0.0)
    out["d_rgb"] = torch.sign(e_rgb) * k_rgb
    passes = torch.ones_like(e_d, dtype=torch.bool) if defect == "depth_passes" else e_d.abs() <= SC.CLAMP
    out["d_depth"] = torch.where(passes, torch.sign(e_d) * k_depth, torch.zeros(())) if case.has_depth else torch.zeros_like(e_d)
    f = k_unit * (nrm - 1) + (k_small * torch.relu(nrm - 1) if case.smaller_on else 0.0)
    f = torch.where(nrm > 0, f / nrm.clamp_min(1e-30), torch.zeros(()))
    out["d_normals"] = f.unsqueeze(1) * inp.normals + torch.where(inside.unsqueeze(1), k_sup * e_ball, torch.zeros(()))
    for k in range(3):
        out[f"d_sup{k}"] = k_sup * e_sup[k]
    return out


LOSS_MUTANT_CASES = [c for c in SC.LOSS_CASES if c.items < 10_000]


def _loss_refused(defect):
    bad = []
    for case in LOSS_MUTANT_CASES:
        run = loss_standin(case, defect)
        bad += SC.failures(SC.loss_scores(case, run), SC.loss_yardstick(case), case.id) + SC.loss_planted_failures(case, run)
    return bad


def test_loss_standin_is_accepted():
    assert _loss_refused(None) == []


@pytest.mark.parametrize("defect", ["no_ball_rows", "depth_passes", "stale_rows"])
def test_loss_mutants_are_refused(defect):
    """Supervision mean over the segment rows without the ball rows; depth gradient passing beyond the clamp; k_sup from a stale row
    count (the forward terms right, the supervision gradients scaled by another call's count)."""
    bad = _loss_refused(defect)
    assert bad, defect
    if defect == "stale_rows":
        assert all(" d_" in b for b in bad), bad        # only gradients


def clip_standin(case, defect=None):
    """vfn_grad_norm_kernel + vfn_grad_scale_kernel: the squared norm in float64, everything after it in float32."""
    inp = SC.make_clip_inputs(case)
    g = inp.grad.numpy().copy()
    mult = SC.mult_vector(case.n, case.regions).numpy()
    m_norm = np.minimum(mult, 1) if defect == "norm_once" else mult
    with np.errstate(all="ignore"):
        total = f32(np.sqrt(np.sum(m_norm.astype(np.float64) * g.astype(np.float64) ** 2)))
        denom = total if defect == "no_eps" else f32(total + f32(1e-6))
        coef = f32(f32(inp.max_norm) / denom)
        if np.isnan(coef):
            coef = f32(1.0) if defect == "nan_is_one" else coef
        elif coef > 1.0:
            coef = f32(1.0)
        for k in range(2):
            times = np.minimum(mult, 1) if defect == "scaled_once" else mult
            g = np.where(times > k, (g * coef).astype(np.float32), g)
    return torch.tensor([total, coef]), torch.from_numpy(g)


def _clip_refused(defect, cases):
    return [b for case in cases for b in SC.clip_failures(case, *clip_standin(case, defect))]


def test_clip_standin_is_accepted():
    assert _clip_refused(None, SC.CLIP_CASES + SC.CLIP_PLANT_CASES) == []


@pytest.mark.parametrize("defect", ["norm_once", "scaled_once", "no_eps", "nan_is_one"])
def test_clip_mutants_are_refused(defect):
    """Duplicates counted once in the norm; duplicates scaled once; the coefficient from the total without the 1e-6; a NaN total
    giving coefficient 1."""
    small = [c for c in SC.CLIP_CASES + SC.CLIP_PLANT_CASES if c.n <= 257]
    bad = _clip_refused(defect, small)
    assert bad, defect
    if defect == "no_eps":
        assert _clip_refused(defect, [c for c in small if c.scale != 1.0]), "the cases with a total near 1e-5 are there for this"
    if defect == "nan_is_one":
        assert _clip_refused(defect, [c for c in small if c.plant == "nan"])


def adam_standin(case, defect=None):
    """vfn_adam_kernel in NumPy float32, operation for operation."""
    inp = SC.make_adam_inputs(case)
    p, m, v = (getattr(inp, k).numpy().copy() for k in SC.ADAM_STATE)
    b1, b2 = SC.ADAM_BETAS
    beta2, eps, wd, omb1, omb2 = f32(b2), f32(SC.ADAM_EPS), f32(case.weight_decay), f32(1.0 - b1), f32(1.0 - b2)
    out = []
    for step, grad in enumerate(inp.grads):
        ss, bc = SC.adam_scalars(case, step)
        g0 = grad.numpy()
        for r, (s, e, mult) in enumerate(case.regions):
            P, M, V, G0 = p[s:e], m[s:e], v[s:e], g0[s:e]
            for k in range(mult):
                ku = 0 if defect == "first_scalars_twice" else k
                G = (G0 + wd * P).astype(np.float32) if case.weight_decay != 0 else G0
                M = (M + omb1 * (G - M)).astype(np.float32)
                V = (V * beta2 + (omb2 * G) * G).astype(np.float32)
                denom = (np.sqrt(V) / f32(bc[2 * r + ku]) + eps).astype(np.float32)
                P = (P - f32(ss[2 * r + ku]) * (M / denom)).astype(np.float32)
            p[s:e], m[s:e], v[s:e] = P, M, V
        out.append(dict(p=torch.from_numpy(p.copy()), m=torch.from_numpy(m.copy()), v=torch.from_numpy(v.copy())))
    return out


def adam_failures(case, run):
    return SC.failures(SC.adam_scores(case, run), SC.adam_yardstick()[case.n], case.id)


def test_adam_standin_is_accepted():
    assert [b for case in SC.ADAM_CASES for b in adam_failures(case, adam_standin(case))] == []


def test_adam_mutant_is_refused():
    """The second update of a multiplicity-2 element taken with the first update's step_size / bc2_sqrt: refused at step counts 0 and
    1, where the two differ by a factor near 2."""
    for case in SC.ADAM_CASES:
        twice = [t0 for (s, e, mult), t0 in zip(case.regions, case.t0) if mult == 2 and e > s]
        if case.n <= 257 and any(t0 in (0, 1) for t0 in twice):
            assert adam_failures(case, adam_standin(case, "first_scalars_twice")), case.id


def select_standin(case, training, defect=None):
    """The three selection kernels: the predicate with its carry between chunks of 64 samples, the one-workgroup scan over chunks of
    ``per`` rays, the compaction into a buffer that holds SENTINEL."""
    inp = SC.make_sel_inputs(case)
    n, s = case.n_rays, case.s
    delta = np.concatenate([inp.z[:, 1:] - inp.z[:, :-1], np.full((n, 1), f32(1e10))], axis=1).astype(np.float32)
    e = (inp.sigma * delta).astype(np.float32).astype(np.float64)
    sel = inp.weights > 0
    if training:
        carry = np.zeros(n)
        before = np.zeros((n, s))
        for j0 in range(0, s, 64):
            if defect == "carry_reset":
                carry = np.zeros(n)
            incl = np.cumsum(e[:, j0:j0 + 64], axis=1)
            before[:, j0:j0 + 64] = carry[:, None] + (incl - e[:, j0:j0 + 64])
            carry = carry + incl[:, -1]
        clause = inp.sigma > 0
        if defect != "no_delta":
            clause &= delta > 0
        if defect != "no_before":
            clause &= before < 110.0
        sel = sel | clause
    cnt = sel.sum(axis=1)
    per = (n + 255) // 256
    off = np.zeros(n, dtype=np.int64)
    sums = [int(cnt[t * per:min(n, t * per + per)].sum()) for t in range(256)]
    incl = np.cumsum(sums)
    for t in range(256):
        lo, hi = t * per, min(n, t * per + per)
        if lo >= hi:
            continue
        run = int(incl[t]) - (int(cnt[lo]) if defect == "scan_chunk" else sums[t])
        for i in range(lo, hi):
            off[i] = run
            run += int(cnt[i])
    index = np.full(n * s, SC.SENTINEL, dtype=np.int32)
    pts, dirs = np.zeros((n * s, 3), dtype=np.float32), np.zeros((n * s, 3), dtype=np.float32)
    for r in range(n):
        js = np.nonzero(sel[r])[0]
        k = off[r] + np.arange(js.size)
        keep = k < n * s
        index[k[keep]] = (r * s + js[keep]).astype(np.int32)
        pts[k[keep]], dirs[k[keep]] = inp.points[r, js[keep]], inp.dirs[r]
    return int(incl[-1]), index, pts, dirs


SEL_MUTANT_CASES = [c for c in SC.SEL_CASES if c.n_rays in (257, 1030) and c.s in (1, 2, 65, 200)]


def test_selection_standin_is_accepted():
    for case in SEL_MUTANT_CASES:
        for training in (False, True):
            assert SC.sel_failures(case, training, *select_standin(case, training)) == [], (case.id, training)


@pytest.mark.parametrize("defect", ["carry_reset", "no_before", "no_delta", "scan_chunk"])
def test_selection_mutants_are_refused(defect):
    """The carry reset at every 64-sample chunk; no `before < 110` clause; no `delta > 0` clause; scan offsets off by one workgroup
    thread's chunk where a thread scans more than one ray (n_rays above 256)."""
    refused = [c.id for c in SEL_MUTANT_CASES if SC.sel_failures(c, True, *select_standin(c, True, defect))]
    assert refused, defect
    if defect == "carry_reset":
        assert all("-S200" in i or "-S65" in i for i in refused)           # one chunk: nothing to carry
    if defect == "scan_chunk":
        assert all("-N257" in i or "-N1030" in i for i in refused)
    if defect == "no_delta":
        assert any(i.startswith(("sparse", "dense", "tiny")) for i in refused)      # the planted duplicate depth
