"""Inputs, float64 evaluation and scoring for the per-ray density tests (tests/test_density_host.py, tests/test_hip_density.py).

The reference is the oracle itself (oracle/vfnerf_oracle.py: ray_density, volsdf_weights) evaluated in float64 by dtype promotion on
the float32 inputs the kernels get; gradients come from torch.autograd on that evaluation.  Nothing of the arithmetic is restated here.
The oracle's float32 constants (ones(W) / W and their sum, the clamps' bounds, the 1e10 of the last interval) stay float32 values, the
ones the kernel uses.

Input families (one ray at a time from a seeded generator; normals are the direction field times a log-normal length, never unit):
  noise     independent Gaussian normals: transparent rays, weights spread over the ray.  The two sharp settings of beta run on this
            family, with the first cosine of every ray put where their density is (see the case list and _draw_ray)
  crossing  v tanh(40 (t0 - t)) + 0.15 Gaussian with t = j / (S - 1): cosine +1 away from the surface, -1 across it; a few samples
            carry all the weight, and where the spacings around the crossing are about 1 (half of the rays) the transmittance saturates.
            Three rays in ten also have one sample among the first or last `start` tilted 61 to 78 degrees away from its neighbours:
            a weak density in front of the surface or behind it, where the cosine is the plain adjacent one
  empty     the crossing placed beyond the last sample, with one to three samples per ray tilted 61 to 78 degrees away from v over
            spacings of about 1e-4: sum(what) is 0 or a few 1e-5, so the + 1e-5 of the normalisation decides the weights
Depths are sorted with spacings log-uniform between 1e-4 and 1 (noise: 1e-2).

Decision margins.  A ray is drawn again from the same generator while one of its samples sits within MARGIN of a discontinuity of the
float64 evaluation (``margin_failures``), so that no float32 evaluation can take another branch and every ray can be compared:
  * the ReLU: |raw| / scale < MARGIN with raw the density before the ReLU.  Where the cdf is flat (a sharp beta puts both of its
    terms below 1e-11) raw is that small for every cosine, however far from the cutoff; there the same decision is stated on the
    cosine itself, which is where the monotone cdf takes it from: such a sample passes when |c - (-cutoff)| >= FLAT_MARGIN = 1e-2.
    With the shipped scalars the slope of raw / scale at the cutoff is 0.045, so the first form already implies |c - 0.5| >= 2.2e-3
    and the second never decides anything;
  * the mask: |c| < MARGIN where c_ray < th, and |c_ray - th| < MARGIN where c < 0;
  * the argmax: the two largest float64 weights differ by less than MARGIN of the larger one (rays without any weight: argmax 0).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, Tuple

import torch

from oracle import vfnerf_oracle as O

N_RAYS = 37                      # odd; more than two workgroups at 16, 8 and 4 rays per workgroup
MARGIN = 1e-4
FLAT_MARGIN = 1e-2
MAX_REDRAWS = 10
DEFAULT_SCALARS = (0.5, 0.7, 100.0)
BOUNDS = dict(beta_bounds=(1e-4, 1e9), mean_bounds=(0.6, 1.0), scale_min=1.0)
CUTOFF = -0.5
FULL = ("rgb", "depth", "weights")
ALONE = (("depth",), ("weights",), ("rgb",), ("sigma",))      # one upstream gradient at a time; sigma: its own entry point
PER_RAY = ("sigma", "weights", "rgb", "depth")
SCALAR_NAMES = ("beta", "mean", "scale")
F64 = torch.float64


@dataclass(frozen=True)
class Case:
    s: int
    w: int
    family: str
    th: float = -0.2
    normalize: int = 1
    scalars: Tuple[float, float, float] = DEFAULT_SCALARS
    n: int = N_RAYS
    zero_normal: bool = False          # one sample per ray with a normal of exactly (0, 0, 0)

    @property
    def backward(self) -> bool:
        return self.s <= 256           # MAX_SAMPLES_BWD; longer rays run the forward only

    @property
    def start(self) -> int:
        return int((self.w + 1) / 2 + 1)

    @property
    def has_interior(self) -> bool:
        return self.s - 1 - self.start > self.start

    @property
    def id(self) -> str:
        tag = f"{self.family}-S{self.s}-W{self.w}-th{self.th:g}"
        if self.normalize != 1:
            tag += "-raw"
        if self.scalars != DEFAULT_SCALARS:
            tag += "-b%g-m%g-s%g" % self.scalars
        if self.n != N_RAYS:
            tag += f"-N{self.n}"
        if self.zero_normal:
            tag += "-zero"
        return tag


def _case_list():
    c = []
    # minimum, no interior (S = 2: 37 cosines in all, too few for the mask to be sure of 8 of them)
    c += [Case(2, 1, "noise", th=-2.0), Case(2, 11, "noise", th=-2.0), Case(3, 1, "noise", th=-2.0), Case(3, 11, "noise")]
    # W = 11: start = 7, interior [7, S - 8): empty at S = 15, exactly sample 7 at S = 16
    c += [Case(15, 11, "noise"), Case(16, 11, "noise", th=-2.0)]
    # one wave of samples: C 1 -> 2
    c += [Case(63, 5, "crossing"), Case(64, 5, "crossing"), Case(64, 5, "crossing", th=-2.0), Case(65, 5, "crossing", th=-2.0)]
    # backward rays per workgroup 16 -> 8 -> 4
    c += [Case(80, 11, "crossing", th=-2.0), Case(81, 11, "crossing"), Case(160, 11, "crossing"), Case(161, 11, "crossing", th=-2.0)]
    # shipped sizes
    c += [Case(135, 11, "crossing"), Case(135, 11, "crossing", th=-2.0), Case(135, 11, "empty", th=-2.0)]
    # backward maximum, C = 4, even window
    c += [Case(256, 4, "crossing"), Case(256, 11, "crossing"), Case(256, 11, "crossing", th=-2.0)]
    # forward only, C = 5 and 8
    c += [Case(257, 11, "crossing"), Case(512, 11, "crossing", th=-2.0)]
    # one ray: one wave works, fifteen wait at the workgroup's barrier
    c += [Case(64, 11, "noise", n=1)]
    # un-normalised weights
    c += [Case(64, 5, "crossing", normalize=0), Case(135, 11, "crossing", normalize=0), Case(256, 11, "crossing", normalize=0)]
    # density scalars: sharp beta; beta below beta_min; mean outside both bounds; negative scale; scale below scale_min
    for sc in ((0.5, 0.5, 100.0), (0.5, 1.2, 100.0), (0.5, 0.7, -100.0), (0.5, 0.7, 0.5)):
        c += [Case(64, 5, "crossing", scalars=sc), Case(135, 11, "crossing", scalars=sc)]
    # The two sharp settings run on the noise family.  Under beta = 0.05 a density worth the name needs c < -0.3 and under beta = 5e-5
    # (clamped to 1e-4: a step at c = -mean) c < -0.7; the crossing family's windowed cosines stay above -0.2, where float32 holds
    # nothing of the cdf 0.5 + 0.5 sg (1 - E) (grain 6e-8 x scale), while the adjacent cosines of noise reach -1.  Under the step
    # the first cosine of every ray is put within 3e-4 of it, under beta = 0.05 beyond -0.6 (_draw_ray), so that every ray has a
    # density and a gradient; no mask, which would take that sample away from four rays in ten.
    for sc in ((0.05, 0.7, 100.0), (5e-5, 0.7, 100.0)):
        c += [Case(64, 5, "noise", th=-2.0, scalars=sc), Case(135, 11, "noise", th=-2.0, scalars=sc)]
    return tuple(c)


CASES = _case_list()
ZERO_NORMAL_CASE = Case(64, 11, "noise", zero_normal=True)
ALL_CASES = CASES + (ZERO_NORMAL_CASE,)


def density_params(case: Case) -> O.DensityParams:
    return O.DensityParams(beta=case.scalars[0], mean=case.scalars[1], scale=case.scalars[2], cutoff=CUTOFF, **BOUNDS)


def scalar_tensors(case: Case, dtype):
    """The three raw scalars as the float32 values the kernel reads, in ``dtype``, each of shape [1]: a 0-dim float64 scalar would not
    promote the oracle's [1]-shaped float32 cutoff tensor, and the cdf of the cutoff would stay a float32 evaluation."""
    return [torch.tensor([v], dtype=torch.float32).to(dtype) for v in case.scalars]


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def _draw_ray(g: torch.Generator, case: Case):
    """One ray -> (normals [S,3], z [S], ray_dir [3], colours [S,3]) in float32."""
    s = case.s

    def rand(*shape):
        return torch.rand(*shape, generator=g, dtype=F64)

    def randn(*shape):
        return torch.randn(*shape, generator=g, dtype=F64)

    # spacings log-uniform from 1e-4 up to 1; up to 1e-2 for noise, whose samples are mostly dense (sigma of 20 and more): those
    # rays stay transparent and their weights spread
    gaps = 10.0 ** (-4.0 + (2.0 if case.family == "noise" else 4.0) * rand(s - 1))
    d = _unit(randn(3))
    if case.family == "noise":
        field = randn(s, 3)
        if case.scalars[0] < DEFAULT_SCALARS[0]:
            # A sharp beta leaves most of a noise ray without density, and a ray whose whole weight is 1e-5 is the empty family's
            # business (1 - exp(-e) holds three digits of it).  The first cosine of the ray is put where the density is: beyond -0.6
            # under beta = 0.05, and under beta_min, where the density is a step of width 1e-4 at c = -mean, on the step itself.
            mean = min(max(case.scalars[1], BOUNDS["mean_bounds"][0]), BOUNDS["mean_bounds"][1])
            c0 = -mean + 3e-4 * (2.0 * rand(1) - 1.0) if case.scalars[0] < BOUNDS["beta_bounds"][0] else -0.6 - 0.35 * rand(1)
            u0 = _unit(field[0])
            field[1] = c0 * u0 + torch.sqrt(1 - c0 ** 2) * _unit(torch.linalg.cross(u0, randn(3)))
    else:
        # the ray meets the field at |cos| >= 0.3, so that c_ray sits on one side of either threshold before the surface and on the
        # other behind it: half of the rays have their crossing under the mask
        cos_d = torch.sign(randn(1)) * (0.3 + 0.65 * rand(1))
        v = _unit(cos_d * d + torch.sqrt(1 - cos_d ** 2) * _unit(torch.linalg.cross(d, randn(3))))
        field_noise = 0.15 * randn(s, 3)
        t = torch.arange(s, dtype=F64) / (s - 1)
        u = rand(4)
        cos_t = 0.2 + 0.28 * rand(3)                       # tilted samples: 61 to 78 degrees away from v, a cosine just under the cutoff
        side = _unit(torch.linalg.cross(v.expand(3, 3), randn(3, 3)))
        if case.family == "crossing":
            kx = int((0.25 + 0.5 * u[1]) * (s - 1))
            t0 = (kx + 0.5) / (s - 1)
            if u[3] < 0.5:      # half of the rays: spacings of about 1 around the crossing, so that the transmittance saturates
                gaps[kx - 1:kx + 2] = 0.5 + rand(3)
            # three rays in ten: one tilted sample among the first or the last `start`, where the cosine is the plain adjacent one
            edge = 1 + int(u[2] * 2 * (case.start - 1))
            k = torch.tensor([edge if edge < case.start else s - 2 - (edge - case.start)] if u[0] < 0.3 else [], dtype=torch.long)
        else:
            t0 = 1.5
            k = torch.randperm(s - 2, generator=g)[: 1 + int(3 * u[0])] + 1
            gaps[k] = 1e-4 * (0.5 + 1.5 * rand(k.numel()))
            gaps[k - 1] = 1e-4 * (0.5 + 1.5 * rand(k.numel()))
        field = v * torch.tanh(40.0 * (t0 - t)).unsqueeze(-1) + field_noise
        m = k.numel()
        field[k] = torch.sign(field[k] @ v).unsqueeze(-1) * (cos_t[:m].unsqueeze(-1) * v + torch.sqrt(1 - cos_t[:m] ** 2).unsqueeze(-1) * side[:m])
    z = 0.5 + rand(1) + torch.cat([torch.zeros(1, dtype=F64), torch.cumsum(gaps, 0)])
    normals = field * torch.exp(1.15 * randn(s, 1))          # lengths over about three decades (+- 3 sigma: e^{+-3.45})
    if case.zero_normal:
        normals[int(torch.randint(0, s, (1,), generator=g))] = 0.0
    colors = rand(s, 3)
    z32 = z.float()
    assert bool((z32[1:] > z32[:-1]).all())
    return normals.float(), z32, d.float(), colors.float()


@dataclass(frozen=True, eq=False)
class Inputs:
    case: Case
    normals: torch.Tensor      # [N,S,3] float32
    z: torch.Tensor            # [N,S]
    ray_dirs: torch.Tensor     # [N,3]
    colors: torch.Tensor       # [N,S,3]
    a: torch.Tensor            # [N,3]   d loss / d rgb
    b: torch.Tensor            # [N,1]   d loss / d depth
    cw: torch.Tensor           # [N,S]   d loss / d weights
    gs: torch.Tensor           # [N,S]   d loss / d sigma (the sigma entry point)
    redraws: Tuple[int, ...]   # per ray


def forward_parts(case: Case, normals, z, ray_dirs, scalars):
    """The two oracle calls of render() -> (sigma, windowed cosine, cosine to the ray, weights), in the dtype of the arguments."""
    sigma, c, c_ray = O.ray_density(normals, ray_dirs, case.w, case.th, density_params(case), *scalars, return_parts=True)
    return sigma, c, c_ray, O.volsdf_weights(z, sigma, bool(case.normalize))


def margin_failures(case: Case, normals, z, ray_dirs) -> torch.Tensor:
    """[N] bool: rays with a sample inside a decision margin of the float64 evaluation (module docstring)."""
    dt = F64
    scal = scalar_tensors(case, dt)
    _, c, c_ray, w = forward_parts(case, normals.to(dt), z.to(dt), ray_dirs.to(dt), scal)
    p = density_params(case)
    beta = torch.clamp(scal[0], torch.tensor(p.beta_bounds[0]), torch.tensor(p.beta_bounds[1]))
    mean = torch.clamp(scal[1], torch.tensor(p.mean_bounds[0]), torch.tensor(p.mean_bounds[1]))
    scale = torch.max(scal[2].abs(), torch.tensor(p.scale_min))
    raw = O.laplace_cdf(-c, beta, scale, mean) - O.laplace_cdf(torch.tensor([p.cutoff], dtype=dt), beta, scale, mean)
    bad = ((raw.abs() / scale < MARGIN) & ((c + p.cutoff).abs() < FLAT_MARGIN)).any(dim=1)
    bad |= ((c.abs() < MARGIN) & (c_ray < case.th)).any(dim=1)
    bad |= (((c_ray - case.th).abs() < MARGIN) & (c < 0)).any(dim=1)
    top = torch.topk(w, 2, dim=1).values
    bad |= (top[:, 0] > 0) & (top[:, 0] - top[:, 1] < MARGIN * top[:, 0])
    return bad


@functools.lru_cache(maxsize=None)
def make_inputs(case: Case) -> Inputs:
    """Deterministic from the case (the seed is a digest of its id).  Every returned ray satisfies the margins."""
    seed = int.from_bytes(__import__("hashlib").sha256(case.id.encode()).digest()[:4], "little")
    g = torch.Generator().manual_seed(seed)
    rays = [_draw_ray(g, case) for _ in range(case.n)]
    redraws = [0] * case.n
    while True:
        normals, z, d, colors = (torch.stack([r[i] for r in rays]) for i in range(4))
        bad = margin_failures(case, normals, z, d)
        if not bool(bad.any()):
            break
        for r in torch.nonzero(bad).reshape(-1).tolist():
            redraws[r] += 1
            assert redraws[r] < MAX_REDRAWS, f"{case.id}: ray {r} drawn {MAX_REDRAWS} times without clearing the margins"
            rays[r] = _draw_ray(g, case)
    n, s = case.n, case.s
    a, b = torch.randn(n, 3, generator=g), torch.randn(n, 1, generator=g)
    cw, gs = torch.randn(n, s, generator=g), torch.randn(n, s, generator=g)
    return Inputs(case, normals.contiguous(), z.contiguous(), d.contiguous(), colors.contiguous(), a, b, cw, gs, tuple(redraws))


# ------------------------------------------------------------------------------------------------
# evaluation: the oracle in ``dtype`` + autograd
# ------------------------------------------------------------------------------------------------
def _graph(inp: Inputs, dtype, upstream, grads: bool, scalars=None):
    """The oracle on ``inp`` -> (outputs, per-ray loss [N], leaves [normals, colours, beta, mean, scale]).  The three scalar leaves
    are [N] copies of the scalar, one per ray, handed to the oracle sample by sample ([N (S - 1), 1], the shape of its cosines): the
    same arithmetic on every element, and one backward pass gives every ray's own contribution to the scalar's gradient."""
    case = inp.case
    normals = inp.normals.to(dtype).requires_grad_(grads)
    colors = inp.colors.to(dtype).requires_grad_(grads)
    scal = [t.to(dtype).expand(case.n).clone().requires_grad_(grads) for t in (scalar_tensors(case, dtype) if scalars is None else scalars)]
    z = inp.z.to(dtype)
    per_sample = [t.reshape(-1, 1).expand(case.n, case.s - 1).reshape(-1, 1) for t in scal]
    sigma, c, c_ray, w = forward_parts(case, normals, z, inp.ray_dirs.to(dtype), per_sample)
    rgb = torch.sum(w.unsqueeze(-1) * colors, dim=1)
    depth = torch.sum(w.unsqueeze(-1) * z.unsqueeze(-1), dim=1)
    out = dict(sigma=sigma, weights=w, rgb=rgb, depth=depth, c=c, c_ray=c_ray)
    loss = torch.zeros(z.shape[0], dtype=dtype)
    if "rgb" in upstream:
        loss = loss + (rgb * inp.a.to(dtype)).sum(dim=1)
    if "depth" in upstream:
        loss = loss + (depth * inp.b.to(dtype)).sum(dim=1)
    if "weights" in upstream:
        loss = loss + (w * inp.cw.to(dtype)).sum(dim=1)
    if "sigma" in upstream:
        loss = loss + (sigma * inp.gs.to(dtype)).sum(dim=1)
    return out, loss, [normals, colors] + scal


def _grad(loss, leaves):
    got = torch.autograd.grad(loss, leaves, allow_unused=True)
    return [torch.zeros_like(x) if y is None else y for x, y in zip(leaves, got)]


def evaluate(inp: Inputs, dtype, upstream=FULL, grads: bool = True) -> Dict[str, torch.Tensor]:
    """The oracle on ``inp`` in ``dtype`` -> sigma, weights, rgb, depth, argmax, c, c_ray and, with ``grads``, the gradients of
        loss = [rgb] sum a rgb + [depth] sum b depth + [weights] sum cw w + [sigma] sum gs sigma      (terms named in ``upstream``)
    with respect to the normals, the colours and the three raw scalars: d_normals, d_colors, scalar_parts [N,3] (every ray's own
    contribution) and d_scalars [3], their sum over the rays."""
    out, loss, leaves = _graph(inp, dtype, upstream, grads)
    out = {k: v.detach() for k, v in out.items()}
    out["argmax"] = torch.argmax(out["weights"], dim=-1)
    if not grads:
        return out
    gr = _grad(loss.sum(), leaves)
    parts = torch.stack(gr[2:], dim=1)
    out.update(d_normals=gr[0], d_colors=gr[1], scalar_parts=parts, d_scalars=parts.sum(dim=0))
    return out


def loss_value(inp: Inputs, upstream=FULL, scalars=None, ray=None) -> float:
    """The loss of ``evaluate`` in float64 (of one ray, if named), without gradients.  ``inp`` may hold float64 tensors and
    ``scalars`` three float64 0-dim tensors: the displaced arguments of a difference quotient."""
    with torch.no_grad():
        loss = _graph(inp, F64, upstream, False, scalars)[1]
        return float(loss.sum() if ray is None else loss[ray])


@functools.lru_cache(maxsize=None)
def reference(case: Case, upstream=FULL) -> Dict[str, torch.Tensor]:
    return evaluate(make_inputs(case), F64, upstream, grads=case.backward)


@functools.lru_cache(maxsize=None)
def host_fp32(case: Case, upstream=FULL) -> Dict[str, torch.Tensor]:
    return evaluate(make_inputs(case), torch.float32, upstream, grads=case.backward)


# ------------------------------------------------------------------------------------------------
# scoring
# ------------------------------------------------------------------------------------------------
def per_ray_error(x: torch.Tensor, ref: torch.Tensor, only: torch.Tensor = None) -> torch.Tensor:
    """[N]: max |x - ref| / max |ref| over each ray's entries; a ray whose reference is all zero scores 0 when x is exactly zero there
    and infinity otherwise.  ``only`` (bool, x's shape): the entries that count, on the scale of those entries alone."""
    n = ref.shape[0]
    x, ref = x.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    if only is not None:
        x, ref = x * only, ref * only
    x, ref = x.reshape(n, -1), ref.reshape(n, -1)
    err, scale = (x - ref).abs().amax(dim=1), ref.abs().amax(dim=1)
    exact = (x == 0).all(dim=1)
    return torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(exact, torch.zeros_like(err), torch.full_like(err, float("inf"))))


def scalar_error(d_scalars: torch.Tensor, ref: Dict[str, torch.Tensor]) -> torch.Tensor:
    """[3]: |x - ref| / sum_rays |ray's float64 contribution| (the sum over rays cancels); where no ray contributes the gradient
    must be exactly 0 (infinity otherwise)."""
    x = d_scalars.detach().to("cpu", F64).reshape(3)
    scale = ref["scalar_parts"].abs().sum(dim=0)
    err = (x - ref["d_scalars"]).abs()
    return torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(x == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))


def zero_normal_mask(inp: Inputs) -> torch.Tensor:
    """[N,S,1] bool: the samples whose normal is exactly zero."""
    return (inp.normals == 0).all(dim=2, keepdim=True)


def score(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor], names, zero: torch.Tensor = None) -> Dict[str, float]:
    """Worst per-ray error of each named per-ray quantity; 'd_scalars' -> d_beta, d_mean, d_scale on their own scale.  With ``zero``
    (zero_normal_mask) d_normals is scored without those samples, whose gradient is 1e8 times their neighbours', and they are scored
    on their own scale as 'd_normals.zero'."""
    out = {}
    for k in names:
        if k == "d_scalars":
            e = scalar_error(got[k], ref)
            out.update({f"d_{name}": float(e[i]) for i, name in enumerate(SCALAR_NAMES)})
        elif k == "d_normals" and zero is not None:
            out[k] = float(per_ray_error(got[k], ref[k], ~zero.expand_as(ref[k])).max())
            out[k + ".zero"] = float(per_ray_error(got[k], ref[k], zero.expand_as(ref[k])).max())
        else:
            out[k] = float(per_ray_error(got[k], ref[k]).max())
    return out


GRAD_NAMES = ("d_normals", "d_colors", "d_scalars")


MARGIN_FACTOR = 8.0


def pool_key(case: Case):
    """Cases whose yardsticks are pooled: one input family under one setting of the density scalars, the rays of two or three
    samples apart (their whole weight is about 1e-5, of which 1 - exp(-e) holds three digits).  (Finer than a pool per family,
    so no bound is wider than that pool's: under a sharp beta or a scale of 1 the float32 form of the cdf, 0.5 + 0.5 sg (1 - E), and
    of 1 - exp(-e) lose digits that the shipped scalars keep, and one such case would set the bound of the whole family.)"""
    return (case.family, case.scalars, case.s <= 3)


def case_scores(case: Case, run, upstream=FULL, prefix="") -> Dict[str, float]:
    """``run`` (host_fp32, or the device's outputs as a dict) against the float64 reference, every quantity the case has."""
    ref = reference(case, upstream)
    zero = zero_normal_mask(make_inputs(case)) if case.zero_normal else None
    names = (PER_RAY if upstream == FULL else ()) + (GRAD_NAMES if case.backward else ())
    return {prefix + k: v for k, v in score(run, ref, [k for k in names if k in run], zero).items()}


@functools.lru_cache(maxsize=None)
def yardstick() -> Dict[tuple, Dict[str, float]]:
    """{pool_key: {quantity: error}}: the oracle in float32 on the host against the oracle in float64, on the inputs of every case,
    scored per ray as the device is and pooled as the maximum over the cases of a pool.  The gradients of one upstream term alone are
    quantities of their own ('depth.d_normals', 'sigma.d_beta', ...): d_depth alone is the worst conditioned of them, its dL/dw_j =
    b z_j are nearly equal over the few samples that carry weight and the normalisation takes their weighted mean off again."""
    pool = {}
    for case in ALL_CASES:
        scores = case_scores(case, host_fp32(case))
        if case.backward:
            for upstream in ALONE:
                host = host_fp32(case, upstream)
                names = ("d_normals", "d_scalars") + (("d_colors",) if upstream == ("rgb",) else ())
                scores.update(case_scores(case, {k: host[k] for k in names}, upstream, upstream[0] + "."))
        mine = pool.setdefault(pool_key(case), {})
        for k, v in scores.items():
            mine[k] = max(mine.get(k, 0.0), v)
    return pool


def bound(case: Case, quantity: str) -> float:
    """MARGIN_FACTOR x the pooled host-float32 yardstick: what the device may differ from float64 by."""
    return MARGIN_FACTOR * yardstick()[pool_key(case)][quantity]


# ------------------------------------------------------------------------------------------------
# what the cases cover (float64 side)
# ------------------------------------------------------------------------------------------------
def coverage(case: Case) -> Dict[str, float]:
    inp, ref = make_inputs(case), reference(case)
    s, start = case.s, case.start
    sigma, c, c_ray = ref["sigma"][:, :-1], ref["c"], ref["c_ray"]
    unmasked = O.ray_density(inp.normals.to(F64), inp.ray_dirs.to(F64), case.w, -2.0, density_params(case), *scalar_tensors(case, F64))[:, :-1]
    j = torch.arange(s - 1)
    border = (j < start) | (j >= s - 1 - start)
    what = O.volsdf_weights(inp.z.to(F64), ref["sigma"], False)
    return dict(masked_active=int(((c_ray < case.th) & (c < 0) & (unmasked > 0)).sum()), relu_off=int((unmasked == 0).sum()),
                active_border=int((sigma[:, border] > 0).sum()), active_interior=int((sigma[:, ~border] > 0).sum()),
                min_final_transmittance=float((1.0 - what.sum(dim=1)).min()), min_what_sum=float(what.sum(dim=1).min()),
                max_what_sum=float(what.sum(dim=1).max()), redraws=int(sum(inp.redraws)), max_redraws=int(max(inp.redraws)))
