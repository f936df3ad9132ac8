"""Networks, inputs, the float64 restatement and scoring for the MLP forward tests (tests/test_mlp_host.py, tests/test_hip_mlp.py).

Restatement.  ``vf64`` / ``rn64`` evaluate the two nets in the dtype of their arguments from the reference's formulas
(vector_field_network.py:177-208, rendering_network.py:62-108, embedder.py:11-37): Linear, then BatchNorm1d applied AS BatchNorm,
(y - running_mean) / sqrt(running_var + 1e-5) * gamma + beta, never folded into the Linear; ReLU between layers, tanh / sigmoid on the
last; the skip layer reads cat([x, pe]) divided by the float32 sqrt(2).  The float32 parameters and inputs are widened exactly and the
encoding arguments x 2^k are exact, so the float64 values are those of the very net the kernels get.  (The packs multiply the skip
layer by 0.70710678f, one ulp from 1 / float32 sqrt(2): below every yardstick here.)  tests/test_mlp_host.py holds the restatement to
the oracle (oracle/vfnerf_oracle.py: vf_mlp, render_mlp) run in float64.

Networks (``build_net``), 256 wide but the narrow one:
  c1_det, trained_256, trained_far            fixtures as stored (every running_mean 0, every running_var 1)
  <fixture>+stats                             the same with BatchNorm statistics drawn per output row (``randomise_statistics``):
                                              running_var log-uniform in [1e-3, 4], gamma such that gamma / sqrt(var + eps) is uniform in
                                              [0.5, 1.5], running_mean 0.3 N(0,1), beta 0.2 N(0,1).  With var at 1e-3 a dropped eps moves a
                                              folded weight by 5e-3 of itself, not 5e-6
  c1_det+stats+hot                            the hidden Linear weights of that net scaled (``_heat``): up by G in the first three hidden
                                              layers (two of the rendering net's four), down in the others by as much in all, G found by
                                              bisection so that the largest float64 pre-activation is about 500 (the f16x3 clamp acts at
                                              937).  The activations are back at their ordinary size before the last Linear, so tanh and
                                              sigmoid do not saturate and hide everything, and no layer needs weights below the range the
                                              guard accepts (one gain on every layer would: a last Linear that maps activations of 500 to
                                              pre-tanh values of 1 has folded weights of 1e-3, which f16 halves hold to 14 bits)
  vf_2h, vf_4h_skip1, vf_8h_skip7             freshly constructed vector-field nets: 2 hidden layers, no skip, no encoding, no features, no
                                              BatchNorm; 4 hidden layers, skip at 1, multires 3, features, BatchNorm; 8 hidden layers with the
                                              skip at layer 7, the last position vfn_make_plan accepts
  rn_<h>h_m<L>                                rendering nets with h = 1, 3 hidden layers and multires L = 0, 2, 5 (6 + 3 + 6 L <= 40 columns
                                              of the encoding tile: 5 is the largest)
  vf_4h_w64                                   a narrow vector field: 4 hidden layers of 64, skip at 2, multires 6, 32 features, BatchNorm.  The
                                              fused kernels have no such geometry: it runs layer by layer (vf_nerf_amd/batchstat.py)
  Fresh nets keep torch's default initialisation with the hidden weights times GAIN (synthetic.scale_hidden_weights) and randomised
  statistics where they have BatchNorm.  They run on the exact-fp32 kernels only (the f16x3 kernels are specialised for the shipped
  geometry).

Inputs.  One family = one network at one coordinate scale s in SCALES: POOL rows drawn once, coordinates uniform in [-s, s]^3, unit view
directions; row 1 is the point (0, 0, 0) and row 2 starts with -0.0.  A drawn row is rejected, by the float64 restatement alone, when
its vector output has max |component| < ROW_FLOOR or its feature row has max |entry| < ROW_FLOOR (a relative error on such a row
measures nothing).  A case of M rows is the first M rows of the pool, so one float64 and one float32 evaluation serve every case of the
family.  M_VALUES touches every tile edge of both kernels (64 points per workgroup in the fp32 kernel; 32 per wave, 128 per workgroup
in the f16x3 kernel); FUSED_CASES are (samples per ray, rays) with ray boundaries inside a wave and M no multiple of 32.

Scoring, per row and per column, never per tensor (``score``):
  vector, colours   max_c |x - x64| / max_c |x64| over the row
  feat_rows         the same over the 256 feature columns of the row
  feat_cols         max_rows |x - x64| / max(max_rows |x64|, ROW_FLOOR) over the rows of the case, per column.  The floor is the one
                    the rows are held to, and it only acts on cases of a few rows: no column can be rejected, and without it the
                    figure at M = 1 is the relative error of single entries, which no float32 evaluation delivers for an entry of
                    1e-4 that a sum of O(1) terms cancelled down to.  (Measured without the floor: the exact-fp32 kernel at 8.2 x a
                    pooled host yardstick of 1e-5 .. 1e-3 at M = 1, and at most 0.48 x from M = 31 on: a bound that is out of
                    float32's reach for one case and lets a column that lost its low half pass in all others.  With it the
                    yardstick is 1e-6 at every M.)
The worst row / column of a case is its score.  Colours are sigmoid outputs: where the rendering net is driven far into saturation
(trained_far at coordinate scale 300: pre-sigmoid values below -88) float32 underflows to 0 against 1e-44 in float64, the host
yardstick is 1 and the bound on the colours of that family says nothing; every other family's does.
Yardstick: the float32 oracle on the host against float64, scored the same way on the same cases and pooled as the worst over the cases
of the family (``yardstick``).  A kernel may differ from float64 by its factor times that (test_hip_mlp.py; 8 at the most, the project's
factor for exact-fp32 kernels).

Gradients (``vf_grad_case`` / ``rn_grad_case``, nets GRAD_VF and GRAD_RN).  The pool rows of a net at coordinate scale 1 that keep every
pre-activation KINK_MARGIN away from zero (fewer than KINK_CAP of the pool may fail that; c1_det+stats and the hot net do and stay
out), a fixed random ``coef``, and float64 autograd of the restatement of sum(out * coef): every parameter and, from the same backward,
every input (``input_grads``).  A case of M rows (GRAD_M) is the first M kink-free rows with the first M rows of ``coef``.
Scoring (``grad_score``), per parameter tensor and never by the tensor alone:
  rows      a weight matrix per output row; an input gradient [M, c] per sample row
  blocks    a weight that reads raw inputs, per named block of input columns (``column_blocks``): xyz and each sin / cos triple of the
            vector field's first layer; the hidden block, then the same, of its skip layer; points, each view-direction block, normals
            and features of the rendering net's first layer
  elems     a bias, gamma or beta per element
  each figure max |err| over the row, block or element / max(largest |float64 entry| there, GRAD_FLOOR x the tensor's largest
  |entry|): a condition, not a measurement, and nothing is rejected; a row below one percent of its tensor is held in absolute terms at
  that percent, so the figure is exactly relative above it and never more than 100 x stricter than max |err| / max |ref| over the
  tensor ('tensor', helpers.grad_rel_err, printed beside it).
Yardstick (``grad_yardstick``): the float32 restatement under float32 autograd on the host, on the same rows and ``coef``, scored the
same way, pooled as the worst over GRAD_M per net, tensor kind (``grad_kind``) and figure.

``emulate_f16x3``: the split arithmetic of csrc/vfn_mlp16.hip in float64 with exact sums, for the host test's question whether the
scoring tells a right kernel from a subtly wrong one: weights folded in float32 as the pack kernel folds them and split as
hi = f16(w), lo = f16(w - hi); operands ride at 64 x their value, hi = f16(64 x), lo = f16(64 x - hi); every product is
hi hi + hi lo + lo hi.  ``plant`` names one deliberate error: "cross" drops the w_lo x_hi term, "eps" the + 1e-5 of the fold,
"mean" turns b - mean into b + mean.
"""
from __future__ import annotations

import functools
import hashlib
import math
import types
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

import helpers
from oracle import vfnerf_oracle as O
from vf_nerf_amd import networks, settings, synthetic

F64 = torch.float64
BN_EPS = 1e-5
SQRT2_F32 = float(torch.sqrt(torch.tensor([2.0]))[0])      # the float32 sqrt(2) of the reference, widened
SCALES = (1.0, 4.0, 30.0, 300.0)
M_VALUES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 513)
FUSED_CASES = ((1, 513), (3, 171), (37, 13), (200, 3))     # (samples per ray, rays): 513, 513, 481 and 600 rows
POOL = 600
DRAWN = 720
ROW_FLOOR = 0.05
REJECT_CAP = 0.05
HOT_INTERVAL = (300.0, 800.0)
HOT_TARGET = 500.0
GAIN = 2.0
KINK_MARGIN = 1e-4
GRAD_ROWS = 513
GRAD_M = (1, 31, 33, 257, None)                            # rows of a gradient case; None: all its rows (at most GRAD_ROWS).  _groups(m) of
                                                           # both backward paths is 1 below 512 rows and 2 from there on
GRAD_FLOOR = 1e-2
MAX_FACTOR = 8.0

FIXTURES = ("c1_det", "trained_256", "trained_far")
STATS = tuple(f + "+stats" for f in FIXTURES)
HOT = "c1_det+stats+hot"
FRESH_VF = {"vf_2h": dict(hidden=2, skip=None, multires=0, feats=0, bn=False),
            "vf_4h_skip1": dict(hidden=4, skip=1, multires=3, feats=256, bn=True),
            "vf_8h_skip7": dict(hidden=8, skip=7, multires=6, feats=256, bn=True)}
NARROW_VF = {"vf_4h_w64": dict(hidden=4, skip=2, multires=6, feats=32, bn=True, width=64)}      # layer-at-a-time kernels only
FRESH_RN = {f"rn_{h}h_m{mr}": dict(hidden=h, multires=mr) for h in (1, 3) for mr in (0, 2, 5)}
GRAD_NETS = ("trained_256+stats", "trained_far+stats")     # stand-alone gradient cases (c1_det+stats: 50.5 % of its rows sit within
                                                           # the margin of a kink in the vector-field net, above the cap of one half)
KINK_CAP = 0.5
SHIPPED_NETS = FIXTURES + STATS + (HOT,)                   # both kernels
ALL_NETS = SHIPPED_NETS + tuple(FRESH_VF) + tuple(FRESH_RN)
GRAD_VF = GRAD_NETS + tuple(FRESH_VF) + tuple(NARROW_VF)   # nets whose vector field / rendering net has gradient cases
GRAD_RN = GRAD_NETS + tuple(FRESH_RN)


F16X3_CLAMP = 937.5            # csrc/vfn_mlp16.hip: VFN16_CLAMP / 2^6
F16X3_INSIDE, F16X3_OUTSIDE = 900.0, 945.0


def f16x3_range(peak: float) -> str:
    """``peak``: the largest float64 pre-activation of a case.  'inside': below 900, the f16x3 kernels promise fp32-equivalent values
    and must leave the status word 0; 'outside': above 945, the ReLU clamp must act and say so; 'edge' in between (neither is asked)."""
    return "inside" if peak < F16X3_INSIDE else ("outside" if peak > F16X3_OUTSIDE else "edge")


def scales_of(name: str) -> Tuple[float, ...]:
    """The hot net is calibrated on, and runs at, coordinate scale 1: its point is the size of the activations."""
    return (1.0,) if name == HOT else SCALES


def _seed(tag: str) -> int:
    return int.from_bytes(hashlib.sha256(tag.encode()).digest()[:4], "little")


# ------------------------------------------------------------------------------------------------
# restatement
# ------------------------------------------------------------------------------------------------
def widen(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {k: v.detach().cpu().to(F64) for k, v in sd.items() if v.is_floating_point()}


def n_layers(sd) -> int:
    return max(int(k.split(".")[1]) for k in sd if k.startswith("layers.")) + 1


def encode(x: torch.Tensor, multires: int) -> torch.Tensor:
    if multires == 0:
        return x
    parts = [x]
    for k in range(multires):
        arg = x * float(2 ** k)
        parts += [torch.sin(arg), torch.cos(arg)]
    return torch.cat(parts, dim=-1)


def _linear_bn(sd, i: int, x: torch.Tensor) -> torch.Tensor:
    if f"layers.{i}.weight" in sd:
        return x @ sd[f"layers.{i}.weight"].T + sd[f"layers.{i}.bias"]
    y = x @ sd[f"layers.{i}.0.weight"].T + sd[f"layers.{i}.0.bias"]
    p = f"layers.{i}.1."
    return (y - sd[p + "running_mean"]) / torch.sqrt(sd[p + "running_var"] + BN_EPS) * sd[p + "weight"] + sd[p + "bias"]


def vf64(points, sd, multires: int, skip_in=(), trace: Optional[list] = None) -> torch.Tensor:
    """[M,3] -> [M, 3 + F]; ``trace`` receives every hidden layer's pre-activation."""
    pe = encode(points, multires)
    x, n = pe, n_layers(sd)
    for i in range(n):
        if i in skip_in:
            x = torch.cat([x, pe], dim=1) / SQRT2_F32
        y = _linear_bn(sd, i, x)
        if i == n - 1:
            return torch.tanh(y)
        if trace is not None:
            trace.append(y.detach())
        x = torch.relu(y)


def rn64(points, normals, view_dirs, feats, sd, multires: int, trace: Optional[list] = None) -> torch.Tensor:
    x, n = torch.cat([points, encode(view_dirs, multires), normals, feats], dim=-1), n_layers(sd)
    for i in range(n):
        y = _linear_bn(sd, i, x)
        if i == n - 1:
            return torch.sigmoid(y)
        if trace is not None:
            trace.append(y.detach())
        x = torch.relu(y)


# ------------------------------------------------------------------------------------------------
# networks
# ------------------------------------------------------------------------------------------------
class Net:
    """A vector-field module and / or a rendering module on the host, in eval mode."""

    def __init__(self, name: str, vf, rn) -> None:
        self.name, self.vf, self.rn = name, vf, rn
        for m in (vf, rn):
            if m is not None:
                m.eval()

    @property
    def f16x3(self) -> bool:
        return self.name in SHIPPED_NETS

    @property
    def vf_args(self):
        return dict(multires=self.vf._multires(), skip_in=tuple(self.vf.skip_connection_in))

    @property
    def has_feats(self) -> bool:
        return self.vf is not None and self.vf._feature_dims() > 0

    def vf_sd(self, dtype=F64):
        return {k: v.detach().to(dtype) for k, v in self.vf.state_dict().items() if v.is_floating_point()}

    def rn_sd(self, dtype=F64):
        return {k: v.detach().to(dtype) for k, v in self.rn.state_dict().items() if v.is_floating_point()}

    def on(self, device):
        """(vf, rn) rebuilt from their configs on ``device`` with these parameters and statistics."""
        out = []
        for m in (self.vf, self.rn):
            if m is None:
                out.append(None)
                continue
            c = type(m)(m.config)
            c.load_state_dict(m.state_dict())
            c.eval()
            out.append(c.to(device))
        return out


def _bn_layers(mod):
    return [mod._bn(i) for i in range(mod.num_layers) if mod._bn(i) is not None]


@torch.no_grad()
def randomise_statistics(mod, gen: torch.Generator) -> None:
    for bn in _bn_layers(mod):
        n = bn.num_features
        var = (10.0 ** (math.log10(1e-3) + (math.log10(4.0) - math.log10(1e-3)) * torch.rand(n, generator=gen, dtype=F64))).float()
        s = 0.5 + torch.rand(n, generator=gen, dtype=F64)
        bn.running_var.copy_(var)
        bn.weight.copy_((s * torch.sqrt(var.double() + BN_EPS)).float())
        bn.running_mean.copy_((0.3 * torch.randn(n, generator=gen, dtype=F64)).float())
        bn.bias.copy_((0.2 * torch.randn(n, generator=gen, dtype=F64)).float())


def _fresh_vf(hidden: int, skip, multires: int, feats: int, bn: bool, width: int = 256):
    cfg = settings.VFNetConfig(input_dims=3, output_dims=3, dimensions=[width] * hidden, feature_vector_dims=feats, embedder_multires=multires,
                               weight_norm=False, batch_norm=bn, skip_connection_in=[skip] if skip is not None else [], bias_init=0.0,
                               dropout=False, dropout_probability=0.0, xavier_init=False, init="")
    return networks.VectorFieldNetwork(cfg)


def _fresh_rn(hidden: int, multires: int):
    cfg = settings.RenderingNetConfig(output_dims=3, dimensions=[256] * hidden, feature_vector_dims=256, weight_norm=False, batch_norm=True,
                                      mode="idr", embedder_multires=multires, detach_normals=True)
    return networks.RenderingNetwork(cfg)


_NOTHING = types.SimpleNamespace(layers=[])


def _hidden_linears(mod):
    return [mod._linear(i) for i in range(mod.num_layers - 1)]


HOT_UP = 3        # the first HOT_UP hidden layers of a hot net (2 of the rendering net's 4) are scaled up, the others down


@torch.no_grad()
def _heat(mod, forward, target: float) -> float:
    """Hidden Linear weights of ``mod`` times G in the first layers and G^-(up / down) in the others, so that the gains multiply to 1:
    the activations rise to the hot layers and come back down before the last Linear, which stays as it is, and every layer keeps folded
    weights of ordinary size (0.02 .. 3: the range guard asks for more than 2^-9 per layer).  G by bisection on log2 G such that the
    largest pre-activation ``forward(trace)`` traces is ``target``.  -> G."""
    lins = _hidden_linears(mod)
    base = [lin.weight.clone() for lin in lins]
    up = min(HOT_UP, len(lins) // 2)
    down = len(lins) - up

    def peak(g):
        for i, (lin, w) in enumerate(zip(lins, base)):
            lin.weight.copy_(w * (g if i < up else g ** (-up / down)))
        trace = []
        forward(trace)
        return max(float(t.max()) for t in trace)

    lo, hi = 0.0, 8.0
    for _ in range(16):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if peak(2.0 ** mid) < target else (lo, mid)
    gain = 2.0 ** (0.5 * (lo + hi))
    peak(gain)
    return gain


@functools.lru_cache(maxsize=None)
def build_net(name: str) -> Net:
    gen = torch.Generator().manual_seed(_seed("net|" + name))
    if name in FRESH_VF or name in FRESH_RN or name in NARROW_VF:
        torch.manual_seed(_seed("init|" + name))
        if name not in FRESH_RN:
            mod = _fresh_vf(**{**FRESH_VF, **NARROW_VF}[name])
            synthetic.scale_hidden_weights(mod, _NOTHING, GAIN)
            net = Net(name, mod, None)
        else:
            mod = _fresh_rn(**FRESH_RN[name])
            synthetic.scale_hidden_weights(_NOTHING, mod, GAIN)
            net = Net(name, None, mod)
        randomise_statistics(mod, gen)
        return net
    parts = name.split("+")
    fx, d = helpers.load_fixture(parts[0])
    model = helpers.build_model(fx, d)
    net = Net(name, model.vector_field_network, model.rendering_network)
    if "stats" in parts:
        randomise_statistics(net.vf, gen)
        randomise_statistics(net.rn, gen)
    if "hot" in parts:
        pts, dirs = _draw(name, 1.0)
        p64, d64 = pts.to(F64), dirs.to(F64)
        _heat(net.vf, lambda tr: vf64(p64, net.vf_sd(), trace=tr, **net.vf_args), HOT_TARGET)
        out = vf64(p64, net.vf_sd(), **net.vf_args)
        _heat(net.rn, lambda tr: rn64(p64, out[:, :3], d64, out[:, 3:], net.rn_sd(), net.rn._multires(), trace=tr), HOT_TARGET)
    return net


# ------------------------------------------------------------------------------------------------
# inputs and references
# ------------------------------------------------------------------------------------------------
def _draw(name: str, scale: float):
    """DRAWN candidate rows: points [DRAWN,3] and unit view directions [DRAWN,3] in float32."""
    gen = torch.Generator().manual_seed(_seed(f"rows|{name}|{scale:g}"))
    pts = ((2.0 * torch.rand(DRAWN, 3, generator=gen, dtype=F64) - 1.0) * scale).float()
    pts[1] = 0.0
    pts[2, 0] = -0.0
    dirs = torch.nn.functional.normalize(torch.randn(DRAWN, 3, generator=gen, dtype=F64), dim=1).float()
    return pts, dirs


@dataclass(eq=False)
class Family:
    """POOL accepted rows of one network at one coordinate scale with their float64 and host-float32 outputs."""
    name: str
    scale: float
    points: torch.Tensor                 # [POOL,3] float32
    dirs: torch.Tensor                   # [POOL,3] float32, unit: per row (rendering net alone) or per ray (fused: the first rays)
    normals_in: Optional[torch.Tensor]   # rendering net alone: its normal and feature inputs in float32
    feats_in: Optional[torch.Tensor]
    ref: Dict[str, torch.Tensor]         # float64: vector, feats, colours_alone
    host: Dict[str, torch.Tensor]        # the oracle in float32: the same
    rejected: float                      # share of the drawn rows that were rejected before POOL were accepted
    peaks: Dict[str, torch.Tensor]       # [POOL] per net: the largest float64 pre-activation of every row

    @property
    def hidden_max(self) -> Dict[str, float]:
        return {k: float(v.max()) for k, v in self.peaks.items()}

    @property
    def id(self) -> str:
        return f"{self.name}-s{self.scale:g}"


def _row_peaks(trace: List[torch.Tensor]) -> torch.Tensor:
    return torch.stack([t.amax(dim=1) for t in trace]).amax(dim=0)


def _ray_dirs(dirs: torch.Tensor, spr: int, rays: int) -> torch.Tensor:
    return dirs[:rays].repeat_interleave(spr, dim=0)


@functools.lru_cache(maxsize=None)
def family(name: str, scale: float) -> Family:
    net = build_net(name)
    pts, dirs = _draw(name, scale)
    ref, host, peaks = {}, {}, {}
    normals_in = feats_in = None
    rejected = 0.0
    with torch.no_grad():
        if net.vf is not None:
            out = vf64(pts.to(F64), net.vf_sd(), **net.vf_args)
            keep = out[:, :3].abs().amax(dim=1) >= ROW_FLOOR
            if net.has_feats:
                keep &= out[:, 3:].abs().amax(dim=1) >= ROW_FLOOR
            idx = torch.nonzero(keep).reshape(-1)
            assert idx.numel() >= POOL, f"{name} at scale {scale:g}: {idx.numel()} of {DRAWN} drawn rows accepted, {POOL} needed"
            idx = idx[:POOL]
            rejected = 1.0 - POOL / float(idx[-1] + 1)
            pts, dirs = pts[idx].contiguous(), dirs[idx].contiguous()
            trace = []
            out = vf64(pts.to(F64), net.vf_sd(), trace=trace, **net.vf_args)
            peaks["vf"] = _row_peaks(trace)
            ref["vector"] = out[:, :3]
            out32 = O.vf_mlp(pts, net.vf_sd(torch.float32), **net.vf_args)
            host["vector"] = out32[:, :3]
            if net.has_feats:
                ref["feats"], host["feats"] = out[:, 3:], out32[:, 3:]
        else:
            pts, dirs = pts[:POOL].contiguous(), dirs[:POOL].contiguous()
        if net.rn is not None:
            if net.vf is not None:      # the rendering net alone reads the float32 roundings of the float64 vector field outputs
                normals_in, feats_in = ref["vector"].float(), ref["feats"].float()
            else:
                gen = torch.Generator().manual_seed(_seed(f"rn inputs|{name}|{scale:g}"))
                normals_in = torch.tanh(torch.randn(POOL, 3, generator=gen))
                feats_in = torch.tanh(torch.randn(POOL, 256, generator=gen))
            trace = []
            mr = net.rn._multires()
            ref["colours_alone"] = rn64(pts.to(F64), normals_in.to(F64), dirs.to(F64), feats_in.to(F64), net.rn_sd(), mr, trace=trace)
            peaks["rn"] = _row_peaks(trace)
            host["colours_alone"] = O.render_mlp(pts, normals_in, dirs, feats_in, net.rn_sd(torch.float32), mr)
    return Family(name, scale, pts, dirs, normals_in, feats_in, ref, host, rejected, peaks)


@functools.lru_cache(maxsize=None)
def fused_reference(name: str, scale: float, spr: int, rays: int):
    """(float64, host float32) colours of the fused pass over the first spr x rays rows, row m seen along dirs[m // spr]: the float64
    vector and features of the vector-field restatement feed the rendering restatement; the float32 oracle feeds itself.  Third: the
    largest float64 pre-activation of the case in either net."""
    fam, net = family(name, scale), build_net(name)
    m = spr * rays
    d = _ray_dirs(fam.dirs, spr, rays)
    mr = net.rn._multires()
    with torch.no_grad():
        trace = []
        c64 = rn64(fam.points[:m].to(F64), fam.ref["vector"][:m], d.to(F64), fam.ref["feats"][:m], net.rn_sd(), mr, trace=trace)
        c32 = O.render_mlp(fam.points[:m], fam.host["vector"][:m], d, fam.host["feats"][:m], net.rn_sd(torch.float32), mr)
    return c64, c32, max(float(_row_peaks(trace).max()), float(fam.peaks["vf"][:m].max()))


# ------------------------------------------------------------------------------------------------
# scoring
# ------------------------------------------------------------------------------------------------
def _ratio(err: torch.Tensor, scale: torch.Tensor, exact: torch.Tensor) -> torch.Tensor:
    inf = torch.full_like(err, float("inf"))
    return torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(exact, torch.zeros_like(err), inf))


def row_error(x: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """[M]: max_c |x - ref| / max_c |ref| of every row (a row that is all zero in float64 must be all zero in x)."""
    x, ref = x.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    return _ratio((x - ref).abs().amax(dim=1), ref.abs().amax(dim=1), (x == 0).all(dim=1))


def col_error(x: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """[C]: max_rows |x - ref| / max(max_rows |ref|, ROW_FLOOR) of every column."""
    x, ref = x.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    return (x - ref).abs().amax(dim=0) / ref.abs().amax(dim=0).clamp_min(ROW_FLOOR)


def score(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """Worst row / column of a case.  ``got`` and ``ref`` hold the same M rows under 'vector', 'feats', 'colours' (any subset)."""
    out = {}
    for k in ("vector", "colours"):
        if k in got:
            out[k] = float(row_error(got[k], ref[k]).max())
    if "feats" in got:
        out["feat_rows"] = float(row_error(got["feats"], ref["feats"]).max())
        out["feat_cols"] = float(col_error(got["feats"], ref["feats"]).max())
    return out


def case_reference(name: str, scale: float, m: int) -> Dict[str, torch.Tensor]:
    """float64 vector / feats / colours (of the rendering net alone) of the first m rows."""
    fam = family(name, scale)
    out = {k: fam.ref[k][:m] for k in ("vector", "feats") if k in fam.ref}
    if "colours_alone" in fam.ref:
        out["colours"] = fam.ref["colours_alone"][:m]
    return out


def fused_case_reference(name: str, scale: float, spr: int, rays: int) -> Dict[str, torch.Tensor]:
    fam, m = family(name, scale), spr * rays
    return dict(vector=fam.ref["vector"][:m], feats=fam.ref["feats"][:m], colours=fused_reference(name, scale, spr, rays)[0])


@functools.lru_cache(maxsize=None)
def yardstick(name: str, scale: float) -> Dict[str, float]:
    """The float32 oracle on the host against float64, scored as the device is on every case of the family and pooled as the worst:
    'vector', 'feat_rows', 'feat_cols', 'colours_alone' (the M_VALUES cases) and 'colours' (the fused cases)."""
    fam, net = family(name, scale), build_net(name)
    pool: Dict[str, float] = {}

    def take(scores, rename=None):
        for k, v in scores.items():
            k = (rename or {}).get(k, k)
            pool[k] = max(pool.get(k, 0.0), v)

    for m in M_VALUES:
        host = {k: fam.host[k][:m] for k in ("vector", "feats") if k in fam.host}
        if "colours_alone" in fam.host:
            host["colours"] = fam.host["colours_alone"][:m]
        take(score(host, case_reference(name, scale, m)), {"colours": "colours_alone"})
    if net.vf is not None and net.rn is not None:
        for spr, rays in FUSED_CASES:
            m = spr * rays
            host = dict(vector=fam.host["vector"][:m], feats=fam.host["feats"][:m], colours=fused_reference(name, scale, spr, rays)[1])
            take(score(host, fused_case_reference(name, scale, spr, rays)))
    return pool


# ------------------------------------------------------------------------------------------------
# float64 emulation of the split arithmetic
# ------------------------------------------------------------------------------------------------
XSCALE = 64.0


def _split(v32: torch.Tensor):
    hi = v32.half()
    lo = (v32 - hi.float()).half()
    return hi.to(F64), lo.to(F64)


def _folded(mod, i: int, scale: float, rows=None, plant: Optional[str] = None):
    """(W', b') of layer i in float32, as vfn_pack16_kernel folds them."""
    lin, bn = mod._linear(i), mod._bn(i)
    w, b = lin.weight.detach().clone(), lin.bias.detach().clone()
    if bn is not None:
        var, eps = bn.running_var.detach(), torch.tensor(0.0 if plant == "eps" else BN_EPS, dtype=torch.float32)
        s = bn.weight.detach() / torch.sqrt(var + eps)
        w = w * s[:, None]
        mean = bn.running_mean.detach()
        b = ((b + mean) if plant == "mean" else (b - mean)) * s + bn.bias.detach()
    w = w * torch.tensor(scale, dtype=torch.float32)
    return (w, b) if rows is None else (w[rows], b[rows])


def _split_layer(x32: torch.Tensor, w32: torch.Tensor, b32: torch.Tensor, plant: Optional[str]) -> torch.Tensor:
    """64 x (pre-activation) from operands at 64 x their value: hi hi + hi lo + lo hi with exact sums, + 64 b'."""
    xh, xl = _split(x32)
    wh, wl = _split(w32)
    acc = xh @ wh.T + xl @ wh.T
    if plant != "cross":
        acc = acc + xh @ wl.T
    return acc + XSCALE * b32.to(F64)


def emulate_f16x3(net: Net, points: torch.Tensor, ray_dirs: torch.Tensor, plant: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """The fused f16x3 pass over points [M,3] seen along ray_dirs [M,3] -> vector, feats, colours in float64 (shipped geometry)."""
    vf, rn = net.vf, net.rn
    skip = vf.skip_connection_in[0]
    pe = (encode(points, vf._multires()) * XSCALE).float()
    x = pe
    n = vf.num_layers
    for i in range(n - 1):
        if i == skip:
            x = torch.cat([x, pe], dim=1)
        w, b = _folded(vf, i, 0.70710678118654752440 if i == skip else 1.0, plant=plant)
        x = torch.relu(_split_layer(x, w, b, plant)).float()
    wv, bv = _folded(vf, n - 1, 1.0, rows=slice(0, 3), plant=plant)
    wf, bf = _folded(vf, n - 1, 1.0, rows=slice(3, None), plant=plant)
    vector = torch.tanh(_split_layer(x, wv, bv, plant) / XSCALE)
    feats = torch.tanh(_split_layer(x, wf, bf, plant) / XSCALE)
    x = (torch.cat([points.to(F64), encode(ray_dirs, rn._multires()).to(F64), vector.float().to(F64), feats.float().to(F64)], dim=1) * XSCALE).float()
    for i in range(rn.num_layers - 1):
        w, b = _folded(rn, i, 1.0, plant=plant)
        x = torch.relu(_split_layer(x, w, b, plant)).float()
    w, b = _folded(rn, rn.num_layers - 1, 1.0, plant=plant)
    colours = torch.sigmoid(_split_layer(x, w, b, plant) / XSCALE)
    return dict(vector=vector, feats=feats, colours=colours)


# ------------------------------------------------------------------------------------------------
# gradients through the fold: rows away from every ReLU kink, float64 autograd of the restatement
# ------------------------------------------------------------------------------------------------
def _away_from_kinks(trace: List[torch.Tensor]) -> torch.Tensor:
    """[M] bool: no pre-activation of the row within KINK_MARGIN x the largest |pre-activation| of its row and layer of zero (a float32
    evaluation of a row is off by 1e-6 of that at the most)."""
    ok = torch.ones(trace[0].shape[0], dtype=torch.bool)
    for t in trace:
        ok &= (t.abs() >= KINK_MARGIN * t.abs().amax(dim=1, keepdim=True)).all(dim=1)
    return ok


@dataclass(eq=False)
class GradCase:
    inputs: Dict[str, torch.Tensor]      # float32
    coef: torch.Tensor                   # the fixed linear functional of the output
    out: torch.Tensor                    # float64 output
    grads: Dict[str, torch.Tensor]       # float64: every parameter by its state_dict key, and 'feats' for the rendering net
    rejected: float                      # share of the pool's rows within the margin of a kink
    input_grads: Dict[str, torch.Tensor]     # float64, from the same backward: 'points' (vector field); 'points', 'dirs', 'normals', 'feats'


def _leaves(sd):
    for k, v in sd.items():
        if "running_" not in k:
            v.requires_grad_(True)
    return {k: v for k, v in sd.items() if v.requires_grad}


def _rows_of(m: Optional[int], full: int) -> int:
    return full if m is None else m


@functools.lru_cache(maxsize=None)
def _vf_grad_rows(name: str):
    """(points, coef, rejected share) of the net's gradient case at its full row count: the pool's rows away from every kink."""
    fam, net = family(name, 1.0), build_net(name)
    trace = []
    with torch.no_grad():
        vf64(fam.points.to(F64), net.vf_sd(), trace=trace, **net.vf_args)
    ok = _away_from_kinks(trace)
    pts = fam.points[ok][:GRAD_ROWS].contiguous()
    assert bool((pts[:3] == 0).all(dim=1).any()), f"{name}: the point (0, 0, 0) sits within the margin of a kink"
    if not bool(((pts[:3, 0] == 0) & torch.signbit(pts[:3, 0])).any()):
        # the pool's row that starts with -0.0 is within the margin of a kink: the first kink-free one of 64 drawn for it takes row 2
        cand = (2.0 * torch.rand(64, 3, generator=torch.Generator().manual_seed(_seed("minus zero|" + name)), dtype=F64) - 1.0).float()
        cand[:, 0] = -0.0
        trace = []
        with torch.no_grad():
            vf64(cand.to(F64), net.vf_sd(), trace=trace, **net.vf_args)
        cand = cand[_away_from_kinks(trace)]
        pts = torch.cat([pts[:2], cand[:1], pts[2:]])[:GRAD_ROWS].contiguous()
    coef = torch.randn(pts.shape[0], 3 + net.vf._feature_dims(), generator=torch.Generator().manual_seed(_seed("vf coef|" + name)))
    return pts, coef, 1.0 - float(ok.double().mean())


def _vf_grads(name: str, m: Optional[int], dtype) -> GradCase:
    net = build_net(name)
    pts, coef, rejected = _vf_grad_rows(name)
    m = _rows_of(m, pts.shape[0])
    pts, coef = pts[:m].contiguous(), coef[:m].contiguous()
    sd = net.vf_sd(dtype)
    leaves = _leaves(sd)
    p = pts.to(dtype).requires_grad_(True)
    out = vf64(p, sd, **net.vf_args)
    (out * coef.to(dtype)).sum().backward()
    return GradCase(dict(points=pts), coef, out.detach(), {k: v.grad for k, v in leaves.items()}, rejected, dict(points=p.grad))


@functools.lru_cache(maxsize=None)
def vf_grad_case(name: str, m: Optional[int] = None) -> GradCase:
    """The first ``m`` kink-free rows (None: all, at most GRAD_ROWS) with the first m rows of ``coef``, float64 autograd of the restatement."""
    return _vf_grads(name, m, F64)


@functools.lru_cache(maxsize=None)
def _rn_grad_rows(name: str):
    fam, net = family(name, 1.0), build_net(name)
    args = (fam.points, fam.normals_in, fam.dirs, fam.feats_in)
    trace = []
    with torch.no_grad():
        rn64(*(a.to(F64) for a in args), net.rn_sd(), net.rn._multires(), trace=trace)
    ok = _away_from_kinks(trace)
    pts, nrm, dirs, feats = (a[ok][:GRAD_ROWS].contiguous() for a in args)
    coef = torch.randn(pts.shape[0], 3, generator=torch.Generator().manual_seed(_seed("rn coef|" + name)))
    return dict(points=pts, normals=nrm, dirs=dirs, feats=feats), coef, 1.0 - float(ok.double().mean())


def _rn_grads(name: str, m: Optional[int], dtype) -> GradCase:
    net = build_net(name)
    rows, coef, rejected = _rn_grad_rows(name)
    m = _rows_of(m, coef.shape[0])
    rows, coef = {k: v[:m].contiguous() for k, v in rows.items()}, coef[:m].contiguous()
    sd = net.rn_sd(dtype)
    leaves = _leaves(sd)
    x = {k: v.to(dtype).requires_grad_(True) for k, v in rows.items()}
    out = rn64(x["points"], x["normals"], x["dirs"], x["feats"], sd, net.rn._multires())
    (out * coef.to(dtype)).sum().backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads["feats"] = x["feats"].grad
    return GradCase(rows, coef, out.detach(), grads, rejected, {k: v.grad for k, v in x.items()})


@functools.lru_cache(maxsize=None)
def rn_grad_case(name: str, m: Optional[int] = None) -> GradCase:
    return _rn_grads(name, m, F64)


def grad_case(name: str, which: str, m: Optional[int] = None) -> GradCase:
    return vf_grad_case(name, m) if which == "vf" else rn_grad_case(name, m)


# ------------------------------------------------------------------------------------------------
# scoring of gradients: per output row, per input-column block, per element; never per tensor alone
# ------------------------------------------------------------------------------------------------
def grad_kind(key: str) -> str:
    """'weight', 'bias' (of a Linear), 'gamma', 'beta' (of a BatchNorm), or the name of an input ('points', 'normals', 'feats', ...)."""
    if not key.startswith("layers."):
        return key
    parts = key.split(".")                # layers.<i>.weight | layers.<i>.0.weight (Linear) | layers.<i>.1.weight (BatchNorm)
    bn = len(parts) == 4 and parts[2] == "1"
    return ("gamma" if bn else "weight") if key.endswith("weight") else ("beta" if bn else "bias")


def _encoding_blocks(multires: int, first: int, tag: str) -> List[Tuple[str, int, int]]:
    out = [(tag, first, first + 3)]
    for k in range(multires):
        out += [(f"{tag}.sin{k}", first + 3 + 6 * k, first + 6 + 6 * k), (f"{tag}.cos{k}", first + 6 + 6 * k, first + 9 + 6 * k)]
    return out


def column_blocks(key: str, net: Net, which: str) -> Optional[List[Tuple[str, int, int]]]:
    """The named input-column blocks (name, first, end) of a weight that reads raw inputs; None for every other tensor."""
    if grad_kind(key) != "weight":
        return None
    layer = int(key.split(".")[1])
    if which == "vf":
        mr = net.vf._multires()
        pe = 3 + 6 * mr if mr > 0 else 3
        if layer == 0:
            return _encoding_blocks(mr, 0, "xyz")
        if layer in net.vf.skip_connection_in:
            n_prev = net.vf._linear(layer).in_features - pe
            return [("hidden", 0, n_prev)] + _encoding_blocks(mr, n_prev, "xyz")
        return None
    if layer != 0:
        return None
    mr = net.rn._multires()
    pe = 3 + 6 * mr if mr > 0 else 3
    return [("points", 0, 3)] + _encoding_blocks(mr, 3, "dirs") + [("normals", 3 + pe, 6 + pe), ("feats", 6 + pe, net.rn._linear(0).in_features)]


def _held(err: torch.Tensor, ref: torch.Tensor, top: float) -> float:
    """max |err| over the group / max(largest |float64 entry| of the group, GRAD_FLOOR x the tensor's largest |entry|), worst group;
    ``err`` and ``ref`` are [groups, entries]."""
    scale = ref.abs().amax(dim=1).clamp_min(GRAD_FLOOR * top)
    e = err.amax(dim=1)
    if top == 0.0:
        return 0.0 if float(e.max()) == 0.0 else float("inf")
    return float((e / scale).max())


def grad_score(got: torch.Tensor, ref: torch.Tensor, key: str, net: Net, which: str = "vf") -> Dict[str, float]:
    """Figures of one gradient tensor against float64: 'tensor' (max |err| / max |ref|, what helpers.grad_rel_err gives) beside
    'rows' (a weight matrix, per output row; an input gradient [M, c], per sample row), 'blocks' (a weight that reads raw inputs, per
    named block of input columns) or 'elems' (a vector, per element).  A row, block or element below GRAD_FLOOR of its tensor's largest
    entry is held in absolute terms at that share."""
    got, ref = got.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    assert got.shape == ref.shape, (key, tuple(got.shape), tuple(ref.shape))
    err, top = (got - ref).abs(), float(ref.abs().max())
    out = {"tensor": _held(err.reshape(1, -1), ref.reshape(1, -1), top)}
    if ref.dim() == 1:
        out["elems"] = _held(err.reshape(-1, 1), ref.reshape(-1, 1), top)
        return out
    out["rows"] = _held(err, ref, top)
    blocks = column_blocks(key, net, which)
    if blocks is not None:
        assert blocks[-1][2] == ref.shape[1] and all(a[2] == b[1] for a, b in zip(blocks, blocks[1:])), (key, blocks)
        out["blocks"] = max(_held(err[:, a:b].reshape(1, -1), ref[:, a:b].reshape(1, -1), top) for _, a, b in blocks)
    return out


def grad_scores(got: Dict[str, torch.Tensor], ref: Dict[str, torch.Tensor], net: Net, which: str) -> Dict[str, Dict[str, float]]:
    return {k: grad_score(v, ref[k], k, net, which) for k, v in got.items()}


def pool_by_kind(scores: Dict[str, Dict[str, float]], pool: Optional[Dict[Tuple[str, str], float]] = None) -> Dict[Tuple[str, str], float]:
    """{(tensor kind, figure): worst over the tensors of that kind}."""
    pool = {} if pool is None else pool
    for key, figs in scores.items():
        for fig, v in figs.items():
            k = (grad_kind(key), fig)
            pool[k] = max(pool.get(k, 0.0), v)
    return pool


def _all_grads(case: GradCase) -> Dict[str, torch.Tensor]:
    return {**case.grads, **case.input_grads}


@functools.lru_cache(maxsize=None)
def grad_yardstick(name: str, which: str = "vf") -> Dict[Tuple[str, str], float]:
    """The float32 restatement under float32 autograd on the host against the float64 case, on the same rows and ``coef``, scored the
    same way and pooled as the worst over GRAD_M: {(tensor kind, figure): value}."""
    net, pool = build_net(name), {}
    for m in GRAD_M:
        ref = grad_case(name, which, m)
        host = (_vf_grads if which == "vf" else _rn_grads)(name, m, torch.float32)
        pool_by_kind(grad_scores(_all_grads(host), _all_grads(ref), net, which), pool)
    return pool
