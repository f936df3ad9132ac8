"""The MLP forward kernels (csrc/vfn_mlp.hip exact fp32, csrc/vfn_mlp16.hip f16x3) against a float64 restatement of both nets, row by
row and column by column, on networks whose BatchNorm layers carry real running statistics; and the gradients through the same fold.

Networks, inputs, restatement and scoring: tests/mlp_cases.py (checked on the host by tests/test_mlp_host.py).  Entry points:
vfn_vf_mlp_fwd with 3 and 259 columns, vfn_render_mlp_fwd, vfn_vf_render_fused_fwd with the features, vfn_vf_mlp16_fwd and
vfn_vf_render_fused16_fwd (three products).  Every output buffer is a window of a larger one filled with a sentinel: the rows before
and behind it must come back untouched, and no entry of the window may still hold the sentinel.

Bounds: FACTOR x the float32 oracle on the host against float64, computed at run time on each family's own rows and pooled over the
cases of one (network, coordinate scale) family (MC.yardstick).  8, the project's factor for exact-fp32 kernels, is the cap; the factor
asserted per kernel and output is the smallest power of two at least twice the worst ratio measured on an MI355X (table below).

Measured on an MI355X, worst case of each family: device | host-float32 yardstick (both against float64).
Worst device / yardstick ratio and the factor asserted:
  exact fp32   vector 2.5 (vf_2h, scale 4) -> 8      feature rows 1.8 -> 4      feature columns 2.9 (trained_far, scale 300, M = 1) -> 8
               colours, fused 3.0 (trained_far+stats, scale 1) -> 8      colours, rendering net alone 1.7 -> 4
  f16x3        vector 6.6 -> 8      colours 5.4 -> 8
The two f16x3 figures are above the 4 x that twice-the-ratio-under-8 needs, so 8 is asserted as the cap and they are accounted for:
  * vector, c1_det+stats at scale 300 (2.6e-04 against 3.9e-05): ONE row among rows 257 .. 512; without it the family measures 2.2 x
    (8.5e-05 at M <= 257).  98 % of this family's vector components are saturated (|tanh| > 0.9999) and score 0 in every evaluation,
    so family and yardstick are the worst of the two dozen rows that are not, rows whose pre-tanh value is what activations of 340
    cancel down to.  The float64 emulation of the split arithmetic with exact sums (tests/test_mlp_host.py) gives 1.2e-04 on the same
    rows, the exact-fp32 kernel's accumulation alone 4.2e-05.  Every other family is at or below 4.2 x (trained_256+stats, scale 30).
  * colours, the hot net (7.9e-07 against 1.5e-07): the emulation gives 7.0e-07 on the same case, i.e. the figure is the arithmetic,
    22-bit operands and weights whose low halves sit in the f16 denormals (the rendering net's two layers that bring activations of
    500 back down have folded weights of 0.0098 at the most, which two f16 halves hold to 17 bits; the range guard accepts a layer
    from 2^-9 = 0.002 on), not the kernel.  Every other family's colours are at or below 2.1 x.
"-": the net has no such output, or (f16x3 colours of trained_far at scale 300) the case is outside the f16x3 range, see below.
  family                  fp32 vector          fp32 feat_rows       fp32 feat_cols       fp32 colours         fp32 colours_alone   f16x3 vector         f16x3 colours
  c1_det-s1               1.3e-05 | 1.5e-05    8.9e-07 | 6.1e-07    2.7e-06 | 1.8e-06    1.7e-07 | 1.5e-07    1.2e-07 | 1.2e-07    1.8e-05 | 1.5e-05    1.9e-07 | 1.5e-07
  c1_det-s4               1.3e-05 | 6.8e-06    1.1e-06 | 6.3e-07    2.7e-06 | 2.5e-06    1.5e-07 | 1.5e-07    1.4e-07 | 1.4e-07    1.1e-05 | 6.8e-06    1.9e-07 | 1.5e-07
  c1_det-s30              1.6e-05 | 1.8e-05    1.5e-06 | 1.1e-06    6.4e-06 | 5.3e-06    3.8e-07 | 4.0e-07    3.2e-07 | 3.8e-07    3.5e-05 | 1.8e-05    5.5e-07 | 4.0e-07
  c1_det-s300             3.6e-05 | 1.1e-04    1.2e-05 | 8.5e-06    3.9e-05 | 2.5e-05    2.0e-06 | 2.1e-06    1.7e-06 | 1.6e-06    6.1e-05 | 1.1e-04    2.8e-06 | 2.1e-06
  trained_256-s1          1.0e-06 | 9.1e-07    3.6e-07 | 2.4e-07    7.8e-07 | 4.9e-07    1.1e-07 | 1.2e-07    1.1e-07 | 1.1e-07    1.6e-06 | 9.1e-07    1.1e-07 | 1.2e-07
  trained_256-s4          1.0e-06 | 7.1e-07    4.0e-07 | 2.7e-07    7.2e-07 | 4.8e-07    1.1e-07 | 1.1e-07    1.1e-07 | 1.1e-07    1.6e-06 | 7.1e-07    1.3e-07 | 1.1e-07
  trained_256-s30         2.6e-06 | 2.2e-06    7.6e-07 | 7.3e-07    1.3e-06 | 1.1e-06    1.8e-07 | 1.5e-07    1.7e-07 | 1.6e-07    5.4e-06 | 2.2e-06    2.3e-07 | 1.5e-07
  trained_256-s300        3.4e-05 | 1.8e-05    1.7e-06 | 2.0e-06    1.3e-05 | 1.5e-05    5.9e-07 | 5.7e-07    4.3e-07 | 6.1e-07    3.2e-05 | 1.8e-05    9.8e-07 | 5.7e-07
  trained_far-s1          8.0e-07 | 6.8e-07    7.3e-07 | 5.1e-07    1.2e-06 | 6.9e-07    1.2e-06 | 1.2e-06    8.1e-07 | 8.5e-07    2.5e-06 | 6.8e-07    2.0e-06 | 1.2e-06
  trained_far-s4          1.2e-06 | 1.1e-06    1.0e-06 | 9.6e-07    1.0e-06 | 8.1e-07    7.5e-06 | 5.8e-06    4.3e-06 | 6.2e-06    2.6e-06 | 1.1e-06    7.6e-06 | 5.8e-06
  trained_far-s30         3.2e-06 | 2.1e-06    1.2e-06 | 1.6e-06    2.3e-06 | 1.3e-06    3.5e-05 | 4.4e-05    2.9e-05 | 3.7e-05    4.6e-06 | 2.1e-06    4.8e-05 | 4.4e-05
  trained_far-s300        2.9e-05 | 1.3e-05    5.9e-06 | 3.3e-06    2.3e-05 | 7.8e-06    1.0e+00 | 1.0e+00    1.0e+00 | 1.0e+00    3.4e-05 | 1.3e-05    -
  c1_det+stats-s1         8.6e-06 | 3.5e-06    7.7e-07 | 5.5e-07    5.4e-06 | 4.1e-06    2.2e-07 | 1.6e-07    2.1e-07 | 1.5e-07    7.5e-06 | 3.5e-06    2.4e-07 | 1.6e-07
  c1_det+stats-s4         4.3e-06 | 5.1e-06    7.1e-07 | 5.0e-07    3.9e-06 | 6.6e-06    2.4e-07 | 1.7e-07    2.3e-07 | 1.5e-07    9.9e-06 | 5.1e-06    2.7e-07 | 1.7e-07
  c1_det+stats-s30        2.1e-05 | 1.9e-05    2.1e-06 | 2.3e-06    9.5e-06 | 5.6e-06    4.8e-07 | 4.5e-07    4.6e-07 | 4.2e-07    2.6e-05 | 1.9e-05    8.4e-07 | 4.5e-07
  c1_det+stats-s300       4.2e-05 | 3.9e-05    1.5e-05 | 1.3e-05    8.0e-05 | 6.9e-05    2.4e-06 | 2.2e-06    2.3e-06 | 2.2e-06    2.6e-04 | 3.9e-05    3.2e-06 | 2.2e-06
  trained_256+stats-s1    6.7e-06 | 5.3e-06    5.6e-07 | 3.1e-07    2.4e-06 | 1.6e-06    1.5e-07 | 1.3e-07    1.5e-07 | 1.1e-07    1.4e-05 | 5.3e-06    1.7e-07 | 1.3e-07
  trained_256+stats-s4    4.3e-06 | 2.7e-06    5.4e-07 | 3.0e-07    2.2e-06 | 1.8e-06    1.6e-07 | 1.3e-07    1.3e-07 | 1.2e-07    5.2e-06 | 2.7e-06    1.8e-07 | 1.3e-07
  trained_256+stats-s30   6.9e-06 | 6.5e-06    5.9e-07 | 5.3e-07    2.0e-06 | 1.3e-06    2.0e-07 | 1.8e-07    1.9e-07 | 1.8e-07    2.8e-05 | 6.5e-06    2.8e-07 | 1.8e-07
  trained_256+stats-s300  2.6e-05 | 2.2e-05    3.2e-06 | 2.4e-06    1.6e-05 | 1.9e-05    9.4e-07 | 1.2e-06    8.3e-07 | 8.5e-07    3.0e-05 | 2.2e-05    1.7e-06 | 1.2e-06
  trained_far+stats-s1    3.5e-06 | 2.5e-06    4.9e-07 | 2.9e-07    3.6e-06 | 3.0e-06    1.1e-06 | 3.8e-07    3.8e-07 | 2.9e-07    5.8e-06 | 2.5e-06    8.0e-07 | 3.8e-07
  trained_far+stats-s4    3.7e-06 | 2.6e-06    4.9e-07 | 3.6e-07    2.8e-06 | 2.4e-06    1.1e-06 | 9.1e-07    1.6e-06 | 9.6e-07    5.1e-06 | 2.6e-06    1.3e-06 | 9.1e-07
  trained_far+stats-s30   5.4e-06 | 4.2e-06    1.2e-06 | 9.4e-07    5.8e-06 | 3.1e-06    4.3e-05 | 2.6e-05    1.7e-05 | 3.4e-05    9.5e-06 | 4.2e-06    2.9e-05 | 2.6e-05
  trained_far+stats-s300  1.9e-05 | 1.5e-05    5.9e-06 | 6.4e-06    2.6e-05 | 2.5e-05    1.0e+00 | 1.0e+00    1.0e+00 | 1.0e+00    2.5e-05 | 1.5e-05    -
  c1_det+stats+hot-s1     6.2e-06 | 3.5e-06    7.9e-07 | 4.7e-07    3.3e-06 | 3.0e-06    1.8e-07 | 1.5e-07    1.6e-07 | 1.3e-07    8.2e-06 | 3.5e-06    7.9e-07 | 1.5e-07
  vf_2h-s1                2.0e-06 | 1.5e-06    -                    -                    -                    -                    -                    -
  vf_2h-s4                2.7e-06 | 1.1e-06    -                    -                    -                    -                    -                    -
  vf_2h-s30               4.5e-06 | 2.6e-06    -                    -                    -                    -                    -                    -
  vf_2h-s300              2.2e-05 | 3.6e-05    -                    -                    -                    -                    -                    -
  vf_4h_skip1-s1          2.9e-06 | 1.6e-06    8.2e-07 | 5.2e-07    3.7e-06 | 2.7e-06    -                    -                    -                    -
  vf_4h_skip1-s4          2.4e-06 | 2.4e-06    1.0e-06 | 6.2e-07    5.1e-06 | 4.3e-06    -                    -                    -                    -
  vf_4h_skip1-s30         1.7e-06 | 1.5e-06    2.9e-06 | 2.7e-06    1.3e-05 | 1.5e-05    -                    -                    -                    -
  vf_4h_skip1-s300        1.6e-05 | 9.3e-06    2.6e-05 | 1.9e-05    1.6e-04 | 1.0e-04    -                    -                    -                    -
  vf_8h_skip7-s1          1.2e-06 | 5.6e-07    7.4e-07 | 4.9e-07    3.3e-06 | 2.9e-06    -                    -                    -                    -
  vf_8h_skip7-s4          1.0e-06 | 6.8e-07    7.6e-07 | 5.3e-07    5.1e-06 | 3.4e-06    -                    -                    -                    -
  vf_8h_skip7-s30         3.9e-06 | 2.8e-06    1.6e-06 | 1.4e-06    1.2e-05 | 8.0e-06    -                    -                    -                    -
  vf_8h_skip7-s300        6.9e-06 | 8.9e-06    1.3e-05 | 1.1e-05    3.7e-05 | 7.4e-05    -                    -                    -                    -

  rendering net alone     scale 1              scale 4              scale 30             scale 300
  rn_1h_m0                2.2e-07 | 1.4e-07    2.4e-07 | 1.7e-07    3.4e-07 | 3.9e-07    8.7e-07 | 2.9e-06
  rn_1h_m2                2.3e-07 | 1.7e-07    2.5e-07 | 1.5e-07    4.2e-07 | 5.0e-07    2.5e-06 | 6.3e-06
  rn_1h_m5                2.4e-07 | 1.7e-07    2.8e-07 | 2.2e-07    4.4e-07 | 4.2e-07    2.4e-06 | 7.5e-06
  rn_3h_m0                2.5e-07 | 1.6e-07    2.8e-07 | 1.7e-07    3.6e-07 | 3.9e-07    2.0e-06 | 2.4e-06
  rn_3h_m2                2.5e-07 | 1.7e-07    2.9e-07 | 1.8e-07    3.7e-07 | 4.8e-07    1.6e-06 | 1.8e-06
  rn_3h_m5                2.1e-07 | 1.6e-07    2.4e-07 | 1.7e-07    2.6e-07 | 3.6e-07    1.7e-06 | 1.6e-06

f16x3 and the range guard: a case whose largest float64 pre-activation is below 900 must leave the status word 0 (the hot net, 500, among
them) and is held like any other; above 945 (trained_far at coordinate scale 300: 970) the ReLU clamp acts at 937.5, the launch must
say so in the status word, and nothing else is asked of its values.

Gradients.  Which of the four packs each path reads (vf_nerf_amd/autograd.py, backward.py, batchstat.py, stepengine.py):
  VectorFieldNetwork.forward under autograd, precision "fp32"      vfn_vf_mlp_fwd_train reads the weight pack (vfn_pack_kernel); the dX
                                                                   chain vfn_mlp_bwd_chain the weight pack and the backward pack
                                                                   (vfn_pack_weights_bwd: the same kernel, transposed tiles); the
                                                                   weight-gradient slabs go through vfn_unfold_kernel
  ... precision "f16x3", with fp32 or with the default 16-bit      vfn_vf_mlp16_fwd_train reads the f16x3 pack (vfn_pack16_kernel); the
  storages                                                         chain vfn_mlp_bwd_chain_bf16 the bf16 backward pack
                                                                   (vfn_pack_weights_bwd16); vfn_unfold_kernel (row-major slabs, or
                                                                   from C inside vfn_net_weight_grads_frag with the flat optimizer)
  RenderingNetwork.forward under autograd                          no pack: the layer-at-a-time kernels of csrc/vfn_bstat.hip with
                                                                   coefficients folded on the host (batchstat._running_coef), a
                                                                   fifth statement of the fold
  model.render under autograd, default storages                    both nets: f16x3 packs forward, bf16 backward packs in the chain,
                                                                   vfn_unfold_kernel inside vfn_net_weight_grads_frag
  model.render under autograd, precision "fp32"                    both nets: weight packs, backward packs, vfn_unfold_kernel
The stepengine's one-call training step reads the same cached packs (net.packed16_weights(), backward._packed_bwd16) and is tied to
the launch-by-launch path of model.render by tests/test_hip_session.py.
Bounds: MODE_TOL of tests/test_hip_backward.py, unchanged.  Measured worst parameter:
  vector field forward   fp32 2.3e-06 / 1.6e-06 (1e-4)   f16x3 8.1e-05 / 8.4e-05 (2e-4)   f16x3+f16act+f16dy 6.2e-04 / 6.0e-04 (1e-3)
                         (trained_256+stats / trained_far+stats; the worst is a BatchNorm gamma in the 16-bit modes)
  rendering forward      fp32 8.6e-07 / 7.9e-07 (1e-4)   f16x3 4.2e-05 / 5.3e-05 (2e-4); features 3.3e-07 / 4.5e-07 and 3.4e-05 / 5.3e-05
  model.render           f16x3+f16act+f16dy 9.6e-04 (1e-3, rn.layers.1.0.weight, 2 units on the other side of zero), fp32 2.6e-05 (1e-4),
                         the two device runs against each other 9.6e-04 (1e-3); the same figures in two runs

Gradients on every geometry, inputs included (test_*_gradients_exact, test_*_gradients_split, test_rendering_inputs_without_a_gradient).
Cases, scoring (per output row, per named block of input columns, per element; an input gradient per sample row) and the yardstick
(float32 autograd of the float32 restatement on the host, worst over GRAD_M per net, tensor kind and figure): tests/mlp_cases.py.
Exact arithmetic (precision "fp32") is asserted at MAX_FACTOR = 8 x the yardstick in every figure at every M of GRAD_M, beside MODE_TOL
per tensor.  "fused": only the parameters ask (vfn_vf_mlp_fwd_train, vfn_mlp_bwd_chain, _weight_grads, vfn_unfold_kernel); "rows": the
layer-at-a-time kernels of batchstat.py with the running statistics and the exact products (the points ask too; the narrow net; the
rendering net, with the normals' and the features' gradients).  Measured on an MI355X, worst over GRAD_M and over the tensors of a net,
as a multiple of the yardstick:
  net, path                                        per tensor        rows              blocks            elements
  trained_256+stats / trained_far+stats vf, fused  2.7 / 2.0         1.4 / 1.1         2.3 / 1.1         2.1 / 1.8
  the same, rows with the points                   1.6 / 1.3         1.4 / 1.0         1.2 / 1.6         1.3 / 1.2
  vf_2h / vf_4h_skip1 / vf_8h_skip7, fused         1.4 / 1.5 / 2.3   1.1 / 1.1 / 1.7   0.7 / 0.9 / 1.3   1.2 / 1.5 / 1.7
  vf_4h_skip1 / vf_8h_skip7, rows with the points  1.5 / 1.6         2.1 / 1.3         1.1 / 1.5         2.1 / 1.7
  vf_4h_w64, rows (with and without the points)    2.0               2.2               1.2               1.7
  trained_256+stats / trained_far+stats rn, rows   1.4 / 2.0         1.8 / 1.4         1.4 / 1.8         1.6 / 1.4
  rn_1h_m0 / m2 / m5, rows                         2.0 / 1.9 / 2.0   1.8 / 1.5 / 1.3   1.1 / 0.9 / 1.5   1.2 / 1.1 / 1.7
  rn_3h_m0 / m2 / m5, rows                         1.3 / 1.6 / 1.6   1.3 / 1.6 / 1.7   1.4 / 1.1 / 2.1   1.4 / 1.1 / 3.3
  (worst: 3.3 x, one gamma element of rn_3h_m5 at M = 257, 4.3e-05 against 1.3e-05; the points' rows 1.0 .. 2.1 x, 4e-06 .. 1e-05)
The 16- and 22-bit arithmetics at the full row count: per tensor inside MODE_TOL (the shipped nets: f16x3 8.4e-05 of 2e-4, default 16-bit
storages 6.0e-04 of 1e-3; the fresh rendering nets on the split products 4.3e-05 of 2e-4) or, for what MODE_TOL has no entry for (the
vector field layer by layer, the normals), inside the 2e-3 of batchstat._arith (worst 9.5e-05); the new figures are printed on MLPGRAD
lines and not bounded.  As multiples of the yardstick:
  fused f16x3 chain, shipped vf                    67 .. 78          7 .. 9            63 .. 72          20 .. 42
  ... with the default 16-bit storages             393 .. 488        92 .. 121         259 .. 318        396 .. 605   (a gamma element 3.6e-02 off)
  rows, split products, vf (5 nets)                75 .. 148         40 .. 143         58 .. 119         31 .. 82
  rows, split products, rn (8 nets)                97 .. 163         81 .. 125         66 .. 111         45 .. 121
Refused at the call, before any launch (REFUSED; the rendering net's inputs in test_rendering_inputs_without_a_gradient):
  vf_2h with points that ask       the points' gradient comes from the layer-at-a-time kernels, which apply BatchNorm after every Linear
                                   but the last; vf_2h has none (NotImplementedError).  Its parameters' gradients: the fused chain
  rendering net, points or dirs    the backward has no gradient for them and the reference's trainer never asks (NotImplementedError,
                                   naming the input); detach_normals=True leaves normals.grad None, as the reference's detach does

What a wrong fold does to these tests (tried on an MI355X, not committed):
  vfn_pack.hip with b + mean for b - mean, and vfn_mlp16.hip's folded_weight without + 1e-5f      118 of the 161 forward tests fail:
      every family of a net with real statistics on the fp32 entry points, every family on the f16x3 ones
  vfn_unfold.hip with b_lin + mean, and vfn_bwd16.hip's pack without + 1e-5f                      the vector-field gradient test fails in
      all three modes (every BatchNorm gamma off by 0.2 .. 2.3 of its largest entry; in the two f16x3 modes every weight and bias as well,
      4e-3 .. 6e-3) and the render test fails (gamma 2.3 .. 5.1); the rendering forward, which reads neither, passes
"""
import copy
import ctypes as C
import functools

import pytest
import torch

import helpers
import mlp_cases as MC
from test_hip_backward import MODE_TOL, _hip_gradients
from vf_nerf_amd import lib

pytestmark = pytest.mark.gpu

GUARD = 64                 # rows of sentinel before and behind every output window (64 rows x 12 bytes and x 1036 bytes: multiples of 256)
SENTINEL = -1234.5         # no tanh or sigmoid output
# factor x yardstick per kernel and output: the smallest power of two >= 2 x the worst measured ratio (docstring), 8 at the most
FACTOR = {"fp32": dict(vector=8.0, feat_rows=4.0, feat_cols=8.0, colours=8.0, colours_alone=4.0),
          "f16x3": dict(vector=8.0, colours=8.0)}
FAMILIES = {kind: [(n, s) for n in nets for s in MC.scales_of(n)] for kind, nets in
            dict(vf=MC.SHIPPED_NETS + tuple(MC.FRESH_VF), rn=MC.SHIPPED_NETS + tuple(MC.FRESH_RN), both=MC.SHIPPED_NETS).items()}
ids = lambda f: f"{f[0]}-s{f[1]:g}"      # noqa: E731


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def device_net(name):
    """(vf, rn) on the device, built once per module; their packs are cached on the modules."""
    lib.load()
    return MC.build_net(name).on(dev())


@functools.lru_cache(maxsize=None)
def device_rows(name, scale):
    fam = MC.family(name, scale)
    return {k: getattr(fam, k).to(dev()) for k in ("points", "dirs", "normals_in", "feats_in") if getattr(fam, k) is not None}


class Window:
    """[rows, cols] output inside a buffer of GUARD + rows + GUARD rows of SENTINEL."""

    def __init__(self, rows, cols):
        self.buf = torch.full((GUARD + rows + GUARD, cols), SENTINEL, device=dev())
        self.out = self.buf[GUARD:GUARD + rows]

    def check(self, what):
        rows = self.out.shape[0]
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + rows:] == SENTINEL).all()), f"{what}: written outside its rows"
        assert not bool((self.out == SENTINEL).any()), f"{what}: an entry was never written"
        return self.out


def _p(t, name, dtype=torch.float32):
    return lib._ptr(t, name, dtype)


def vf_mlp_fwd(vf, pts, cols):
    w = Window(pts.shape[0], cols)
    lib._check(lib.load().vfn_vf_mlp_fwd(C.byref(vf.geometry()), _p(vf.packed_weights(), "packed"), _p(pts, "points"), C.c_int64(pts.shape[0]),
                                         C.c_int32(cols), _p(w.out, "out"), lib._stream()), "vfn_vf_mlp_fwd")
    return w.check(f"vfn_vf_mlp_fwd, {cols} columns, M = {pts.shape[0]}")


def render_mlp_fwd(rn, pts, normals, dirs, feats):
    w = Window(pts.shape[0], 3)
    lib._check(lib.load().vfn_render_mlp_fwd(C.byref(rn.geometry()), _p(rn.packed_weights(), "packed"), _p(pts, "points"), _p(normals, "normals"),
                                             _p(dirs, "view_dirs"), _p(feats, "feats"), C.c_int64(pts.shape[0]), _p(w.out, "colors"),
                                             lib._stream()), "vfn_render_mlp_fwd")
    return w.check(f"vfn_render_mlp_fwd, M = {pts.shape[0]}")


def fused_fwd(vf, rn, pts, ray_dirs, spr):
    m = pts.shape[0]
    n, c, f = Window(m, 3), Window(m, 3), Window(m, lib.HIDDEN)
    lib._check(lib.load().vfn_vf_render_fused_fwd(C.byref(vf.geometry()), _p(vf.packed_weights(), "vf_packed"), C.byref(rn.geometry()),
                                                  _p(rn.packed_weights(), "rn_packed"), _p(pts, "points"), _p(ray_dirs, "ray_dirs"), C.c_int64(m),
                                                  C.c_int32(spr), _p(n.out, "normals"), _p(c.out, "colors"), _p(f.out, "feats"), lib._stream()),
               "vfn_vf_render_fused_fwd")
    what = f"vfn_vf_render_fused_fwd, {spr} samples per ray, M = {m}"
    return dict(vector=n.check(what), colours=c.check(what), feats=f.check(what))


def vf_mlp16_fwd(vf, pts):
    w = Window(pts.shape[0], 3)
    lib._check(lib.load().vfn_vf_mlp16_fwd(C.byref(vf.geometry()), _p(vf.packed16_weights(), "packed16", torch.uint8), _p(pts, "points"),
                                           C.c_int64(pts.shape[0]), _p(w.out, "out"), lib._stream()), "vfn_vf_mlp16_fwd")
    return w.check(f"vfn_vf_mlp16_fwd, M = {pts.shape[0]}")


def fused16_fwd(vf, rn, pts, ray_dirs, spr):
    m = pts.shape[0]
    n, c = Window(m, 3), Window(m, 3)
    lib._check(lib.load().vfn_vf_render_fused16_fwd(C.byref(vf.geometry()), _p(vf.packed16_weights(), "vf_packed16", torch.uint8),
                                                    C.byref(rn.geometry()), _p(rn.packed16_weights(), "rn_packed16", torch.uint8), _p(pts, "points"),
                                                    _p(ray_dirs, "ray_dirs"), C.c_int64(m), C.c_int32(spr), _p(n.out, "normals"), _p(c.out, "colors"),
                                                    lib._stream()), "vfn_vf_render_fused16_fwd")
    what = f"vfn_vf_render_fused16_fwd, {spr} samples per ray, M = {m}"
    return dict(vector=n.check(what), colours=c.check(what))


class Status:
    """The f16x3 range reports of the launches inside the block, in ``word``."""

    def __enter__(self):
        self.t = torch.zeros(1, dtype=torch.int32, device=dev())
        lib.f16x3_set_status(self.t)
        return self

    def __exit__(self, *exc):
        lib.f16x3_set_status(None)
        self.word = int(self.t.item())


def held(fam_key, kernel, what, got, ref, rename=None):
    """Scores ``got`` against float64, prints every figure beside its yardstick, asserts FACTOR x; -> {quantity: (device, yardstick)}."""
    yard = MC.yardstick(*fam_key)
    rows = {}
    for k, v in MC.score(got, ref).items():
        k = (rename or {}).get(k, k)
        rows[k] = (v, yard[k])
    print(f"MLPTAB {ids(fam_key)} {kernel} {what}: " + "  ".join(f"{k} {v:.2e} | {y:.2e}" for k, (v, y) in rows.items()))
    for k, (v, y) in rows.items():
        f = FACTOR[kernel][k]
        assert v <= f * y, f"{ids(fam_key)} {kernel} {what} {k}: {v:.3e} on the device, {y:.3e} float32 on the host (x {f:g} allowed)"
    return rows


@pytest.mark.parametrize("fam_key", FAMILIES["vf"], ids=ids)
def test_vf_mlp_fwd(fam_key):
    """vfn_vf_mlp_fwd with 3 columns and, where the net has features, with 259: vector and feature rows and feature columns of every M;
    the vector columns of both launches are the same bits."""
    vf, _ = device_net(fam_key[0])
    g = device_rows(*fam_key)
    for m in MC.M_VALUES:
        ref = MC.case_reference(fam_key[0], fam_key[1], m)
        vec = vf_mlp_fwd(vf, g["points"][:m].contiguous(), 3)
        held(fam_key, "fp32", f"vector-only M={m}", dict(vector=vec), ref)
        if vf._feature_dims() > 0:
            full = vf_mlp_fwd(vf, g["points"][:m].contiguous(), 3 + vf._feature_dims())
            held(fam_key, "fp32", f"full row M={m}", dict(vector=full[:, :3], feats=full[:, 3:]), ref)
            assert torch.equal(full[:, :3], vec)


@pytest.mark.parametrize("fam_key", FAMILIES["rn"], ids=ids)
def test_render_mlp_fwd(fam_key):
    """vfn_render_mlp_fwd on its own: normals and features are the float32 roundings of the float64 vector-field outputs (fresh
    rendering nets: random ones), every row has its own view direction."""
    _, rn = device_net(fam_key[0])
    g = device_rows(*fam_key)
    for m in MC.M_VALUES:
        got = render_mlp_fwd(rn, *(g[k][:m].contiguous() for k in ("points", "normals_in", "dirs", "feats_in")))
        held(fam_key, "fp32", f"rendering net alone M={m}", dict(colours=got), MC.case_reference(fam_key[0], fam_key[1], m), rename={"colours": "colours_alone"})


@pytest.mark.parametrize("fam_key", FAMILIES["both"], ids=ids)
def test_fused_fwd(fam_key):
    """vfn_vf_render_fused_fwd with the features written out: ray boundaries inside a workgroup, M no multiple of the tile."""
    vf, rn = device_net(fam_key[0])
    g = device_rows(*fam_key)
    for spr, rays in MC.FUSED_CASES:
        m = spr * rays
        got = fused_fwd(vf, rn, g["points"][:m].contiguous(), g["dirs"][:rays].contiguous(), spr)
        held(fam_key, "fp32", f"fused {spr}x{rays}", got, MC.fused_case_reference(fam_key[0], fam_key[1], spr, rays))


@pytest.mark.parametrize("fam_key", FAMILIES["both"], ids=ids)
def test_vf_mlp16_fwd(fam_key):
    vf, _ = device_net(fam_key[0])
    g = device_rows(*fam_key)
    fam = MC.family(*fam_key)
    for m in MC.M_VALUES:
        rng = MC.f16x3_range(float(fam.peaks["vf"][:m].max()))
        with Status() as st:
            vec = vf_mlp16_fwd(vf, g["points"][:m].contiguous())
        if rng == "inside":
            assert st.word == 0, f"M={m}: status {st.word} with every float64 pre-activation below {MC.F16X3_INSIDE:g}"
            held(fam_key, "f16x3", f"vector-only M={m}", dict(vector=vec), MC.case_reference(fam_key[0], fam_key[1], m))
        elif rng == "outside":
            print(f"MLPTAB {ids(fam_key)} f16x3 vector-only M={m}: outside the range, status {st.word}")
            assert st.word & lib.STATUS_ACT_SATURATED, f"M={m}: a pre-activation of {float(fam.peaks['vf'][:m].max()):.0f} went unreported"


@pytest.mark.parametrize("fam_key", FAMILIES["both"], ids=ids)
def test_fused16_fwd(fam_key):
    """vfn_vf_render_fused16_fwd, three products in the colour branch."""
    vf, rn = device_net(fam_key[0])
    g = device_rows(*fam_key)
    for spr, rays in MC.FUSED_CASES:
        m = spr * rays
        rng = MC.f16x3_range(MC.fused_reference(fam_key[0], fam_key[1], spr, rays)[2])
        with Status() as st:
            got = fused16_fwd(vf, rn, g["points"][:m].contiguous(), g["dirs"][:rays].contiguous(), spr)
        if rng == "inside":
            assert st.word == 0, f"{spr}x{rays}: status {st.word} with every float64 pre-activation below {MC.F16X3_INSIDE:g}"
            held(fam_key, "f16x3", f"fused {spr}x{rays}", got, MC.fused_case_reference(fam_key[0], fam_key[1], spr, rays))
        elif rng == "outside":
            print(f"MLPTAB {ids(fam_key)} f16x3 fused {spr}x{rays}: outside the range, status {st.word}")
            assert st.word & lib.STATUS_ACT_SATURATED


# ------------------------------------------------------------------------------------------------
# gradients through the fold
# ------------------------------------------------------------------------------------------------
def _model(name, mode):
    """The facade on the device with the networks of ``name`` and the arithmetic and storages of ``mode`` (test_hip_backward.py)."""
    fx, d = helpers.load_fixture(name.split("+")[0])
    model = helpers.build_model(fx, d, device="cuda:0")
    net = MC.build_net(name)
    model.vector_field_network.load_state_dict(net.vf.state_dict())
    model.rendering_network.load_state_dict(net.rn.state_dict())
    opts = mode.split("+")
    model.precision = opts[0]
    model.activation_storage = "f16" if "f16act" in opts else "fp32"
    model.gradient_storage = "f16" if "f16dy" in opts else "fp32"
    return fx, d, model


GRAD_MODES = ("fp32", "f16x3", "f16x3+f16act+f16dy")


def figures(tag, got, case, name, which):
    """The per-row, per-block and per-element figures of ``got`` against float64 beside the host-float32 yardstick, on an MLPGRAD line
    (printed for the 16- and 22-bit arithmetics, asserted for the exact one: test_*_gradients_exact).  -> {(kind, figure): (device, yardstick)}."""
    scores = MC.grad_scores(got, {**case.grads, **case.input_grads}, MC.build_net(name), which)
    yard = MC.grad_yardstick(name, which)
    rows = {k: (v, yard[k]) for k, v in MC.pool_by_kind(scores).items()}
    print(f"MLPGRAD {tag}: " + "  ".join(f"{k}.{f} {v:.2e} | {y:.2e} ({v / y:.1f} x)" for (k, f), (v, y) in sorted(rows.items())))
    return scores, yard, rows


@pytest.mark.parametrize("mode", GRAD_MODES)
@pytest.mark.parametrize("name", MC.GRAD_NETS)
def test_vector_field_forward_gradients(name, mode):
    """VectorFieldNetwork.forward (full row) under autograd on rows away from every ReLU kink, a fixed random linear functional of the
    259 columns: every parameter's gradient, BatchNorm gamma and beta among them, against float64 autograd of the restatement, per
    tensor; the per-row, per-block and per-element figures are printed.  (Points that ask: test_vector_field_gradients_exact.)"""
    case = MC.vf_grad_case(name)
    _, _, model = _model(name, mode)
    vf = model.vector_field_network
    for p in vf.parameters():
        p.grad = None
    out = vf(case.inputs["points"].to(dev()))
    (out * case.coef.to(dev())).sum().backward()
    assert out.shape == case.out.shape and float((out.detach().cpu().double() - case.out).abs().max()) < 1e-4
    errs = {k: helpers.grad_rel_err(p.grad, case.grads[k]) for k, p in vf.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"MLPGRAD {name} vector field forward {mode}: worst {errs[worst]:.2e} at {worst}; gamma/beta worst "
          f"{max(v for k, v in errs.items() if '.1.' in k):.2e} (bound {MODE_TOL[mode]:g})")
    assert set(errs) == set(case.grads)
    assert all(v < MODE_TOL[mode] for v in errs.values()), {k: v for k, v in errs.items() if v >= MODE_TOL[mode]}
    figures(f"{name} vector field params {mode} M={case.coef.shape[0]}", {k: p.grad for k, p in vf.named_parameters()}, case, name, "vf")


@pytest.mark.parametrize("mode", ("fp32", "f16x3"))
@pytest.mark.parametrize("name", MC.GRAD_NETS)
def test_rendering_forward_gradients(name, mode):
    """RenderingNetwork.forward under autograd: every parameter's gradient and the features' against float64 autograd."""
    case = MC.rn_grad_case(name)
    _, _, model = _model(name, mode)
    rn = model.rendering_network
    for p in rn.parameters():
        p.grad = None
    g = {k: v.to(dev()) for k, v in case.inputs.items()}
    feats = g["feats"].requires_grad_(True)
    out = rn(g["points"], g["normals"], g["dirs"], feats)
    (out * case.coef.to(dev())).sum().backward()
    assert float((out.detach().cpu().double() - case.out).abs().max()) < 1e-4
    errs = {k: helpers.grad_rel_err(p.grad, case.grads[k]) for k, p in rn.named_parameters()}
    errs["feats"] = helpers.grad_rel_err(feats.grad, case.grads["feats"])
    worst = max(errs, key=errs.get)
    print(f"MLPGRAD {name} rendering forward {mode}: worst {errs[worst]:.2e} at {worst}; features {errs['feats']:.2e} (bound {MODE_TOL[mode]:g})")
    assert set(errs) == set(case.grads)
    assert all(v < MODE_TOL[mode] for v in errs.values()), {k: v for k, v in errs.items() if v >= MODE_TOL[mode]}
    figures(f"{name} rendering {mode} M={case.coef.shape[0]}", {**{k: p.grad for k, p in rn.named_parameters()}, "feats": feats.grad}, case, name, "rn")


def _open_units(model):
    """The ReLU masks the backward applied, in sorted sample order (as test_hip_backward.test_render_gradients reads them)."""
    units = lib.unpack_sign_words(model._debug_masks).cpu() if model._debug_masks is not None else model._debug_saved.cpu() > 0
    if getattr(model, "_debug_dst", None) is not None:
        dst = model._debug_dst.cpu().long()
        by_sample = torch.empty_like(units)
        by_sample[:, dst] = units
        units = by_sample
    return units


def test_render_gradients_with_real_statistics():
    """model.render with the fixture's uniforms under autograd on trained_far+stats (44 % of its rays meet a surface), default 16-bit
    storages and precision "fp32": identical sampling in both device runs and in the oracle, then every parameter's gradient against
    the oracle's autograd with this run's ReLU masks pinned (helpers.oracle_gradients), and the two device runs against each other."""
    name = "trained_far+stats"
    grads, z = {}, {}
    for mode in ("f16x3+f16act+f16dy", "fp32"):
        fx, d, model = _model(name, mode)
        loss, out = _hip_gradients(fx, d, model)
        z[mode] = out.z_vals.detach().cpu()
        masks = [_open_units(model)[slot] for slot in list(range(8)) + list(range(9, 13))]
        cpu = helpers.build_model(fx, d)
        cpu.vector_field_network.load_state_dict(MC.build_net(name).vf.state_dict())
        cpu.rendering_network.load_state_dict(MC.build_net(name).rn.state_dict())
        probe_loss, probe = helpers.oracle_gradients(fx, d, cpu)
        assert torch.equal(z[mode], probe["_out"]["z_vals"]), "sampling must be the oracle's for the comparison to mean anything"
        masks = [mk[:, :act.shape[1]] for mk, act in zip(masks, probe["_hidden"])]
        flips = sum(int((mk != (act > 0)).sum()) for mk, act in zip(masks, probe["_hidden"]))
        ref_loss, ref = helpers.oracle_gradients(fx, d, cpu, masks=masks)
        assert abs(loss - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss))
        assert float(ref["_out"]["weights"].sum(dim=-1).max()) > 0.5
        nets = {"vf": model.vector_field_network, "rn": model.rendering_network}
        grads[mode] = {f"{tag}.{k}": p.grad.detach().cpu() for tag, net in nets.items() for k, p in net.named_parameters()}
        errs = {k: helpers.grad_rel_err(v, ref[k]) for k, v in grads[mode].items()}
        worst = max(errs, key=errs.get)
        print(f"MLPGRAD {name} render {mode}: worst {errs[worst]:.2e} at {worst}, {flips} units on the other side of zero (bound {MODE_TOL[mode]:g})")
        assert all(v < MODE_TOL[mode] for v in errs.values()), {k: v for k, v in errs.items() if v >= MODE_TOL[mode]}
    a, b = grads["f16x3+f16act+f16dy"], grads["fp32"]
    assert torch.equal(z["f16x3+f16act+f16dy"], z["fp32"]), "sampling differs between the two device runs"
    between = {k: helpers.grad_rel_err(a[k], b[k]) for k in a}
    worst = max(between, key=between.get)
    print(f"MLPGRAD {name} render, default storages against precision fp32: worst {between[worst]:.2e} at {worst}")
    assert all(v < MODE_TOL["f16x3+f16act+f16dy"] for v in between.values())


# ------------------------------------------------------------------------------------------------
# gradients on every geometry, inputs included: per row, block and element against float64
# ------------------------------------------------------------------------------------------------
SPLIT_TOL = 2e-3           # batchstat._arith: the documented bound of the layer-at-a-time split arithmetic (per tensor)
# (net, what asks for a gradient) the backward refuses at the call, before any launch.  Never listed because its numbers were off:
#   vf_2h, points   the points' gradient comes from the layer-at-a-time kernels, which apply BatchNorm after every Linear but the
#                   last (batchstat._require_shape); vf_2h has none.  Its parameters' gradients come from the fused chain.
REFUSED = {("vf_2h", "points"): NotImplementedError}
VF_ASKS = [(n, a) for n in MC.GRAD_VF for a in ("params", "points")]
RN_INPUTS = ("feats", "normals")
aid = lambda c: f"{c[0]}-{c[1]}"      # noqa: E731


def _module(name, which, precision):
    """A fresh copy of the net's module on the device with the arithmetic ``precision`` ("fp32": exact products on both paths)."""
    lib.load()
    vf, rn = MC.build_net(name).on(dev())
    mod = vf if which == "vf" else rn
    mod.precision = precision
    mod.config = copy.copy(mod.config)
    return mod


def _no_launch(monkeypatch):
    """Every launch takes its stream from lib._stream: none may happen while this is in place."""
    def stream():
        raise AssertionError("a kernel was launched by a call that had to be refused")
    monkeypatch.setattr(lib, "_stream", stream)


def _vf_gradients(mod, case, points_ask):
    for p in mod.parameters():
        p.grad = None
    pts = case.inputs["points"].to(dev()).requires_grad_(points_ask)
    out = mod(pts)
    (out * case.coef.to(dev())).sum().backward()
    got = {k: p.grad for k, p in mod.named_parameters()}
    if points_ask:
        got["points"] = pts.grad
    return out, got


def _rn_gradients(mod, case, asks=RN_INPUTS):
    for p in mod.parameters():
        p.grad = None
    g = {k: v.to(dev()).requires_grad_(k in asks) for k, v in case.inputs.items()}
    out = mod(g["points"], g["normals"], g["dirs"], g["feats"])
    (out * case.coef.to(dev())).sum().backward()
    got = {k: p.grad for k, p in mod.named_parameters()}
    got.update({k: g[k].grad for k in asks})
    return out, got


def grads_held(tag, out, got, case, name, which, factor, tol):
    """Every delivered gradient against float64: the output first, then per tensor kind the worst figure beside its host-float32
    yardstick on an MLPGRAD line; asserts ``tol(key)`` per tensor (the project's existing measure) and, where ``factor`` is given,
    factor x yardstick for every figure.  -> {(kind, figure): (device, yardstick)}."""
    missing = [k for k, v in got.items() if v is None]
    assert not missing, f"{tag}: no gradient delivered for {missing}"
    assert out.shape == case.out.shape and float((out.detach().cpu().double() - case.out).abs().max()) < 1e-4
    scores, yard, rows = figures(tag, got, case, name, which)
    over = {k: s["tensor"] for k, s in scores.items() if not s["tensor"] < tol(k)}
    assert not over, f"{tag}: per tensor {over}"
    if factor is not None:
        bad = {(k, f): (v, factor * yard[(MC.grad_kind(k), f)]) for k, s in scores.items() for f, v in s.items()
               if not v <= factor * yard[(MC.grad_kind(k), f)]}
        assert not bad, f"{tag}: above {factor:g} x the host-float32 yardstick: {bad}"
    return rows


@pytest.mark.parametrize("ask", VF_ASKS, ids=aid)
def test_vector_field_gradients_exact(ask, monkeypatch):
    """VectorFieldNetwork.forward in eval mode with precision "fp32" on every gradient net at every M of GRAD_M.  "params": only the
    parameters ask (the fused chain, vfn_mlp_bwd_chain with _weight_grads and vfn_unfold_kernel; the narrow net layer by layer).
    "points": the points ask too, which sends the call through the layer-at-a-time kernels with the running statistics
    (batchstat._VFTrainMode, embed_rows_bwd with the skip piece).  Every figure within MAX_FACTOR x the host-float32 yardstick, or the
    listed refusal before a launch."""
    name, what = ask
    mod = _module(name, "vf", "fp32")
    if ask in REFUSED:
        case = MC.vf_grad_case(name, 33)
        pts = case.inputs["points"].to(dev()).requires_grad_(True)
        torch.cuda.synchronize()
        _no_launch(monkeypatch)
        with pytest.raises(REFUSED[ask]):
            mod(pts)
        return
    for m in MC.GRAD_M:
        case = MC.vf_grad_case(name, m)
        out, got = _vf_gradients(mod, case, what == "points")
        assert set(got) == set(case.grads) | ({"points"} if what == "points" else set())
        grads_held(f"{name} vector field {what} fp32 M={case.coef.shape[0]}", out, got, case, name, "vf", MC.MAX_FACTOR, lambda k: MODE_TOL["fp32"])


@pytest.mark.parametrize("name", MC.GRAD_RN)
def test_rendering_gradients_exact(name):
    """RenderingNetwork.forward in eval mode with precision "fp32" (the exact products of the layer-at-a-time path) and
    detach_normals=False, at every M of GRAD_M: every parameter, the features and the normals, per row."""
    mod = _module(name, "rn", "fp32")
    mod.config.detach_normals = False
    for m in MC.GRAD_M:
        case = MC.rn_grad_case(name, m)
        out, got = _rn_gradients(mod, case)
        assert set(got) == set(case.grads) | set(RN_INPUTS)
        grads_held(f"{name} rendering fp32 M={case.coef.shape[0]}", out, got, case, name, "rn", MC.MAX_FACTOR, lambda k: MODE_TOL["fp32"])


@pytest.mark.parametrize("name", MC.GRAD_RN)
def test_rendering_inputs_without_a_gradient(name, monkeypatch):
    """detach_normals=True (the reference detaches): normals.grad stays None while the features get theirs.  Points or view directions
    that ask are refused at the call, by name, before any launch: the backward has no gradient for them."""
    mod = _module(name, "rn", "fp32")
    case = MC.rn_grad_case(name, 33)
    mod.config.detach_normals = True
    _, got = _rn_gradients(mod, case)
    assert got["normals"] is None and got["feats"] is not None
    torch.cuda.synchronize()
    _no_launch(monkeypatch)
    for asked, word in (("points", "points"), ("dirs", "view_dirs")):
        g = {k: v.to(dev()).requires_grad_(k == asked) for k, v in case.inputs.items()}
        with pytest.raises(NotImplementedError, match=word):
            mod(g["points"], g["normals"], g["dirs"], g["feats"])


SPLIT_VF = [n for n in MC.GRAD_VF if (n, "points") not in REFUSED]


@pytest.mark.parametrize("name", SPLIT_VF)
def test_vector_field_gradients_split(name):
    """The split products of the layer-at-a-time path (precision "f16x3" with points that ask) at the full row count: parameters and
    points inside the path's documented per-tensor bound; the per-row, per-block and per-element figures are printed, not bounded (a
    bound for 16- and 22-bit arithmetic has to come from an emulation of its roundings)."""
    mod = _module(name, "vf", "f16x3")
    case = MC.vf_grad_case(name)
    out, got = _vf_gradients(mod, case, True)
    grads_held(f"{name} vector field points split M={case.coef.shape[0]}", out, got, case, name, "vf", None, lambda k: SPLIT_TOL)


@pytest.mark.parametrize("name", MC.GRAD_RN)
def test_rendering_gradients_split(name):
    """The rendering nets, fresh and shipped, on the split products with detach_normals=False: parameters and features inside
    MODE_TOL["f16x3"] (as in test_rendering_forward_gradients), the normals, which MODE_TOL has no entry for, inside the path's 2e-3;
    figures printed."""
    mod = _module(name, "rn", "f16x3")
    mod.config.detach_normals = False
    case = MC.rn_grad_case(name)
    out, got = _rn_gradients(mod, case)
    grads_held(f"{name} rendering split M={case.coef.shape[0]}", out, got, case, name, "rn", None,
               lambda k: SPLIT_TOL if k == "normals" else MODE_TOL["f16x3"])


@pytest.mark.parametrize("scale", MC.SCALES)
def test_narrow_vector_field_forward(scale):
    """The narrow net (hidden width 64, 32 features, BatchNorm) in eval mode under no_grad, vf_forward_eval_rows with the exact
    products: vector and feature rows and feature columns at every M against float64, MAX_FACTOR x the forward yardstick."""
    name = next(iter(MC.NARROW_VF))
    mod = _module(name, "vf", "fp32")
    assert not mod.supports_fused()
    g, yard = device_rows(name, scale), MC.yardstick(name, scale)
    for m in MC.M_VALUES:
        with torch.no_grad():
            out = mod(g["points"][:m].contiguous())
        assert out.shape == (m, 3 + mod._feature_dims())
        scores = MC.score(dict(vector=out[:, :3], feats=out[:, 3:]), MC.case_reference(name, scale, m))
        print(f"MLPTAB {name}-s{scale:g} rows fp32 M={m}: " + "  ".join(f"{k} {v:.2e} | {yard[k]:.2e}" for k, v in scores.items()))
        for k, v in scores.items():
            assert v <= MC.MAX_FACTOR * yard[k], f"{name} scale {scale:g} M={m} {k}: {v:.3e} on the device, {yard[k]:.3e} float32 on the host"
