"""The f16x3 launch modes that tests/golden/f16x3_phase_bits.npz does not hold — two colour products, the saving forwards in both
storages, the single-product training forwards, the feature-block pair — at 1, 127, 128, 129 and 128 x 257 + 5 points (a partial
wave, a full group, a second workgroup with one valid point, more workgroups than CUs): every output value, every workspace and
every status word is held to the BITS recorded from the commit before the chunk loop's issue stream was budgeted gap by gap
(tests/golden/f16x3_schedule_bits.npz, recorded by tests/golden/make_f16x3_schedule_bits.py, which also defines the cases).  A change
of the schedule, of the register fragment ring or of the ring hand-over of csrc/vfn_mlp16.hip must return them; a fragment read
before its chunk has landed shows here as other bits in some workgroup of the largest launch.

And, without a GPU: tools/mlp16_instruction_mix.py --gaps on a ten-line listing gives the table worked out by hand."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maker():
    spec = importlib.util.spec_from_file_location("make_f16x3_schedule_bits", os.path.join(GOLDEN_DIR, "make_f16x3_schedule_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    """(the generator module, its inputs, the recorded outputs, the same cases on the library under test) — computed once."""
    mk = _maker()
    raw = np.load(os.path.join(GOLDEN_DIR, "f16x3_schedule_bits.npz"))
    want = {k[4:]: torch.from_numpy(raw[k]) for k in raw.files if k.startswith("out.")}
    inp = mk.make_inputs()
    got = mk.record(inp, device="cuda:0")
    return mk, inp, want, got


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _assert_recorded(want, got, prefix):
    names = sorted(k for k in want if k.startswith(prefix))
    assert names, prefix
    for k in names:
        assert k in got, f"{k} is in the recorded file but the library under test did not produce it"
        if k.endswith("_status") or k.endswith("_sum"):
            assert int(got[k][0]) == int(want[k][0]), (k, int(got[k][0]), int(want[k][0]))
        else:
            assert _same_bits(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))


@pytest.mark.gpu
def test_every_recorded_case_is_produced(recorded):
    mk, _, want, got = recorded
    assert set(want) == set(got), set(want) ^ set(got)
    for m in mk.COUNTS:
        for tag in ("c2", "vftrain_fp32", "vftrain_f16frag", "fusedtrain_fp32", "fusedtrain_f16frag", "p1vec", "p1fused", "blocks"):
            assert f"{tag}_{m}_status" in want, (tag, m)
    assert mk.COUNTS[-1] == 128 * 257 + 5 and want[f"c2_{mk.COUNTS[-1]}_normals_tail"].shape == (mk.TAIL_ROWS, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["c2", "vftrain_fp32", "vftrain_f16frag", "fusedtrain_fp32", "fusedtrain_f16frag", "p1vec", "p1fused",
                                  "blocks", "fused3"])
def test_launch_mode_returns_the_recorded_bits(recorded, case):
    """Outputs, workspace checksums and status words of one launch mode at every recorded size; in family, so every status is 0."""
    _, _, want, got = recorded
    _assert_recorded(want, got, case + "_")
    assert all(int(want[k][0]) == 0 for k in want if k.startswith(case + "_") and k.endswith("_status"))


@pytest.mark.gpu
def test_largest_fused_launch_repeats_to_the_same_bits(recorded):
    """128 x 257 + 5 points, three launches in a row: each returns the recorded bits (a race on the weight ring or on the fragment
    ring would not repeat)."""
    mk, inp, want, _ = recorded
    dev = torch.device("cuda:0")
    m = mk.COUNTS[-1]
    model = mk.build_model(dev)
    g = {k: inp[k].to(dev) for k in (f"pts_{m}", f"dirs_{m}")}
    for rep in range(3):
        out = {}
        n, c, status = mk.fused3(model, g, m, dev)
        mk.rows(out, f"fused3_{m}_normals", n); mk.rows(out, f"fused3_{m}_colors", c); out[f"fused3_{m}_status"] = status
        _assert_recorded(want, out, f"fused3_{m}_")


# ---- the tool (no GPU) ----------------------------------------------------------------------------------------------------
LISTING = """\
_Z16vfn_mlp16_kernelILi3EEv9Mlp16Args:
	v_mfma_f32_32x32x16_f16 v[0:15], v[20:23], a[0:3], v[0:15]
	v_mfma_f32_32x32x16_f16 v[0:15], v[20:23], a[4:7], v[0:15]
	v_max3_i32 v40, v1, v2, v40
	v_med3_f32 v41, v1, 0, v60
	v_med3_f32 v42, v2, 0, v60
	v_cvt_pk_f16_f32 v43, v41, v42
	v_fma_mix_f32 v44, v43, -1.0, v41 op_sel_hi:[1,0,0]
	s_nop 0
	v_mfma_f32_32x32x16_f16 v[0:15], v[24:27], a[0:3], v[0:15]
	s_mov_b32 m0, s9
	buffer_load_dwordx4 v50, s[12:15], s8 offen lds
	v_mfma_f32_32x32x16_f16 v[0:15], v[28:31], a[8:11], v[0:15]
	ds_read_b128 v[20:23], v48 offset:2048
	v_exp_f32_e32 v45, v44
	s_waitcnt lgkmcnt(0)
	v_mfma_f32_32x32x16_f16 v[0:15], v[20:23], a[12:15], v[0:15]
	v_add_f32 v1, v2, v3
	v_add_f32 v1, v2, v3
	v_add_f32 v1, v2, v3
	v_add_f32 v1, v2, v3
	v_add_f32 v1, v2, v3
	v_add_f32 v1, v2, v3
	v_add_f32 v1, v2, v3
	v_add_f32 v1, v2, v3
	v_add_f32 v1, v2, v3
	v_add_f32 v1, v2, v3
	v_mfma_f32_32x32x16_f16 v[16:31], v[20:23], a[0:3], v[16:31]
	v_mfma_f32_32x32x16_f16 v[16:31], v[20:23], a[4:7], v[16:31]
.Lfunc_end0:
"""
# By hand (prices: VALU 4, v_cvt_pk_f16_f32 5, transcendental 8, ds_read 4, s_nop 0 -> 4, SALU 1, piece 60; budget 24):
#   gap 1  empty                                                   0
#   gap 2  4 VALU + cvt_pk + s_nop 0 = 16 + 5 + 4                  25   5 VALU, no piece: overrun 1 in "any other gap"
#   gap 3  s_mov + piece = 1 + 60                                  61   a piece that shares its gap: overrun 37 = 36 own + 1
#   gap 4  ds_read + v_exp + s_waitcnt = 4 + 8 + 1                 13
#   gap 5  10 VALU                                                 40   the LONGEST gap: not a steady-state gap, left out
#   gap 6  empty                                                   0
EXPECTED = """\
### `vfn_mlp16_kernel<3>`: gap budget

Steady-state gaps: 5; empty: 2; priced cost: total 99, mean 19.8 against a budget of 24; priced above 24 without a piece: 1; pieces that share their gap: 1.

| priced cost of a gap | gaps |
|---|---|
| 0 | 2 |
| 1-8 | 0 |
| 9-16 | 1 |
| 17-24 | 0 |
| 25-32 | 1 |
| 33-48 | 0 |
| 49-64 | 1 |
| 65-96 | 0 |
| above 96 | 0 |

| overrun (priced cost above the budget) | gaps | cycles |
|---|---|---|
| gap with a piece | 1 | 37 |
| ... of it the pieces themselves (60 does not fit into 24) | | 36 |
| ... of it what shares the gap with them | | 1 |
| gap with >= 6 VALU, no piece | 0 | 0 |
| any other gap | 1 | 1 |

Per tile, the priced cost of every gap in order (`p`: the gap holds a piece; the last gap of a tile is its boundary):

    tile   0: 0 25 61p 13
    tile   1: 0

"""


def test_gap_table_of_a_synthetic_listing(tmp_path):
    path = tmp_path / "listing.s"
    path.write_text(LISTING)
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "mlp16_instruction_mix.py"), "--gaps", str(path), "3"],
                         check=True, capture_output=True, text=True).stdout
    assert out == EXPECTED
