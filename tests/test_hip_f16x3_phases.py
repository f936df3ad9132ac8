"""The f16x3 inference launches after their prologue, encoding boundary and tail were trimmed (csrc/vfn_mlp16.hip: encoding geometry
at compile time, lane-half swap instead of LDS shuffles, range bookkeeping over the raw coordinate columns only, the saturation mask
in one scalar pair): only selection logic, data movement and bookkeeping changed, so every output value and every status word is
held to the BITS the commit before that change returned (tests/golden/f16x3_phase_bits.npz, recorded by
tests/golden/make_f16x3_phase_bits.py, which also defines the cases); the run-time form of the encoding still serves the other
geometries the plan admits; and the compiled-in form equals the run-time form on the shipped geometry."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, build_model, load_fixture, rel_err

pytestmark = pytest.mark.gpu
TIGHT = 2e-5


def _maker():
    spec = importlib.util.spec_from_file_location("make_f16x3_phase_bits", os.path.join(GOLDEN_DIR, "make_f16x3_phase_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    """(the generator module, stored inputs, the recorded outputs, the same cases on the library under test) — computed once."""
    mk = _maker()
    raw = np.load(os.path.join(GOLDEN_DIR, "f16x3_phase_bits.npz"))
    inp = {k[3:]: torch.from_numpy(raw[k]) for k in raw.files if k.startswith("in.")}
    want = {k[4:]: torch.from_numpy(raw[k]) for k in raw.files if k.startswith("out.")}
    got = mk.record(inp, device="cuda:0")
    return mk, inp, want, got


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal, and the same bit patterns where that says less (NaN payloads, the sign of zero)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a, b) and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _names(want, prefixes):
    return sorted(k for k in want if any(k.startswith(p) for p in prefixes))


def _assert_recorded(want, got, prefixes):
    names = _names(want, prefixes)
    assert names, prefixes
    for k in names:
        assert k in got, f"{k} is in the recorded file but the library under test did not produce it"
        if k.endswith("_status"):
            assert int(got[k][0]) == int(want[k][0]), (k, int(got[k][0]), int(want[k][0]))
        else:
            assert _same_bits(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))


def test_every_recorded_case_is_produced(recorded):
    mk, inp, want, got = recorded
    assert set(want) == set(got), set(want) ^ set(got)
    for m in mk.COUNTS:
        assert want[f"fused_{m}_normals"].shape == (m, 3) and want[f"vector_{m}_vec"].shape == (m, 3)


def test_fused_launches_return_the_recorded_bits(recorded):
    """1, 31, 33, 129 and 299 points, 23 samples per ray: a wave spans rays, the last tile is partial."""
    _, _, want, got = recorded
    _assert_recorded(want, got, ("fused_",))
    assert all(int(want[k][0]) == 0 for k in _names(want, ("fused_",)) if k.endswith("_status"))


def test_vector_only_launches_return_the_recorded_bits(recorded):
    _, _, want, got = recorded
    _assert_recorded(want, got, ("vector_",))


def test_scatter_launch_returns_the_recorded_bits(recorded):
    """out_index with -1 rows: the dropped rows keep what the caller had there (7.0), the others the recorded bits."""
    mk, inp, want, got = recorded
    _assert_recorded(want, got, ("scatter_",))
    dropped = inp["perm"].long()[inp["scatter_index"] < 0]
    kept = inp["scatter_index"].long()[inp["scatter_index"] >= 0]
    assert len(dropped) > 0 and bool((got["scatter_colors"][dropped] == 7.0).all()) and bool((got["scatter_normals"][dropped] == 7.0).all())
    # the scatter launch writes what the in-place launch computes for the same samples
    m = mk.COUNTS[-1]
    assert _same_bits(got["scatter_colors"][kept], got[f"fused_{m}_colors"][kept])
    assert _same_bits(got["scatter_normals"][kept], got[f"fused_{m}_normals"][kept])


def test_block_pair_returns_the_recorded_bits(recorded):
    """vf_feat16_fwd + render16_from_blocks on 299 rows (the last group of 32 holds 11)."""
    mk, _, want, got = recorded
    _assert_recorded(want, got, ("blocks_",))
    m = mk.COUNTS[-1]
    assert _same_bits(got["blocks_colors"], got[f"fused_{m}_colors"]) and _same_bits(got["blocks_normals"], got[f"fused_{m}_normals"])


def test_range_guard_situations_return_the_recorded_bits_and_status(recorded):
    """In family: status 0.  Hidden gain 8 / BatchNorm gamma up to 30: bit 0 (an activation reached the clamp).  Points x 2000:
    bit 1 (an input did) — raised through the raw coordinate column, the only bookkeeping the encoding operand still carries."""
    _, _, want, got = recorded
    _assert_recorded(want, got, ("guard_",))
    for launch in ("vector", "fused"):
        assert int(got[f"guard_in_family_{launch}_status"][0]) == 0
        assert int(got[f"guard_gain8_gamma30_{launch}_status"][0]) & 1
        assert int(got[f"guard_points_2000_{launch}_status"][0]) & 2
    for k in _names(got, ("guard_",)):
        assert bool(torch.isfinite(got[k].float()).all()), k


def test_run_time_form_serves_the_other_geometries(recorded):
    """A rendering net with 3 octaves (odd: the `upper octave of the pair does not exist` arm) and with none, a vector-field net
    with 5 where the plan admits it: the recorded bits, and the exact-fp32 kernels within TIGHT."""
    from vf_nerf_amd import lib
    mk, inp, want, got = recorded
    _assert_recorded(want, got, ("rn3_", "rn0_", "vf5_"))
    fx, d = load_fixture(mk.FIXTURE)
    model = build_model(fx, d, device="cuda:0")
    nets = mk.other_geometries(model, fx, torch.device("cuda:0"))
    assert {"rn3", "rn0"} <= set(nets)
    assert ("vf5" in nets) == ("vf5_fused_colors" in want)
    pts, dirs = inp[f"pts_{mk.OTHER_M}"].to("cuda:0"), inp[f"dirs_{mk.OTHER_M}"].to("cuda:0")
    for tag, (vf, rn) in nets.items():
        assert (vf._multires(), rn._multires()) != (6, 4)
        n32, c32, _ = lib.vf_render_fused_fwd(vf.geometry(), vf.packed_weights(), rn.geometry(), rn.packed_weights(), pts, dirs, mk.S)
        en, ec = rel_err(got[f"{tag}_fused_normals"].to("cuda:0"), n32), rel_err(got[f"{tag}_fused_colors"].to("cuda:0"), c32)
        print(f"{tag}: f16x3 (run-time encoding geometry) vs the exact-fp32 kernels: normals {en:.2e}, colours {ec:.2e}")
        assert en < TIGHT and ec < TIGHT, (tag, en, ec)
        assert int(got[f"{tag}_fused_status"][0]) == 0


def test_compiled_in_geometry_equals_the_run_time_form(recorded):
    """The shipped pair both ways on the same 299 points: the inference launch has (6, 4) compiled in, the saving forward of the
    training path (vfn_vf_render_fused16_fwd_train: the same arithmetic plus the workspace) reads the geometry at run time — that is
    what its launcher keys on.  Normals and colours bit for bit."""
    from vf_nerf_amd import lib
    from vf_nerf_amd.backward import _Workspace, _entries
    mk, inp, _, got = recorded
    fx, d = load_fixture(mk.FIXTURE)
    model = build_model(fx, d, device="cuda:0")
    vf, rn = model.vector_field_network, model.rendering_network
    dev = torch.device("cuda:0")
    m = mk.COUNTS[-1]
    pts, dirs = inp[f"pts_{m}"].to(dev), inp[f"dirs_{m}"].to(dev)
    ws = _Workspace(m, len(_entries(vf)) + len(_entries(rn)), dev)
    n_rt, c_rt = lib.vf_render_fused16_fwd_train(vf.geometry(), vf.packed16_weights(), rn.geometry(), rn.packed16_weights(), pts, dirs, mk.S,
                                                 ws.saved, ws.aux_vf, ws.aux_rn, ws.masks)
    assert _same_bits(n_rt.cpu(), got[f"fused_{m}_normals"]) and _same_bits(c_rt.cpu(), got[f"fused_{m}_colors"])
