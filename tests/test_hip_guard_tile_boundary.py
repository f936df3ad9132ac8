"""The f16x3 range guard after it left the tile boundary (csrc/vfn_mlp16.hip): a finished ReLU tile is looked at while its epilogue
runs, in the first K steps of the NEXT tile — for a layer's last tile that is the next layer's first tile, for the tile in front of a
head the head's only tile — as a signed-integer maximum over the accumulators' bit patterns.  What could go wrong is a tile whose
look never happens (the last tile of a layer, the head's input tile) or a changed value; so: the fused launch against the split
launches and the exact-fp32 kernels at the point counts around a wave and a workgroup, the status word tile by tile, and one training
step against the launch-by-launch path."""
import pytest
import torch

from helpers import build_model, load_fixture, rel_err
from oracle import vfnerf_oracle as O
from vf_nerf_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIGHT = 2e-5                  # the f16x3 kernels' bound against the exact-fp32 kernels (tests/test_hip_f16x3.py)
ACT_LIMIT = 60000.0 / 64.0    # VFN16_CLAMP / VFN16_XSCALE: the activation at which the clamp acts


def _fresh():
    fx, d = load_fixture("c1_perturb")
    return build_model(fx, d, device=DEV)


@pytest.fixture(scope="module")
def model():
    return _fresh()


def _inputs(m, seed=7):
    gen = torch.Generator().manual_seed(seed)
    pts = (torch.rand(m, 3, generator=gen) * 2 - 1).to(DEV)
    dirs = torch.nn.functional.normalize(torch.randn(m, 3, generator=gen), dim=1).to(DEV)
    return pts.contiguous(), dirs.contiguous()


def _fused(model, pts, dirs):
    vf, rn = model.vector_field_network, model.rendering_network
    return lib.vf_render_fused16_fwd(vf.geometry(), vf.packed16_weights(), rn.geometry(), rn.packed16_weights(), pts, dirs, 1)


def _status_of(launch):
    """The range-report word after ``launch()``: bit 0 a hidden activation reached the clamp, bit 1 an input did."""
    word = torch.zeros(4, dtype=torch.int32, device=DEV)
    lib.f16x3_set_status(word)
    try:
        launch()
        torch.cuda.synchronize()
        return int(word[0])
    finally:
        lib.f16x3_set_status(None)


@pytest.mark.parametrize("m", [1, 127, 128, 129, 257])
def test_fused_launch_equals_split_launches_and_follows_fp32(model, m):
    """The fused VF + rendering launch (what render() issues with model.reuse_proposal = False) against vfn_vf_feat16_fwd +
    vfn_render16_from_blocks (the split path) on the same inputs: bit-equal normals and colours; both within the f16x3 bound of the
    exact-fp32 fused kernel.  1 point: a partial wave; 127 / 128: one workgroup; 129 / 257: a second / third workgroup with one live row."""
    vf, rn = model.vector_field_network, model.rendering_network
    pts, dirs = _inputs(m, seed=100 + m)
    want_n, want_c = _fused(model, pts, dirs)
    vecs = torch.empty(m, 3, device=DEV)
    blocks = torch.empty(lib.block_rows(m), lib.BLOCK_BYTES, dtype=torch.uint8, device=DEV)
    lib.vf_feat16_fwd(vf.geometry(), vf.packed16_weights(), pts, vecs, blocks)
    rows = torch.arange(m, dtype=torch.int32, device=DEV)
    got_n, got_c = lib.render16_from_blocks(rn.geometry(), rn.packed16_weights(), blocks, vecs, rows, pts, dirs, 1)
    assert torch.equal(got_n, want_n) and torch.equal(got_c, want_c)
    ref_n, ref_c, _ = lib.vf_render_fused_fwd(vf.geometry(), vf.packed_weights(), rn.geometry(), rn.packed_weights(), pts, dirs, 1)
    en, ec = rel_err(want_n, ref_n), rel_err(want_c, ref_c)
    print(f"{m} points: f16x3 fused vs exact-fp32 fused: normals {en:.3e} colours {ec:.3e}")
    assert en < TIGHT and ec < TIGHT


def test_status_word_in_family_is_clear(model):
    pts, dirs = _inputs(257)
    vf = model.vector_field_network
    assert _status_of(lambda: _fused(model, pts, dirs)) == 0
    assert _status_of(lambda: lib.vf_mlp16_fwd(vf.geometry(), vf.packed16_weights(), pts)) == 0


def test_status_word_gain8_gamma30_sets_bit0():
    """Hidden gain 2 -> 8 with BatchNorm gamma spread over 1..30 (the recipe of test_range_guard_* in tests/test_hip_f16x3.py)."""
    model = _fresh()
    with torch.no_grad():
        for net in (model.vector_field_network, model.rendering_network):
            for i in range(net.num_layers - 1):
                net._linear(i).weight.mul_(4.0)
                bn = net._bn(i)
                bn.weight.copy_(torch.linspace(1.0, 30.0, bn.weight.numel(), device=bn.weight.device))
    pts, dirs = _inputs(257)
    assert _status_of(lambda: _fused(model, pts, dirs)) == lib.STATUS_ACT_SATURATED


def test_status_word_far_points_set_bit1(model):
    pts, dirs = _inputs(257)
    far = (torch.nn.functional.normalize(pts, dim=1) * 2000.0).contiguous()          # |p| = 2000: beyond the f16 range once scaled by 2^6
    st = _status_of(lambda: _fused(model, far, dirs))
    assert st & lib.STATUS_INPUT_SATURATED


def _hidden(model, pts, dirs):
    """Post-ReLU activations of the 8 VF and 4 rendering layers for these inputs, from the CPU oracle."""
    vf_sd = {k: v.detach().cpu() for k, v in model.vector_field_network.state_dict().items()}
    rn_sd = {k: v.detach().cpu() for k, v in model.rendering_network.state_dict().items()}
    h_vf, h_rn = [], []
    y = O.vf_mlp(pts.cpu(), vf_sd, 6, (4,), hidden=h_vf)
    O.render_mlp(pts.cpu(), y[:, :3], dirs.cpu(), y[:, 3:], rn_sd, 4, hidden=h_rn)
    return {"vf": h_vf, "rn": h_rn}


# (net, layer, output row): the tile that holds the row is the only one that saturates
ONE_TILE = [("vf", 2, 0),        # a layer's first tile (its look rides in the same layer's second tile)
            ("vf", 2, 255),      # a layer's last tile: its look rides in the NEXT layer's first tile
            ("vf", 0, 255),      # the last tile of the encoding-only layer (three K steps)
            ("vf", 3, 216),      # the last tile of the 217-wide layer in front of the skip layer (seven tiles, another hand-over block)
            ("vf", 7, 255),      # the input tile of the VF heads (vector-only launch: the head's tile; fused: the feature layer's first)
            ("rn", 0, 255),      # the last tile of the rendering net's first layer
            ("rn", 3, 255)]      # the input tile of the colour head


@pytest.mark.parametrize("net_name,layer,row", ONE_TILE, ids=[f"{n}{l}_row{r}" for n, l, r in ONE_TILE])
def test_status_word_one_saturating_tile_sets_bit0(net_name, layer, row):
    """Only ONE tile of the whole launch holds a value at the clamp: output row ``row`` of that layer's Linear is scaled until its largest
    activation is ~2000 (the clamp acts at 937.5), and the next layer's column for it is zeroed, so nothing downstream moves.  The CPU
    oracle confirms the construction (every other hidden activation stays below 900); the launch must report bit 0 and nothing else."""
    model = _fresh()
    pts, dirs = _inputs(257)
    net = model.vector_field_network if net_name == "vf" else model.rendering_network
    before = _hidden(model, pts, dirs)[net_name][layer][:, row]
    assert float(before.max()) > 0.0, "the chosen row is dead for these inputs: choose another"
    with torch.no_grad():
        k = 2000.0 / float(before.max())
        net._linear(layer).weight[row].mul_(k)
        net._linear(layer).bias[row].mul_(k)
        bn = net._bn(layer)
        if bn is not None:          # eval-mode BatchNorm is affine: keep its shift in proportion, so the row as a whole scales by k
            bn.running_mean[row].mul_(k)
            bn.bias[row].mul_(k)
        if layer + 1 < net.num_layers - 1:          # (a head reads the saturated value; there is no ReLU tile behind a head)
            net._linear(layer + 1).weight[:, row].zero_()
    hid = _hidden(model, pts, dirs)
    peak = float(hid[net_name][layer][:, row].max())
    assert 1500.0 < peak < 2500.0, peak
    for name, acts in hid.items():
        for i, h in enumerate(acts):
            h = h.clone()
            if name == net_name and i == layer:
                h[:, row] = 0.0
            assert float(h.max()) < 900.0 < ACT_LIMIT, (name, i, float(h.max()))
    vf = model.vector_field_network
    assert _status_of(lambda: _fused(model, pts, dirs)) == lib.STATUS_ACT_SATURATED
    if net_name == "vf":
        assert _status_of(lambda: lib.vf_mlp16_fwd(vf.geometry(), vf.packed16_weights(), pts)) == lib.STATUS_ACT_SATURATED
        vecs = torch.empty(257, 3, device=DEV)
        blocks = torch.empty(lib.block_rows(257), lib.BLOCK_BYTES, dtype=torch.uint8, device=DEV)
        assert _status_of(lambda: lib.vf_feat16_fwd(vf.geometry(), vf.packed16_weights(), pts, vecs, blocks)) == lib.STATUS_ACT_SATURATED


def test_training_step_forward_equals_the_launch_by_launch_step():
    """One vfn_train_step (the step session: training modes of the same kernel template) at 8 rays x (4 + 4) samples against the
    launch-by-launch step: rgb, depth and the compositing weights bit-identical, as tests/test_hip_session.py checks at its size."""
    from vf_nerf_amd import backward, stepengine
    fx, d = load_fixture("w1_det")
    fx = dict(fx, n_samples=4, n_importance=4)
    n = 8
    gen = torch.Generator().manual_seed(21)
    uni = {"u_fine": torch.rand(n, 4, generator=gen).to(DEV), "u_add": torch.rand(n, 4, generator=gen).to(DEV)}
    got = {}
    for sessions in (True, False):
        model = build_model(fx, d, device=DEV)
        model.step_sessions = sessions
        seen = {}
        real = backward.StoredFinePass.finish

        def finish(self, *a, _real=real, _seen=seen, **kw):
            out = _real(self, *a, **kw)
            _seen["weights"] = out[4].detach().clone()
            return out

        backward.StoredFinePass.finish = finish
        try:
            model.optimizer.zero_grad()
            out = model.render(d["pose"][:n].to(DEV) if d["pose"].dim() == 3 else d["pose"].to(DEV), d["uv"][:n].to(DEV).contiguous(),
                               d["intrinsics"][:n].to(DEV) if d["intrinsics"].dim() == 3 else d["intrinsics"].to(DEV), epoch=0, uniforms=uni)
        finally:
            backward.StoredFinePass.finish = real
        eng = stepengine.StepEngine.of(model)
        assert (eng.session is not None and eng.why_not is None) == sessions, eng.why_not
        weights = eng.session.weights.detach().clone().view(n, 8) if sessions else seen["weights"].view(n, 8)
        got[sessions] = (out.coarse_rgb_values.detach().clone(), out.coarse_depth_map.detach().clone(), weights,
                         out.coarse_normals.detach().clone(), out.z_vals.detach().clone())
        (out.coarse_rgb_values.sum() + out.coarse_depth_map.sum()).backward()          # closes the step
    for name, a, b in zip(("rgb", "depth", "weights", "normals", "z_vals"), got[True], got[False]):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
