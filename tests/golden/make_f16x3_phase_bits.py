#!/usr/bin/env python3
"""Records what the f16x3 inference launches return, bit for bit, into tests/golden/f16x3_phase_bits.npz.

    VFN_LIB=<libvfn.so of the commit to record> python tests/golden/make_f16x3_phase_bits.py        (needs the GPU)

The file was recorded from the commit BEFORE the fused kernel's prologue, encoding boundary and tail were trimmed (compile-time
encoding geometry, lane-half swap, range bookkeeping on the raw columns only, one scalar pair for the saturation mask):
tests/test_hip_f16x3_phases.py holds every later library to those bits — outputs and status words.  The test runs `record()` below
on the inputs stored in the file, so the cases are defined once, here.

Networks: the fixture c1_perturb through helpers.build_model; the other encoding geometries (rendering net with 3 and 0 octaves, a
vector-field net with 5 where the f16x3 plan admits it) are fresh nets of the same configuration, seeded, with the fixture's gain.
"""
import dataclasses
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                      # tests/: helpers
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository: vf_nerf_amd

OUT = os.path.join(HERE, "f16x3_phase_bits.npz")
FIXTURE = "c1_perturb"
COUNTS = (1, 31, 33, 129, 299)      # points per launch: one lane, a partial wave, two waves, two workgroups, 9 groups of 32 + 11
S = 23                              # samples per ray: a wave of 32 points spans rays, the last ray is partial
OTHER_M = 129                       # points of the launches with another encoding geometry
GUARD_M = 299                       # points of the range-guard situations (the fixture's first samples)


def _base(device):
    from helpers import build_model, load_fixture
    fx, d = load_fixture(FIXTURE)
    return fx, d, build_model(fx, d, device=device)


def _fresh_net(model, fx, kind: str, multires: int, device):
    """A net of the model's configuration with another octave count: seeded default init, hidden weights x the fixture's gain."""
    from vf_nerf_amd.networks import RenderingNetwork, VectorFieldNetwork
    torch.manual_seed(7000 + 10 * multires + (kind == "vf"))
    if kind == "rn":
        net = RenderingNetwork(dataclasses.replace(model.config.rendering_net_config, embedder_multires=multires))
    else:
        net = VectorFieldNetwork(dataclasses.replace(model.config.vf_net_config, embedder_multires=multires))
    with torch.no_grad():
        for i in range(net.num_layers - 1):
            net._linear(i).weight.mul_(float(fx.get("gain", 1.0)))
    return net.eval().to(device)


def other_geometries(model, fx, device):
    """tag -> (vf, rn): the launches these go through take the run-time form of the encoding."""
    vf, rn = model.vector_field_network, model.rendering_network
    nets = {"rn3": (vf, _fresh_net(model, fx, "rn", 3, device)), "rn0": (vf, _fresh_net(model, fx, "rn", 0, device))}
    vf5 = _fresh_net(model, fx, "vf", 5, device)
    if vf5.supports_f16x3():
        nets["vf5"] = (vf5, rn)
    return nets


def make_inputs(d):
    """The inputs of every case as CPU tensors (stored in the file; the test reads them back)."""
    gen = torch.Generator().manual_seed(20)
    inp = {}
    for m in COUNTS + (OTHER_M,):
        if f"pts_{m}" in inp:
            continue
        inp[f"pts_{m}"] = torch.rand(m, 3, generator=gen) * 2 - 1
        inp[f"dirs_{m}"] = torch.nn.functional.normalize(torch.randn((m + S - 1) // S, 3, generator=gen), dim=1)
    m = COUNTS[-1]
    perm = torch.cat([r * S + torch.randperm(S, generator=gen) for r in range(m // S)]).to(torch.int32)     # 299 = 13 rays x 23
    inp["perm"] = perm
    idx = perm.clone()
    idx[::7] = -1
    inp["scatter_index"] = idx
    inp["guard_pts"] = d["points"].reshape(-1, 3)[:GUARD_M].contiguous().clone()
    inp["guard_dirs"] = d["ray_dirs"].contiguous().clone()
    inp["guard_s"] = torch.tensor([d["points"].shape[-2]], dtype=torch.int32)
    return inp


class _Status:
    """The status word of the f16x3 launches made inside the block."""
    def __init__(self, device):
        self.word = torch.zeros(1, dtype=torch.int32, device=device)

    def __enter__(self):
        from vf_nerf_amd import lib
        lib.f16x3_set_status(self.word)
        return self

    def __exit__(self, *exc):
        from vf_nerf_amd import lib
        lib.f16x3_set_status(None)

    def value(self):
        return torch.tensor([int(self.word.cpu()[0])], dtype=torch.int32)


def record(inp, device="cuda:0"):
    """Every case on the library in use -> {name: CPU tensor}; float outputs as they are, status words as int32[1]."""
    from vf_nerf_amd import lib
    fx, d, model = _base(device)
    vf, rn = model.vector_field_network, model.rendering_network
    dev = torch.device(device)
    g = {k: v.to(dev) for k, v in inp.items()}
    out = {}

    def fused(tag, vfn, rnn, pts, dirs, s):
        with _Status(dev) as st:
            n, c = lib.vf_render_fused16_fwd(vfn.geometry(), vfn.packed16_weights(), rnn.geometry(), rnn.packed16_weights(), pts, dirs, s)
            torch.cuda.synchronize()
        out[f"{tag}_normals"], out[f"{tag}_colors"], out[f"{tag}_status"] = n.cpu(), c.cpu(), st.value()

    def vector(tag, vfn, pts):
        with _Status(dev) as st:
            v = lib.vf_mlp16_fwd(vfn.geometry(), vfn.packed16_weights(), pts)
            torch.cuda.synchronize()
        out[f"{tag}_vec"], out[f"{tag}_status"] = v.cpu(), st.value()

    for m in COUNTS:
        fused(f"fused_{m}", vf, rn, g[f"pts_{m}"], g[f"dirs_{m}"], S)
        vector(f"vector_{m}", vf, g[f"pts_{m}"])
    # the scatter launch: stored (permuted) samples, one direction per sample, rows with index -1 are dropped
    m = COUNTS[-1]
    pts, dirs, perm = g[f"pts_{m}"], g[f"dirs_{m}"], g["perm"].long()
    stored = pts[perm].contiguous()
    out_n, out_c = torch.full((m, 3), 7.0, device=dev), torch.full((m, 3), 7.0, device=dev)
    with _Status(dev) as st:
        lib.vf_render_fused16_scatter(vf.geometry(), vf.packed16_weights(), rn.geometry(), rn.packed16_weights(), stored,
                                      dirs[perm // S].contiguous(), 1, g["scatter_index"], out_n, out_c)
        torch.cuda.synchronize()
    out["scatter_normals"], out["scatter_colors"], out["scatter_status"] = out_n.cpu(), out_c.cpu(), st.value()
    # the block pair: VF net with feature blocks out, rendering net over the stored rows
    vecs = torch.empty(m, 3, device=dev)
    blocks = torch.zeros(lib.block_rows(m), lib.BLOCK_BYTES, dtype=torch.uint8, device=dev)
    with _Status(dev) as st:
        lib.vf_feat16_fwd(vf.geometry(), vf.packed16_weights(), stored, vecs, blocks)
        bn, bc = lib.render16_from_blocks(rn.geometry(), rn.packed16_weights(), blocks, vecs, g["perm"], pts, dirs, S)
        torch.cuda.synchronize()
    out["blocks_vecs"], out["blocks_normals"], out["blocks_colors"], out["blocks_status"] = vecs.cpu(), bn.cpu(), bc.cpu(), st.value()
    # other encoding geometries
    for tag, (vfn, rnn) in other_geometries(model, fx, dev).items():
        fused(f"{tag}_fused", vfn, rnn, g[f"pts_{OTHER_M}"], g[f"dirs_{OTHER_M}"], S)
    # the range guard's three situations (tests/test_hip_f16x3.py, _out_of_family)
    s_guard = int(inp["guard_s"][0])
    for case in ("in_family", "gain8_gamma30", "points_2000"):
        _, _, mdl = _base(device)
        pts = g["guard_pts"]
        with torch.no_grad():
            if case == "gain8_gamma30":
                for net in (mdl.vector_field_network, mdl.rendering_network):
                    for i in range(net.num_layers - 1):
                        net._linear(i).weight.mul_(4.0)
                        bn_ = net._bn(i)
                        bn_.weight.copy_(torch.linspace(1.0, 30.0, bn_.weight.numel(), device=bn_.weight.device))
            elif case == "points_2000":
                pts = (pts * 2000.0).contiguous()
        vector(f"guard_{case}_vector", mdl.vector_field_network, pts)
        fused(f"guard_{case}_fused", mdl.vector_field_network, mdl.rendering_network, pts, g["guard_dirs"], s_guard)
    return out


def main():
    from helpers import load_fixture
    from vf_nerf_amd import lib
    _, d = load_fixture(FIXTURE)
    inp = make_inputs(d)
    out = record(inp)
    arrays = {f"in.{k}": v.numpy() for k, v in inp.items()}
    arrays.update({f"out.{k}": v.numpy() for k, v in out.items()})
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {len(arrays)} arrays, {os.path.getsize(OUT)} bytes, library {lib.LIB_PATH}")
    for k, v in out.items():
        if k.endswith("_status"):
            print(f"  {k} = {int(v[0])}")


if __name__ == "__main__":
    main()
