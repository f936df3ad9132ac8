#!/usr/bin/env python3
"""Records what the f16x3 launch modes that tests/golden/f16x3_phase_bits.npz does not hold return, bit for bit, into
tests/golden/f16x3_schedule_bits.npz.

    VFN_LIB=<libvfn.so of the commit to record> python tests/golden/make_f16x3_schedule_bits.py        (needs the GPU)

The file was recorded from the commit BEFORE the steady-state issue stream of the chunk loop (csrc/vfn_mlp16.hip, layer16) was
looked at gap by gap: a change of how the same instructions are scheduled, of the register fragment ring or of the ring hand-over
must return these bits — outputs, workspaces and status words.  tests/test_hip_f16x3_schedule.py runs `record()` below on the
library under test, so the cases are defined once, here.

Launch modes: the fused launch with two colour products (and, at the largest size, with three: the headline's launch); the saving
forwards vfn_vf_mlp16_fwd_train ([vector | features]) and vfn_vf_render_fused16_fwd_train with a row-major fp32 workspace and with
the default one (f16 values in fragment order); the single-product training forwards (vector columns only, and fused); the
feature-block pair vfn_vf_feat16_fwd -> vfn_render16_from_blocks.

Sizes: 1 point (one lane), 127 (a partial last wave), 128 (exactly one workgroup), 129 (a second workgroup with one valid point),
128 x 257 + 5 (more workgroups than the chip has CUs: staggered starts, every ring slot reused under contention).

Network: the shipped geometry, default initialisation under a fixed seed, hidden weights x 2 (synthetic.scale_hidden_weights);
points uniform in the frustum box, one unit direction per ray of S = 23 samples.  Nothing here depends on the library under test.

What is stored: [M, 3] outputs whole up to 389 rows, otherwise rows 0 .. 255 and the last 133 plus a 64-bit checksum of the rest;
workspaces (every slot, the sign words, the encoding rows; zero-filled before the launch) as 64-bit checksums; status words.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))     # the repository: vf_nerf_amd

OUT = os.path.join(HERE, "f16x3_schedule_bits.npz")
COUNTS = (1, 127, 128, 129, 128 * 257 + 5)
S = 23                              # samples per ray: a wave of 32 points spans rays, the last ray is partial
HEAD_ROWS, TAIL_ROWS = 256, 133     # what of a large [M, 3] output is stored as values
MODEL_SEED, GAIN = 2500, 2.0


def build_model(device):
    """The shipped networks with seeded default weights (the modules are initialised on the CPU, under the CPU generator, and moved)."""
    import vf_nerf_amd
    from vf_nerf_amd import synthetic
    torch.manual_seed(MODEL_SEED)
    model = vf_nerf_amd.VectorFieldNerf(vf_nerf_amd.shipped_config(device, n_samples=64, n_importance=64))
    model.eval()
    with torch.no_grad():
        synthetic.scale_hidden_weights(model.vector_field_network, model.rendering_network, GAIN)
    return model


def make_inputs():
    """The inputs of every case as CPU tensors, from seeds."""
    from vf_nerf_amd import synthetic
    inp = {}
    for m in COUNTS:
        gen = torch.Generator().manual_seed(100 + m)
        inp[f"pts_{m}"] = synthetic.frustum_points(m, seed=200 + m)
        inp[f"dirs_{m}"] = torch.nn.functional.normalize(torch.randn((m + S - 1) // S, 3, generator=gen), dim=1)
        inp[f"perm_{m}"] = torch.randperm(m, generator=gen).to(torch.int32)
    return inp


def checksum64(t: torch.Tensor) -> torch.Tensor:
    """Position-weighted sum of the tensor's bytes taken as int64 words, modulo 2^64 -> int64[1] on the CPU."""
    b = t.contiguous().reshape(-1).view(torch.uint8)
    if b.numel() % 8:
        b = torch.cat([b, b.new_zeros(8 - b.numel() % 8)])
    v = b.view(torch.int64)
    w = torch.arange(v.numel(), dtype=torch.int64, device=v.device) * 2 + 1
    return (v * w).sum().reshape(1).cpu()


def rows(out: dict, name: str, t: torch.Tensor) -> None:
    """An [M, 3] output: whole, or its first HEAD_ROWS and last TAIL_ROWS rows and the checksum of the rows between."""
    if t.shape[0] <= HEAD_ROWS + TAIL_ROWS:
        out[name] = t.cpu()
    else:
        out[f"{name}_head"], out[f"{name}_tail"] = t[:HEAD_ROWS].cpu(), t[-TAIL_ROWS:].cpu()
        out[f"{name}_sum"] = checksum64(t[HEAD_ROWS:-TAIL_ROWS])


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


def fused3(model, g, m, dev):
    """The three-product fused launch (the headline's) -> (normals, colors, status word)."""
    from vf_nerf_amd import lib
    vf, rn = model.vector_field_network, model.rendering_network
    with _Status(dev) as st:
        n, c = lib.vf_render_fused16_fwd(vf.geometry(), vf.packed16_weights(), rn.geometry(), rn.packed16_weights(), g[f"pts_{m}"],
                                         g[f"dirs_{m}"], S)
        torch.cuda.synchronize()
    return n, c, st.value()


def record(inp, device="cuda:0", counts=COUNTS):
    """Every case on the library in use -> {name: CPU tensor}."""
    from vf_nerf_amd import lib
    from vf_nerf_amd.backward import _Workspace, _entries
    dev = torch.device(device)
    model = build_model(dev)
    vf, rn = model.vector_field_network, model.rendering_network
    vfg, vfw, rng, rnw = vf.geometry(), vf.packed16_weights(), rn.geometry(), rn.packed16_weights()
    vf_h, rn_h = len(_entries(vf)), len(_entries(rn))
    g = {k: v.to(dev) for k, v in inp.items()}
    out = {}

    def workspace(m, slots, **kw):
        ws = _Workspace(m, slots, dev, **kw)
        for t in (ws.saved, ws.masks, ws.aux_vf, ws.aux_rn):
            t.zero_()
        return ws

    def ws_sums(tag, ws, with_rn):
        out[f"{tag}_saved_sum"], out[f"{tag}_masks_sum"], out[f"{tag}_auxvf_sum"] = checksum64(ws.saved), checksum64(ws.masks), checksum64(ws.aux_vf)
        if with_rn:
            out[f"{tag}_auxrn_sum"] = checksum64(ws.aux_rn)

    storages = {"fp32": dict(), "f16frag": dict(f16=True, frag=True, dy16="f16")}
    for m in counts:
        pts, dirs = g[f"pts_{m}"], g[f"dirs_{m}"]
        # fused, two colour products
        with _Status(dev) as st:
            n, c = lib.vf_render_fused16_fwd(vfg, vfw, rng, rnw, pts, dirs, S, colour_products=2)
            torch.cuda.synchronize()
        rows(out, f"c2_{m}_normals", n); rows(out, f"c2_{m}_colors", c); out[f"c2_{m}_status"] = st.value()
        # the saving forwards, both storages
        for sname, kw in storages.items():
            ws = workspace(m, vf_h, **kw)
            with _Status(dev) as st:
                v = lib.vf_mlp16_fwd_train(vfg, vfw, pts, True, ws.saved, ws.aux_vf, ws.masks, save_f16=ws.fwd_flags())
                torch.cuda.synchronize()
            tag = f"vftrain_{sname}_{m}"
            rows(out, f"{tag}_vec", v); ws_sums(tag, ws, False); out[f"{tag}_status"] = st.value()
            ws = workspace(m, vf_h + rn_h, **kw)
            with _Status(dev) as st:
                n, c = lib.vf_render_fused16_fwd_train(vfg, vfw, rng, rnw, pts, dirs, S, ws.saved, ws.aux_vf, ws.aux_rn, ws.masks,
                                                       save_f16=ws.fwd_flags())
                torch.cuda.synchronize()
            tag = f"fusedtrain_{sname}_{m}"
            rows(out, f"{tag}_normals", n); rows(out, f"{tag}_colors", c); ws_sums(tag, ws, True); out[f"{tag}_status"] = st.value()
        # single-product training forwards (the default storages)
        ws = workspace(m, vf_h, f16=True, frag=True, dy16="f16p1")
        with _Status(dev) as st:
            v = lib.vf_mlp16_fwd_train(vfg, vfw, pts, False, ws.saved, ws.aux_vf, ws.masks, save_f16=ws.fwd_flags())
            torch.cuda.synchronize()
        tag = f"p1vec_{m}"
        rows(out, f"{tag}_vec", v); ws_sums(tag, ws, False); out[f"{tag}_status"] = st.value()
        ws = workspace(m, vf_h + rn_h, f16=True, frag=True, dy16="f16p1")
        with _Status(dev) as st:
            n, c = lib.vf_render_fused16_fwd_train(vfg, vfw, rng, rnw, pts, dirs, S, ws.saved, ws.aux_vf, ws.aux_rn, ws.masks,
                                                   save_f16=ws.fwd_flags(), colour_products=1)
            torch.cuda.synchronize()
        tag = f"p1fused_{m}"
        rows(out, f"{tag}_normals", n); rows(out, f"{tag}_colors", c); ws_sums(tag, ws, True); out[f"{tag}_status"] = st.value()
        # the block pair: VF net with feature blocks out over the permuted rows, rendering net over the stored rows
        perm = g[f"perm_{m}"]
        stored = pts[perm.long()].contiguous()
        vecs = torch.zeros(m, 3, device=dev)
        blocks = torch.zeros(lib.block_rows(m), lib.BLOCK_BYTES, dtype=torch.uint8, device=dev)
        with _Status(dev) as st:
            lib.vf_feat16_fwd(vfg, vfw, stored, vecs, blocks)
            bn, bc = lib.render16_from_blocks(rng, rnw, blocks, vecs, perm, pts, dirs, S)
            torch.cuda.synchronize()
        tag = f"blocks_{m}"
        rows(out, f"{tag}_vecs", vecs); rows(out, f"{tag}_normals", bn); rows(out, f"{tag}_colors", bc)
        out[f"{tag}_blocks_sum"], out[f"{tag}_status"] = checksum64(blocks), st.value()
    m = counts[-1]
    n, c, status = fused3(model, g, m, dev)
    rows(out, f"fused3_{m}_normals", n); rows(out, f"fused3_{m}_colors", c); out[f"fused3_{m}_status"] = status
    return out


def main():
    from vf_nerf_amd import lib
    out = record(make_inputs())
    np.savez_compressed(OUT, **{f"out.{k}": v.numpy() for k, v in out.items()})
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes, library {lib.LIB_PATH}")
    for k, v in out.items():
        if k.endswith("_status"):
            print(f"  {k} = {int(v[0])}")


if __name__ == "__main__":
    main()
