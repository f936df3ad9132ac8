#!/usr/bin/env python3
"""Golden vectors for the mesh triangulation (evaluation/utils/marching_cubes_vt.py:186-315, contrastive_marching_cubes) by running
the REFERENCE's own functions: mc_utils (divergence, unify_direction, make_comb_format), smooth_vf and contrastive_marching_cubes,
with the glue of evaluation/methods.py:168-291 restated here.  Build container only (needs /root/reference, read-only); the fixture
holds inputs, the recorded case tables and expected outputs, nothing of the reference's source.

The reference cannot run next to the numpy this project ships with as it stands: ``np.int`` (marching_cubes_vt.py:216,280) is gone
since NumPy 1.24, and the module imports numba for a function the triangulation does not call.  For the run, ``np.int = int`` and
``numba.jit`` is the identity.

    python tests/golden/make_mesh_golden.py            # writes tests/golden/mesh_stages.npz
    python tests/golden/make_mesh_golden.py --time     # also times the reference's loop (reported, not recorded)
"""
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
np.int = int                                   # noqa: the reference's marching_cubes_vt.py:216,280
_numba = types.ModuleType("numba")
_numba.jit = lambda *a, **k: (lambda f: f)
sys.modules.setdefault("numba", _numba)
from evaluation.utils import marching_cubes_lookup as lookup  # noqa: E402
from evaluation.utils import marching_cubes_vt, mc_utils  # noqa: E402
from evaluation.utils.guassian_smoothing import smooth_vf  # noqa: E402

INC = np.array([[0, 0, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0], [0, 0, 1], [0, 1, 1], [1, 1, 1], [1, 0, 1]])


def field(n, seed, zeros=0):
    """Converges onto a sphere (radius 0.45, off-centre) plus noise, quantised to 1/64 (the fixture compresses); ``zeros`` random
    vectors set to exactly 0 (norm 0, F.normalize -> 0)."""
    g = torch.Generator().manual_seed(seed)
    ax = torch.linspace(-1, 1, n)
    p = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3)
    d = p - torch.tensor([0.1, -0.05, 0.08])
    r = d.norm(dim=1, keepdim=True)
    v = -torch.sign(r - 0.45) * d / r.clamp_min(1e-6) * (0.3 + (r - 0.45).abs()) + 0.04 * torch.randn(n ** 3, 3, generator=g)
    v = torch.round(v * 64) / 64
    if zeros:
        v[torch.randperm(n ** 3, generator=g)[:zeros]] = 0
    return v.float()


def methods_glue(pred, res, smooth_after=False, smooth_all=False):
    """evaluation/methods.py:184-188 and :212-291, restated (the reference function also queries a model and writes files)."""
    sel = np.moveaxis(np.mgrid[: int(res / 2), : int(res / 2), : int(res / 2)], 0, -1).reshape(-1, 3)
    sel = (sel[:, None] * 2 + INC[None]).reshape(-1, 3)
    if smooth_all:
        pred = smooth_vf(pred.reshape(res, res, res, 3), k=3, sigma=1).reshape(res ** 3, 3)
    div = mc_utils.extract_divergence(pred, res)
    if smooth_after or smooth_all:
        pred = smooth_vf(pred.reshape(res, res, res, 3), k=9, sigma=2).reshape(res ** 3, 3)
    norms = torch.norm(pred.clone(), dim=1)
    vt = F.normalize(pred, dim=1).reshape(res, res, res, 3)
    choice = mc_utils.unify_direction(div, vt.permute(3, 0, 1, 2), N=res)
    comb, pn = mc_utils.make_comb_format(choice, norms, res)
    comb = comb.reshape(res, res, res, 28)[sel[:, 0], sel[:, 1], sel[:, 2]].reshape(res, res, res, 28)
    pn = pn.reshape(res, res, res, 28, 2)[sel[:, 0], sel[:, 1], sel[:, 2]]
    udf = pn.clone().cpu().numpy()
    comb = comb.clone().cpu().numpy().reshape(-1, 28)
    mask = comb.sum(-1)
    sel_m = sel[mask > 0]
    udf = udf[mask > 0].reshape(-1, 2)
    comb_m = comb[mask > 0].reshape(-1)
    vs, fs = marching_cubes_vt.contrastive_marching_cubes(comb_m, isovalue=0.0, selected_indices=sel_m, res=res, udf=udf)
    sides = (choice.numpy().astype(np.uint8) << np.arange(8, dtype=np.uint8)).sum(1).astype(np.uint8)
    return dict(div=div.numpy(), norms=norms.numpy(), sides=sides, cells=sel_m.astype(np.int64), comb=comb_m.reshape(-1, 28).astype(np.float32),
                udf=udf.reshape(-1, 28, 2).astype(np.float32)), vs, fs


def pack(vs, fs):
    v = np.array(list(vs.keys()), dtype=np.float64).reshape(-1, 3)
    ids = np.array(list(vs.values()), dtype=np.int64)
    assert np.array_equal(ids, np.arange(1, len(ids) + 1))          # dict ids are 1..V in insertion order
    return v, np.array(fs, dtype=np.int64).reshape(-1, 3)


def general_cases(rng):
    """comb [M,28] / udf [M,28,2] / cells [M,3] inputs for the general form, each with (res, size, isovalue)."""
    cases = {}
    m, res = 120, 10

    def q(a):                                   # values on a 1/256 grid: the fixture compresses
        return (np.round(a * 256) / 256).astype(np.float32)
    cells = rng.integers(0, res, size=(m, 3))
    cases["random"] = (q(rng.random((m, 28))), q(rng.random((m, 28, 2)) * 2 - 0.5), cells, res, 2.0, 0.0)
    ties = rng.choice(np.array([0.0, 0.5, 0.75, 1.0], dtype=np.float32), size=(m, 28), p=[0.4, 0.2, 0.2, 0.2])
    cases["ties"] = (ties, q(rng.random((m, 28, 2))), cells, res, 2.0, 0.0)
    cases["nonxor"] = (rng.integers(0, 2, size=(m, 28)).astype(np.float32), q(rng.random((m, 28, 2))), cells, res, 2.0, 0.1)
    # |v1 - v2| <= 1e-5 on cut edges and exact zero norms: the edge vertices snap to corners, several edges share one
    snap_udf = rng.choice(np.array([0.0, 0.0, 3e-6, 8e-6, 0.5], dtype=np.float32), size=(m, 28, 2))
    cases["snap"] = (rng.integers(0, 2, size=(m, 28)).astype(np.float32), snap_udf, cells, res, 2.0, 0.0)
    cases["size3"] = (q(rng.random((m, 28))), q(rng.random((m, 28, 2))), rng.integers(0, 7, size=(m, 3)), 7, 3.0, 0.0)
    return cases


def main():
    timing = "--time" in sys.argv
    rng = np.random.default_rng(20261016)
    out = {"tables.edge": np.array(lookup.EDGE_TABLE, dtype=np.int32), "tables.edge_vertex": np.array(lookup.EDGE_VERTEX, dtype=np.int32),
           "tables.tri": np.array(lookup.TRI_TABLE, dtype=np.int8)}
    fields = []
    for res, seed, zeros, variants in ((16, 3, 0, ((False, False), (True, False), (False, True))), (24, 4, 0, ((False, False),)),
                                       (32, 5, 0, ((False, False),))):
        pred = field(res, seed, zeros)
        out[f"f{res}.pred"] = pred.numpy()
        for after, all_ in variants:
            tag = f"f{res}" + (".after" if after else ".all" if all_ else "")
            t0 = time.perf_counter()
            st, vs, fs = methods_glue(pred, res, after, all_)
            v, f = pack(vs, fs)
            for k, a in st.items():
                if (k in ("comb", "udf") and tag != "f16") or (k == "norms" and res != 16):
                    continue                    # (rebuilt by the tests: udf from norms + sides, norms = torch.norm of the field; keeps the file small)
                out[f"{tag}.{k}"] = a
            out[f"{tag}.vs"], out[f"{tag}.fs"] = v, f
            fields.append(tag)
            print(f"{tag}: {len(st['cells'])} cells, {len(f)} faces, {len(v)} vertices ({time.perf_counter() - t0:.1f} s)")
    gen = []
    for name, (comb, udf, cells, res, size, iso) in general_cases(rng).items():
        vs, fs = marching_cubes_vt.contrastive_marching_cubes(comb.reshape(-1), isovalue=iso, res=res, size=size, udf=udf.reshape(-1, 2),
                                                              selected_indices=cells)
        v, f = pack(vs, fs)
        out.update({f"g.{name}.comb": comb, f"g.{name}.udf": udf, f"g.{name}.cells": cells.astype(np.int64), f"g.{name}.vs": v,
                    f"g.{name}.fs": f, f"g.{name}.args": np.array([res, size, iso], dtype=np.float64)})
        gen.append(name)
        print(f"general {name}: {len(f)} faces, {len(v)} vertices")
    # the dense branch (selected_indices=None), with udf and without it (corner values 0 / 1, so an isovalue inside (0, 1))
    res = 4
    bits = rng.integers(0, 2, size=(res ** 3, 8))
    comb = np.stack([(bits[:, a] != bits[:, b]) for a in range(8) for b in range(a + 1, 8)], axis=1).astype(np.float32)
    udf = (np.round(rng.random((res ** 3, 28, 2)) * 256) / 256).astype(np.float32)
    for name, u, iso in (("dense", udf, 0.0), ("dense_noudf", None, 0.5)):
        vs, fs = marching_cubes_vt.contrastive_marching_cubes(comb.reshape(-1), isovalue=iso, res=res, size=2.0, udf=u)
        v, f = pack(vs, fs)
        out.update({f"d.{name}.comb": comb, f"d.{name}.vs": v, f"d.{name}.fs": f, f"d.{name}.args": np.array([res, 2.0, iso])})
        if u is not None:
            out[f"d.{name}.udf"] = u
        gen.append(name)
        print(f"dense {name}: {len(f)} faces, {len(v)} vertices")
    out["index.fields"] = np.array(fields)
    out["index.general"] = np.array([g for g in gen if not g.startswith("dense")])
    out["index.dense"] = np.array([g for g in gen if g.startswith("dense")])
    path = os.path.join(HERE, "mesh_stages.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")
    if timing:
        # the reference's loop alone, at the sizes it finishes in on the build machine (reported in profiles/, not recorded here)
        for res in (32, 64, 128):
            st, _, _ = methods_glue(field(res, 7), res)
            t0 = time.perf_counter()
            vs, fs = marching_cubes_vt.contrastive_marching_cubes(st["comb"].reshape(-1), isovalue=0.0, selected_indices=st["cells"], res=res,
                                                                  udf=st["udf"].reshape(-1, 2))
            dt = time.perf_counter() - t0
            print(f"TIMING res {res}: {len(st['cells'])} cells, {len(fs)} faces, {len(vs)} vertices: contrastive_marching_cubes {dt:.3f} s "
                  f"({len(st['cells']) / dt:.0f} cells/s)")


if __name__ == "__main__":
    main()
