"""A CPU restatement of contrastive marching cubes (evaluation/utils/marching_cubes_vt.py:186-315 with combs_to_verts :62-101 and
vertex_interpolate :9-16), written from the contract csrc/vfn_mesh.hip documents, in plain Python floats (IEEE double, no
contraction).  tests/golden/mesh_stages.npz pins it to the reference's own results; the GPU tests then compare the device against it
where the fixture has no recorded answer.  Not part of the package: tests only."""
from __future__ import annotations

import numpy as np

INC = ((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1), (1, 0, 1))
PAIRS = tuple((a, b) for a in range(8) for b in range(a + 1, 8))
PAIR_INDEX = {p: i for i, p in enumerate(PAIRS)}


def corner_values(comb, udf):
    """combs_to_verts for one cell: comb[28] (numpy row, compared in its own dtype), udf[28,2] or None -> (8 floats, from_udf)."""
    if np.isnan(comb).any() or not comb.max() > 0.5:
        return [0.0] * 8, False
    a0, a1 = PAIRS[int(np.argmax(comb))]
    cls1 = {a1}
    for v in range(8):
        if v in (a0, a1):
            continue
        if comb[PAIR_INDEX[(min(v, a0), max(v, a0))]] > comb[PAIR_INDEX[(min(v, a1), max(v, a1))]]:
            cls1.add(v)
    if udf is None:
        return [1.0 if v in cls1 else 0.0 for v in range(8)], True
    mags = [float(udf[0, 0])] + [float(udf[v - 1, 1]) for v in range(1, 8)]
    return [(1.0 if v in cls1 else -1.0) * mags[v] for v in range(8)], True


def fused_values(bits, corner_norms):
    """The same for a make_comb_format cell (XOR comb, pair norms): side bits -> values, or None when the comb row is all zero."""
    if bits in (0, 255):
        return None
    b0 = bits & 1
    return [(1.0 if ((bits >> v) & 1) != b0 else -1.0) * float(corner_norms[v]) for v in range(8)]


def cell_triangles(c, values, res, size, iso, tri_table, edge_vertex):
    """-> the cell's triangles as lists of three (x, y, z) float tuples (table order), [] if no edge is cut."""
    top = sum(1 << q for q in range(8) if values[q] < iso)
    if top in (0, 255):
        return []
    pos = [tuple((c[d] + INC[q][d]) / res * size - size / 2 for d in range(3)) for q in range(8)]
    out = []
    row = [int(e) for e in tri_table[top]]
    for t in range(5):
        if row[3 * t] < 0:
            break
        tri = []
        for e in row[3 * t:3 * t + 3]:
            e1, e2 = int(edge_vertex[e][0]), int(edge_vertex[e][1])
            if any(pos[e1][d] > pos[e2][d] for d in range(3)):
                e1, e2 = e2, e1
            v1, v2 = values[e1], values[e2]
            if abs(v1 - v2) > 1e-5:
                tri.append(tuple(pos[e1][d] + (pos[e2][d] - pos[e1][d]) * (iso - v1) / (v2 - v1) for d in range(3)))
            else:
                tri.append(pos[e1])
        out.append(tri)
    return out


def _collect(cell_iter, res, size, iso, tables):
    tri_table, edge_vertex = tables
    ids, verts, faces = {}, [], []
    for c, values in cell_iter:
        for tri in cell_triangles(c, values, res, size, iso, tri_table, edge_vertex):
            f = []
            for v in tri:
                if v not in ids:                # float equality: 0.0 == -0.0, the first occurrence's bits stay
                    ids[v] = len(verts)
                    verts.append(v)
                f.append(ids[v])
            faces.append(f)
    return np.array(verts, dtype=np.float64).reshape(-1, 3), np.array(faces, dtype=np.int64).reshape(-1, 3)


def triangulate_general(comb, udf, cells, res, size, iso, tables):
    """comb [M,28], udf [M,28,2] | None, cells [M,3] | None (dense raster) -> (vertices [V,3], faces [F,3] 0-based)."""
    comb = np.asarray(comb).reshape(-1, 28)
    udf = None if udf is None else np.asarray(udf).reshape(-1, 28, 2)
    if cells is None:
        cells = np.moveaxis(np.mgrid[:res, :res, :res], 0, -1).reshape(-1, 3)

    def it():
        for p in range(comb.shape[0]):
            yield [int(x) for x in cells[p]], corner_values(comb[p], None if udf is None else udf[p])[0]
    return _collect(it(), res, size, iso, tables)


def block_order(res):
    """The cell positions of evaluation/methods.py:184-188: (res/2)^3 blocks in raster order, corner order inside a block."""
    sel = np.moveaxis(np.mgrid[: res // 2, : res // 2, : res // 2], 0, -1).reshape(-1, 3)
    return (sel[:, None] * 2 + np.array(INC)[None]).reshape(-1, 3)


def triangulate_fused(sides, norms, res, tables, iso=0.0, size=2.0):
    """side bytes [res^3] + norms [res^3] -> (vertices, faces): the glue of evaluation/methods.py:248-290 on make_comb_format's tables."""
    sides = np.asarray(sides).reshape(res, res, res)
    npad = np.zeros((res + 1, res + 1, res + 1), dtype=np.float32)
    npad[:res, :res, :res] = np.asarray(norms, dtype=np.float32).reshape(res, res, res)

    def it():
        for c in block_order(res):
            i, j, k = (int(x) for x in c)
            vals = fused_values(int(sides[i, j, k]), [npad[i + a, j + b, k + d] for a, b, d in INC])
            if vals is not None:
                yield (i, j, k), vals
    return _collect(it(), res, size, iso, tables)


def comb_udf_from_sides(sides, norms, res, cells):
    """make_comb_format's rows (XOR comb, pair norms; norm 0 outside the grid) for the given cells -> comb [M,28], udf [M,28,2] fp32."""
    sides = np.asarray(sides).reshape(-1)
    npad = np.zeros((res + 1, res + 1, res + 1), dtype=np.float32)
    npad[:res, :res, :res] = np.asarray(norms, dtype=np.float32).reshape(res, res, res)
    cells = np.asarray(cells)
    bits = sides[(cells[:, 0] * res + cells[:, 1]) * res + cells[:, 2]].astype(np.int64)
    b = (bits[:, None] >> np.arange(8)[None]) & 1
    corner = np.stack([npad[cells[:, 0] + a, cells[:, 1] + bb, cells[:, 2] + d] for a, bb, d in INC], axis=1)
    comb = np.stack([(b[:, a] != b[:, q]) for a, q in PAIRS], axis=1).astype(np.float32)
    udf = np.stack([np.stack([corner[:, a], corner[:, q]], axis=1) for a, q in PAIRS], axis=1).astype(np.float32)
    return comb, udf
