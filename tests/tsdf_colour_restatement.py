"""The colour half of the TSDF unit's contract (include/vfn.h, vfn_tsdf_integrate_rgb / vfn_tsdf_emit_colours / vfn_tsdf_vertex_colours)
restated in NumPy on top of tests/tsdf_restatement.py: the per-view arithmetic once more with the colour's running mean beside the
tsdf's (float32 operation for operation, every intermediate checked to BE float32), its tsdf / weight asserted equal to
``tsdf_restatement.integrate``'s bit for bit; vertex colours in float64, a vertex taking the colour of the slot at which it first
appears.  And analytic colour images for the scenes of tsdf_restatement.  Tests only — the package never imports this module."""
from __future__ import annotations

import numpy as np

import tsdf_restatement as R
from tsdf_restatement import F, INC, f32


def integrate_view_rgb(tsdf, weight, colour, origin, vl, trunc, depth, rgb, k4, e12):
    """One observation into tsdf / weight [nx,ny,nz] and colour [nx,ny,nz,3] (float32, byte units), in place; rgb uint8 [H,W,3]."""
    assert tsdf.dtype == np.float32 and weight.dtype == np.float32 and colour.dtype == np.float32 and depth.dtype == np.float32
    assert rgb.dtype == np.uint8 and rgb.shape == depth.shape + (3,) and colour.shape == tsdf.shape + (3,)
    k4, e12, vl, trunc = np.asarray(k4, dtype=np.float32), np.asarray(e12, dtype=np.float32), F(vl), F(trunc)
    nx, ny, nz = tsdf.shape
    h, w = depth.shape
    x = R.centres(origin[0], nx, vl)[:, None, None]
    y = R.centres(origin[1], ny, vl)[None, :, None]
    z = R.centres(origin[2], nz, vl)[None, None, :]
    fx, fy, cx, cy = (F(v) for v in k4)
    e = [F(v) for v in e12]
    with np.errstate(all="ignore"):
        xc = f32(f32(f32(f32(e[0] * x) + f32(e[1] * y)) + f32(e[2] * z)) + e[3])
        yc = f32(f32(f32(f32(e[4] * x) + f32(e[5] * y)) + f32(e[6] * z)) + e[7])
        zc = f32(f32(f32(f32(e[8] * x) + f32(e[9] * y)) + f32(e[10] * z)) + e[11])
        ok = zc > 0
        u = f32(np.floor(f32(f32(f32(f32(xc * fx) / zc) + cx) + F(0.5))))
        v = f32(np.floor(f32(f32(f32(f32(yc * fy) / zc) + cy) + F(0.5))))
        ok &= (u >= 0) & (u < F(w)) & (v >= 0) & (v < F(h))
        ui, vi = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
        d = f32(depth[vi, ui])
        ok &= d > 0
        a = f32(f32(u - cx) / fx)
        b = f32(f32(v - cy) / fy)
        m = f32(np.sqrt(f32(f32(F(1.0) + f32(a * a)) + f32(b * b))))
        sdf = f32(f32(d - zc) * m)
        ok &= sdf > -trunc
        t = f32(np.minimum(F(1.0), f32(sdf / trunc)))
        new = f32(f32(f32(tsdf * weight) + t) / f32(weight + F(1.0)))
        # colour_c = (colour_c weight + (float)rgb[v, u, c]) / (weight + 1.0f), with the weight BEFORE its increment
        p = f32(rgb[vi, ui].astype(np.float32))                                   # [nx,ny,nz,3]
        new_colour = f32(f32(f32(colour * weight[..., None]) + p) / f32(weight + F(1.0))[..., None])
    # the geometry half is tsdf_restatement's, bit for bit
    ts, wt = tsdf.copy(), weight.copy()
    R.integrate_view(ts, wt, origin, vl, trunc, depth, k4, e12)
    colour[ok] = new_colour[ok]
    tsdf[ok] = new[ok]
    weight[ok] = f32(weight + F(1.0))[ok]
    assert np.array_equal(tsdf.view(np.uint32), ts.view(np.uint32)) and np.array_equal(weight.view(np.uint32), wt.view(np.uint32))


def integrate_rgb(tsdf, weight, colour, origin, vl, trunc, depths, rgbs, k4s, e12s):
    """Views 0 .. V-1 in index order, rounded to float32 after each."""
    for i in range(len(depths)):
        integrate_view_rgb(tsdf, weight, colour, origin, vl, trunc, depths[i], rgbs[i], k4s[i], e12s[i])


def fused_rgb(dims, origin, vl, trunc, depths, rgbs, k4s, e12s):
    tsdf, weight = np.zeros(dims, dtype=np.float32), np.zeros(dims, dtype=np.float32)
    colour = np.zeros(tuple(dims) + (3,), dtype=np.float32)
    integrate_rgb(tsdf, weight, colour, origin, vl, trunc, depths, rgbs, k4s, e12s)
    return tsdf, weight, colour


def scene_fused_rgb(s, rgbs, views=None):
    """A ``tsdf_restatement.Scene`` fused with ``rgbs`` [V,H,W,3] -> (tsdf, weight, colour)."""
    sl = slice(None) if views is None else views
    return fused_rgb(s.dims, s.origin, s.vl, s.trunc, s.depths[sl], rgbs[sl], s.k4s[sl], s.e12s[sl])


def slot_colours(tsdf, weight, colour, tables):
    """The emitted slots in order (C order of the cells, the table row's order inside a cell) -> (positions-free keys, colours): a list
    of ((lower endpoint index, axis), float64 colour [3]) — what vfn_tsdf_emit_colours writes, with the edge each slot lies on."""
    tri, edge_vertex = tables
    nx, ny, nz = tsdf.shape
    out = []
    if min(nx, ny, nz) < 2:
        return out
    valid = np.ones((nx - 1, ny - 1, nz - 1), dtype=bool)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for q, (di, dj, dk) in enumerate(INC):
        sl = (slice(di, nx - 1 + di), slice(dj, ny - 1 + dj), slice(dk, nz - 1 + dk))
        valid &= weight[sl] != 0
        case |= (tsdf[sl] < 0).astype(np.int64) << q
    active = valid & (case != 0) & (case != 255)
    for i, j, k in np.argwhere(active):                      # C order
        c = (int(i), int(j), int(k))
        for e in tri[case[i, j, k]]:
            if e < 0:
                break
            qa, qb = (int(q) for q in edge_vertex[e])
            axis = [d for d in range(3) if INC[qa][d] != INC[qb][d]][0]
            ql, qu = (qa, qb) if INC[qa][axis] < INC[qb][axis] else (qb, qa)
            il = tuple(c[d] + INC[ql][d] for d in range(3))
            iu = tuple(c[d] + INC[qu][d] for d in range(3))
            fl, fu = np.abs(np.float64(tsdf[il])), np.abs(np.float64(tsdf[iu]))
            r = fl / (fl + fu)
            cl, cu = colour[il].astype(np.float64), colour[iu].astype(np.float64)
            col = ((np.float64(1.0) - r) * cl + r * cu) / np.float64(255.0)
            assert col.dtype == np.float64
            out.append(((il, axis), col))
    return out


def extract_coloured(tsdf, weight, colour, origin, vl, tables):
    """The zero level set with vertex colours -> (vertices float64 [n,3], faces int64 [m,3], colours float64 [n,3]): the mesh of
    ``tsdf_restatement.extract``; a vertex takes the colour of the slot at which it first appears (the lowest slot with its id)."""
    vertices, faces = R.extract(tsdf, weight, origin, vl, tables)
    slots = slot_colours(tsdf, weight, colour, tables)
    assert len(slots) == faces.size
    colours = np.zeros((len(vertices), 3), dtype=np.float64)
    seen = np.zeros(len(vertices), dtype=bool)
    for vid, (_, col) in zip(faces.reshape(-1), slots):
        if not seen[vid]:
            seen[vid] = True
            colours[vid] = col
    assert seen.all()
    return vertices, faces, colours


# ---- analytic colour images -------------------------------------------------------------------------------------------
def pattern_images(n_views, h, w):
    """uint8 [V,h,w,3]: a byte pattern of pixel row, column and view index (odd multipliers mod 256 / 251) in which neighbouring pixels
    differ in every channel, and so do the same pixels of neighbouring views: a wrong pixel, channel or view shows."""
    v = np.arange(n_views, dtype=np.int64)[:, None, None]
    r = np.arange(h, dtype=np.int64)[None, :, None]
    c = np.arange(w, dtype=np.int64)[None, None, :]
    red = (7 * r + 13 * c + 31 * v) % 256
    green = (29 * r + 3 * c + 57 * v + 101) % 256
    blue = (11 * r + 17 * c + 83 * v + 50) % 251
    return np.stack(np.broadcast_arrays(red, green, blue), axis=-1).astype(np.uint8)


def scene_images(s):
    """The pattern images that go with a ``tsdf_restatement.Scene``'s depth maps."""
    return pattern_images(*s.depths.shape)


def constant_images(n_views, h, w, colour):
    return np.broadcast_to(np.asarray(colour, dtype=np.uint8), (n_views, h, w, 3)).copy()


# ---- what the host and the device tests share -------------------------------------------------------------------------
CONSTANT_COLOURS = ((255, 0, 37), (1, 254, 128))
# A vertex of a constant-colour volume holds ((1 - r) c + r c) / 255: 1 - r, the two products, the sum and the quotient are rounded once
# each, 2^-53 relative, on a value of at most 1.  Derived, not measured.
CONSTANT_BOUND = 2.0 ** -50


def absorbed_cell():
    """A 2x2x2 volume whose origin (2^60) absorbs every offset: the three cut edges of the one triangle round to ONE position — one
    vertex, three slots, three different colours.  The vertex takes slot 0's: edge 0 of case 1, from corner 0 towards corner 1 = (0,1,0)."""
    t = np.full((2, 2, 2), 0.75, dtype=np.float32)
    t[0, 0, 0] = -0.25
    w = np.ones_like(t)
    c = np.arange(24, dtype=np.float32).reshape(2, 2, 2, 3) * 10
    return t, w, c, (2.0 ** 60,) * 3, 1.0


def zero_corner_volume():
    """tests/test_tsdf_host.py's volume with a voxel at exactly 0 between two negative ones, and a colour per voxel."""
    t = np.full((2, 3, 2), 0.5, dtype=np.float32)
    t[0, 0, 0] = t[0, 2, 0] = -0.5
    t[0, 1, 0] = 0.0
    w = np.ones_like(t)
    c = (np.arange(36, dtype=np.float32).reshape(2, 3, 2, 3) * 7) % 256
    return t, w, c
