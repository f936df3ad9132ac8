"""The contract of the block-sparse TSDF volume (include/vfn.h, "A block-sparse TSDF volume") restated in NumPy on top of
tests/tsdf_restatement.py: the allocation rule in float64 operation for operation, the dense per-voxel arithmetic evaluated at listed
global voxels (float32, every intermediate checked to BE float32), the "zero until the call that opened the block" fusion, and the
extraction that walks blocks in id order and cells in local C order with the dense vertex formulas.  Tests only — the package never
imports this module."""
from __future__ import annotations

import numpy as np

import tsdf_restatement as R
from tsdf_restatement import F, INC, f32

BLOCK = 8
D = np.float64


def block_lattice(dims):
    return tuple((int(n) + BLOCK - 1) // BLOCK for n in dims)


def cameras(k4, e12):
    """What the host hands the marking kernel per view: C = the first three rows of inv(4x4 of the float32 extrinsic rows promoted), the
    float32 intrinsics promoted, q = sqrt(1 / (fx fx) + 1 / (fy fy))."""
    m = np.eye(4, dtype=np.float64)
    m[:3] = np.asarray(e12, dtype=np.float32).astype(np.float64).reshape(3, 4)
    c = np.linalg.inv(m)[:3]
    fx, fy, cx, cy = (D(v) for v in np.asarray(k4, dtype=np.float32))
    q = np.sqrt(D(1.0) / (fx * fx) + D(1.0) / (fy * fy))
    return c, fx, fy, cx, cy, q


def mark(dims, origin, vl, trunc, depths, k4s, e12s):
    """marks[nbx,nby,nbz] bool of the views: include/vfn.h, vfn_tsdf_sparse_mark, in float64."""
    nb = block_lattice(dims)
    marks = np.zeros(nb, dtype=bool)
    o = [D(F(c)) for c in origin]
    vl, tr = D(F(vl)), D(F(trunc))
    for depth, k4, e12 in zip(depths, k4s, e12s):
        assert depth.dtype == np.float32
        c, fx, fy, cx, cy, q = cameras(k4, e12)
        h, w = depth.shape
        v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        d = depth.astype(np.float64)
        ok = d > 0
        a, b = (u - cx) / fx, (v - cy) / fy
        ad, bd = a * d, b * d
        r = (tr + (D(0.5) * (d + tr)) * q) + D(2.0) * vl
        edge = D(8.0) * vl
        lo, hi = [], []
        with np.errstate(all="ignore"):
            for ax in range(3):
                p = ((c[ax, 0] * ad + c[ax, 1] * bd) + c[ax, 2] * d) + c[ax, 3]
                l, g = np.floor(((p - r) - o[ax]) / edge), np.floor(((p + r) - o[ax]) / edge)
                ok &= (g >= 0) & (l <= nb[ax] - 1)
                lo.append(np.clip(np.where(ok, l, 0), 0, nb[ax] - 1).astype(np.int64))
                hi.append(np.clip(np.where(ok, g, 0), 0, nb[ax] - 1).astype(np.int64))
        assert all(x.dtype == np.float64 for x in (a, b, ad, bd, r, p))
        box = np.stack(lo + hi, axis=-1)[ok]
        for l0, l1, l2, h0, h1, h2 in np.unique(box, axis=0):
            marks[l0:h0 + 1, l1:h1 + 1, l2:h2 + 1] = True
    return marks


class State:
    """The sparse volume's state: block_of [nb] int32, block_coords [n,3] int32, tsdf / weight [n,8,8,8] float32, colour [n,8,8,8,3] or None."""

    def __init__(self, dims, colour=False):
        self.dims = tuple(int(n) for n in dims)
        self.block_of = np.full(block_lattice(dims), -1, dtype=np.int32)
        self.block_coords = np.zeros((0, 3), dtype=np.int32)
        self.tsdf = np.zeros((0, BLOCK, BLOCK, BLOCK), dtype=np.float32)
        self.weight = np.zeros_like(self.tsdf)
        self.colour = np.zeros((0, BLOCK, BLOCK, BLOCK, 3), dtype=np.float32) if colour else None

    @property
    def n_blocks(self):
        return len(self.block_coords)

    def indices(self):
        """The global voxel index of every stored voxel [n,8,8,8,3] and whether it lies inside dims [n,8,8,8]."""
        loc = np.stack(np.meshgrid(*(np.arange(BLOCK),) * 3, indexing="ij"), axis=-1)
        g = self.block_coords.astype(np.int64)[:, None, None, None, :] * BLOCK + loc[None]
        return g, (g < np.asarray(self.dims)).all(-1)


def allocate(state, origin, vl, trunc, depths, k4s, e12s):
    """New blocks = marks & (block_of < 0), numbered in ascending C order of the block lattice after the existing ones -> their count."""
    new = mark(state.dims, origin, vl, trunc, depths, k4s, e12s) & (state.block_of < 0)
    coords = np.argwhere(new)
    n0 = state.n_blocks
    state.block_of[new] = np.arange(n0, n0 + len(coords), dtype=np.int32)
    state.block_coords = np.concatenate([state.block_coords, coords.astype(np.int32)])
    pad = np.zeros((len(coords), BLOCK, BLOCK, BLOCK), dtype=np.float32)
    state.tsdf, state.weight = np.concatenate([state.tsdf, pad]), np.concatenate([state.weight, pad])
    if state.colour is not None:
        state.colour = np.concatenate([state.colour, np.zeros(pad.shape + (3,), dtype=np.float32)])
    return len(coords)


def integrate_at(indices, tsdf, weight, origin, vl, trunc, depths, k4s, e12s, colour=None, rgbs=None):
    """The dense contract of include/vfn.h at the listed GLOBAL voxels indices[n,3]: views in order into tsdf[n] / weight[n] (and
    colour[n,3] from rgbs uint8 [V,H,W,3]), in place.  The style of ``tsdf_restatement.integrate_view``: float32 operation for operation."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1, 3)
    assert tsdf.dtype == np.float32 and weight.dtype == np.float32 and tsdf.shape == weight.shape == (len(idx),)
    assert (colour is None) == (rgbs is None) and idx.max(initial=0) <= 1 << 24
    vl, trunc = F(vl), F(trunc)
    x, y, z = (f32(F(origin[c]) + f32(f32(idx[:, c].astype(np.float32) + F(0.5)) * vl)) for c in range(3))
    for i in range(len(depths)):
        depth = depths[i]
        assert depth.dtype == np.float32
        h, w = depth.shape
        fx, fy, cx, cy = (F(v) for v in np.asarray(k4s[i], dtype=np.float32))
        e = [F(v) for v in np.asarray(e12s[i], dtype=np.float32)]
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
            if colour is not None:
                assert rgbs[i].dtype == np.uint8 and colour.dtype == np.float32
                p = f32(rgbs[i][vi, ui].astype(np.float32))
                new_colour = f32(f32(f32(colour * weight[:, None]) + p) / f32(weight + F(1.0))[:, None])
                colour[ok] = new_colour[ok]
        tsdf[ok] = new[ok]
        weight[ok] = f32(weight + F(1.0))[ok]


def integrate(state, origin, vl, trunc, depths, k4s, e12s, rgbs=None):
    """The views into EVERY block allocated so far; voxels beyond dims are never updated."""
    g, inside = state.indices()
    ts, wt = state.tsdf[inside], state.weight[inside]
    col = None if state.colour is None else state.colour[inside]
    integrate_at(g[inside], ts, wt, origin, vl, trunc, depths, k4s, e12s, col, rgbs)
    state.tsdf[inside], state.weight[inside] = ts, wt
    if col is not None:
        state.colour[inside] = col


def fuse(scene, calls=None, rgbs=None, allocate_first=False):
    """``calls`` (default: one call with all views) is a list of view slices, each one ``integrate`` call: allocate for its views, then
    apply them to every block allocated so far — a block holds a dense volume that was zero until the call that opened it.
    ``allocate_first``: all views allocate before the first call and the calls run with allocate=False."""
    s = scene
    state = State(s.dims, colour=rgbs is not None)
    calls = [slice(None)] if calls is None else calls
    if allocate_first:
        allocate(state, s.origin, s.vl, s.trunc, s.depths, s.k4s, s.e12s)
    for sl in calls:
        if not allocate_first:
            allocate(state, s.origin, s.vl, s.trunc, s.depths[sl], s.k4s[sl], s.e12s[sl])
        integrate(state, s.origin, s.vl, s.trunc, s.depths[sl], s.k4s[sl], s.e12s[sl], None if rgbs is None else rgbs[sl])
    return state


def to_dense(state):
    """(tsdf, weight[, colour]) [nx,ny,nz]: absent voxels zero."""
    nx, ny, nz = state.dims
    nb = state.block_of.shape
    bi, bj, bk = state.block_coords.astype(np.int64).T

    def spread(blocks, tail=()):
        out = np.zeros((nb[0], BLOCK, nb[1], BLOCK, nb[2], BLOCK) + tail, dtype=blocks.dtype)
        out[bi, :, bj, :, bk, :] = blocks
        return np.ascontiguousarray(out.reshape((nb[0] * BLOCK, nb[1] * BLOCK, nb[2] * BLOCK) + tail)[:nx, :ny, :nz])

    dense = (spread(state.tsdf), spread(state.weight))
    return dense if state.colour is None else dense + (spread(state.colour, (3,)),)


def allocated_mask(state):
    """bool [nx,ny,nz]: the lattice voxels that lie in an allocated block."""
    nx, ny, nz = state.dims
    return np.repeat(np.repeat(np.repeat(state.block_of >= 0, BLOCK, 0), BLOCK, 1), BLOCK, 2)[:nx, :ny, :nz]


def active_cells(tsdf, weight):
    """The cells the dense extraction triangulates, bool [nx-1,ny-1,nz-1] (``tsdf_restatement.extract``'s test)."""
    nx, ny, nz = tsdf.shape
    valid = np.ones((nx - 1, ny - 1, nz - 1), dtype=bool)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for q, (di, dj, dk) in enumerate(INC):
        sl = (slice(di, nx - 1 + di), slice(dj, ny - 1 + dj), slice(dk, nz - 1 + dk))
        valid &= weight[sl] != 0
        case |= (tsdf[sl] < 0).astype(np.int64) << q
    return valid & (case != 0) & (case != 255)


def uncovered_cells(state, tsdf, weight):
    """The number of dense active cells with a corner outside the allocated blocks."""
    nx, ny, nz = tsdf.shape
    if min(nx, ny, nz) < 2:
        return 0
    inside = allocated_mask(state)
    covered = np.ones((nx - 1, ny - 1, nz - 1), dtype=bool)
    for di, dj, dk in INC:
        covered &= inside[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk]
    return int((active_cells(tsdf, weight) & ~covered).sum())


def extract_sparse(state, origin, vl, tables):
    """Blocks in id order, cells in local C order, vertices numbered by first appearance, the formulas of ``tsdf_restatement.extract``
    with the GLOBAL lattice index -> (vertices float64 [n,3], faces int64 [m,3]) and, for a state with colour, colours float64 [n,3] (a
    vertex takes the colour of the slot at which it first appears)."""
    tri, edge_vertex = tables
    dims = np.asarray(state.dims, dtype=np.int64)
    has_colour = state.colour is not None
    empty = (np.zeros((0, 3), dtype=np.float64), np.zeros((0, 3), dtype=np.int64)) + ((np.zeros((0, 3), dtype=np.float64),) if has_colour else ())
    if state.n_blocks == 0:
        return empty
    g, _ = state.indices()                                       # the cell's lower corner
    valid = (g + 1 < dims).all(-1)
    case = np.zeros(valid.shape, dtype=np.int64)
    nb = np.asarray(state.block_of.shape, dtype=np.int64)
    store = []                                                  # per corner: (block id, local index) of every cell
    for q, inc in enumerate(INC):
        gg = g + np.asarray(inc, dtype=np.int64)
        bb = np.minimum(gg >> 3, nb - 1)
        ids = state.block_of[bb[..., 0], bb[..., 1], bb[..., 2]].astype(np.int64)
        valid &= ids >= 0                                       # an absent neighbour voids the cell
        ids0, l = np.maximum(ids, 0), gg & 7
        valid &= state.weight[ids0, l[..., 0], l[..., 1], l[..., 2]] != 0
        case |= (state.tsdf[ids0, l[..., 0], l[..., 1], l[..., 2]] < 0).astype(np.int64) << q
        store.append((ids0, l))
    active = valid & (case != 0) & (case != 255)
    o = [np.float64(F(c)) for c in origin]
    vl64 = np.float64(F(vl))
    ids, verts, faces, cols = {}, [], [], []
    for b, i, j, k in np.argwhere(active):                      # block id order, then local C order
        c = [int(x) for x in g[b, i, j, k]]
        face = []
        for e in tri[case[b, i, j, k]]:
            if e < 0:
                break
            qa, qb = (int(q) for q in edge_vertex[e])
            axis = [d for d in range(3) if INC[qa][d] != INC[qb][d]]
            assert len(axis) == 1
            axis = axis[0]
            ql, qu = (qa, qb) if INC[qa][axis] < INC[qb][axis] else (qb, qa)
            at = []
            for q in (ql, qu):
                bid, l = store[q][0][b, i, j, k], store[q][1][b, i, j, k]
                at.append((bid, l[0], l[1], l[2]))
            il = [c[d] + INC[ql][d] for d in range(3)]
            pos = [o[d] + (np.float64(il[d]) + np.float64(0.5)) * vl64 for d in range(3)]
            fl, fu = np.abs(np.float64(state.tsdf[at[0]])), np.abs(np.float64(state.tsdf[at[1]]))
            r = fl / (fl + fu)
            pos[axis] = pos[axis] + r * vl64
            key = tuple(float(p) for p in pos)
            if key not in ids:
                ids[key] = len(verts)
                verts.append(pos)
                if has_colour:
                    cl, cu = state.colour[at[0]].astype(np.float64), state.colour[at[1]].astype(np.float64)
                    cols.append(((np.float64(1.0) - r) * cl + r * cu) / np.float64(255.0))
            face.append(ids[key])
            if len(face) == 3:
                faces.append(face)
                face = []
    if not faces:
        return empty
    mesh = (np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    return mesh + ((np.asarray(cols, dtype=np.float64).reshape(-1, 3),) if has_colour else ())


def triangle_set(vertices, faces):
    """A mesh as the set of its triangles, each the bits of its three vertices in order — the numbering drops out."""
    bits = np.ascontiguousarray(vertices, dtype=np.float64).view(np.uint64)[faces]            # [m,3,3]
    return set(map(bytes, bits.reshape(len(faces), -1)))


def canonical(vertices, faces):
    """Vertices sorted by bits, faces remapped and sorted -> (vertex bits uint64 [n,3], faces int64 [m,3])."""
    bits = np.ascontiguousarray(vertices, dtype=np.float64).view(np.uint64).reshape(-1, 3)
    order = np.lexsort((bits[:, 2], bits[:, 1], bits[:, 0]))
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    f = rank[np.asarray(faces, dtype=np.int64)]
    f = f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))] if len(f) else f
    return bits[order], f


def far_scene():
    """Beyond the dense limit: dims (4096, 4096, 2048) at 1/1024 m with a truncation of 4 voxels; one 24 x 32 view of focal 400 px that
    sees a constant depth of 0.5 m, rotated off-axis and placed so that the patch lies near lattice index (3900, 3000, 1500)."""
    vl = F(1.0 / 1024.0)
    dims, origin = (4096, 4096, 2048), (-2.0, -2.0, -1.0)
    target = np.asarray(origin, dtype=np.float64) + (np.array([3900.0, 3000.0, 1500.0]) + 0.5) * np.float64(vl)
    fwd = np.array([0.36, -0.48, 0.8])
    pose = R.look_at(target - 0.5 * fwd, target)
    h, w = 24, 32
    k4 = R.pinhole(h, w, 400.0)
    depth = np.full((h, w), 0.5, dtype=np.float32)
    return R.Scene(dims, origin, vl, F(4.0) * vl, [pose], [k4], [depth])
