"""The contract of the raster unit (include/vfn.h, "Rasterising a mesh's depth") restated in NumPy — the depth rasteriser with its
candidate rules, and Laplacian smoothing — and the meshes the tests draw.  Everything is float64 with the float32 inputs promoted;
NumPy rounds every operation once and never contracts, so an expression written here in the header's association has the header's
bits.  Tests only — the package never imports this module."""
from __future__ import annotations

import numpy as np

from tsdf_restatement import Scene, extrinsic, look_at, pinhole  # noqa: F401  (re-exported for the tests)

F, D = np.float32, np.float64


def _cross(a, b):
    """(a x b).x = a.y b.z - a.z b.y, cyclic; a, b [..., 3]"""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def rasterize_view(vertices, faces, k4, e12, h, w, near=0.05, far=100.0, c=0.5, candidates=True, counts=None):
    """One view -> depth float32 [h,w].  ``candidates=False`` evaluates every (face, pixel) pair of the faces the z and D rules keep
    (the candidate rules must not change a bit).  ``counts`` (a dict) collects how the faces were treated."""
    vertices, faces = np.asarray(vertices, dtype=D), np.asarray(faces, dtype=np.int64)
    fx, fy, cx, cy = (D(F(x)) for x in k4)
    e = [D(F(x)) for x in e12]
    near, far, c = D(F(near)), D(F(far)), D(F(c))
    depth = np.full((h, w), np.inf, dtype=F)
    tally = {"faces": len(faces), "z_culled": 0, "edge_on": 0, "off_screen": 0, "straddling": 0, "fragments": 0}
    if len(faces):
        X = vertices[faces]                                                   # [m, 3 vertices, 3]
        with np.errstate(all="ignore"):
            P = np.stack([((e[4 * r] * X[..., 0] + e[4 * r + 1] * X[..., 1]) + e[4 * r + 2] * X[..., 2]) + e[4 * r + 3] for r in range(3)], axis=-1)
            z = P[..., 2]
            culled = (z < near).all(axis=1) | (z > far).all(axis=1)
            n = np.stack([_cross(P[:, 1], P[:, 2]), _cross(P[:, 2], P[:, 0]), _cross(P[:, 0], P[:, 1])], axis=1)      # [m, 3 edges, 3]
            det = (P[:, 0, 0] * n[:, 0, 0] + P[:, 0, 1] * n[:, 0, 1]) + P[:, 0, 2] * n[:, 0, 2]
            flat = ~culled & ((det == 0) | ~np.isfinite(det))
            front = (z >= near).all(axis=1)
            px = (P[..., 0] * fx) / z + cx
            py = (P[..., 1] * fy) / z + cy
            ulo = np.maximum(D(0), np.ceil(px.min(axis=1) - c) - D(1))
            uhi = np.minimum(D(w - 1), np.floor(px.max(axis=1) - c) + D(1))
            vlo = np.maximum(D(0), np.ceil(py.min(axis=1) - c) - D(1))
            vhi = np.minimum(D(h - 1), np.floor(py.max(axis=1) - c) + D(1))
        tally["z_culled"], tally["edge_on"] = int(culled.sum()), int(flat.sum())
        for i in np.flatnonzero(~culled & ~flat):
            if not candidates or not front[i]:
                u0, u1, v0, v1 = 0, w - 1, 0, h - 1
                tally["straddling"] += int(not front[i])
            elif ulo[i] <= uhi[i] and vlo[i] <= vhi[i]:
                u0, u1, v0, v1 = int(ulo[i]), int(uhi[i]), int(vlo[i]), int(vhi[i])
            else:
                tally["off_screen"] += 1
                continue
            dx = ((np.arange(u0, u1 + 1, dtype=D) + c) - cx) / fx
            dy = (((np.arange(v0, v1 + 1, dtype=D) + c) - cy) / fy)[:, None]
            with np.errstate(all="ignore"):
                ee = [(n[i, j, 0] * dx + n[i, j, 1] * dy) + n[i, j, 2] for j in range(3)]
                s = (ee[0] + ee[1]) + ee[2]
                sigma = D(1) if det[i] > 0 else D(-1)
                covered = (s != 0) & (sigma * ee[0] >= 0) & (sigma * ee[1] >= 0) & (sigma * ee[2] >= 0)
                zz = det[i] / s
                kept = covered & (zz >= near) & (zz <= far)
                value = np.where(kept, zz, np.inf).astype(F)
            tally["fragments"] += int(kept.sum())
            window = depth[v0:v1 + 1, u0:u1 + 1]
            np.minimum(window, value, out=window)
    if counts is not None:
        for key, val in tally.items():
            counts[key] = counts.get(key, 0) + val
    depth[np.isinf(depth)] = 0
    return depth


def rasterize(vertices, faces, k4s, e12s, h, w, near=0.05, far=100.0, c=0.5, candidates=True, counts=None):
    """All views -> float32 [V,h,w]."""
    return np.stack([rasterize_view(vertices, faces, k4, e12, h, w, near, far, c, candidates, counts) for k4, e12 in zip(k4s, e12s)])


# ---- smoothing --------------------------------------------------------------------------------------------------------
def neighbours(faces, n):
    """Per vertex the ascending list of its edge-neighbours: three undirected edges per face, self-edges dropped, each neighbour once."""
    sets = [set() for _ in range(n)]
    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for p, q in ((a, b), (b, c), (c, a)):
            if p != q:
                sets[p].add(q)
                sets[q].add(p)
    return [sorted(s) for s in sets]


def smooth_laplacian(vertices, faces, iterations=10, lam=0.5):
    v = np.array(vertices, dtype=D)
    nbs = neighbours(faces, len(v))
    lam = D(lam)
    for _ in range(iterations):
        new = v.copy()
        for i, nb in enumerate(nbs):
            if not nb:
                continue
            s = v[nb[0]].copy()
            for q in nb[1:]:
                s = s + v[q]
            new[i] = v[i] + lam * (s / D(len(nb)) - v[i])
        v = new
    return v


# ---- meshes -----------------------------------------------------------------------------------------------------------
def icosphere(subdivisions, radius=0.5, centre=(0.0, 0.0, 0.0)):
    """A subdivided icosahedron pushed onto the sphere: 20 x 4^subdivisions faces, closed, every edge shared by exactly two faces."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [np.asarray(p, dtype=D) / np.linalg.norm(p) for p in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = verts[key[0]] + verts[key[1]]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]

        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.asarray(verts, dtype=D) * D(radius) + np.asarray(centre, dtype=D), np.asarray(faces, dtype=np.int64)


def box(half=0.6):
    """The axis-aligned box [-half, half]^3 as 12 triangles."""
    v = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], dtype=D)
    quads = ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3))
    return v, np.asarray([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int64)


def plane(z=2.0, cells=8, half=4.0):
    """The square [-half, half]^2 at depth z as cells x cells x 2 triangles."""
    xs = np.linspace(-half, half, cells + 1)
    v = np.array([[x, y, z] for y in xs for x in xs], dtype=D)
    f = []
    for j in range(cells):
        for i in range(cells):
            a = j * (cells + 1) + i
            f += [(a, a + 1, a + cells + 2), (a, a + cells + 2, a + cells + 1)]
    return v, np.asarray(f, dtype=np.int64)


def soup(count=3000, seed=7, spread=3.0, size=0.6):
    """``count`` unrelated triangles around the origin (where the test puts a camera): in front, behind, across the camera plane, off
    screen; vertices on a 1/64 lattice."""
    g = np.random.default_rng(seed)
    centres = g.uniform(-spread, spread, (count, 1, 3))
    v = np.round((centres + g.uniform(-size, size, (count, 3, 3))) * 64.0) / 64.0
    return v.reshape(-1, 3).astype(D), np.arange(3 * count, dtype=np.int64).reshape(count, 3)


def merged(*meshes):
    """Several meshes as one (vertices stacked, faces re-based)."""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs)
