"""The contract of the TSDF unit (include/vfn.h, "Fusing depth maps into a mesh") restated in NumPy, and the analytic scenes the tests
fuse.  Integration is float32 operation for operation (every intermediate is checked to BE float32: NumPy widens silently when a Python
float or a float64 scalar slips in); vertex positions are float64; the triangle and edge tables are the ones ``lib.mesh_tables()``
returns; vertices merge by position in order of first appearance.  Tests only — the package never imports this module."""
from __future__ import annotations

import numpy as np

INC = ((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1), (1, 0, 1))
F = np.float32


def f32(x):
    assert isinstance(x, (np.ndarray, np.floating)) and x.dtype == np.float32, f"an operand was widened to {getattr(x, 'dtype', type(x))}"
    return x


def centres(o, n, vl):
    """x = o + ((float)i + 0.5f) * vl"""
    return f32(F(o) + f32(f32(np.arange(n, dtype=np.float32) + F(0.5)) * F(vl)))


def extrinsic(pose):
    """float32(inv(float64 pose)), rows [3,4] flattened to 12"""
    return np.linalg.inv(np.asarray(pose, dtype=np.float64)).astype(np.float32)[:3].reshape(12)


def integrate_view(tsdf, weight, origin, vl, trunc, depth, k4, e12):
    """One observation into tsdf / weight (float32 [nx,ny,nz]), in place."""
    assert tsdf.dtype == np.float32 and weight.dtype == np.float32 and depth.dtype == np.float32
    k4, e12, vl, trunc = np.asarray(k4, dtype=np.float32), np.asarray(e12, dtype=np.float32), F(vl), F(trunc)
    nx, ny, nz = tsdf.shape
    h, w = depth.shape
    x = centres(origin[0], nx, vl)[:, None, None]
    y = centres(origin[1], ny, vl)[None, :, None]
    z = centres(origin[2], nz, vl)[None, None, :]
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
    tsdf[ok] = new[ok]
    weight[ok] = f32(weight + F(1.0))[ok]


def integrate(tsdf, weight, origin, vl, trunc, depths, k4s, e12s):
    """Views 0 .. V-1 in index order, rounded to float32 after each."""
    for i in range(len(depths)):
        integrate_view(tsdf, weight, origin, vl, trunc, depths[i], k4s[i], e12s[i])


def fused(dims, origin, vl, trunc, depths, k4s, e12s):
    tsdf, weight = np.zeros(dims, dtype=np.float32), np.zeros(dims, dtype=np.float32)
    integrate(tsdf, weight, origin, vl, trunc, depths, k4s, e12s)
    return tsdf, weight


def extract(tsdf, weight, origin, vl, tables):
    """The zero level set -> (vertices float64 [n,3], faces int64 [m,3]).  ``tables`` = (tri_table[256,16], edge_vertex[12,2])."""
    tri, edge_vertex = tables
    nx, ny, nz = tsdf.shape
    empty = np.zeros((0, 3), dtype=np.float64), np.zeros((0, 3), dtype=np.int64)
    if min(nx, ny, nz) < 2:
        return empty
    valid = np.ones((nx - 1, ny - 1, nz - 1), dtype=bool)
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for q, (di, dj, dk) in enumerate(INC):
        sl = (slice(di, nx - 1 + di), slice(dj, ny - 1 + dj), slice(dk, nz - 1 + dk))
        valid &= weight[sl] != 0
        case |= (tsdf[sl] < 0).astype(np.int64) << q
    active = valid & (case != 0) & (case != 255)
    o = [np.float64(F(c)) for c in origin]
    vl64 = np.float64(F(vl))
    ids, verts, faces = {}, [], []
    for i, j, k in np.argwhere(active):                      # C order
        c = (int(i), int(j), int(k))
        row = tri[case[i, j, k]]
        face = []
        for e in row:
            if e < 0:
                break
            qa, qb = (int(q) for q in edge_vertex[e])
            axis = [d for d in range(3) if INC[qa][d] != INC[qb][d]]
            assert len(axis) == 1
            axis = axis[0]
            ql, qu = (qa, qb) if INC[qa][axis] < INC[qb][axis] else (qb, qa)
            il = [c[d] + INC[ql][d] for d in range(3)]
            iu = [c[d] + INC[qu][d] for d in range(3)]
            pos = [o[d] + (np.float64(il[d]) + np.float64(0.5)) * vl64 for d in range(3)]
            fl, fu = np.abs(np.float64(tsdf[tuple(il)])), np.abs(np.float64(tsdf[tuple(iu)]))
            pos[axis] = pos[axis] + (fl / (fl + fu)) * vl64
            key = tuple(float(p) for p in pos)                 # (0.0 == -0.0 as dict keys; the first occurrence's bits stay)
            if key not in ids:
                ids[key] = len(verts)
                verts.append(pos)
            face.append(ids[key])
            if len(face) == 3:
                faces.append(face)
                face = []
    if not faces:
        return empty
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3), np.asarray(faces, dtype=np.int64).reshape(-1, 3)


def reference_depth(depth, depth_scale=1000.0, depth_trunc=10.0):
    """(depth * 1000).astype(uint16) on the float64 array the reference loads, /1000 in float32, zero at or beyond depth_trunc."""
    q = (np.asarray(depth).astype(np.float64) * depth_scale).astype(np.uint16)
    d = q.astype(np.float32) / np.float32(depth_scale)
    d[d >= depth_trunc] = 0
    return d


# ---- analytic scenes --------------------------------------------------------------------------------------------------
def look_at(eye, target=(0.0, 0.0, 0.0)):
    """Camera-to-world [4,4] float64, +z forward (OpenCV), looking from eye at target."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    fwd = (target - eye) / np.linalg.norm(target - eye)
    up = np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([0.0, 0.0, 1.0])
    right = np.cross(up, fwd)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, down, fwd, eye
    return pose


def pinhole(h, w, focal=None):
    """fx fy cx cy: fx = fy = 0.9 W unless given, principal point at the image centre."""
    f = 0.9 * w if focal is None else focal
    return np.array([f, f, (w - 1) / 2.0, (h - 1) / 2.0], dtype=np.float32)


def _rays(pose, k4, h, w):
    k = np.asarray(k4, dtype=np.float64)
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    cam = np.stack([(u - k[2]) / k[0], (v - k[3]) / k[1], np.ones_like(u)], axis=-1)      # z = 1: the ray parameter IS the depth
    return pose[:3, 3], cam @ pose[:3, :3].T


def sphere_depth(pose, k4, h, w, radius=0.5):
    """z-depth of the unit-parameter rays against the sphere |p| = radius at the origin (float64 geometry), 0 where a ray misses."""
    eye, d = _rays(pose, k4, h, w)
    a, b, c = (d * d).sum(-1), 2.0 * (d @ eye), eye @ eye - radius * radius
    disc = b * b - 4 * a * c
    t = (-b - np.sqrt(np.maximum(disc, 0.0))) / (2 * a)
    return np.where((disc > 0) & (t > 0), t, 0.0).astype(np.float32)


def room_depth(pose, k4, h, w, half=0.6):
    """z-depth against the inside of the axis-aligned box [-half, half]^3 (the eye is inside: every ray hits a wall)."""
    eye, d = _rays(pose, k4, h, w)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.stack([(np.where(d > 0, half, -half)[..., c] - eye[c]) / d[..., c] for c in range(3)], axis=-1)
    t = np.where(np.isfinite(t) & (t > 0), t, np.inf).min(-1)
    return t.astype(np.float32)


class Scene:
    def __init__(self, dims, origin, vl, trunc, poses, k4s, depths):
        self.dims, self.origin, self.vl, self.trunc = tuple(dims), tuple(float(F(o)) for o in origin), float(F(vl)), float(F(trunc))
        self.poses = np.asarray(poses, dtype=np.float64)
        self.k4s = np.asarray(k4s, dtype=np.float32)
        self.depths = np.asarray(depths, dtype=np.float32)
        self.e12s = np.stack([extrinsic(p) for p in self.poses])

    def intrinsics_matrices(self):
        k = np.tile(np.eye(3, dtype=np.float32), (len(self.k4s), 1, 1))
        k[:, 0, 0], k[:, 1, 1], k[:, 0, 2], k[:, 1, 2] = self.k4s.T
        return k

    def fused(self, views=None):
        s = slice(None) if views is None else views
        return fused(self.dims, self.origin, self.vl, self.trunc, self.depths[s], self.k4s[s], self.e12s[s])


SPHERE_EYES = ((2.0, 0.0, 0.0), (-2.0, 0.0, 0.0), (0.0, 2.0, 0.0), (0.0, -2.0, 0.0), (0.0, 0.0, 2.0), (0.0, 0.0, -2.0), (1.3, 1.2, 1.1))


def sphere_scene(dims=(32, 32, 29), h=48, w=64, eyes=SPHERE_EYES):
    """A sphere of radius 0.5 at the origin seen by look-at cameras; the volume starts at -0.7 with voxels of 1.4 / dims[0] and a
    truncation of three voxels."""
    vl = F(1.4) / F(dims[0])
    poses = [look_at(e) for e in eyes]
    k4 = pinhole(h, w)
    return Scene(dims, (-0.7, -0.7, -0.7), vl, F(3.0) * vl, poses, [k4] * len(poses), [sphere_depth(p, k4, h, w) for p in poses])


ROOM_VIEWS = (((0.1, -0.05, 0.0), (0.6, 0.0, 0.1)), ((0.1, -0.05, 0.0), (-0.6, 0.1, 0.0)), ((-0.2, 0.1, 0.15), (0.0, 0.6, 0.0)),
              ((0.0, 0.0, 0.2), (0.1, 0.0, -0.6)), ((0.3, 0.25, -0.2), (-0.6, -0.6, 0.6)))


def room_scene(dims=(32, 32, 32), h=30, w=40, views=ROOM_VIEWS, focal=None):
    """Cameras INSIDE the box [-0.6, 0.6]^3 looking at its walls: voxels behind a camera, projections outside the image and zc <= 0 all
    occur.  A short focal length (0.6 W) so that a view covers a wall's worth of voxels."""
    vl = F(1.4) / F(dims[0])
    poses = [look_at(e, t) for e, t in views]
    k4 = pinhole(h, w, 0.6 * w if focal is None else focal)
    return Scene(dims, (-0.7, -0.7, -0.7), vl, F(3.0) * vl, poses, [k4] * len(poses), [room_depth(p, k4, h, w) for p in poses])
