"""Orientation of a triangle mesh (include/vfn.h: vfn_orient_union_runs, vfn_orient_flatten, vfn_orient_votes; vf_nerf_amd/meshops.py:
orientation, orient, inconsistent_edges) restated in NumPy from its contract.

The parities are restated TWICE, by two methods that share nothing but the definition of a manifold edge and of its constraint:
* ``parity_serial`` — a serial parity union-find over the sorted items in item order (``items``, the list the device kernel is fed);
* ``parity_colouring`` — a breadth-first two-colouring from every component's lowest face, over a dictionary from an undirected edge to
  the half-edges that name it, built in face order: no sort, no forest.
Both give (root[m], parity[m], conflict[m]): every face's component as its lowest face index, its flip relative to that face, and
whether a constraint was found broken at it.  Integers only: they agree exactly or not at all — except on the parities of a component
that is not orientable, which depend on the order of the walk and are zeroed before anything is compared.

The votes follow the header's formulas operation for operation, and a component's votes are added by ``cc_restatement.wave_sum``.  Not
part of the package: tests only."""
import os
from collections import deque

import numpy as np

import cc_restatement as CC

REFERENCES = ("first", "majority", "volume", "viewpoints")
VIEWPOINTS = np.array([[0.0, 0.0, 6.0], [5.0, 0.5, -1.0], [-4.0, 3.0, 0.25], [0.5, -6.0, 1.0], [0.0, 0.0, 6.0]])      # (the last repeats the first: a tie)


# ---------------------------------------------------------------------------------------------------------------------------------
# the items the device kernel is fed
# ---------------------------------------------------------------------------------------------------------------------------------
def items(faces, n_vertices):
    """-> (keys, nodes, dirs): the 3m half-edges (0,1) of all faces, then (1,2), then (2,0); for a -> b key = min * n + max (-1 where
    a == b), node = the face, dir = (a < b); ascending by key, a STABLE sort."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    face = np.arange(len(f), dtype=np.int64)
    a = np.concatenate((f[:, 0], f[:, 1], f[:, 2]))
    b = np.concatenate((f[:, 1], f[:, 2], f[:, 0]))
    keys = np.where(a == b, -1, np.minimum(a, b) * n_vertices + np.maximum(a, b))
    order = np.argsort(keys, kind="stable")
    return keys[order], np.concatenate((face, face, face))[order], (a < b).astype(np.uint8)[order]


def manifold_edges(faces, n_vertices):
    """-> (f, g, want) in item order: the runs of exactly two equal keys >= 0 whose items belong to two faces; want = (dir_f == dir_g)."""
    keys, nodes, dirs = items(faces, n_vertices)
    out = []
    i, k = 0, len(keys)
    while i < k:
        j = i
        while j + 1 < k and keys[j + 1] == keys[i]:
            j += 1
        if keys[i] >= 0 and j - i == 1 and nodes[i] != nodes[j]:
            out.append((int(nodes[i]), int(nodes[j]), int(dirs[i] == dirs[j])))
        i = j + 1
    e = np.array(out, dtype=np.int64).reshape(-1, 3)
    return e[:, 0], e[:, 1], e[:, 2]


# ---------------------------------------------------------------------------------------------------------------------------------
# the parities, twice
# ---------------------------------------------------------------------------------------------------------------------------------
def parity_serial(faces, n_vertices):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    m = len(f)
    parent, bit = list(range(m)), [0] * m          # bit[x]: x relative to parent[x]
    conflict = np.zeros(m, dtype=bool)

    def find(x):
        path, acc = [], 0
        while parent[x] != x:
            path.append(x)
            acc ^= bit[x]
            x = parent[x]
        root, total = x, acc
        for y in path:                             # compression: every node of the path straight under the root
            step = bit[y]
            parent[y], bit[y] = root, acc
            acc ^= step
        return root, total

    for a, b, want in zip(*manifold_edges(f, n_vertices)):
        (ra, pa), (rb, pb) = find(int(a)), find(int(b))
        if ra == rb:
            if pa ^ pb != want:
                conflict[a] = True
        elif ra < rb:
            parent[rb], bit[rb] = ra, pa ^ pb ^ int(want)
        else:
            parent[ra], bit[ra] = rb, pa ^ pb ^ int(want)
    found = [find(j) for j in range(m)]
    return (np.array([r for r, _ in found], dtype=np.int64).reshape(m), np.array([p for _, p in found], dtype=np.uint8).reshape(m), conflict)


def parity_colouring(faces, n_vertices):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    m = len(f)
    named = {}                                     # undirected edge -> [(face, a < b)] in face order, corner pair after corner pair
    for j in range(m):
        tri = [int(q) for q in f[j]]
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
            if a != b:
                named.setdefault((min(a, b), max(a, b)), []).append((j, a < b))
    neighbours = [[] for _ in range(m)]
    for held in named.values():
        if len(held) == 2 and held[0][0] != held[1][0]:
            (p, dp), (q, dq) = held
            neighbours[p].append((q, int(dp == dq)))
            neighbours[q].append((p, int(dp == dq)))
    root = np.full(m, -1, dtype=np.int64)
    parity = np.zeros(m, dtype=np.uint8)
    conflict = np.zeros(m, dtype=bool)
    for start in range(m):                         # ascending: a walk starts at its component's lowest face
        if root[start] >= 0:
            continue
        root[start] = start
        queue = deque([start])
        while queue:
            x = queue.popleft()
            for y, want in neighbours[x]:
                if root[y] < 0:
                    root[y], parity[y] = start, parity[x] ^ want
                    queue.append(y)
                elif parity[x] ^ parity[y] != want:
                    conflict[x] = True
    return root, parity, conflict


# ---------------------------------------------------------------------------------------------------------------------------------
# the votes, in the written association
# ---------------------------------------------------------------------------------------------------------------------------------
def corners(vertices, faces, parity):
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    swap = np.asarray(parity).astype(bool)
    return v[f[:, 0]], v[np.where(swap, f[:, 2], f[:, 1])], v[np.where(swap, f[:, 1], f[:, 2])]


def cross(a, b):
    return np.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), axis=1)


def votes_volume(vertices, faces, parity):
    v0, v1, v2 = corners(vertices, faces, parity)
    c = cross(v1, v2)
    return (v0[:, 0] * c[:, 0] + v0[:, 1] * c[:, 1]) + v0[:, 2] * c[:, 2]


def votes_viewpoints(vertices, faces, parity, viewpoints):
    v0, v1, v2 = corners(vertices, faces, parity)
    p = np.asarray(viewpoints, dtype=np.float64).reshape(-1, 3)
    c = cross(v1 - v0, v2 - v0)
    g = ((v0 + v1) + v2) / 3.0
    d = p[None, :, :] - g[:, None, :]                                                     # [m, C, 3]
    s = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    j = np.argmin(s, axis=1)                                                              # the first of the least: ties to the lowest j
    row = np.arange(len(g))
    d, s = d[row, j], s[row, j]
    dot = (c[:, 0] * d[:, 0] + c[:, 1] * d[:, 1]) + c[:, 2] * d[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s == 0.0, 0.0, dot / np.sqrt(s))


# ---------------------------------------------------------------------------------------------------------------------------------
# the public results
# ---------------------------------------------------------------------------------------------------------------------------------
def rewind(faces, flip):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.stack((f[:, 0], np.where(flip, f[:, 2], f[:, 1]), np.where(flip, f[:, 1], f[:, 2])), axis=1)


def count_inconsistent(faces, n_vertices):
    return int(manifold_edges(faces, n_vertices)[2].sum())


def orientation(vertices, faces, reference="first", viewpoints=None, parities=parity_serial):
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    m = len(f)
    root, parity, conflict = parities(f, len(v))
    first_face, face_label = np.unique(root, return_inverse=True)
    face_label = face_label.reshape(-1).astype(np.int64)
    k = len(first_face)
    count = np.bincount(face_label, minlength=k).astype(np.int64)
    orientable = np.bincount(face_label[conflict], minlength=k) == 0
    parity = np.where(orientable[face_label], parity, 0).astype(np.uint8)
    sign = np.zeros(k, dtype=bool)
    sums = None
    if reference == "majority":
        sign = 2 * np.bincount(face_label, weights=parity, minlength=k).astype(np.int64) > count
    elif reference in ("volume", "viewpoints"):
        t = (votes_volume(v, f, parity) if reference == "volume" else votes_viewpoints(v, f, parity, viewpoints)) if m else np.zeros(0)
        order = np.argsort(face_label, kind="stable")
        start = np.concatenate(([0], np.cumsum(count)))
        sums = np.array([CC.wave_sum(t[order[start[c]:start[c + 1]]]) for c in range(k)], dtype=np.float64)
        sign = (sums < 0) & orientable
    else:
        assert reference == "first"
    flip = parity.astype(bool) ^ sign[face_label]
    return {"flip": flip, "face_label": face_label, "n_components": k, "first_face": first_face.astype(np.int64), "face_count": count,
            "orientable": orientable, "flipped_count": np.bincount(face_label, weights=flip, minlength=k).astype(np.int64),
            "inconsistent_edges": count_inconsistent(f, len(v)), "votes": sums, "faces": rewind(f, flip)}


def signed_volume6(vertices, faces):
    """Six times the volume a closed mesh encloses: the sum of v0 . (v1 x v2) (math.fsum: a check, not the device's order)."""
    import math
    return math.fsum(votes_volume(vertices, faces, np.zeros(len(faces), dtype=np.uint8)).tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes (tests/test_orient_host.py and tests/test_hip_orient.py share them): the smallest at which each thing can go wrong
# ---------------------------------------------------------------------------------------------------------------------------------
def flipped(faces, which):
    return rewind(faces, np.asarray(which, dtype=bool))


def sheet(nx, ny, seed, origin=(0.0, 0.0, 0.0)):
    """An nx x ny grid of quads, each cut into two triangles, consistently wound, over a bumpy height field: 2 nx ny faces."""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    g = np.random.default_rng(seed)
    v = np.stack((i / nx, j / ny, 0.05 * g.uniform(-1.0, 1.0, i.shape)), axis=-1).reshape(-1, 3) + np.asarray(origin)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    idx = lambda p, q: (p * (ny + 1) + q).reshape(-1)          # noqa: E731
    f = np.stack((np.stack((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), axis=1),
                  np.stack((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)), axis=1)), axis=1).reshape(-1, 3).astype(np.int64)
    return v, f


def random_flips(faces, seed):
    """A seeded random half of the faces rewound."""
    which = np.zeros(len(faces), dtype=bool)
    which[np.random.default_rng(seed).permutation(len(faces))[:len(faces) // 2]] = True
    return flipped(faces, which)


def strip(k):
    """k triangles in a row, consistently wound, then every other one flipped: face j = (j, j + 1, j + 2).  As a forest the deepest chain
    there is, with the parities alternating along it."""
    return CC.strip(k, seed=11)


def moebius(k):
    """k (odd) triangles (j, j + 1, j + 2) over k vertices, indices modulo k: the strip closed with a half twist.  Every edge {j, j + 1} is
    held by two faces, the edges {j, j + 2} form ONE boundary loop: one component, not orientable."""
    assert k % 2 == 1 and k >= 5
    a = 4.0 * np.pi * np.arange(k) / k                       # twice round: neighbours in the index lie on opposite rims
    half = 0.5 * a
    w = np.where(np.arange(k) % 2 == 0, 0.3, -0.3)
    v = np.stack(((1.0 + w * np.cos(half)) * np.cos(a), (1.0 + w * np.cos(half)) * np.sin(a), w * np.sin(half)), axis=1)
    j = np.arange(k)
    return v, np.stack((j, (j + 1) % k, (j + 2) % k), axis=1).astype(np.int64)


def sphere(rings=16, sectors=32, centre=(0.3, -0.2, 0.1)):
    """A closed latitude-longitude sphere wound outwards: two pole fans and (rings - 2) bands, 2 sectors (rings - 1) faces."""
    v = [[0.0, 0.0, 1.0]]
    for r in range(1, rings):
        t = np.pi * r / rings
        for s in range(sectors):
            p = 2.0 * np.pi * s / sectors
            v.append([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)])
    v.append([0.0, 0.0, -1.0])
    ring = lambda r, s: 1 + (r - 1) * sectors + s % sectors          # noqa: E731
    south = len(v) - 1
    f = []
    for s in range(sectors):
        f.append([0, ring(1, s), ring(1, s + 1)])
        f.append([south, ring(rings - 1, s + 1), ring(rings - 1, s)])
        for r in range(1, rings - 1):
            f.append([ring(r, s), ring(r + 1, s), ring(r + 1, s + 1)])
            f.append([ring(r, s), ring(r + 1, s + 1), ring(r, s + 1)])
    return np.array(v) + np.asarray(centre), np.array(f, dtype=np.int64)


def golden(tag):
    fix = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_stages.npz"))
    return fix[f"{tag}.vs"].astype(np.float64), fix[f"{tag}.fs"].astype(np.int64) - 1          # the reference's faces are 1-based


GOLDEN = ("f16", "f16.after", "f16.all", "f24", "f32")
_shapes = {}


def shapes():
    """{name: (vertices, faces)}, built once"""
    if _shapes:
        return _shapes
    sq = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0], [2, 0.5, 1], [2, 1.5, 1], [3, 0, 1], [3, 1, 2], [0.5, 0.5, 3]])
    out = {"one_face": (sq[:3], np.array([[0, 1, 2]]))}
    v, f = sheet(64, 64, seed=1)
    out["sheet_64"] = (v, random_flips(f, seed=2))                                   # 8192 faces: many lanes on one root, 96 blocks
    out["strip_4096"] = strip(4096)
    out["moebius_4097"] = moebius(4097)
    v, f = sphere()
    out["sphere"] = (v, random_flips(f, seed=3))
    v, f = CC.torus(40, 40)
    out["torus"] = (v, random_flips(f, seed=4))
    v, f = sphere(6, 8)
    out["inside_out_sphere"] = (v, flipped(f, np.ones(len(f), dtype=bool)))                 # consistent, and enclosing a negative volume
    (va, fa), (vb, fb) = sheet(8, 8, seed=5), sheet(8, 5, seed=6, origin=(3.0, 0.0, 0.0))
    out["two_sheets"] = (np.concatenate((va, vb)), np.concatenate((random_flips(fa, seed=7), random_flips(fb, seed=8) + len(va))))
    # three faces on the edge {0, 1}: the run of three is ignored, and each of them carries a sheet of its own
    out["fin"] = (sq[:8], np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [2, 1, 5], [3, 6, 0], [4, 7, 1]]))
    out["duplicate_pair"] = (sq[:6], np.array([[0, 1, 2], [3, 4, 5], [2, 0, 1], [3, 5, 4]]))      # the same winding twice; the opposite winding
    # (0, 1, 1) holds {0, 1} twice itself — a run of two items of ONE face —, (6, 6, 6) no edge at all, the other two share {2, 3}
    out["repeated_vertex"] = (sq[:7], np.array([[0, 1, 1], [2, 3, 4], [2, 3, 5], [6, 6, 6]]))
    out["repeated_vertex_run_of_three"] = (sq[:4], np.array([[0, 1, 1], [0, 1, 2], [3, 3, 3]]))
    v, f = out["sheet_64"]
    out["sheet_64_permuted"] = (v, f[np.random.default_rng(9).permutation(len(f))])
    for tag in GOLDEN:
        out[tag] = golden(tag)
    _shapes.update(out)
    return _shapes


def ORIENTABLE(name):
    """Whether every component of the shape can be wound consistently (by construction; the tests assert what the restatement finds)."""
    return name != "moebius_4097"
