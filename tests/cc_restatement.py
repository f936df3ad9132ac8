"""Connected components of a triangle mesh (include/vfn.h: vfn_cc_union_runs, vfn_cc_flatten, vfn_cc_segment_sums; vf_nerf_amd/meshops.py:
connected_components, filter_components, remove_degenerate_faces, remove_duplicate_faces) restated in NumPy from their contracts.

The partition is restated TWICE, by two methods that share nothing but the definition of "connected":
* ``roots_serial`` — a serial union-find over the faces in face order, with a dictionary from an edge (a vertex) to the first face that
  named it;
* ``roots_propagate`` — minimum-label propagation over the pairs (first face of a key's run, every other face of the run) with pointer
  jumping, repeated to a fixed point.
Both give root[m]: every face's component as its lowest face index.  Integers only: they agree exactly or not at all.

The area of a component follows the header's rule operation for operation (``wave_sum``).  Not part of the package: tests only."""
import numpy as np

CONNECTIVITIES = ("edge", "vertex")
WAVE = 64


# ---------------------------------------------------------------------------------------------------------------------------------
# the items the device kernel is fed: sorted keys with their nodes
# ---------------------------------------------------------------------------------------------------------------------------------
def items(faces, n_vertices, connectivity):
    """-> (keys, nodes), int64, keys ascending (a STABLE sort).  edge: the 3m corner pairs (0,1), (1,2), (2,0) of all faces, pair after
    pair, key = min * n + max, -1 where the two ends are one vertex.  vertex: the (vertex, face) incidences, each once, key = vertex."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    m = len(f)
    face = np.arange(m, dtype=np.int64)
    if connectivity == "edge":
        a = np.concatenate((f[:, 0], f[:, 1], f[:, 2]))
        b = np.concatenate((f[:, 1], f[:, 2], f[:, 0]))
        keys = np.where(a == b, -1, np.minimum(a, b) * n_vertices + np.maximum(a, b))
        nodes = np.concatenate((face, face, face))
        order = np.argsort(keys, kind="stable")
        return keys[order], nodes[order]
    assert connectivity == "vertex"
    both = np.unique(np.concatenate((f[:, 0] * max(m, 1) + face, f[:, 1] * max(m, 1) + face, f[:, 2] * max(m, 1) + face)))
    return both // max(m, 1), both % max(m, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the partition, twice
# ---------------------------------------------------------------------------------------------------------------------------------
def roots_serial(faces, n_vertices, connectivity):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    m = len(f)
    parent = list(range(m))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    first = {}
    for j in range(m):
        tri = [int(q) for q in f[j]]
        if connectivity == "edge":
            names = [(min(a, b), max(a, b)) for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])) if a != b]
        else:
            names = tri
        for name in names:
            if name in first:
                a, b = find(first[name]), find(j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
            else:
                first[name] = j
    return np.array([find(j) for j in range(m)], dtype=np.int64)


def pairs(faces, n_vertices, connectivity):
    """-> (u, v): for every key held by more than one face, (the first face of its run, each later face of the run)."""
    keys, nodes = items(faces, n_vertices, connectivity)
    keep = keys >= 0
    keys, nodes = keys[keep], nodes[keep]
    if len(keys) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)
    u, v = nodes[first[inverse]], nodes
    return u[u != v], v[u != v]


def roots_propagate(faces, n_vertices, connectivity):
    m = len(np.asarray(faces).reshape(-1, 3))
    u, v = pairs(faces, n_vertices, connectivity)
    label = np.arange(m, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, u, label[v])
        np.minimum.at(new, v, label[u])
        while True:                                   # pointer jumping: a label is a face, whose label may already be lower
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            return label
        label = new


def renumber_by_lowest(labels):
    """Any labelling of the faces -> the labels 0..K-1 in order of every class's lowest face."""
    labels = np.asarray(labels)
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inverse.reshape(-1)]


# ---------------------------------------------------------------------------------------------------------------------------------
# areas
# ---------------------------------------------------------------------------------------------------------------------------------
def tri_areas(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = v1 - v0, v2 - v0
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def wave_sum(x):
    """The header's rule: lane t adds x[t], x[t + 64], ... serially, STARTING from x[t]; a lane without elements holds +0.0; then
    s[t] = s[t] + s[t + 32] for t < 32, then 16, 8, 4, 2, 1; s[0] is the sum."""
    x = np.asarray(x, dtype=np.float64)
    s = np.zeros(WAVE)
    head = min(WAVE, len(x))
    s[:head] = x[:head]
    for b in range(WAVE, len(x), WAVE):
        row = x[b:b + WAVE]
        s[:len(row)] = s[:len(row)] + row
    o = WAVE // 2
    while o:
        s[:o] = s[:o] + s[o:2 * o]
        o //= 2
    return s[0]


# ---------------------------------------------------------------------------------------------------------------------------------
# the public results
# ---------------------------------------------------------------------------------------------------------------------------------
def components(vertices, faces, connectivity="edge", roots=roots_serial):
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n, m = len(v), len(f)
    root = roots(f, n, connectivity)
    first_face, face_label = np.unique(root, return_inverse=True)
    face_label = face_label.reshape(-1).astype(np.int64)
    k = len(first_face)
    vertex_label = np.full(n, k, dtype=np.int64)
    np.minimum.at(vertex_label, f.reshape(-1), np.repeat(face_label, 3))
    vertex_label[vertex_label == k] = -1
    areas = tri_areas(v, f) if m else np.zeros(0)
    order = np.argsort(face_label, kind="stable")
    count = np.bincount(face_label, minlength=k).astype(np.int64)
    start = np.concatenate(([0], np.cumsum(count)))
    area = np.array([wave_sum(areas[order[start[c]:start[c + 1]]]) for c in range(k)], dtype=np.float64)
    return {"face_label": face_label, "vertex_label": vertex_label, "n_components": k, "face_count": count, "area": area,
            "first_face": first_face.astype(np.int64)}


def filter_components(vertices, faces, min_faces=None, min_area=None, keep_largest=None, by="faces", connectivity="edge"):
    """-> (vertices, faces, kept_faces, inverse, kept component labels)"""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    c = components(v, f, connectivity)
    keep = np.ones(c["n_components"], dtype=bool)
    if min_faces is not None:
        keep &= c["face_count"] >= min_faces
    if min_area is not None:
        keep &= c["area"] >= min_area
    if keep_largest is not None:
        size = c["face_count"] if by == "faces" else c["area"]
        ranked = sorted(range(c["n_components"]), key=lambda j: (-size[j], j))[:keep_largest]
        top = np.zeros(c["n_components"], dtype=bool)
        top[ranked] = True
        keep &= top
    kept_faces = np.nonzero(keep[c["face_label"]])[0].astype(np.int64)
    used = np.zeros(len(v), dtype=bool)
    used[f[kept_faces].reshape(-1)] = True
    inverse = np.where(used, np.cumsum(used) - 1, -1).astype(np.int64)
    return v[used], inverse[f[kept_faces]].reshape(-1, 3), kept_faces, inverse, np.nonzero(keep)[0]


def remove_degenerate_faces(vertices, faces, zero_area=False):
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bad = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
    if zero_area and len(f):
        a, b = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        c = np.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), axis=1)
        bad |= (c == 0).all(axis=1)
    kept = np.nonzero(~bad)[0].astype(np.int64)
    return f[kept], kept


def remove_duplicate_faces(faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    seen, kept = set(), []
    for j, tri in enumerate(f):
        name = tuple(sorted(int(q) for q in tri))
        if name not in seen:
            seen.add(name)
            kept.append(j)
    kept = np.array(kept, dtype=np.int64)
    return f[kept], kept


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes (tests/test_cc_host.py and tests/test_hip_cc.py share them): the smallest at which each thing can go wrong
# ---------------------------------------------------------------------------------------------------------------------------------
def _coords(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))


def strip(k, seed=0, order="ascending"):
    """k triangles in a row, face j = (j, j + 1, j + 2): each shares an edge with the next — one component, and as a forest the
    longest chain there is.  ``order``: how the faces are numbered along the strip."""
    faces = np.stack((np.arange(k), np.arange(k) + 1, np.arange(k) + 2), axis=1).astype(np.int64)
    if order == "descending":
        faces = faces[::-1].copy()
    elif order == "shuffled":
        faces = faces[np.random.default_rng(k).permutation(k)]
    return _coords(k + 2, seed + k), faces


def separate(k, seed=1):
    """k triangles that share nothing: k components."""
    return _coords(3 * k, seed + k), np.arange(3 * k, dtype=np.int64).reshape(k, 3)


def tetrahedra(k=300):
    """k separate tetrahedra, face q of tetrahedron t at face index q k + t: the faces of one component lie k apart."""
    corners = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], dtype=np.int64)
    faces = np.concatenate([corners[q] + 4 * np.arange(k)[:, None] for q in range(4)])
    return _coords(4 * k, 4), faces


def torus(nu=100, nv=100):
    """A closed surface of 2 nu nv triangles, every vertex shared by six of them."""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    a, b = 2 * np.pi * i / nu, 2 * np.pi * j / nv
    v = np.stack(((2.0 + 0.7 * np.cos(b)) * np.cos(a), (2.0 + 0.7 * np.cos(b)) * np.sin(a), 0.7 * np.sin(b)), axis=-1).reshape(-1, 3)
    idx = lambda p, q: ((p % nu) * nv + (q % nv)).reshape(-1)          # noqa: E731
    f = np.concatenate((np.stack((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), axis=1),
                        np.stack((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)), axis=1))).astype(np.int64)
    return v, f


_scene = {}


def floater_scene():
    """A 20 000-face torus plus 200 floaters — strips of 1 to 50 faces, each of every size four times — with the floaters' faces spread
    through the face list by a fixed permutation.  -> (vertices, faces, is_big[m])"""
    if "s" not in _scene:
        v, f = torus()
        vs, fs, big = [v], [f], [np.ones(len(f), dtype=bool)]
        at = len(v)
        g = np.random.default_rng(200)
        for t in range(200):
            k = t % 50 + 1
            sv, sf = strip(k, seed=1000 + t)
            vs.append(0.05 * sv + g.uniform(-4.0, 4.0, 3))
            fs.append(sf + at)
            big.append(np.zeros(k, dtype=bool))
            at += len(sv)
        v, f, big = np.concatenate(vs), np.concatenate(fs), np.concatenate(big)
        perm = g.permutation(len(f))
        _scene["s"] = (v, f[perm].copy(), big[perm].copy())
    return _scene["s"]


def _tiny():
    sq = np.array([[0.0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0.5, 0], [2, 1.5, 1], [3, 0, 1], [3, 1, 2], [0.5, 0.5, 3]])
    return {
        "no_faces": (sq[:3], np.zeros((0, 3), dtype=np.int64)),
        "nothing": (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)),
        "one_face": (sq[:3], np.array([[0, 1, 2]])),
        "shared_edge": (sq[:4], np.array([[0, 1, 2], [0, 2, 3]])),
        "bow_tie": (sq[:5], np.array([[0, 1, 2], [2, 3, 4]])),                       # 2 components by edge, 1 by vertex
        "disjoint": (sq[:6], np.array([[0, 1, 2], [3, 4, 5]])),
        "repeated_vertex": (sq[:4], np.array([[0, 1, 1], [0, 1, 2], [3, 3, 3]])),      # (0, 1, 1) has the edge {0, 1}; (3, 3, 3) has none
        "three_on_an_edge": (sq[:5], np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])),
        "duplicate_face": (sq[:6], np.array([[0, 1, 2], [3, 4, 5], [2, 0, 1]])),
        "unreferenced_vertex": (sq, np.array([[0, 1, 2], [5, 6, 7], [2, 1, 3]])),
    }


def shapes():
    """{name: (vertices, faces)}"""
    out = dict(_tiny())
    for k in (1, 63, 64, 65, 129):
        out[f"sum_{k}"] = strip(k, seed=7)
    for k in (255, 256, 257):
        out[f"count_{k}"] = separate(k)
    for order in ("ascending", "descending", "shuffled"):
        out[f"strip_4097_{order}"] = strip(4097, seed=3, order=order)
    out["tetrahedra_300"] = tetrahedra(300)
    out["floaters"] = floater_scene()[:2]
    return out
