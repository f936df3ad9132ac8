"""Reading and writing triangle meshes as PLY 1.0 files (host, NumPy only): the layout viewers read and the reference writes for
``tsdf-mesh/tsdf.ply`` (evaluation/methods.py:665) — vertices ``x y z`` (``float``, or ``double``), optionally ``red green blue`` as
``uchar``, faces as ``property list uchar int vertex_indices`` — ASCII or ``binary_little_endian``.

* ``write_ply(path, vertices, faces, colours=None, *, binary=True, vertex_dtype="f4", normals=None)`` — colours in [0, 1] are written
  as ``rint(c 255)`` clipped to [0, 255] (for ``c = b / 255`` that is b again); uint8 colours are written as they are.  ``normals``
  ([n,3] floating point) are written as ``nx ny nz`` in the vertex type, after ``x y z`` and before the colours — Open3D's order.
* ``read_ply(path)`` -> ``(vertices float64 [n,3], faces int64 [m,3], colours uint8 [n,3] | None)`` for those layouts;
  ``read_ply(path, normals=True)`` returns a fourth value, the normals as float64 [n,3], or None when the file has no ``nx ny nz``.
  Other vertex properties (``alpha``, ...) are skipped, ``uint`` / ``int`` indices and the name ``vertex_index`` are accepted: enough to
  load a ground-truth ``*_mesh.ply`` into ``refuse.metrics_3d``.  Anything else is refused by name: big-endian files, faces that are
  not triangles, elements other than ``vertex`` and ``face`` in front of them, list properties on vertices.

The reference calls ``compute_vertex_normals()`` before it writes: ``meshops.vertex_normals`` computes them, ``normals=`` writes them.
Device tensors are accepted and downloaded."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

_SCALARS = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
            "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


class PlyError(ValueError):
    pass


def _host(x) -> np.ndarray:
    if hasattr(x, "detach"):                      # a torch tensor, on any device
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def colour_bytes(colours) -> np.ndarray:
    """[n,3] colours -> uint8: uint8 as given; floating point in [0, 1] as rint(c 255) clipped to [0, 255] (NaN is refused)."""
    c = _host(colours)
    if c.ndim != 2 or c.shape[1] != 3:
        raise ValueError(f"colours must be [n,3], got {c.shape}")
    if c.dtype == np.uint8:
        return np.ascontiguousarray(c)
    if c.dtype.kind != "f":
        raise ValueError(f"colours must be uint8 or floating point in [0, 1], got {c.dtype}")
    if np.isnan(c).any():
        raise ValueError("colours hold NaN")
    return np.clip(np.rint(c.astype(np.float64) * 255.0), 0.0, 255.0).astype(np.uint8)


def write_ply(path, vertices, faces, colours=None, *, binary: bool = True, vertex_dtype: str = "f4", normals=None) -> None:
    """Write the mesh (vertices [n,3] floating point, faces [m,3] integers, 0-based, optional colours [n,3], optional normals [n,3]
    floating point) to ``path``.  Without ``normals`` the file has no ``nx ny nz`` properties."""
    if vertex_dtype not in ("f4", "f8"):
        raise ValueError(f"vertex_dtype must be 'f4' or 'f8', got {vertex_dtype!r}")
    v, f = _host(vertices), _host(faces)
    if v.ndim != 2 or v.shape[1] != 3 or v.dtype.kind != "f":
        raise ValueError(f"vertices must be floating point [n,3], got {v.dtype} {v.shape}")
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
        raise ValueError(f"faces must be integers [m,3], got {f.dtype} {f.shape}")
    if f.size and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):
        raise ValueError(f"a face index lies outside [0, {v.shape[0]})")
    if v.shape[0] >= (1 << 31):
        raise ValueError(f"{v.shape[0]} vertices exceed the int index of the file")
    c = None if colours is None else colour_bytes(colours)
    if c is not None and c.shape[0] != v.shape[0]:
        raise ValueError(f"{c.shape[0]} colours for {v.shape[0]} vertices")
    nrm = None
    if normals is not None:
        nrm = _host(normals)
        if nrm.ndim != 2 or nrm.shape[1] != 3 or nrm.dtype.kind != "f":
            raise ValueError(f"normals must be floating point [n,3], got {nrm.dtype} {nrm.shape}")
        if nrm.shape[0] != v.shape[0]:
            raise ValueError(f"{nrm.shape[0]} normals for {v.shape[0]} vertices")
        nrm = nrm.astype("<" + vertex_dtype)
    v = v.astype("<" + vertex_dtype)
    f = f.astype("<i4")
    header = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0", f"element vertex {v.shape[0]}"]
    header += [f"property {'float' if vertex_dtype == 'f4' else 'double'} {a}" for a in "xyz"]
    if nrm is not None:
        header += [f"property {'float' if vertex_dtype == 'f4' else 'double'} {a}" for a in ("nx", "ny", "nz")]
    if c is not None:
        header += [f"property uchar {a}" for a in ("red", "green", "blue")]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        if binary:
            fields = ([("p", "<" + vertex_dtype, (3,))] + ([("n", "<" + vertex_dtype, (3,))] if nrm is not None else [])
                      + ([("c", "u1", (3,))] if c is not None else []))
            rec = np.empty(v.shape[0], dtype=np.dtype(fields))            # (packed: no padding between the fields)
            rec["p"] = v
            if nrm is not None:
                rec["n"] = nrm
            if c is not None:
                rec["c"] = c
            fh.write(rec.tobytes())
            frec = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
            frec["n"] = 3
            frec["i"] = f
            fh.write(frec.tobytes())
        else:
            lines = []
            for i in range(v.shape[0]):                                   # str of a NumPy scalar: the shortest text that reads back to its bits
                row = [str(x) for x in v[i]]
                if nrm is not None:
                    row += [str(x) for x in nrm[i]]
                if c is not None:
                    row += [str(int(b)) for b in c[i]]
                lines.append(" ".join(row))
            lines += [f"3 {int(a)} {int(b)} {int(d)}" for a, b, d in f]
            fh.write(("\n".join(lines) + "\n").encode("ascii") if lines else b"")


def _parse_header(fh):
    """-> (format, [(element name, count, [(property name, dtype | ("list", count dtype, item dtype))])])"""
    if fh.readline().strip() != b"ply":
        raise PlyError("not a PLY file: the first line is not 'ply'")
    fmt, elements = None, []
    while True:
        raw = fh.readline()
        if not raw:
            raise PlyError("the header has no end_header")
        words = raw.decode("ascii", errors="replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            break
        if words[0] == "format":
            fmt = words[1]
            if fmt == "binary_big_endian":
                raise PlyError("big-endian PLY files are not supported")
            if fmt not in ("ascii", "binary_little_endian") or words[2:] != ["1.0"]:
                raise PlyError(f"unsupported PLY format line: {' '.join(words)}")
        elif words[0] == "element":
            elements.append((words[1], int(words[2]), []))
        elif words[0] == "property":
            if not elements:
                raise PlyError("a property comes before any element")
            if words[1] == "list":
                if words[2] not in _SCALARS or words[3] not in _SCALARS:
                    raise PlyError(f"unknown list types: {' '.join(words)}")
                elements[-1][2].append((words[4], ("list", _SCALARS[words[2]], _SCALARS[words[3]])))
            else:
                if words[1] not in _SCALARS:
                    raise PlyError(f"unknown property type '{words[1]}'")
                elements[-1][2].append((words[2], _SCALARS[words[1]]))
        else:
            raise PlyError(f"unknown header line: {' '.join(words)}")
    if fmt is None:
        raise PlyError("the header has no format line")
    return fmt, elements


def read_ply(path, normals: bool = False):
    """-> (vertices float64 [n,3], faces int64 [m,3], colours uint8 [n,3] or None); with ``normals=True`` a fourth value: the ``nx ny nz``
    of the vertices as float64 [n,3], or None when the file has none."""
    with open(path, "rb") as fh:
        fmt, elements = _parse_header(fh)
        names = [e[0] for e in elements]
        if names[:1] != ["vertex"] or (len(names) > 1 and names[1] != "face"):
            raise PlyError(f"expected the elements 'vertex' then 'face', got {names}")
        _, n, vprops = elements[0]
        if any(isinstance(t, tuple) for _, t in vprops):
            raise PlyError("list properties on vertices are not supported")
        pnames = [p for p, _ in vprops]
        if len(set(pnames)) != len(pnames) or not all(a in pnames for a in "xyz"):
            raise PlyError(f"the vertex element needs distinct properties with x, y and z, got {pnames}")
        has_colour = all(a in pnames for a in ("red", "green", "blue"))
        has_normals = all(a in pnames for a in ("nx", "ny", "nz"))
        if has_normals and any(t not in ("f4", "f8") for p, t in vprops if p in ("nx", "ny", "nz")):
            raise PlyError("vertex normals must be float or double")
        if has_colour and any(t != "u1" for p, t in vprops if p in ("red", "green", "blue")):
            raise PlyError("vertex colours must be uchar")
        m, fprops = (elements[1][1], elements[1][2]) if len(elements) > 1 else (0, [])
        if m or fprops:
            if len(fprops) != 1 or not isinstance(fprops[0][1], tuple) or fprops[0][0] not in ("vertex_indices", "vertex_index"):
                raise PlyError(f"the face element must be one list property vertex_indices, got {[p for p, _ in fprops]}")
            _, count_t, item_t = fprops[0][1]
            if item_t not in ("i4", "u4") or count_t not in ("u1", "i1", "u2", "i2", "u4", "i4"):
                raise PlyError(f"face indices must be int or uint with an integer count, got {item_t} counted by {count_t}")
        vdtype = np.dtype([(p, "<" + t) for p, t in vprops])
        if fmt == "ascii":
            tokens = fh.read().split()
            width = len(vprops)
            if len(tokens) < n * width + 4 * m:
                raise PlyError("the file ends before its elements do")
            table = np.array([float(t) for t in tokens[:n * width]], dtype=np.float64).reshape(n, width)      # (every scalar type fits a double)
            cols = {p: table[:, i] for i, p in enumerate(pnames)}
            ftok = np.array([int(t) for t in tokens[n * width:n * width + 4 * m]], dtype=np.int64).reshape(m, 4)
            if m and not (ftok[:, 0] == 3).all():
                raise PlyError("non-triangle faces are not supported")
            faces = ftok[:, 1:].copy()
        else:
            data = np.frombuffer(fh.read(n * vdtype.itemsize), dtype=vdtype)
            if data.shape[0] != n:
                raise PlyError("the file ends before its vertices do")
            cols = {p: data[p] for p in pnames}
            faces = np.zeros((0, 3), dtype=np.int64)
            if m:
                fdtype = np.dtype([("n", "<" + count_t), ("i", "<" + item_t, (3,))])
                raw = fh.read(m * fdtype.itemsize)
                # a triangle-only file has records of one size: anything else shows in the counts (or in the length)
                frec = np.frombuffer(raw[:(len(raw) // fdtype.itemsize) * fdtype.itemsize], dtype=fdtype)
                if (frec["n"] != 3).any():
                    raise PlyError("non-triangle faces are not supported")
                if frec.shape[0] != m:
                    raise PlyError("the file ends before its faces do")
                faces = frec["i"].astype(np.int64)
    vertices = np.stack([cols[a].astype(np.float64) for a in "xyz"], axis=1) if n else np.zeros((0, 3), dtype=np.float64)
    colours = None
    if has_colour:
        colours = np.stack([cols[a].astype(np.uint8) for a in ("red", "green", "blue")], axis=1) if n else np.zeros((0, 3), dtype=np.uint8)
    if faces.size and (faces.min() < 0 or faces.max() >= n):
        raise PlyError(f"a face index lies outside [0, {n})")
    if not normals:
        return vertices, faces.reshape(-1, 3), colours
    vertex_normals = None
    if has_normals:
        vertex_normals = np.stack([cols[a].astype(np.float64) for a in ("nx", "ny", "nz")], axis=1) if n else np.zeros((0, 3), dtype=np.float64)
    return vertices, faces.reshape(-1, 3), colours, vertex_normals
