"""PLY files of triangle meshes: ``write_ply`` (binary little-endian, what Mesher.get_mesh and the cull command write) and
``read_mesh`` (binary little-endian or ASCII, triangle faces)."""
from __future__ import annotations

from typing import Optional

import numpy as np

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}
_COLORS = ("red", "green", "blue", "alpha")


def write_ply(path: str, verts: np.ndarray, faces: np.ndarray, colors: Optional[np.ndarray] = None):
    """Binary little-endian PLY: float32 x y z [+ uchar red green blue alpha], faces as `list uchar int`."""
    verts = np.asarray(verts, dtype="<f4").reshape(-1, 3)
    faces = np.asarray(faces, dtype="<i4").reshape(-1, 3)
    hdr = ["ply", "format binary_little_endian 1.0", f"element vertex {len(verts)}",
           "property float x", "property float y", "property float z"]
    if colors is not None:
        hdr += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    hdr += [f"element face {len(faces)}", "property list uchar int vertex_indices", "end_header"]
    vdt = [("xyz", "<f4", 3)] + ([("rgba", "u1", 4)] if colors is not None else [])
    vrec = np.empty(len(verts), dtype=vdt)
    vrec["xyz"] = verts
    if colors is not None:
        c = np.asarray(colors, dtype=np.uint8).reshape(len(verts), -1)
        rgba = np.full((len(verts), 4), 255, dtype=np.uint8)
        rgba[:, :c.shape[1]] = c
        vrec["rgba"] = rgba
    frec = np.empty(len(faces), dtype=[("n", "u1"), ("idx", "<i4", 3)])
    frec["n"] = 3
    frec["idx"] = faces
    with open(path, "wb") as fh:
        fh.write(("\n".join(hdr) + "\n").encode("ascii"))
        fh.write(vrec.tobytes())
        fh.write(frec.tobytes())


def read_mesh(path: str, colors: bool = False):
    """(vertices float64 [V, 3], faces int64 [F, 3]) of a PLY file: binary little-endian or ASCII, any extra vertex properties
    (normals, colours, alpha) skipped, the face list counted by uchar / int / uint with int / uint indices.  Other elements
    are skipped; a face that is not a triangle is an error.  ``colors=True`` adds a third item: the vertex colour
    properties present of red, green, blue, alpha as uint8 [V, k] in that order, or None when there is no colour."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:end].decode("ascii", "replace").splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property" and elements:
            if tok[1] == "list":
                elements[-1][2].append((tok[4], "list", _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported (ascii, binary_little_endian)")
    verts = np.zeros((0, 3), np.float64)
    faces = np.zeros((0, 3), np.int64)
    rgba = None
    if fmt == "ascii":
        lines = data[body:].decode("ascii").split("\n")
        pos = 0
        for name, count, props in elements:
            rows = []
            for _ in range(count):
                while not lines[pos].strip():
                    pos += 1
                rows.append(lines[pos].split())
                pos += 1
            if name == "vertex":
                names = [p[0] for p in props]
                cols = [names.index(c) for c in ("x", "y", "z")]
                verts = np.array([[float(r[c]) for c in cols] for r in rows], dtype=np.float64).reshape(-1, 3)
                if colors and "red" in names:
                    ccols = [names.index(c) for c in _COLORS if c in names]
                    rgba = np.array([[int(r[c]) for c in ccols] for r in rows], dtype=np.uint8).reshape(-1, len(ccols))
            elif name == "face":
                fl = []
                for r in rows:
                    k = int(r[0])
                    if k != 3:
                        raise ValueError(f"{path}: face with {k} vertices (only triangles are supported)")
                    fl.append([int(x) for x in r[1:4]])
                faces = np.array(fl, dtype=np.int64).reshape(-1, 3)
        return (verts, faces, rgba) if colors else (verts, faces)
    off = body
    for name, count, props in elements:
        if any(p[1] == "list" for p in props):
            if len(props) != 1:
                raise ValueError(f"{path}: element {name!r} mixes a list with other properties")
            _, _, ct, it = props[0]
            ct, it = np.dtype("<" + ct), np.dtype("<" + it)
            if count == 0:
                continue
            # every face a triangle: fixed-size records; anything else is caught by the count check
            rec = np.dtype([("n", ct), ("idx", it, 3)])
            need = off + rec.itemsize * count
            if need > len(data):
                raise ValueError(f"{path}: truncated, or not every face is a triangle")
            arr = np.frombuffer(data, dtype=rec, count=count, offset=off)
            if not (arr["n"] == 3).all():
                bad = int(arr["n"][arr["n"] != 3][0])
                raise ValueError(f"{path}: face with {bad} vertices (only triangles are supported)")
            if name == "face":
                faces = arr["idx"].astype(np.int64)
            off = need
        else:
            rec = np.dtype([(p[0], "<" + p[1]) for p in props])
            arr = np.frombuffer(data, dtype=rec, count=count, offset=off)
            if name == "vertex":
                verts = np.stack([arr["x"], arr["y"], arr["z"]], 1).astype(np.float64)
                if colors and "red" in rec.names:
                    rgba = np.stack([arr[c] for c in _COLORS if c in rec.names], 1).astype(np.uint8)
            off += rec.itemsize * count
    return (verts, faces, rgba) if colors else (verts, faces)
