"""Labels onto a mesh and the mesh into a file: `label_mesh` (the 5-NN mode transfer of utils/eval_utils.py, with a distance cut-off), `label_colors`
(one fixed colour per id), `write_ply` / `read_ply` (binary little-endian PLY through numpy structured arrays; plyfile is not needed).  The mesh
itself comes from `TsdfVolume.extract_mesh` (csrc/mesh.hip)."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import eval_utils as E


def label_mesh(vertices: torch.Tensor, points_3d: torch.Tensor, point_labels: torch.Tensor, max_dist: Optional[float] = None, grid=None) -> torch.Tensor:
    """i32[V]: every vertex takes the most frequent label among its 5 nearest map points (ties to the smallest label, `ovo_knn5_labels`); a vertex
    whose NEAREST map point is farther than `max_dist` gets -1 (squared f64 distances are compared with float(max_dist) ** 2).  Both clouds in one
    frame, f32 [*, 3]; labels one per point, 32-bit.  `grid`: a `PointGrid` already built over `points_3d` (e.g. for several meshes of one map)."""
    labels = point_labels.reshape(-1).to(torch.int32).contiguous()
    if grid is None:
        grid = E.PointGrid(points_3d.to(torch.float32).contiguous())
    if vertices.shape[0] == 0:
        return torch.empty(0, dtype=torch.int32, device=vertices.device)
    _, d2, label, _ = grid.query(vertices.to(torch.float32).contiguous(), labels, want_d2=max_dist is not None)
    if max_dist is not None:
        far = d2.min(dim=1).values > float(max_dist) ** 2
        label = torch.where(far, torch.full_like(label, -1), label)
    return label


def label_colors(ids) -> np.ndarray:
    """u8[n, 3]: a fixed colour per non-negative id (three bytes of a multiplicative hash, each kept at 64 or above), mid-grey for negative ones."""
    ids = np.asarray(ids.detach().cpu() if isinstance(ids, torch.Tensor) else ids).astype(np.int64).reshape(-1)
    x = ((ids + 1).astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    rgb = np.stack([(x >> np.uint64(s)) & np.uint64(0xFF) for s in (24, 16, 8)], 1).astype(np.uint8)
    rgb = (64 + (rgb.astype(np.uint16) * 3) // 4).astype(np.uint8)
    rgb[ids < 0] = 128
    return rgb


def _host(a, dtype, shape_tail) -> np.ndarray:
    a = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a)
    if a.dtype != np.dtype(dtype):
        if np.dtype(dtype).kind == "i" and a.dtype.kind in "iu" and (a.size == 0 or (a.min() >= -2**31 and a.max() < 2**31)):
            a = a.astype(dtype)
        else:
            raise ValueError(f"write_ply: expected {np.dtype(dtype)} (got {a.dtype})")
    if a.shape[1:] != shape_tail:
        raise ValueError(f"write_ply: expected [n{''.join(', %d' % s for s in shape_tail)}] (got {a.shape})")
    return a


def _vertex_dtype(rgb: bool, instance: bool, cls: bool, normals: bool = False) -> np.dtype:
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:                                            # directly after the position: the order MeshLab and Open3D read
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if rgb:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    if instance:
        fields.append(("instance", "<i4"))
    if cls:
        fields.append(("class", "<i4"))
    return np.dtype(fields)


_FACE = np.dtype([("n", "u1"), ("vertex_indices", "<i4", (3,))])
_PLY_TYPE = {"<f4": "float", "u1": "uchar", "|u1": "uchar", "<i4": "int"}


def write_ply(path, vertices, faces, rgb=None, instance=None, cls=None, normals=None) -> None:
    """binary_little_endian 1.0: `element vertex` with x y z (float), optionally nx ny nz (float), red green blue (uchar), `int instance`,
    `int class`; `element face` with `list uchar int vertex_indices`.  Tensors or arrays; vertices f32[V, 3], faces i32[T, 3], rgb u8[V, 3],
    instance / cls integer [V], normals f32[V, 3] (their bits are written as they are; a wrong dtype or row count is a ValueError)."""
    v, f = _host(vertices, np.float32, (3,)), _host(faces, np.int32, (3,))
    vd = _vertex_dtype(rgb is not None, instance is not None, cls is not None, normals is not None)
    rec = np.zeros(len(v), dtype=vd)
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    for name, col, dt, tail in (("normals", normals, np.float32, (3,)), ("rgb", rgb, np.uint8, (3,)), ("instance", instance, np.int32, ()),
                                ("class", cls, np.int32, ())):
        if col is None:
            continue
        col = _host(col, dt, tail)
        if len(col) != len(v):
            raise ValueError(f"write_ply: {name} has {len(col)} rows for {len(v)} vertices")
        if name == "rgb":
            rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
        elif name == "normals":
            rec["nx"], rec["ny"], rec["nz"] = col[:, 0], col[:, 1], col[:, 2]
        else:
            rec[name] = col
    fr = np.zeros(len(f), dtype=_FACE)
    fr["n"], fr["vertex_indices"] = 3, f
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    lines += [f"property {_PLY_TYPE[vd[name].str]} {name}" for name in vd.names]
    lines += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(lines) + "\n").encode("ascii"))
        out.write(rec.tobytes())
        out.write(fr.tobytes())


def read_ply(path) -> Dict[str, Optional[np.ndarray]]:
    """What `write_ply` wrote, and only that form: {"vertices" f32[V, 3], "faces" i32[T, 3], "rgb" u8[V, 3] | None, "instance" i32[V] | None,
    "cls" i32[V] | None, "normals" f32[V, 3] | None}."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if end < 0:
        raise ValueError("read_ply: no end_header")
    lines = data[:end].decode("ascii").split("\n")[:-1]
    body = data[end + len(b"end_header\n"):]
    if lines[:2] != ["ply", "format binary_little_endian 1.0"] or not lines[2].startswith("element vertex "):
        raise ValueError("read_ply: not a binary little-endian PLY as write_ply writes it")
    n_v = int(lines[2].split()[2])
    k = 3
    props = []
    while k < len(lines) and lines[k].startswith("property ") and not lines[k].startswith("property list"):
        props.append(tuple(lines[k].split()[1:]))
        k += 1
    names = [p[1] for p in props]
    vd = _vertex_dtype("red" in names, "instance" in names, "class" in names, "nx" in names)
    if props != [(_PLY_TYPE[vd[name].str], name) for name in vd.names]:
        raise ValueError(f"read_ply: vertex properties {props} are not of write_ply's form")
    if lines[k + 1:] != ["property list uchar int vertex_indices"] or not lines[k].startswith("element face "):
        raise ValueError("read_ply: the face element is not of write_ply's form")
    n_f = int(lines[k].split()[2])
    if len(body) != n_v * vd.itemsize + n_f * _FACE.itemsize:
        raise ValueError("read_ply: the body does not have the size the header announces")
    rec = np.frombuffer(body, dtype=vd, count=n_v)
    fr = np.frombuffer(body, dtype=_FACE, count=n_f, offset=n_v * vd.itemsize)
    if n_f and not (fr["n"] == 3).all():
        raise ValueError("read_ply: a face that is not a triangle")
    return {"vertices": np.stack([rec["x"], rec["y"], rec["z"]], 1) if n_v else np.zeros((0, 3), np.float32),
            "faces": np.ascontiguousarray(fr["vertex_indices"]),
            "rgb": np.stack([rec["red"], rec["green"], rec["blue"]], 1) if "red" in names else None,
            "instance": np.ascontiguousarray(rec["instance"]) if "instance" in names else None,
            "cls": np.ascontiguousarray(rec["class"]) if "class" in names else None,
            "normals": np.stack([rec["nx"], rec["ny"], rec["nz"]], 1) if "nx" in names else None}
