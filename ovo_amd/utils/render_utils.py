"""The map seen from a camera pose: a headless view renderer over libovo_hip.so (csrc/render.hip).

The reference's only way to look at a map is its Open3D visualiser (ovo/entities/visualizer.py), GUI code that stays out of scope; what it
draws is available here as images.  `render_rows` is the inverse of the tracking pass: it projects the map into a view that has no depth
image and finds the nearest point of every pixel itself (a z-buffered splat, one 64-bit atomic minimum per covered pixel); `resolve` turns the
row image into per-point and per-instance pictures (instance ids, colours, the dense class map, classes / query heat per instance).  The
contract -- which points contribute, which one a pixel takes -- is written out in include/ovo_hip.h; the result is a pure function of the
inputs, bit-identical from launch to launch.  No CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import torch

from .. import _lib as L
from .geometry_utils import _cpu32


def make_view(c2w, K, h: int, w: int, radius: int = 1, near: float = 0.05, far: float = float("inf")) -> L.View:
    """ovo_view_t of a camera pose.  `w2c` is inverted on the CPU in f32 with `torch.linalg.inv`, the way the tracking path builds
    `ovo_camera_t.w2c` (geometry_utils._build_cameras): a view at a keyframe's pose uses that keyframe's own matrix."""
    view = L.View()
    view.w2c[:] = torch.linalg.inv(_cpu32(c2w).contiguous()).reshape(-1).tolist()
    view.K[:] = _cpu32(K).reshape(-1).tolist()
    view.near, view.far = float(near), float(far)
    view.h, view.w, view.radius = int(h), int(w), int(radius)
    return view


def render_rows(points_3d: torch.Tensor, view: L.View) -> Tuple[torch.Tensor, torch.Tensor]:
    """(row i32[h,w], depth f32[h,w]) of the map points f32[n,3] seen through `view`, on the current stream: per pixel the nearest covering point
    (-1: none) and its camera-frame depth (0: none).  Only the first `points_3d.shape[0]` rows are read: pass the map's live prefix, not its
    capacity buffer."""
    pts = L.dev(points_3d, torch.float32, "points_3d")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise L.OvoHipError(f"points_3d must be [n, 3] (got {tuple(pts.shape)})")
    lib = L.load()
    h, w = int(view.h), int(view.w)
    nb = int(lib.ovo_render_workspace_bytes(h, w))
    if nb == 0:
        raise L.OvoHipError(f"render_rows: image size {h} x {w}")
    row = torch.empty((h, w), dtype=torch.int32, device=pts.device)
    depth = torch.empty((h, w), dtype=torch.float32, device=pts.device)
    ws = L.workspace(nb, pts.device)
    L.check(lib.ovo_render_points(L.ptr(pts), pts.shape[0], C.byref(view), L.ptr(row), L.ptr(depth), L.ptr(ws), nb, L.stream()))
    return row, depth


def resolve(row: torch.Tensor, *, point_ins: Optional[torch.Tensor] = None, point_rgb: Optional[torch.Tensor] = None,
            background: Sequence[int] = (0, 0, 0), point_cls: Optional[torch.Tensor] = None, point_conf: Optional[torch.Tensor] = None,
            ins_cls: Optional[torch.Tensor] = None, ins_val: Optional[torch.Tensor] = None, fill_cls: int = -1,
            fill_val: float = 0.0) -> Dict[str, torch.Tensor]:
    """A row image i32[h,w] -> the images of the sources given, one launch, pure gather:
      point_ins i32[n]     -> "ins" i32[h,w], -1 on empty pixels
      point_rgb u8[n,3]    -> "rgb" u8[h,w,3], `background` on empty pixels
      point_cls i64[n]     -> "cls" i64[h,w]      point_conf f32[n] -> "conf" f32[h,w]         (the dense map's resident arrays)
      ins_cls i64[n_slots] -> "ins_cls" i64[h,w]  ins_val f32[n_slots] -> "val" f32[h,w]       (tables over instance ids; need point_ins)
    Empty pixels, unassigned points (id < 0) and ids >= n_slots get `fill_cls` / `fill_val`.  Rows at or past the shortest per-point source
    count as empty pixels."""
    row = L.dev(row, torch.int32, "row")
    if row.dim() != 2:
        raise L.OvoHipError(f"row must be [h, w] (got {tuple(row.shape)})")
    h, w = row.shape
    dev = row.device
    per_point = {"point_ins": (point_ins, torch.int32), "point_rgb": (point_rgb, torch.uint8), "point_cls": (point_cls, torch.int64),
                 "point_conf": (point_conf, torch.float32)}
    per_ins = {"ins_cls": (ins_cls, torch.int64), "ins_val": (ins_val, torch.float32)}
    src = {}
    for name, (t, dtype) in {**per_point, **per_ins}.items():
        if t is not None:
            src[name] = L.dev(t.reshape(-1, 3) if name == "point_rgb" else t.reshape(-1), dtype, name)
            if src[name].device != dev:
                raise L.OvoHipError(f"{name} on {src[name].device}, row on {dev}")
    if ("ins_cls" in src or "ins_val" in src) and "point_ins" not in src:
        raise L.OvoHipError("resolve: a per-instance table needs point_ins")
    if "ins_cls" in src and "ins_val" in src and src["ins_cls"].shape[0] != src["ins_val"].shape[0]:
        raise L.OvoHipError("resolve: ins_cls and ins_val cover different numbers of instance ids")
    n = min([src[k].shape[0] for k in per_point if k in src], default=0)
    n_slots = min([src[k].shape[0] for k in per_ins if k in src], default=0)
    shapes = {"point_ins": ("ins", (h, w), torch.int32), "point_rgb": ("rgb", (h, w, 3), torch.uint8), "point_cls": ("cls", (h, w), torch.int64),
              "point_conf": ("conf", (h, w), torch.float32), "ins_cls": ("ins_cls", (h, w), torch.int64), "ins_val": ("val", (h, w), torch.float32)}
    out = {key: torch.empty(shape, dtype=dtype, device=dev) for name, (key, shape, dtype) in shapes.items() if name in src}
    r, g, b = (int(c) & 255 for c in background)
    L.check(L.load().ovo_render_resolve(L.ptr(row), h, w, n, L.ptr(src.get("point_ins")), L.ptr(src.get("point_rgb")), r | g << 8 | b << 16,
                                        L.ptr(src.get("point_cls")), L.ptr(src.get("point_conf")), L.ptr(src.get("ins_cls")),
                                        L.ptr(src.get("ins_val")), n_slots, int(fill_cls), float(fill_val), L.ptr(out.get("ins")),
                                        L.ptr(out.get("rgb")), L.ptr(out.get("cls")), L.ptr(out.get("conf")), L.ptr(out.get("ins_cls")),
                                        L.ptr(out.get("val")), L.stream()))
    return out


def render_boxes(corners: torch.Tensor, box_id: torch.Tensor, view: L.View, half_width: float = 1.0, scene_depth: Optional[torch.Tensor] = None,
                 depth_slack: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(box i32[h,w], box_depth f32[h,w]) of the 12 edges of every box, drawn `2 half_width` pixels wide into `view` (`ovo_render_boxes`; its
    `radius` and `far` are not used): per pixel the `box_id` of the nearest visible edge (-1: none) and its depth (0: none).  corners
    f32[m,8,3] in the world, in the order of `instance_geometry.box_corners`; box_id i32[m].  `scene_depth` f32[h,w] (the "depth" of
    `render_rows` through the same view): an edge is hidden where it lies more than `depth_slack` behind a non-empty scene pixel."""
    corners = L.dev(corners, torch.float32, "corners")
    if corners.dim() != 3 or tuple(corners.shape[1:]) != (8, 3):
        raise L.OvoHipError(f"corners must be [m, 8, 3] (got {tuple(corners.shape)})")
    box_id = L.dev(box_id.reshape(-1), torch.int32, "box_id")
    m, dev = corners.shape[0], corners.device
    if box_id.shape[0] != m or box_id.device != dev:
        raise L.OvoHipError(f"box_id: {box_id.shape[0]} ids on {box_id.device} for {m} boxes on {dev}")
    h, w = int(view.h), int(view.w)
    if scene_depth is not None:
        scene_depth = L.dev(scene_depth, torch.float32, "scene_depth")
        if tuple(scene_depth.shape) != (h, w) or scene_depth.device != dev:
            raise L.OvoHipError(f"scene_depth must be [{h}, {w}] on {dev} (got {tuple(scene_depth.shape)} on {scene_depth.device})")
    lib = L.load()
    nb = int(lib.ovo_render_boxes_workspace_bytes(m))
    out_id = torch.empty((max(h, 0), max(w, 0)), dtype=torch.int32, device=dev)
    out_depth = torch.empty((max(h, 0), max(w, 0)), dtype=torch.float32, device=dev)
    ws = L.workspace(nb, dev) if nb else None
    L.check(lib.ovo_render_boxes(L.ptr(corners), L.ptr(box_id), m, C.byref(view), float(half_width), L.ptr(scene_depth), float(depth_slack),
                                 L.ptr(out_id), L.ptr(out_depth), L.ptr(ws), nb, L.stream()))
    return out_id, out_depth
