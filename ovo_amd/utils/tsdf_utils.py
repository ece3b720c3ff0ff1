"""A fused geometric model on the GPU: `TsdfVolume`, a dense truncated-signed-distance volume integrated from depth frames (`ovo_tsdf_integrate`)
ray-cast back into a depth image from any pose (`ovo_tsdf_raycast`) and turned into a triangle mesh (`ovo_tsdf_mesh_plan` / `ovo_tsdf_mesh_emit`):
csrc/tsdf.hip, csrc/mesh.hip, DESIGN.md sections 17 and 18.  With `color=True` a second array holds the fused colour of every voxel, and the
same three steps carry it along (`ovo_tsdf_integrate_color`, `ovo_tsdf_raycast_color`, `ovo_tsdf_mesh_colors`: section 20).  The gradient of F is the surface
normal: `raycast(normals=True)` and `extract_mesh(normals=True)` return it (`ovo_tsdf_raycast_normals`, `ovo_tsdf_mesh_normals`: section 21) and `shade_normals` makes a lit picture of it.  `TsdfHistory` keeps the depth images a volume was fused from, and
`TsdfVolume.refuse` fuses it again from them at other poses -- what a loop closure needs (section 19).  With `labels=True` a label array (L, C) beside the
volume takes the instance images of the keyframes as votes (`integrate_labels`), follows the map's instance merges (`remap_labels`), and `raycast(labels=True)` /
`extract_mesh(labels=True)` read it back (`ovo_tsdf_integrate_labels`, `ovo_tsdf_labels_remap`, `ovo_tsdf_raycast_labels`, `ovo_tsdf_mesh_labels`: section 22).  `sample(points, ...)` reads all of it -- distance, gradient, colour, instance -- at arbitrary points
(`ovo_tsdf_sample_points`: section 23), and `transform_points` takes points of another frame into the volume's.  `frustum_box`, `rigid_inverse_f32` and `volume_desc` / `camera_desc` are pure numpy / ctypes and need no GPU."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L

Box = Tuple[Tuple[int, int, int], Tuple[int, int, int]]
MAX_HISTORY = 4096                                         # frames a `TsdfHistory` may keep: 4.6 GB of depth images at 456 x 616


def _np(a, dtype) -> np.ndarray:
    return np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, dtype=dtype)


def rigid_inverse_f32(c2w) -> np.ndarray:
    """The rigid inverse of an f32 pose, formed in f64 (R^T, -R^T t) and rounded to f32 once: 4 x 4."""
    m = _np(c2w, np.float32).astype(np.float64)
    out = np.eye(4)
    out[:3, :3] = m[:3, :3].T
    out[:3, 3] = -(m[:3, :3].T @ m[:3, 3])
    return out.astype(np.float32)


def volume_desc(dims: Sequence[int], voxel: float, origin: Sequence[float], trunc: float, max_weight: float) -> L.TsdfVolume:
    nx, ny, nz = (int(d) for d in dims)
    return L.TsdfVolume(nx, ny, nz, float(voxel), (C.c_float * 3)(*(float(o) for o in origin)), float(trunc), float(max_weight))


def camera_desc(K, h: int, w: int, c2w, near: float, far: float) -> L.TsdfCamera:
    K, pose = _np(K, np.float32), np.eye(4, dtype=np.float32)
    pose[:3] = _np(c2w, np.float32)[:3]
    return L.TsdfCamera((C.c_float * 12)(*pose[:3].reshape(12)), (C.c_float * 12)(*rigid_inverse_f32(pose)[:3].reshape(12)), float(K[0, 0]), float(K[1, 1]),
                        float(K[0, 2]), float(K[1, 2]), int(h), int(w), float(near), float(far))


def frustum_box(dims: Sequence[int], voxel: float, origin: Sequence[float], trunc: float, K, h: int, w: int, c2w, near: float,
                far: float) -> Optional[Box]:
    """The index box (lo, hi), half-open, that holds every voxel a frame at `c2w` can update, or None when it misses the volume.  Host, f64: the
    bounding box of the eight corners of the view frustum (the pixel square [-0.5, w - 0.5] x [-0.5, h - 0.5] at depth `near` and at depth
    `far + trunc`: a voxel is updated up to `trunc` behind the deepest surface) and of the camera centre (a voxel in front of `near` is free space
    and is updated too), grown by `trunc` plus one voxel, clipped to the volume."""
    K, pose = _np(K, np.float32).astype(np.float64), _np(c2w, np.float32).astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    f32 = lambda x: float(np.float32(x))
    near, far, trunc, voxel = f32(near), f32(far), f32(trunc), f32(voxel)
    pts = [pose[:3, 3]]
    for z in (near, far + trunc):
        for u in (-0.5, w - 0.5):
            for v in (-0.5, h - 0.5):
                pts.append(pose[:3, :3] @ np.array([(u - cx) / fx * z, (v - cy) / fy * z, z]) + pose[:3, 3])
    pts = np.stack(pts)
    if not np.isfinite(pts).all():
        raise L.OvoHipError("frustum_box: pose or intrinsics not finite")
    grow = trunc + voxel
    org = np.array([f32(o) for o in origin], dtype=np.float64)
    lo = np.floor((pts.min(0) - grow - org) / voxel).astype(np.int64)
    hi = np.ceil((pts.max(0) + grow - org) / voxel).astype(np.int64) + 1
    lo, hi = np.maximum(lo, 0), np.minimum(hi, np.asarray([int(d) for d in dims], dtype=np.int64))
    if (lo >= hi).any():
        return None
    return tuple(int(x) for x in lo), tuple(int(x) for x in hi)


class TsdfVolume:
    """A dense TSDF volume on the device: `vol` is f32[nz, ny, nx, 2] = (F, W), zero = unobserved.  dims = (nx, ny, nz); voxel (i, j, k) sits at
    origin + voxel * (i, j, k) in the frame the poses are given in.  512^3 is 1 GB.  `color=True`: `col` is int16[nz, ny, nx, 4] holding the bits of
    u16 (R, G, B, spare), a channel = level * 256, zero = unobserved; it shares W with `vol`, and every `integrate` then needs `rgb`.  1 GB more.
    `labels=True`: `lab` is int32[nz, ny, nx, 2] = (L, C), L = instance id + 1 (0: none), C the label's confidence count, zero = no label; it is
    voted on by `integrate_labels` alone, never by `integrate`.  1 GB more."""

    def __init__(self, dims: Sequence[int], voxel: float, origin: Sequence[float], trunc: float, max_weight: float = 64, device="cuda",
                 color: bool = False, labels: bool = False) -> None:
        self.dims = tuple(int(d) for d in dims)
        self.voxel, self.trunc, self.max_weight = float(voxel), float(trunc), float(max_weight)
        self.origin = tuple(float(o) for o in origin)
        if len(self.dims) != 3 or len(self.origin) != 3:
            raise L.OvoHipError("TsdfVolume: dims and origin have three entries, x first")
        self.desc = volume_desc(self.dims, self.voxel, self.origin, self.trunc, self.max_weight)
        nbytes = int(L.load().ovo_tsdf_volume_bytes(C.byref(self.desc)))
        if nbytes == 0:
            raise L.OvoHipError(f"TsdfVolume: dims {self.dims} (each 2 .. 4096, at most 2^31 voxels), voxel {voxel}, trunc {trunc} (> 0) or "
                                f"max_weight {max_weight} (>= 1) outside the limits")
        nx, ny, nz = self.dims
        self.vol = torch.zeros((nz, ny, nx, 2), dtype=torch.float32, device=device)
        L.dev(self.vol, torch.float32, "volume")
        self.col = None
        if color:
            if int(L.load().ovo_tsdf_color_bytes(C.byref(self.desc))) != nbytes:
                raise L.OvoHipError("TsdfVolume: the library's colour volume is not 8 bytes a voxel")
            self.col = torch.zeros((nz, ny, nx, 4), dtype=torch.int16, device=device)
        self.lab = None
        if labels:
            if int(L.load().ovo_tsdf_label_bytes(C.byref(self.desc))) != nbytes:
                raise L.OvoHipError("TsdfVolume: the library's label volume is not 8 bytes a voxel")
            self.lab = torch.zeros((nz, ny, nx, 2), dtype=torch.int32, device=device)

    def reset(self) -> None:
        self.vol.zero_()
        if self.col is not None:
            self.col.zero_()
        if getattr(self, "lab", None) is not None:
            self.lab.zero_()

    def _labelled(self, what: str) -> torch.Tensor:
        lab = getattr(self, "lab", None)
        if lab is None:
            raise L.OvoHipError(f"TsdfVolume.{what}: needs a volume made with labels=True")
        return lab

    def integrate_labels(self, depth: torch.Tensor, ins: torch.Tensor, K, c2w, near: float = 0.05, far: float = 10.0, box: Optional[Box] = None,
                         max_count: int = 255) -> Optional[Box]:
        """Votes the instance image ins i32[h, w] (device; negative = no label) of the frame depth f32[h, w] seen from `c2w` into `lab` on the current
        stream (`ovo_tsdf_integrate_labels`): a voxel that `integrate` would update from this depth with a sample f < 1 takes its pixel's id as a vote.
        `vol` is neither read nor written.  `box=None` visits `frustum_box(...)`, as `integrate` does; returns the box (None: nothing queued)."""
        lab = self._labelled("integrate_labels")
        L.dev(depth, torch.float32, "depth")
        L.dev(ins, torch.int32, "ins")
        if depth.dim() != 2 or tuple(ins.shape) != tuple(depth.shape):
            raise L.OvoHipError(f"TsdfVolume.integrate_labels: depth and ins must both be [h, w] (got {tuple(depth.shape)} and {tuple(ins.shape)})")
        h, w = int(depth.shape[0]), int(depth.shape[1])
        if box is None:
            box = self.frustum_box(K, h, w, c2w, near, far)
            if box is None:
                return None
        cam = camera_desc(K, h, w, c2w, near, far)
        lo, hi = (C.c_int32 * 3)(*(int(x) for x in box[0])), (C.c_int32 * 3)(*(int(x) for x in box[1]))
        L.check(L.load().ovo_tsdf_integrate_labels(L.ptr(lab), C.byref(self.desc), L.ptr(depth), L.ptr(ins), C.byref(cam), lo, hi, int(max_count), L.stream()))
        return box

    def remap_labels(self, table: torch.Tensor) -> None:
        """Every voxel's instance id i becomes table[i] (i32[n] on the device: `OVO.last_instance_table`); a negative entry clears the voxel, an id at or
        above n stays.  Counts are kept.  Queued on the current stream (`ovo_tsdf_labels_remap`)."""
        lab = self._labelled("remap_labels")
        L.dev(table, torch.int32, "table")
        if table.dim() != 1:
            raise L.OvoHipError(f"TsdfVolume.remap_labels: table must be i32 [n] (got {tuple(table.shape)})")
        if table.numel() > 0:
            L.check(L.load().ovo_tsdf_labels_remap(L.ptr(lab), C.byref(self.desc), L.ptr(table), int(table.numel()), L.stream()))

    def _rgb(self, rgb, shape, what: str):
        """The colour image of a call, checked against the volume's kind -- u8 on the device for a colour volume, None for a plain one -- and, when
        `shape` is given, against (h, w, 3)."""
        if (rgb is None) != (self.col is None):
            raise L.OvoHipError(f"TsdfVolume.{what}: " + ("a colour volume needs rgb u8[h, w, 3] with every depth image" if rgb is None else
                                                         "rgb given to a volume made without color=True"))
        if rgb is not None and shape is not None:
            L.dev(rgb, torch.uint8, "rgb")
            if tuple(rgb.shape) != tuple(shape):
                raise L.OvoHipError(f"TsdfVolume.{what}: rgb must be {list(shape)} (got {tuple(rgb.shape)})")
        return rgb

    def frustum_box(self, K, h: int, w: int, c2w, near: float, far: float) -> Optional[Box]:
        return frustum_box(self.dims, self.voxel, self.origin, self.trunc, K, h, w, c2w, near, far)

    def integrate(self, depth: torch.Tensor, K, c2w, near: float = 0.05, far: float = 10.0, box: Optional[Box] = None,
                  rgb: Optional[torch.Tensor] = None) -> Optional[Box]:
        """Fuses depth f32[h, w] (device) seen from `c2w` into the volume on the current stream; returns the box it visited (None: the frame's
        frustum misses the volume and nothing was queued).  `box=None` visits `frustum_box(...)`, with the same bits as the whole volume.
        A colour volume takes `rgb` u8[h, w, 3] (device) with it and updates a voxel's colour where it updates (F, W); without it, or with it on a
        plain volume, `OvoHipError`."""
        self._rgb(rgb, None, "integrate")                   # the wrong kind of call is refused before anything else is looked at
        L.dev(depth, torch.float32, "depth")
        if depth.dim() != 2:
            raise L.OvoHipError(f"TsdfVolume.integrate: depth must be [h, w] (got {tuple(depth.shape)})")
        h, w = int(depth.shape[0]), int(depth.shape[1])
        rgb = self._rgb(rgb, (h, w, 3), "integrate")
        if box is None:
            box = self.frustum_box(K, h, w, c2w, near, far)
            if box is None:
                return None
        cam = camera_desc(K, h, w, c2w, near, far)
        lo, hi = (C.c_int32 * 3)(*(int(x) for x in box[0])), (C.c_int32 * 3)(*(int(x) for x in box[1]))
        if rgb is None:
            L.check(L.load().ovo_tsdf_integrate(L.ptr(self.vol), C.byref(self.desc), L.ptr(depth), C.byref(cam), lo, hi, L.stream()))
        else:
            L.check(L.load().ovo_tsdf_integrate_color(L.ptr(self.vol), L.ptr(self.col), C.byref(self.desc), L.ptr(depth), L.ptr(rgb), C.byref(cam), lo, hi,
                                                      L.stream()))
        return box

    def refuse(self, history: "TsdfHistory", K, poses, near: float, far: float) -> None:
        """Fuses the volume again from the frames of `history` at `poses` (one per live entry, oldest first: `history.poses(X)`): `reset()`, then
        one `integrate` (`ovo_tsdf_integrate`, the single-frame kernel) per entry in the history's order.  Queues work and never waits.
        40 us a frame on the device at 456 x 616 into 512^3.  A colour volume fuses its colour again too, from the
        history's `colors` (a history made with color=True).  A label volume then votes every live entry that has labels (`TsdfHistory.set_labels`)
        again, in the history's order, at its new pose: `reset()` has zeroed `lab`."""
        entries = history.entries()
        if len(entries) != len(poses):
            raise L.OvoHipError(f"TsdfVolume.refuse: {len(poses)} poses for {len(entries)} frames of the history")
        color = getattr(self, "col", None) is not None
        if color and getattr(history, "colors", None) is None:
            raise L.OvoHipError("TsdfVolume.refuse: a colour volume needs a TsdfHistory made with color=True")
        self.reset()
        for e, c2w in zip(entries, poses):
            rgb = {"rgb": history.colors[e["slot"]]} if color else {}      # (a plain volume is called as before colour existed: stand-ins take no `rgb`)
            self.integrate(history.depths[e["slot"]], K, c2w, near, far, **rgb)
        if getattr(self, "lab", None) is not None and getattr(history, "labels", None) is not None:
            for e, c2w in zip(entries, poses):
                if history.has_labels[e["slot"]]:
                    self.integrate_labels(history.depths[e["slot"]], history.labels[e["slot"]], K, c2w, near, far)

    def _image(self, given: Optional[torch.Tensor], shape: tuple, dtype: torch.dtype, name: str) -> torch.Tensor:
        """An output image of a ray cast: `given`, checked to be on the device with this shape and dtype, or a new one."""
        out = torch.empty(shape, dtype=dtype, device=self.vol.device) if given is None else given
        L.dev(out, dtype, name)
        if tuple(out.shape) != shape:
            raise L.OvoHipError(f"TsdfVolume.raycast: {name} must be {list(shape)} (got {tuple(out.shape)})")
        return out

    def raycast(self, K, h: int, w: int, c2w, near: float, far: float, dz: Optional[float] = None, out: Optional[torch.Tensor] = None,
                color: bool = False, out_rgb: Optional[torch.Tensor] = None, normals: bool = False, out_normals: Optional[torch.Tensor] = None,
                labels: bool = False, min_count: int = 1, out_ins: Optional[torch.Tensor] = None):
        """The model's depth image f32[h, w] from `c2w` on the current stream (0 = no surface); dz defaults to trunc / 2.  `color=True` (a colour
        volume only): (depth, rgb u8[h, w, 3]), the colour blended at the hit, (0, 0, 0) where there is none; the depth has the same bits.
        `normals=True` appends the normal image f32[h, w, 3] (`ovo_tsdf_raycast_normals`): the unit gradient of F at the hit, in
        the volume's frame, pointing into free space, zeros where there is no surface -- (depth, normals) or (depth, rgb, normals), same bits.
        `labels=True` (a label volume only) appends the instance image i32[h, w] (`ovo_tsdf_raycast_labels`): the id of the voxel nearest
        to the hit if its count is >= min_count, else -1; -1 where there is no surface.  Alone it is one launch, which writes the depth too; beside `color` / `normals` it is a second launch of the march, with the same depth bits."""
        dz = self.trunc / 2 if dz is None else float(dz)
        if labels:
            self._labelled("raycast")
        if out_ins is not None and not labels:
            raise L.OvoHipError("TsdfVolume.raycast: out_ins is only written with labels=True")
        if color and self.col is None:
            raise L.OvoHipError("TsdfVolume.raycast: color=True needs a volume made with color=True")
        if out_rgb is not None and not color:
            raise L.OvoHipError("TsdfVolume.raycast: out_rgb is only written with color=True")
        if out_normals is not None and not normals:
            raise L.OvoHipError("TsdfVolume.raycast: out_normals is only written with normals=True")
        h, w = int(h), int(w)
        out = self._image(out, (h, w), torch.float32, "out")
        cam = camera_desc(K, h, w, c2w, near, far)
        out_normals = self._image(out_normals, (h, w, 3), torch.float32, "out_normals") if normals else None
        out_rgb = self._image(out_rgb, (h, w, 3), torch.uint8, "out_rgb") if color else None
        vol, col, desc, cam, d, c, n = L.ptr(self.vol), L.ptr(self.col), C.byref(self.desc), C.byref(cam), L.ptr(out), L.ptr(out_rgb), L.ptr(out_normals)
        name, args, result = {(False, False): ("ovo_tsdf_raycast", (vol, desc, cam, dz, d), out),
                              (True, False): ("ovo_tsdf_raycast_color", (vol, col, desc, cam, dz, d, c), (out, out_rgb)),
                              (False, True): ("ovo_tsdf_raycast_normals", (vol, None, desc, cam, dz, d, None, n), (out, out_normals)),
                              (True, True): ("ovo_tsdf_raycast_normals", (vol, col, desc, cam, dz, d, c, n), (out, out_rgb, out_normals))}[bool(color), bool(normals)]
        if labels and not (color or normals):               # the label form writes the depth too: one launch
            out_ins = self._image(out_ins, (h, w), torch.int32, "out_ins")
            L.check(L.load().ovo_tsdf_raycast_labels(vol, L.ptr(self.lab), desc, cam, dz, int(min_count), d, L.ptr(out_ins), L.stream()))
            return (out, out_ins)
        L.check(getattr(L.load(), name)(*args, L.stream()))
        if labels:
            out_ins = self._image(out_ins, (h, w), torch.int32, "out_ins")
            L.check(L.load().ovo_tsdf_raycast_labels(vol, L.ptr(self.lab), desc, cam, dz, int(min_count), d, L.ptr(out_ins), L.stream()))
            result += (out_ins,)
        return result

    def extract_mesh(self, box: Optional[Box] = None, min_weight: float = 1.0, colors: bool = False, normals: bool = False, labels: bool = False,
                     min_count: int = 1):
        """The surface inside the index box (None: the whole volume) as a welded triangle mesh on the device: (vertices f32[V, 3] in the volume's
        frame, faces i32[T, 3]); marching tetrahedra over the cells whose eight corners have W >= min_weight (include/ovo_hip.h states the
        contract).  Normals point into free space.  One host wait, for (V, T); V = 0 returns empty tensors and queues no second call.
        `colors=True` (a colour volume only): (vertices, faces, rgb u8[V, 3]), each vertex's colour blended between the two ends of its edge.
        `normals=True` appends vertex normals f32[V, 3] (`ovo_tsdf_mesh_normals`): the unit gradient of F blended between the two
        ends of the vertex's edge, in the volume's frame; the zero vector where the gradient vanishes.  V = 0: an empty [0, 3] tensor and no call.
        `labels=True` (a label volume only) appends vertex instance ids i32[V] (`ovo_tsdf_mesh_labels`): the id of the nearer end of
        the vertex's edge if its count is >= min_count, else the other end's, else -1 -- what `OVO.semantic_mesh(instance=)` takes."""
        if labels:
            self._labelled("extract_mesh")
        if colors and self.col is None:
            raise L.OvoHipError("TsdfVolume.extract_mesh: colors=True needs a volume made with color=True")
        box = ((0, 0, 0), self.dims) if box is None else box
        lo, hi = (C.c_int32 * 3)(*(int(x) for x in box[0])), (C.c_int32 * 3)(*(int(x) for x in box[1]))
        lib, dev = L.load(), self.vol.device
        nbytes = int(lib.ovo_tsdf_mesh_workspace_bytes(C.byref(self.desc), lo, hi))
        if nbytes == 0:
            raise L.OvoHipError(f"TsdfVolume.extract_mesh: the box {box} must lie inside the volume {self.dims} and span at least 2 voxels on every axis")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        L.check(lib.ovo_tsdf_mesh_plan(L.ptr(self.vol), C.byref(self.desc), lo, hi, float(min_weight), L.ptr(ws), nbytes, L.ptr(counts), L.stream()))
        V, T = (int(x) for x in counts.tolist())
        if max(V, T) > 2**31 - 1:
            raise L.OvoHipError(f"TsdfVolume.extract_mesh: {V} vertices and {T} triangles do not fit 32-bit indices -- extract box by box")
        vertices, faces = torch.empty((V, 3), dtype=torch.float32, device=dev), torch.empty((T, 3), dtype=torch.int32, device=dev)
        if V > 0:
            L.check(lib.ovo_tsdf_mesh_emit(L.ptr(self.vol), C.byref(self.desc), lo, hi, float(min_weight), L.ptr(ws), nbytes, L.ptr(vertices), L.ptr(faces),
                                           V, T, L.stream()))
        result = (vertices, faces)
        if colors:
            rgb = torch.empty((V, 3), dtype=torch.uint8, device=dev)
            if V > 0:
                L.check(lib.ovo_tsdf_mesh_colors(L.ptr(self.vol), L.ptr(self.col), C.byref(self.desc), lo, hi, float(min_weight), L.ptr(ws), nbytes, L.ptr(rgb), V,
                                                 L.stream()))
            result += (rgb,)
        if normals:
            nrm = torch.empty((V, 3), dtype=torch.float32, device=dev)
            if V > 0:
                L.check(lib.ovo_tsdf_mesh_normals(L.ptr(self.vol), C.byref(self.desc), lo, hi, float(min_weight), L.ptr(ws), nbytes, L.ptr(nrm), V, L.stream()))
            result += (nrm,)
        if labels:
            ins = torch.empty((V,), dtype=torch.int32, device=dev)
            if V > 0:
                L.check(lib.ovo_tsdf_mesh_labels(L.ptr(self.vol), L.ptr(self.lab), C.byref(self.desc), lo, hi, float(min_weight), L.ptr(ws), nbytes, int(min_count),
                                                 L.ptr(ins), V, L.stream()))
            result += (ins,)
        return result

    def sample(self, points: torch.Tensor, transform=None, normals: bool = False, colors: bool = False, labels: bool = False, min_count: int = 1,
               label_mode: str = "nearest"):
        """What the model says at points f32[n, 3] (device, in the volume's frame; `transform` X 4 x 4: `transform_points(points, X)` first) on the
        current stream, never waiting (`ovo_tsdf_sample_points`): F f32[n], the trilinear blend of the eight voxels around a point, 2.0
        where the point lies outside the volume or one of the eight is unobserved.  The outputs asked for follow in `extract_mesh`'s order:
        `colors=True` (a colour volume only) rgb u8[n, 3]; `normals=True` the unit gradient f32[n, 3] in the volume's frame; `labels=True` (a label volume
        only) instance ids i32[n] -- label_mode "nearest": the nearest voxel's id if its count is >= min_count, else -1 (the ray cast's rule);
        "vote": the id with the largest sum of counts over the eight voxels with a count >= min_count, ties to the nearest voxel's id, then to
        the smallest.  A point that is not seen answers (0, 0, 0), three zeros and -1."""
        if label_mode not in LABEL_MODES:
            raise L.OvoHipError(f"TsdfVolume.sample: label_mode must be one of {sorted(LABEL_MODES)} (got {label_mode!r})")
        if labels:
            self._labelled("sample")
        if colors and self.col is None:
            raise L.OvoHipError("TsdfVolume.sample: colors=True needs a volume made with color=True")
        if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
            raise L.OvoHipError(f"TsdfVolume.sample: points must be f32 [n, 3] (got {tuple(getattr(points, 'shape', ()))})")
        L.dev(points, torch.float32, "points")
        if transform is not None:
            points = transform_points(points, transform)
        n, dev = int(points.shape[0]), points.device
        f = torch.empty((n,), dtype=torch.float32, device=dev)
        rgb = torch.empty((n, 3), dtype=torch.uint8, device=dev) if colors else None
        nrm = torch.empty((n, 3), dtype=torch.float32, device=dev) if normals else None
        ins = torch.empty((n,), dtype=torch.int32, device=dev) if labels else None
        if n > 0:                                            # (no point: empty tensors have no address, and there is nothing to queue)
            L.check(L.load().ovo_tsdf_sample_points(L.ptr(self.vol), L.ptr(self.col) if colors else None, L.ptr(self.lab) if labels else None, C.byref(self.desc),
                                                    L.ptr(points), n, LABEL_MODES[label_mode], int(min_count), L.ptr(f), L.ptr(nrm), L.ptr(rgb), L.ptr(ins),
                                                    L.stream()))
        extra = tuple(x for x in (rgb, nrm, ins) if x is not None)
        return (f,) + extra if extra else f


LABEL_MODES = {"nearest": 0, "vote": 1}                    # ovo_tsdf_sample_points' label_mode


def transform_points(points: torch.Tensor, X) -> torch.Tensor:
    """(points.double() @ R.T + t).float() on the points' device for a 4 x 4 X = [R t; 0 1]: the product and the sum in f64, one rounding to f32.
    The one documented way from world-frame points (the map, a GT mesh under world_ref) into a volume's frame: `TsdfVolume.sample(transform=X)` is
    exactly `sample(transform_points(points, X))`."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise L.OvoHipError(f"transform_points: points must be [n, 3] (got {tuple(getattr(points, 'shape', ()))})")
    X = _np(X, np.float64)                                 # (a host X: its twelve numbers travel as kernel arguments, and nothing waits)
    if X.shape != (4, 4):
        raise L.OvoHipError(f"transform_points: X must be 4 x 4 (got {X.shape})")
    p = points.double()
    # the product row by row, ((p0 R[a, 0] + p1 R[a, 1]) + p2 R[a, 2]) + t[a]: one f64 operation at a time, so that numpy restates every bit
    cols = [((p[:, 0] * float(X[a, 0]) + p[:, 1] * float(X[a, 1])) + p[:, 2] * float(X[a, 2])) + float(X[a, 3]) for a in range(3)]
    return torch.stack(cols, 1).float().contiguous()


class TsdfHistory:
    """The depth images a volume was fused from, so that it can be fused again from corrected poses (`TsdfVolume.refuse`): a ring `depths`
    f32[capacity, h, w] on the device -- f32, the exact bits that were fused live -- and, on the host, each entry's time stamp, the index `kf`
    of the keyframe it hangs on and `rel` = inv(kf_c2w) @ c2w in f64 (the exact identity for a keyframe itself).  When the ring is full the
    oldest entry is overwritten: after the next re-fusion the model no longer holds that frame.  1.12 MB a frame at 456 x 616, 1.15 GB at 1024.
    `color=True`: a ring `colors` u8[capacity, h, w, 3] beside it, slot for slot (0.84 MB a frame more), and `add` needs `rgb`.
    `labels=True`: a ring `labels` i32[capacity, h, w] beside it (1.12 MB a frame more) and a flag per slot, `has_labels`: `add` clears the slot's
    flag, `set_labels(slot, ins)` fills the slot after the fact -- instance images exist for keyframes only, and later than the frame."""

    def __init__(self, capacity: int, h: int, w: int, device="cuda", color: bool = False, labels: bool = False) -> None:
        self.capacity, self.h, self.w = int(capacity), int(h), int(w)
        if not 1 <= self.capacity <= MAX_HISTORY:
            raise ValueError(f"TsdfHistory: capacity must be 1 .. {MAX_HISTORY}")
        self.depths = torch.zeros((self.capacity, self.h, self.w), dtype=torch.float32, device=device)
        self.colors = torch.zeros((self.capacity, self.h, self.w, 3), dtype=torch.uint8, device=device) if color else None
        self.labels = torch.zeros((self.capacity, self.h, self.w), dtype=torch.int32, device=device) if labels else None
        self.has_labels = [False] * self.capacity
        self._entries: list = []                           # live entries, oldest first
        self._next = 0                                     # the slot the next frame is written to

    def __len__(self) -> int:
        return len(self._entries)

    def add(self, depth: torch.Tensor, t, kf: int, rel, rgb: Optional[torch.Tensor] = None) -> int:
        """Copies depth f32[h, w] (and, in a colour history, rgb u8[h, w, 3]) into the ring on the current stream (device to device, no host
        wait); returns its slot."""
        if tuple(depth.shape) != (self.h, self.w) or depth.dtype != torch.float32:
            raise ValueError(f"TsdfHistory.add: depth must be f32 [{self.h}, {self.w}] (got {depth.dtype} {tuple(depth.shape)})")
        if (rgb is None) != (self.colors is None):
            raise ValueError("TsdfHistory.add: rgb goes with a history made with color=True, and only with one")
        if rgb is not None and (tuple(rgb.shape) != (self.h, self.w, 3) or rgb.dtype != torch.uint8):
            raise ValueError(f"TsdfHistory.add: rgb must be u8 [{self.h}, {self.w}, 3] (got {rgb.dtype} {tuple(rgb.shape)})")
        slot = self._next
        self.depths[slot].copy_(depth)
        if rgb is not None:
            self.colors[slot].copy_(rgb)
        self.has_labels[slot] = False                      # whatever instance image the slot held belonged to the frame it held
        if len(self._entries) == self.capacity:
            self._entries.pop(0)                           # it held `slot`
        self._entries.append({"slot": slot, "t": t, "kf": int(kf), "rel": np.array(rel, dtype=np.float64)})
        self._next = (slot + 1) % self.capacity
        return slot

    def set_labels(self, slot: int, ins: torch.Tensor) -> None:
        """Copies ins i32[h, w] into slot `slot` (what `add` returned for the frame) on the current stream and marks the slot as labelled."""
        if self.labels is None:
            raise ValueError("TsdfHistory.set_labels: needs a history made with labels=True")
        if not any(e["slot"] == int(slot) for e in self._entries):
            raise ValueError(f"TsdfHistory.set_labels: slot {slot} holds no live frame")
        if tuple(ins.shape) != (self.h, self.w) or ins.dtype != torch.int32:
            raise ValueError(f"TsdfHistory.set_labels: ins must be i32 [{self.h}, {self.w}] (got {ins.dtype} {tuple(ins.shape)})")
        self.labels[int(slot)].copy_(ins)
        self.has_labels[int(slot)] = True

    def entries(self) -> list:
        return list(self._entries)

    def poses(self, X) -> list:
        """The live entries' poses under the keyframe poses X (f64, by keyframe index): X[kf] @ rel in f64, rounded to f32 once."""
        return [(np.asarray(X[e["kf"]], dtype=np.float64) @ e["rel"]).astype(np.float32) for e in self._entries]


def shade_normals(normals: torch.Tensor, K, c2w, rgb: Optional[torch.Tensor] = None, ambient: float = 0.2) -> torch.Tensor:
    """A head-light Lambert picture u8[h, w, 3] of a normal image f32[h, w, 3] (`TsdfVolume.raycast(normals=True)`, `IcpTracker.render_model(normals=True)`)
    seen from `c2w` with intrinsics K: with d the unit ray of the pixel in the normals' frame, i = ambient + (1 - ambient) * clamp(-n . d, 0, 1); the
    picture is rint(255 i) in all three channels, or rint(i * rgb) with `rgb` u8[h, w, 3]; a pixel whose normal is the zero vector is (0, 0, 0).
    Plain torch on the normals' device, f32: a viewer's step, not a hot path."""
    if normals.dim() != 3 or normals.shape[2] != 3 or normals.dtype != torch.float32:
        raise ValueError(f"shade_normals: normals must be f32 [h, w, 3] (got {normals.dtype} {tuple(normals.shape)})")
    if rgb is not None and (tuple(rgb.shape) != tuple(normals.shape) or rgb.dtype != torch.uint8):
        raise ValueError(f"shade_normals: rgb must be u8 {list(normals.shape)} (got {rgb.dtype} {tuple(rgb.shape)})")
    if not 0.0 <= float(ambient) <= 1.0:
        raise ValueError("shade_normals: ambient must lie in [0, 1]")
    h, w = int(normals.shape[0]), int(normals.shape[1])
    dev = normals.device
    K, pose = _np(K, np.float32), _np(c2w, np.float32)
    u = (torch.arange(w, dtype=torch.float32, device=dev) - float(K[0, 2])) / float(K[0, 0])
    v = (torch.arange(h, dtype=torch.float32, device=dev) - float(K[1, 2])) / float(K[1, 1])
    dc = torch.stack([u[None, :].expand(h, w), v[:, None].expand(h, w), torch.ones((h, w), dtype=torch.float32, device=dev)], -1)
    d = dc @ torch.from_numpy(np.ascontiguousarray(pose[:3, :3])).to(dev).T
    d = d / d.norm(dim=-1, keepdim=True)
    i = float(ambient) + (1.0 - float(ambient)) * (-(normals * d).sum(-1)).clamp(0.0, 1.0)
    base = torch.full((h, w, 3), 255.0, dtype=torch.float32, device=dev) if rgb is None else rgb.to(torch.float32)
    out = torch.round(i[..., None] * base).clamp(0.0, 255.0)
    lit = (normals != 0).any(-1, keepdim=True)
    return torch.where(lit, out, torch.zeros_like(out)).to(torch.uint8)


def march_steps(near: float, far: float, dz: float) -> int:
    """kmax of a ray cast: ceil((far - near) / dz) of the f32 values in f64."""
    return int(math.ceil((float(np.float32(far)) - float(np.float32(near))) / float(np.float32(dz))))
