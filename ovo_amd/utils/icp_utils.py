"""Point-to-plane ICP between two depth frames: `ovo_icp_prepare` / `ovo_icp_align` (csrc/icp.hip) and the host-side
arithmetic around them.  The host helpers (`se3_exp`, `level_intrinsics`, `keyframe_decision`) are pure numpy and need no GPU."""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L

OK, LOST = 2, 3                                            # `state` of a result (ORB-SLAM3's TrackingState values: the tracker seam's convention)
RESULT_WORDS = 40                                          # ovo_hip.h: the pinned result block, 8-byte words
MAX_LEVELS = 4


def se3_exp(xi) -> np.ndarray:
    """exp of a twist (rotation | translation) as a 4 x 4 f64 matrix: Rodrigues for the rotation, the SE(3) V matrix for the translation."""
    xi = np.asarray(xi, dtype=np.float64).reshape(6)
    w, v = xi[:3], xi[3:]
    th2 = float(w @ w)
    th = math.sqrt(th2)
    if th < 1e-4:
        a, b, c = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        a, b, c = math.sin(th) / th, (1.0 - math.cos(th)) / th2, (th - math.sin(th)) / (th2 * th)
    k = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    k2 = np.outer(w, w) - th2 * np.eye(3)
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + a * k + b * k2
    out[:3, 3] = (np.eye(3) + b * k + c * k2) @ v
    return out


def level_intrinsics(K, levels: int) -> np.ndarray:
    """(fx, fy, cx, cy) of every pyramid level as f32[levels, 4]: halved focal lengths, principal point (c + 0.5) / 2 - 0.5, carried in f64 from
    the f32 level-0 values and rounded to f32 once per level."""
    K = np.asarray(K, dtype=np.float32)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    out = np.zeros((levels, 4), dtype=np.float32)
    for l in range(levels):
        out[l] = (fx, fy, cx, cy)
        fx, fy, cx, cy = fx * 0.5, fy * 0.5, (cx + 0.5) * 0.5 - 0.5, (cy + 0.5) * 0.5 - 0.5
    return out


def level_shapes(h: int, w: int, levels: int):
    return [(h >> l, w >> l) for l in range(levels)]


def keyframe_decision(T, pairs: int, pixels: int, kf_translation: float, kf_rotation_deg: float, kf_min_overlap: float) -> bool:
    """Whether a frame at relative pose `T` (keyframe camera <- frame camera) with `pairs` associated pixels out of `pixels` becomes the new
    keyframe: its translation or rotation to the keyframe EXCEEDS the threshold, or the pair fraction is UNDER kf_min_overlap."""
    T = np.asarray(T, dtype=np.float64)
    translation = float(np.linalg.norm(T[:3, 3]))
    cos = min(1.0, max(-1.0, (float(np.trace(T[:3, :3])) - 1.0) * 0.5))
    rotation = math.degrees(math.acos(cos))
    return translation > kf_translation or rotation > kf_rotation_deg or pairs < kf_min_overlap * pixels


class Frame:
    """A prepared frame: the pyramid buffer (u8 on the device) and the descriptor `ovo_icp_align` reads it with."""

    def __init__(self, pyramid: torch.Tensor, desc: L.IcpFrame) -> None:
        self.pyramid, self.desc = pyramid, desc
        self.h, self.w, self.levels = int(desc.h), int(desc.w), int(desc.levels)

    def level(self, l: int) -> torch.Tensor:
        """Level l as f32[h_l, w_l, 8]: vertex xyz, depth flag, normal xyz, normal flag (the flags are bit patterns: view them as int32)."""
        shapes = level_shapes(self.h, self.w, self.levels)
        first = sum(a * b for a, b in shapes[:l]) * 32
        hl, wl = shapes[l]
        return self.pyramid[first:first + hl * wl * 32].view(torch.float32).view(hl, wl, 8)


def frame_desc(h: int, w: int, K, levels: int, max_depth: float, depth_jump: float) -> L.IcpFrame:
    K = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float32)
    return L.IcpFrame(int(h), int(w), int(levels), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), float(max_depth), float(depth_jump))


def prepare_frame(depth: torch.Tensor, K, levels: int = 3, max_depth: float = 10.0, depth_jump: float = 0.1, out: Optional[torch.Tensor] = None) -> Frame:
    """`ovo_icp_prepare` on the current stream: depth f32[h,w] on the device -> a `Frame`.  `out`: a pyramid buffer to write into (u8, large enough)."""
    lib = L.load()
    L.dev(depth, torch.float32, "depth")
    if depth.dim() != 2:
        raise L.OvoHipError(f"prepare_frame: depth must be [h, w] (got {tuple(depth.shape)})")
    h, w = int(depth.shape[0]), int(depth.shape[1])
    desc = frame_desc(h, w, K, levels, max_depth, depth_jump)
    nbytes = int(lib.ovo_icp_pyramid_bytes(h, w, int(levels)))
    if out is None:
        out = torch.empty(max(nbytes, 32), dtype=torch.uint8, device=depth.device)
    L.check(lib.ovo_icp_prepare(L.ptr(depth), C.byref(desc), L.ptr(out), out.numel(), L.stream()))
    return Frame(out, desc)


def align_desc(iters: Sequence[int], dist_th: float, normal_th_deg: float, min_pairs: int, min_pivot_ratio: float, seq: int) -> L.IcpAlign:
    its = [int(i) for i in iters]
    if not 1 <= len(its) <= MAX_LEVELS:
        raise L.OvoHipError(f"align: iters must name 1 .. {MAX_LEVELS} levels, coarse to fine (got {len(its)})")
    return L.IcpAlign((C.c_int32 * 4)(*(its + [0] * (4 - len(its)))), float(dist_th), float(np.float32(math.cos(math.radians(normal_th_deg)))),
                      int(min_pairs), float(min_pivot_ratio), int(seq))


def decode_result(block: np.ndarray) -> Dict[str, Any]:
    """The pinned result block (int64[40]) as the dict `align` returns."""
    block = np.array(block, dtype=np.int64)                # a copy: the slot is reused
    T = np.eye(4, dtype=np.float32)
    T[:3] = block[34:40].view(np.float32).reshape(3, 4)
    sums = block[5:34].view(np.float64).copy()
    pairs = int(block[2])
    return {"T": T, "state": int(block[1]), "pairs": pairs, "iterations": int(block[3]), "sum_r2": float(block[4:5].view(np.float64)[0]),
            "rms": math.sqrt(float(block[4:5].view(np.float64)[0]) / pairs) if pairs > 0 else 0.0, "sums": sums}


class Aligner:
    """What a sequence of `ovo_icp_align` calls shares: the device pose T (12 f32), the workspace and the ring of pinned result blocks."""

    def __init__(self, device) -> None:
        self.device = torch.device(device)
        self.T = torch.zeros(12, dtype=torch.float32, device=self.device)
        self.ws = torch.empty(int(L.load().ovo_icp_align_workspace_bytes()), dtype=torch.uint8, device=self.device)
        self.ring = L.PinnedRing(RESULT_WORDS, np.int64, slots=8)

    def set_pose(self, T) -> None:
        top = np.ascontiguousarray(np.asarray(T.detach().cpu() if isinstance(T, torch.Tensor) else T, dtype=np.float32)[:3]).reshape(12)
        self.T.copy_(torch.from_numpy(top))

    def queue(self, ref: Frame, cur: Frame, iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio) -> int:
        """Queues one alignment on the current stream, T read and advanced in place; returns the sequence number `wait` takes."""
        if len(iters) != ref.levels:
            raise L.OvoHipError(f"align: {len(iters)} entries in iters for {ref.levels} levels")
        seq, slot = self.ring.next()
        desc = align_desc(iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio, seq)
        L.check(L.load().ovo_icp_align(L.ptr(ref.pyramid), C.byref(ref.desc), L.ptr(cur.pyramid), C.byref(cur.desc), C.byref(desc), L.ptr(self.T),
                                       C.c_void_p(slot), L.ptr(self.ws), self.ws.numel(), L.stream()))
        return seq

    def wait(self, seq: int) -> Dict[str, Any]:
        return decode_result(self.ring.wait(seq))


def align(ref: Frame, cur: Frame, T0, iters=(10, 5, 4), dist_th: float = 0.1, normal_th_deg: float = 30.0, min_pairs: int = 1,
          min_pivot_ratio: float = 1e-6, aligner: Optional[Aligner] = None) -> Dict[str, Any]:
    """One alignment, start to result: T0 (4 x 4, reference camera <- current camera) -> {"T": 4 x 4 f32 on the host, "state": OK / LOST,
    "pairs", "rms", "sums" (the 29 f64 sums of the last executed iteration), "iterations"}.  One host wait."""
    aligner = aligner or Aligner(ref.pyramid.device)
    aligner.set_pose(T0)
    return aligner.wait(aligner.queue(ref, cur, iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio))
