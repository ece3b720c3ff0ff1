"""Point-to-plane ICP between two depth frames: `ovo_icp_prepare` / `ovo_icp_align` (csrc/icp.hip) and the host-side
arithmetic around them, and `ovo_icp_align_batch` with the loop-closing rules that `LoopCloser` (slam/loop_closer.py) applies for
`IcpTracker(close_loops=True)`.  `prepare_frame`, `Aligner` and `BatchAligner` are what the tracker's frame loop reaches on the
device; it looks them up here when it calls them.  The host
helpers (`se3_exp`, `se3_log`, `level_intrinsics`, `keyframe_decision`, `pose_offset`, `select_candidates`, `accept_loop`, `information`) are pure
numpy and need no GPU."""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L

OK, LOST = 2, 3                                            # `state` of a result (ORB-SLAM3's TrackingState values: the tracker seam's convention)
RESULT_WORDS = 40                                          # ovo_hip.h: the pinned result block, 8-byte words
MAX_LEVELS = 4
MAX_BATCH = 16                                             # ovo_hip.h: OVO_ICP_MAX_BATCH


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


def se3_log(T) -> np.ndarray:
    """The twist (rotation | translation) of a 4 x 4 rigid transform, the inverse of `se3_exp`, in f64; for rotation angles below pi (at pi the
    axis is not determined by R - R^T; the residuals of a pose graph are nowhere near it)."""
    T = np.asarray(T, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])      # sin(th) * axis
    s, c = float(np.linalg.norm(v)), 0.5 * (float(np.trace(R)) - 1.0)
    th = math.atan2(s, c)
    th2 = th * th
    w = v * (1.0 + th2 / 6.0) if th < 1e-4 else v * (th / s)      # th / sin(th)
    if th < 1e-2:                                          # (1 - A / 2B) / th^2 cancels: its series, the next term th^6 / 1 209 600
        d = 1.0 / 12.0 + th2 / 720.0 + th2 * th2 / 30240.0
    else:
        d = (1.0 - 0.5 * th / math.tan(0.5 * th)) / th2    # A / 2B = (th / 2) cot(th / 2), from th itself: 1 - cos of the matrix's trace is not used
    k = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    k2 = np.outer(w, w) - float(w @ w) * np.eye(3)
    return np.concatenate([w, (np.eye(3) - 0.5 * k + d * k2) @ t])      # V^-1 t


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


def pose_offset(T) -> Tuple[float, float]:
    """(translation in metres, rotation angle in degrees) of a 4 x 4 rigid transform."""
    T = np.asarray(T, dtype=np.float64)
    v = 0.5 * np.array([T[2, 1] - T[1, 2], T[0, 2] - T[2, 0], T[1, 0] - T[0, 1]])
    return float(np.linalg.norm(T[:3, 3])), math.degrees(math.atan2(float(np.linalg.norm(v)), 0.5 * (float(np.trace(T[:3, :3])) - 1.0)))


def rigid_inverse(T) -> np.ndarray:
    T = np.asarray(T, dtype=np.float64)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def select_candidates(poses: Sequence[np.ndarray], n: int, available: Sequence[int], min_gap: int, radius: float, angle_deg: float,
                      max_candidates: int) -> List[Tuple[int, np.ndarray]]:
    """The old keyframes a new keyframe n is verified against: of the `available` ones (those whose pyramid is kept) with k <= n - min_gap, those
    whose guess G_k = X_k^-1 X_n has a translation <= radius and a rotation <= angle_deg; the max_candidates with the smallest translation, ties
    to the lower index.  Returns [(k, G_k)] in that order; `poses[k]` is X_k (4 x 4 f64, keyframe camera k -> the first camera)."""
    found = []
    for k in sorted(int(k) for k in available):
        if k > n - min_gap:
            continue
        G = rigid_inverse(poses[k]) @ np.asarray(poses[n], dtype=np.float64)
        t, a = pose_offset(G)
        if t <= radius and a <= angle_deg:
            found.append((t, k, G))
    found.sort(key=lambda e: (e[0], e[1]))
    return [(k, G) for _, k, G in found[:max_candidates]]


def extend_by_appearance(chosen: List[Tuple[int, np.ndarray]], matches: Sequence[Tuple[int, int]], available: Sequence[int], n: int, min_gap: int,
                         max_distance: float, max_candidates: int) -> List[Tuple[int, np.ndarray]]:
    """Loop candidates by appearance: `chosen` (what `select_candidates` gave, or nothing) extended by the fern `matches`
    [(k, block distance)], taken in the order given -- (distance, k) -- while slots are free: an `available` keyframe
    k <= n - min_gap with distance <= max_distance that is not chosen already, with the identity as its guess."""
    out, taken, kept = list(chosen), {k for k, _ in chosen}, {int(k) for k in available}
    for k, d in matches:
        if len(out) >= max_candidates:
            break
        k = int(k)
        if k in kept and k not in taken and k <= n - min_gap and d <= max_distance:
            out.append((k, np.eye(4)))
            taken.add(k)
    return out


def accept_loop(res: Dict[str, Any], guess, pixels: int, min_overlap: float, max_rms: float, max_correction: Tuple[float, float]) -> bool:
    """Whether a verified candidate becomes a loop edge: OK, pairs >= min_overlap * pixels, rms <= max_rms, and a result within max_correction
    (metres, degrees) of the guess it started from."""
    if res["state"] != OK or res["pairs"] < min_overlap * pixels or not res["rms"] <= max_rms:
        return False
    t, a = pose_offset(rigid_inverse(guess) @ np.asarray(res["T"], dtype=np.float64))
    return t <= max_correction[0] and a <= max_correction[1]


def information(sums) -> np.ndarray:
    """The 6 x 6 J^T J of an alignment's last iteration (the first 21 of its 29 sums: the upper triangle, row-major): the weight of its edge in the
    pose graph.  J is the derivative with respect to a LEFT perturbation exp(xi) T of the result, rotation first -- the tangent the graph's
    residual log(X_i^-1 X_j Z^-1) lives in."""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = np.asarray(sums, dtype=np.float64)[:21]
    return A + np.triu(A, 1).T


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

    def queue_volume(self, volume, cur: Frame, iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio) -> int:
        """`queue` with a fused TSDF volume (`tsdf_utils.TsdfVolume`) as the reference (`ovo_icp_align_volume`): T is
        (volume frame <- current camera), read and advanced in place.  The volume is only read."""
        if len(iters) != cur.levels:
            raise L.OvoHipError(f"align_volume: {len(iters)} entries in iters for {cur.levels} levels")
        L.dev(volume.vol, torch.float32, "volume")
        seq, slot = self.ring.next()
        desc = align_desc(iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio, seq)
        L.check(L.load().ovo_icp_align_volume(L.ptr(volume.vol), C.byref(volume.desc), L.ptr(cur.pyramid), C.byref(cur.desc), C.byref(desc), L.ptr(self.T),
                                              C.c_void_p(slot), L.ptr(self.ws), self.ws.numel(), L.stream()))
        return seq

    def wait(self, seq: int) -> Dict[str, Any]:
        return decode_result(self.ring.wait(seq))


def align_volume(volume, cur: Frame, T0, iters=(10, 5, 4), dist_th: float = 0.1, normal_th_deg: float = 30.0, min_pairs: int = 1,
                 min_pivot_ratio: float = 1e-6, aligner: Optional[Aligner] = None) -> Dict[str, Any]:
    """One alignment of a frame to a fused volume, start to result: T0 (4 x 4, volume frame <- current camera) -> what `align` returns.  One host wait."""
    aligner = aligner or Aligner(cur.pyramid.device)
    aligner.set_pose(T0)
    return aligner.wait(aligner.queue_volume(volume, cur, iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio))


def align(ref: Frame, cur: Frame, T0, iters=(10, 5, 4), dist_th: float = 0.1, normal_th_deg: float = 30.0, min_pairs: int = 1,
          min_pivot_ratio: float = 1e-6, aligner: Optional[Aligner] = None) -> Dict[str, Any]:
    """One alignment, start to result: T0 (4 x 4, reference camera <- current camera) -> {"T": 4 x 4 f32 on the host, "state": OK / LOST,
    "pairs", "rms", "sums" (the 29 f64 sums of the last executed iteration), "iterations"}.  One host wait."""
    aligner = aligner or Aligner(ref.pyramid.device)
    aligner.set_pose(T0)
    return aligner.wait(aligner.queue(ref, cur, iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio))


class BatchAligner:
    """`ovo_icp_align_batch`: one current frame against up to MAX_BATCH references in the launches of one alignment.  Holds the device poses
    (f32[16, 12]), the workspace for 16 entries and a ring of pinned slots of 16 result blocks each."""

    def __init__(self, device) -> None:
        self.device = torch.device(device)
        self.T = torch.zeros((MAX_BATCH, 12), dtype=torch.float32, device=self.device)
        self.ws = torch.empty(int(L.load().ovo_icp_align_batch_workspace_bytes(MAX_BATCH)), dtype=torch.uint8, device=self.device)
        self.ring = L.PinnedRing(RESULT_WORDS * MAX_BATCH, np.int64, slots=4)
        self._m = {}

    def queue(self, refs: Sequence[Frame], cur: Frame, T0s, iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio) -> int:
        """Queues the m alignments on the current stream from the start poses T0s (m of 4 x 4); returns the sequence number `wait` takes."""
        m = len(refs)
        if not 1 <= m <= MAX_BATCH or len(T0s) != m:
            raise L.OvoHipError(f"align_batch: 1 .. {MAX_BATCH} references with one start pose each (got {m} and {len(T0s)})")
        if len(iters) != cur.levels:
            raise L.OvoHipError(f"align_batch: {len(iters)} entries in iters for {cur.levels} levels")
        top = np.stack([np.asarray(T, dtype=np.float32)[:3].reshape(12) for T in T0s])
        self.T[:m].copy_(torch.from_numpy(top))
        seq, slot = self.ring.next()
        self.ring.view[seq % self.ring.slots, ::RESULT_WORDS] = 0      # every block's sequence word
        desc = align_desc(iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio, seq)
        table = (C.c_void_p * m)(*[r.pyramid.data_ptr() for r in refs])
        L.check(L.load().ovo_icp_align_batch(C.cast(table, C.c_void_p), C.byref(refs[0].desc), L.ptr(cur.pyramid), C.byref(cur.desc), C.byref(desc), m,
                                             L.ptr(self.T), C.c_void_p(slot), L.ptr(self.ws), self.ws.numel(), L.stream()))
        self._m[seq] = m
        return seq

    def wait(self, seq: int) -> List[Dict[str, Any]]:
        m = self._m.pop(seq)
        base = self.ring.slot(seq)
        for k in range(m):                                 # the blocks are written by m workgroups in no particular order
            L.check(L.load().ovo_host_wait64(base + k * RESULT_WORDS * 8, seq, 20_000_000))
        blocks = self.ring.view[seq % self.ring.slots].reshape(MAX_BATCH, RESULT_WORDS)
        return [decode_result(blocks[k]) for k in range(m)]


def align_batch(refs: Sequence[Frame], cur: Frame, T0s, iters=(10, 5, 4), dist_th: float = 0.1, normal_th_deg: float = 30.0, min_pairs: int = 1,
                min_pivot_ratio: float = 1e-6, aligner: Optional[BatchAligner] = None) -> List[Dict[str, Any]]:
    """`align` for every (refs[k], T0s[k]) against one current frame in one set of launches; entry k's result is bit-equal to `align`'s.  One host wait."""
    aligner = aligner or BatchAligner(cur.pyramid.device)
    return aligner.wait(aligner.queue(refs, cur, T0s, iters, dist_th, normal_th_deg, min_pairs, min_pivot_ratio))
