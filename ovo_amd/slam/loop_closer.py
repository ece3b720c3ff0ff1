"""Loop closing on the keyframes of `IcpTracker(close_loops=True)` (DESIGN.md sections 15.1 and 16): the pose graph (slam/pose_graph.py), the kept keyframe
pyramids and their batched verification (`ovo_icp_align_batch`).  The tracker tells it of every new keyframe and applies the poses it hands back;
nothing here reaches into the tracker."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np

from ..utils import icp_utils as U
from . import pose_graph


class LoopCloser:
    def __init__(self, iters, normal_th_deg: float, min_pivot_ratio: float, loop_min_gap: int, loop_radius: float, loop_angle_deg: float,
                 loop_max_candidates: int, loop_iters, loop_dist_th: float, loop_min_overlap: float, loop_max_rms: float, loop_max_correction,
                 loop_min_shift, loop_max_keyframes: int) -> None:
        """`iters`, `normal_th_deg` and `min_pivot_ratio` are the tracker's own; the loop_* parameters are described at `IcpTracker`."""
        self.normal_th_deg, self.min_pivot_ratio = normal_th_deg, min_pivot_ratio
        self.min_gap, self.max_candidates, self.max_keyframes = int(loop_min_gap), int(loop_max_candidates), int(loop_max_keyframes)
        self.radius, self.angle_deg, self.dist_th = float(loop_radius), float(loop_angle_deg), float(loop_dist_th)
        self.iters = tuple(iters) if loop_iters is None else tuple(int(i) for i in loop_iters)
        self.min_overlap, self.max_rms = float(loop_min_overlap), float(loop_max_rms)
        self.max_correction = tuple(float(x) for x in loop_max_correction)
        self.min_shift = tuple(float(x) for x in loop_min_shift)
        if not (self.min_gap >= 1 and 1 <= self.max_candidates <= U.MAX_BATCH and self.max_keyframes >= 1):
            raise ValueError(f"IcpTracker: loop_min_gap and loop_max_keyframes must be >= 1 and loop_max_candidates 1 .. {U.MAX_BATCH}")
        if len(self.iters) != len(iters) or min(self.iters) < 0 or sum(self.iters) < 1:
            raise ValueError("IcpTracker: loop_iters needs one entry per level, coarse to fine, none negative and not all 0")
        if len(self.max_correction) != 2 or len(self.min_shift) != 2 or min(self.max_correction) <= 0 or min(self.min_shift) < 0:
            raise ValueError("IcpTracker: loop_max_correction (> 0) and loop_min_shift (>= 0) are (metres, degrees)")
        if not (self.radius > 0 and self.angle_deg > 0 and self.dist_th > 0 and 0 <= self.min_overlap <= 1 and self.max_rms > 0):
            raise ValueError("IcpTracker: loop_radius, loop_angle_deg, loop_dist_th and loop_max_rms must be > 0 and loop_min_overlap in [0, 1]")
        # the pose graph (f64), the kept pyramids by keyframe index (oldest first), what the last closure did
        self._batch: Optional[U.BatchAligner] = None
        self._X: List[np.ndarray] = [np.eye(4)]
        self._edges: List[Any] = []
        self._db: Dict[int, U.Frame] = {}
        self.big_change = 0                                # goes up when a closure moved the keyframes
        self.loop_edges: List[Any] = []                    # (reference keyframe index, current keyframe index) of every accepted edge
        self.last_loop: Any = None                         # the last verification: {"n", "candidates", "results", "accepted", "applied", "graph"}

    def keyframe(self, n: int, old: U.Frame, cur: U.Frame, res, pixels: int, min_pairs: int, edge_T=None):
        """The new keyframe n, `cur`, aligned to the outgoing keyframe `old` with result `res`: extends the graph, keeps `old`'s pyramid and
        verifies the candidates in one batch.  Returns (the corrected poses of keyframes 0 .. n in f64 when the optimised graph moved one, else
        None; the pyramid buffer that became free, else None).
        edge_T (model="tsdf"): the transform of the odometry edge n-1 -> n and of X[n] when it is not res["T"] -- there `res` aligned the frame to
        the MODEL, and the edge is keyframe n's pose in keyframe n-1's frame.  The edge's information stays `U.information(res["sums"])`, that of
        the keyframe frame's alignment to the model: a judgement, not a measurement of the edge's own uncertainty."""
        T = (res["T"] if edge_T is None else np.asarray(edge_T)).astype(np.float64)
        self._X.append(self._X[n - 1] @ T)
        self._edges.append((n - 1, n, T, U.information(res["sums"])))
        self._db[n - 1] = old
        free = None
        if len(self._db) > self.max_keyframes:            # the oldest leaves the candidate set (it stays a node); its buffer takes the next frame
            free = self._db.pop(next(iter(self._db))).pyramid
        candidates = U.select_candidates(self._X, n, list(self._db), self.min_gap, self.radius, self.angle_deg, self.max_candidates)
        self.last_loop = {"n": n, "candidates": [k for k, _ in candidates], "results": [], "accepted": [], "applied": False, "graph": None}
        if not candidates:
            return None, free
        if self._batch is None:
            self._batch = U.BatchAligner(cur.pyramid.device)
        seq = self._batch.queue([self._db[k] for k, _ in candidates], cur, [G for _, G in candidates], self.iters, self.dist_th, self.normal_th_deg,
                                min_pairs, self.min_pivot_ratio)
        results = self._batch.wait(seq)                    # the one extra host wait of such a keyframe
        self.last_loop["results"] = results
        for (k, G), r in zip(candidates, results):
            if U.accept_loop(r, G, pixels, self.min_overlap, self.max_rms, self.max_correction):
                self._edges.append((k, n, r["T"].astype(np.float64), U.information(r["sums"])))
                self.loop_edges.append((k, n))
                self.last_loop["accepted"].append(k)
        if not self.last_loop["accepted"]:
            return None, free
        X, info = pose_graph.optimise(self._X, self._edges)
        self.last_loop["graph"] = info
        shifts = [U.pose_offset(U.rigid_inverse(a) @ b) for a, b in zip(self._X, X)]
        if not (info["improved"] and any(t > self.min_shift[0] or a > self.min_shift[1] for t, a in shifts)):
            return None, free                              # the edges stay in the graph; nothing else changes
        self._X = X
        self.big_change += 1
        self.last_loop["applied"] = True
        return X, free

    @property
    def poses(self) -> List[np.ndarray]:
        """The graph's keyframe poses, f64, by keyframe index (the keyframe rows are these rounded to f32)."""
        return list(self._X)

    def release(self) -> None:
        self._batch, self._db = None, {}
