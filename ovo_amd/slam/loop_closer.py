"""Loop closing on the keyframes of `IcpTracker(close_loops=True)` (DESIGN.md sections 15.1 and 16): the pose graph (slam/pose_graph.py), the kept keyframe
pyramids and their batched verification (`ovo_icp_align_batch`).  The tracker tells it of every new keyframe and applies the poses it hands back;
nothing here reaches into the tracker."""
from __future__ import annotations

from typing import Any, List, Optional

import numpy as np

from ..utils import icp_utils as U
from . import pose_graph
from .keyframe_store import KeyframeStore


class LoopCloser:
    def __init__(self, iters, normal_th_deg: float, min_pivot_ratio: float, loop_min_gap: int, loop_radius: float, loop_angle_deg: float,
                 loop_max_candidates: int, loop_iters, loop_dist_th: float, loop_min_overlap: float, loop_max_rms: float, loop_max_correction,
                 loop_min_shift, loop_max_keyframes: int, loop_candidates: str = "pose", loop_max_dissimilarity: float = 0.3,
                 fern_count: int = 256, store: Optional[KeyframeStore] = None) -> None:
        """`iters`, `normal_th_deg` and `min_pivot_ratio` are the tracker's own; the loop_* parameters are described at `IcpTracker`.  `store`: the
        keyframe store to keep the pyramids in (None: one of its own, of loop_max_keyframes)."""
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
        self.candidates, self.max_dissimilarity, self.fern_count = str(loop_candidates), float(loop_max_dissimilarity), int(fern_count)
        if self.candidates not in ("pose", "fern", "both"):
            raise ValueError(f"IcpTracker: loop_candidates must be 'pose', 'fern' or 'both' (got {loop_candidates!r})")
        if not 0 <= self.max_dissimilarity <= 1:
            raise ValueError("IcpTracker: loop_max_dissimilarity is a fraction of the ferns, in [0, 1]")
        # the pose graph (f64), the kept pyramids by keyframe index (oldest first), what the last closure did
        self._batch: Optional[U.BatchAligner] = None
        self._X: List[np.ndarray] = [np.eye(4)]
        self._edges: List[Any] = []
        self._db = KeyframeStore(self.max_keyframes) if store is None else store
        self.big_change = 0                                # goes up when a closure moved the keyframes
        self.loop_edges: List[Any] = []                    # (reference keyframe index, current keyframe index) of every accepted edge
        self.last_loop: Any = None                         # the last verification: {"n", "candidates", "results", "accepted", "applied", "graph"}

    def keyframe(self, n: int, old: U.Frame, cur: U.Frame, res, pixels: int, min_pairs: int, edge_T=None, parent: Optional[int] = None, fern=None):
        """The new keyframe n, `cur`, aligned to the outgoing keyframe `old` with result `res`: extends the graph, keeps `old`'s pyramid and
        verifies the candidates in one batch.  Returns (the corrected poses of keyframes 0 .. n in f64 when the optimised graph moved one, else
        None; the pyramid buffer that became free, else None).
        edge_T (model="tsdf"): the transform of the odometry edge n-1 -> n and of X[n] when it is not res["T"] -- there `res` aligned the frame to
        the MODEL, and the edge is keyframe n's pose in keyframe n-1's frame.  The edge's information stays `U.information(res["sums"])`, that of
        the keyframe frame's alignment to the model: a judgement, not a measurement of the edge's own uncertainty.
        parent: the keyframe that `old` is and that the odometry edge hangs on, when it is not n - 1 -- a relocalised tracker
        aligns against an old keyframe k, and its next keyframe's edge is (k, n).
        fern (loop_candidates "fern" / "both"): the keyframe's appearance matches [(k, block distance)] in (distance, k) order;
        those within loop_max_dissimilarity * fern_count that are kept, at least loop_min_gap back and not already chosen by pose fill the free slots, each with
        the identity as its guess (`icp_utils.extend_by_appearance`)."""
        p = n - 1 if parent is None else int(parent)
        T = (res["T"] if edge_T is None else np.asarray(edge_T)).astype(np.float64)
        self._X.append(self._X[p] @ T)
        self._edges.append((p, n, T, U.information(res["sums"])))
        self._db.put(p, old)
        free = self._db.trim()                             # the oldest leaves the candidate set (it stays a node); its buffer takes the next frame
        candidates = []
        if self.candidates != "fern":
            candidates = U.select_candidates(self._X, n, self._db.keys(), self.min_gap, self.radius, self.angle_deg, self.max_candidates)
        if self.candidates != "pose":
            candidates = U.extend_by_appearance(candidates, fern or [], self._db.keys(), n, self.min_gap, self.max_dissimilarity * self.fern_count,
                                                  self.max_candidates)
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
        self._batch = None
        self._db.release()
