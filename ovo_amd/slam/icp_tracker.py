"""A live tracker behind the seam `WrapperORBSLAM` calls (slam/orbslam.py): geometry-only pose from depth, multi-scale projective point-to-plane
ICP of every frame against the last keyframe (csrc/icp.hip).  The reference gets the same capability from Open3D's RGB-D
odometry in its Gaussian-SLAM back end (ovo/submodules/gaussian_slam/entities/visual_odometer.py); here the alignment runs on the GPU with the
pose device-resident, and the host reads one pinned result block per frame.

The seven methods follow `ReplayTracker`'s conventions: a trajectory / keyframe row is 13 f32 -- the frame's time stamp, then the top three rows
of its pose (camera to the FIRST frame's camera; `WrapperORBSLAM` puts `world_ref` in front).

`close_loops=True` adds loop detection, verification and correction on keyframes: the new keyframe is aligned against
the old keyframes its own pose estimate puts nearby -- all of them in the launches of one alignment (`ovo_icp_align_batch`) -- the ones that
pass become edges of a pose graph (slam/pose_graph.py), and when the optimised graph moves a keyframe the keyframe rows are replaced and the
big-change index goes up, which is what `WrapperORBSLAM.map` re-anchors its map on.

`model="tsdf"` tracks frame to MODEL: every tracked frame is fused into a dense TSDF volume (utils/tsdf_utils.py,
csrc/tsdf.hip), and a frame is aligned to the volume's ray-cast depth image from the last good pose instead of to the keyframe's raw image."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np
import torch

from ..utils import icp_utils as U
from . import pose_graph


class IcpTracker:
    OK = U.OK
    LOST = U.LOST

    def __init__(self, K, levels: int = 3, iters=(10, 5, 4), dist_th: float = 0.1, normal_th_deg: float = 30.0, max_depth: float = 10.0,
                 depth_jump: float = 0.1, min_pairs_frac: float = 0.05, min_pivot_ratio: float = 1e-6, kf_translation: float = 0.15,
                 kf_rotation_deg: float = 10.0, kf_min_overlap: float = 0.5, device="cuda", close_loops: bool = False, loop_min_gap: int = 10,
                 loop_radius: float = 0.5, loop_angle_deg: float = 30.0, loop_max_candidates: int = 8, loop_iters=None, loop_dist_th: float = 0.2,
                 loop_min_overlap: float = 0.3, loop_max_rms: float = 0.02, loop_max_correction=(0.3, 10.0), loop_min_shift=(0.01, 0.2),
                 loop_max_keyframes: int = 256, model: str = "keyframe", tsdf_dims=(512, 512, 512), tsdf_voxel: float = 0.02, tsdf_origin=None,
                 tsdf_trunc=None, tsdf_max_weight: float = 64, tsdf_near: float = 0.05, tsdf_far=None) -> None:
        """No GPU work happens here: buffers are made with the first frame.

        close_loops: every new keyframe n (its position in the keyframe list) is verified against the kept keyframes k <= n - loop_min_gap whose
        guess X_k^-1 X_n lies within loop_radius (m) and loop_angle_deg -- the loop_max_candidates (<= 16) nearest, one `ovo_icp_align_batch` call
        with loop_iters (default: iters) and loop_dist_th, one extra host wait on such a keyframe and none on any other frame.  An entry becomes
        a loop edge when it is OK, has pairs >= loop_min_overlap * pixels and rms <= loop_max_rms, and lies within loop_max_correction (m, deg)
        of its guess.  The graph is optimised when an edge was added and applied when some keyframe moves by more than loop_min_shift (m or deg).
        The loop_* defaults are JUDGEMENT, not measurement: no real sequence was available when they were chosen.
        Memory: the pyramids of the last loop_max_keyframes keyframes stay on the device, 11.8 MB each at 456 x 616 with 3 levels (3 GB at the
        default 256); an older keyframe leaves the candidate set but stays a node of the graph.

        model: "keyframe" (every frame against the last keyframe's depth image) or "tsdf": the first frame takes the identity pose, is a keyframe and
        is fused into a volume of tsdf_dims voxels of tsdf_voxel metres (tsdf_origin None: centred on the first camera, in the first camera's frame --
        the tracker's own; tsdf_trunc None: 4 voxels; tsdf_far None: max_depth).  Every later frame is aligned, from the identity, to the volume
        ray-cast at the last good pose (`model_depth`), c2w = c2w_last @ T, and is fused at c2w when it is OK; a LOST frame fuses nothing, and the
        same model image serves the next frame.  Keyframes are decided on inv(kf_c2w) @ c2w and the alignment's pairs against the model.  A ray-cast
        sample needs all eight corners observed, so a model built from one frame with many depth holes is sparse (with 5 % holes about a fifth of
        the pixels pair on the second frame, three fifths from the third): choose kf_min_overlap with that in mind.  1 GB at 512^3.
        model="tsdf" with close_loops=True raises ValueError: a corrected trajectory would need the volume fused again, which is not built."""
        self.K = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float32)[:3, :3].copy()
        self.levels, self.iters = int(levels), tuple(int(i) for i in iters)
        if not 1 <= self.levels <= U.MAX_LEVELS or len(self.iters) != self.levels:
            raise ValueError(f"IcpTracker: levels must be 1 .. {U.MAX_LEVELS} with one entry of iters per level, coarse to fine")
        self.dist_th, self.normal_th_deg, self.max_depth, self.depth_jump = float(dist_th), float(normal_th_deg), float(max_depth), float(depth_jump)
        self.min_pairs_frac, self.min_pivot_ratio = float(min_pairs_frac), float(min_pivot_ratio)
        self.kf_translation, self.kf_rotation_deg, self.kf_min_overlap = float(kf_translation), float(kf_rotation_deg), float(kf_min_overlap)
        self.close_loops = bool(close_loops)
        self.loop_min_gap, self.loop_max_candidates, self.loop_max_keyframes = int(loop_min_gap), int(loop_max_candidates), int(loop_max_keyframes)
        self.loop_radius, self.loop_angle_deg, self.loop_dist_th = float(loop_radius), float(loop_angle_deg), float(loop_dist_th)
        self.loop_iters = self.iters if loop_iters is None else tuple(int(i) for i in loop_iters)
        self.loop_min_overlap, self.loop_max_rms = float(loop_min_overlap), float(loop_max_rms)
        self.loop_max_correction = tuple(float(x) for x in loop_max_correction)
        self.loop_min_shift = tuple(float(x) for x in loop_min_shift)
        if not (self.loop_min_gap >= 1 and 1 <= self.loop_max_candidates <= U.MAX_BATCH and self.loop_max_keyframes >= 1):
            raise ValueError(f"IcpTracker: loop_min_gap and loop_max_keyframes must be >= 1 and loop_max_candidates 1 .. {U.MAX_BATCH}")
        if len(self.loop_iters) != self.levels or min(self.loop_iters) < 0 or sum(self.loop_iters) < 1:
            raise ValueError("IcpTracker: loop_iters needs one entry per level, coarse to fine, none negative and not all 0")
        if len(self.loop_max_correction) != 2 or len(self.loop_min_shift) != 2 or min(self.loop_max_correction) <= 0 or min(self.loop_min_shift) < 0:
            raise ValueError("IcpTracker: loop_max_correction (> 0) and loop_min_shift (>= 0) are (metres, degrees)")
        if not (self.loop_radius > 0 and self.loop_angle_deg > 0 and self.loop_dist_th > 0 and 0 <= self.loop_min_overlap <= 1 and self.loop_max_rms > 0):
            raise ValueError("IcpTracker: loop_radius, loop_angle_deg, loop_dist_th and loop_max_rms must be > 0 and loop_min_overlap in [0, 1]")
        self.model = str(model)
        if self.model not in ("keyframe", "tsdf"):
            raise ValueError(f"IcpTracker: model must be 'keyframe' or 'tsdf' (got {model!r})")
        if self.model == "tsdf" and self.close_loops:
            raise ValueError("IcpTracker: model='tsdf' with close_loops=True is not built: a corrected trajectory would need the volume fused again")
        self.tsdf_dims, self.tsdf_voxel = tuple(int(d) for d in tsdf_dims), float(tsdf_voxel)
        self.tsdf_origin = None if tsdf_origin is None else tuple(float(o) for o in tsdf_origin)
        self.tsdf_trunc = 4.0 * self.tsdf_voxel if tsdf_trunc is None else float(tsdf_trunc)
        self.tsdf_max_weight, self.tsdf_near = float(tsdf_max_weight), float(tsdf_near)
        self.tsdf_far = self.max_depth if tsdf_far is None else float(tsdf_far)
        self.volume: Any = None                            # model="tsdf": the TsdfVolume, made with the first frame
        self.model_depth: Optional[torch.Tensor] = None    # model="tsdf": the last ray-cast image, what the next frame is aligned to
        self._model: Optional[U.Frame] = None              # its pyramid
        self._eye: Optional[torch.Tensor] = None           # the identity start pose, on the device
        self.device = device
        self._aligner: Optional[U.Aligner] = None
        self._kf: Optional[U.Frame] = None                 # the last keyframe's pyramid
        self._spare: Optional[torch.Tensor] = None         # the buffer the next frame's pyramid is written into
        self._kf_c2w = np.eye(4, dtype=np.float32)
        self._c2w = np.eye(4, dtype=np.float32)            # the pose of the last good frame
        self._row = None
        self._state = self.LOST
        self._is_kf = False
        self._keyframes: List[np.ndarray] = []
        self.last: Any = None                              # the last alignment's result (None for a keyframe-initialising first frame)
        self.closed = False
        # close_loops: the pose graph (f64), the kept pyramids by keyframe index (oldest first), what the last closure did
        self._batch: Optional[U.BatchAligner] = None
        self._X: List[np.ndarray] = [np.eye(4)]
        self._edges: List[Any] = []
        self._db: Dict[int, U.Frame] = {}
        self._big_change = 0
        self.loop_edges: List[Any] = []                    # (reference keyframe index, current keyframe index) of every accepted edge
        self.last_loop: Any = None                         # the last verification: {"n", "candidates", "results", "accepted", "applied", "graph"}

    def _row_of(self, t, c2w: np.ndarray) -> np.ndarray:
        return np.concatenate([np.asarray([t], dtype=np.float32), np.asarray(c2w, dtype=np.float32)[:3].reshape(12)])

    def _depth(self, depth) -> torch.Tensor:
        if not isinstance(depth, torch.Tensor):
            depth = torch.from_numpy(np.ascontiguousarray(np.asarray(depth, dtype=np.float32)))
        return depth.to(device=self.device, dtype=torch.float32).contiguous()

    def process_image_rgbd(self, rgb, depth, t) -> None:
        """Tracks one frame (the colour image takes no part); returns when its pose is on the host: one host wait per frame."""
        if self.closed:
            raise RuntimeError("IcpTracker: shut down")
        depth = self._depth(depth)
        if self.model == "tsdf":
            return self._process_model(depth, t)
        cur = U.prepare_frame(depth, self.K, self.levels, self.max_depth, self.depth_jump, out=self._spare)
        self._spare = None
        if self._kf is None:                               # the first frame: the identity pose, a keyframe
            self._aligner = U.Aligner(depth.device)
            self._aligner.set_pose(np.eye(4, dtype=np.float32))
            self._kf, self._state, self._is_kf, self.last = cur, self.OK, True, None
            self._row = self._row_of(t, self._c2w)
            self._keyframes.append(self._row)
            return
        pixels = cur.h * cur.w
        seq = self._aligner.queue(self._kf, cur, self.iters, self.dist_th, self.normal_th_deg, int(np.ceil(self.min_pairs_frac * pixels)),
                                  self.min_pivot_ratio)
        self.last = res = self._aligner.wait(seq)
        self._is_kf = False
        if res["state"] != U.OK:                           # the pose stays that of the last good frame; the device T kept its value too
            self._state = self.LOST
            self._spare = cur.pyramid
            return
        self._state = self.OK
        self._c2w = (self._kf_c2w @ res["T"]).astype(np.float32)
        self._row = self._row_of(t, self._c2w)
        if U.keyframe_decision(res["T"], res["pairs"], pixels, self.kf_translation, self.kf_rotation_deg, self.kf_min_overlap):
            old = self._kf
            self._kf, self._kf_c2w, self._is_kf = cur, self._c2w, True
            self._aligner.set_pose(np.eye(4, dtype=np.float32))
            self._keyframes.append(self._row)
            if self.close_loops:
                self._close_loop(old, cur, res, pixels)
            else:
                self._spare = old.pyramid                  # (stream order: the next prepare is queued behind this frame's alignment)
        else:
            self._spare = cur.pyramid

    def _process_model(self, depth: torch.Tensor, t) -> None:
        """model="tsdf": one frame against the ray-cast model; one host wait."""
        h, w = int(depth.shape[0]), int(depth.shape[1])
        if self.volume is None:                            # the first frame: the identity pose, a keyframe, fused
            from ..utils.tsdf_utils import TsdfVolume
            origin = self.tsdf_origin
            if origin is None:
                origin = tuple(-0.5 * self.tsdf_voxel * (n - 1) for n in self.tsdf_dims)
            self.volume = TsdfVolume(self.tsdf_dims, self.tsdf_voxel, origin, self.tsdf_trunc, self.tsdf_max_weight, device=depth.device)
            self._aligner = U.Aligner(depth.device)
            self._eye = torch.eye(4, dtype=torch.float32, device=depth.device)[:3].reshape(12).contiguous()
            self._state, self._is_kf, self.last = self.OK, True, None
            self._row = self._row_of(t, self._c2w)
            self._keyframes.append(self._row)
            self._fuse(depth, h, w)
            return
        cur = U.prepare_frame(depth, self.K, self.levels, self.max_depth, self.depth_jump, out=self._spare)
        self._spare = cur.pyramid                          # (stream order: the next prepare is queued behind this frame's alignment)
        self._aligner.T.copy_(self._eye)                   # device to device: no host wait
        pixels = h * w
        seq = self._aligner.queue(self._model, cur, self.iters, self.dist_th, self.normal_th_deg, int(np.ceil(self.min_pairs_frac * pixels)),
                                  self.min_pivot_ratio)
        self.last = res = self._aligner.wait(seq)
        self._is_kf = False
        if res["state"] != U.OK:                           # pose, volume and model image stay
            self._state = self.LOST
            return
        self._state = self.OK
        self._c2w = (self._c2w.astype(np.float64) @ res["T"].astype(np.float64)).astype(np.float32)
        self._row = self._row_of(t, self._c2w)
        if U.keyframe_decision(U.rigid_inverse(self._kf_c2w) @ self._c2w.astype(np.float64), res["pairs"], pixels, self.kf_translation,
                               self.kf_rotation_deg, self.kf_min_overlap):
            self._kf_c2w, self._is_kf = self._c2w, True
            self._keyframes.append(self._row)
        self._fuse(depth, h, w)

    def _fuse(self, depth: torch.Tensor, h: int, w: int) -> None:
        """Fuses a tracked frame at the current pose and ray-casts the model there for the next frame: queued, not waited for."""
        self.volume.integrate(depth, self.K, self._c2w, self.tsdf_near, self.tsdf_far)
        self.model_depth = self.volume.raycast(self.K, h, w, self._c2w, self.tsdf_near, self.tsdf_far, out=self.model_depth)
        self._model = U.prepare_frame(self.model_depth, self.K, self.levels, self.max_depth, self.depth_jump,
                                      out=None if self._model is None else self._model.pyramid)

    def _close_loop(self, old: U.Frame, cur: U.Frame, res, pixels: int) -> None:
        """The new keyframe `cur` (aligned to the outgoing keyframe `old` with result `res`): extend the graph, keep `old`'s pyramid, verify the
        candidates in one batch, and apply the optimised graph if it moves a keyframe."""
        n = len(self._keyframes) - 1
        self._X.append(self._X[n - 1] @ res["T"].astype(np.float64))
        self._edges.append((n - 1, n, res["T"].astype(np.float64), U.information(res["sums"])))
        self._db[n - 1] = old
        if len(self._db) > self.loop_max_keyframes:       # the oldest leaves the candidate set (it stays a node); its buffer takes the next frame
            self._spare = self._db.pop(next(iter(self._db))).pyramid
        candidates = U.select_candidates(self._X, n, list(self._db), self.loop_min_gap, self.loop_radius, self.loop_angle_deg, self.loop_max_candidates)
        self.last_loop = {"n": n, "candidates": [k for k, _ in candidates], "results": [], "accepted": [], "applied": False, "graph": None}
        if not candidates:
            return
        if self._batch is None:
            self._batch = U.BatchAligner(cur.pyramid.device)
        seq = self._batch.queue([self._db[k] for k, _ in candidates], cur, [G for _, G in candidates], self.loop_iters, self.loop_dist_th,
                                self.normal_th_deg, int(np.ceil(self.min_pairs_frac * pixels)), self.min_pivot_ratio)
        results = self._batch.wait(seq)                    # the one extra host wait of such a keyframe
        self.last_loop["results"] = results
        for (k, G), r in zip(candidates, results):
            if U.accept_loop(r, G, pixels, self.loop_min_overlap, self.loop_max_rms, self.loop_max_correction):
                self._edges.append((k, n, r["T"].astype(np.float64), U.information(r["sums"])))
                self.loop_edges.append((k, n))
                self.last_loop["accepted"].append(k)
        if not self.last_loop["accepted"]:
            return
        X, info = pose_graph.optimise(self._X, self._edges)
        self.last_loop["graph"] = info
        shifts = [U.pose_offset(U.rigid_inverse(a) @ b) for a, b in zip(self._X, X)]
        if not (info["improved"] and any(t > self.loop_min_shift[0] or a > self.loop_min_shift[1] for t, a in shifts)):
            return                                         # the edges stay in the graph; nothing else changes
        self._X = X
        self._keyframes = [self._row_of(row[0], x) for row, x in zip(self._keyframes, X)]      # rounded to f32
        self._kf_c2w = self._c2w = X[n].astype(np.float32)
        self._row = self._keyframes[n]
        self._big_change += 1
        self.last_loop["applied"] = True

    def _need_frame(self) -> None:
        if self._row is None:
            raise RuntimeError("IcpTracker: no frame processed yet")

    def get_tracking_state(self):
        self._need_frame()
        return self._state

    def get_last_trajectory_point(self):
        self._need_frame()
        return self._row

    def is_last_frame_kf(self) -> bool:
        self._need_frame()
        return self._is_kf

    def get_last_big_change_idx(self) -> int:
        return self._big_change                            # goes up when a closure moved the keyframes (always 0 without close_loops)

    def get_keyframe_points(self):
        return list(self._keyframes)

    def shutdown(self) -> None:
        self._aligner = self._kf = self._spare = self._batch = None
        self.volume = self.model_depth = self._model = self._eye = None
        self._db = {}
        self.closed = True
