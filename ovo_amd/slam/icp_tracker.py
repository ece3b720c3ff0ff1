"""A live tracker behind the seam `WrapperORBSLAM` calls (slam/orbslam.py): geometry-only pose from depth, multi-scale projective point-to-plane
ICP of every frame against the last keyframe (csrc/icp.hip).  The reference gets the same capability from Open3D's RGB-D
odometry in its Gaussian-SLAM back end (ovo/submodules/gaussian_slam/entities/visual_odometer.py); here the alignment runs on the GPU with the
pose device-resident, and the host reads one pinned result block per frame.

The seven methods follow `ReplayTracker`'s conventions: a trajectory / keyframe row is 13 f32 -- the frame's time stamp, then the top three rows
of its pose (camera to the FIRST frame's camera; `WrapperORBSLAM` puts `world_ref` in front)."""
from __future__ import annotations

from typing import Any, List, Optional

import numpy as np
import torch

from ..utils import icp_utils as U


class IcpTracker:
    OK = U.OK
    LOST = U.LOST

    def __init__(self, K, levels: int = 3, iters=(10, 5, 4), dist_th: float = 0.1, normal_th_deg: float = 30.0, max_depth: float = 10.0,
                 depth_jump: float = 0.1, min_pairs_frac: float = 0.05, min_pivot_ratio: float = 1e-6, kf_translation: float = 0.15,
                 kf_rotation_deg: float = 10.0, kf_min_overlap: float = 0.5, device="cuda") -> None:
        """No GPU work happens here: buffers are made with the first frame."""
        self.K = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float32)[:3, :3].copy()
        self.levels, self.iters = int(levels), tuple(int(i) for i in iters)
        if not 1 <= self.levels <= U.MAX_LEVELS or len(self.iters) != self.levels:
            raise ValueError(f"IcpTracker: levels must be 1 .. {U.MAX_LEVELS} with one entry of iters per level, coarse to fine")
        self.dist_th, self.normal_th_deg, self.max_depth, self.depth_jump = float(dist_th), float(normal_th_deg), float(max_depth), float(depth_jump)
        self.min_pairs_frac, self.min_pivot_ratio = float(min_pairs_frac), float(min_pivot_ratio)
        self.kf_translation, self.kf_rotation_deg, self.kf_min_overlap = float(kf_translation), float(kf_rotation_deg), float(kf_min_overlap)
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
            self._spare = self._kf.pyramid                 # (stream order: the next prepare is queued behind this frame's alignment)
            self._kf, self._kf_c2w, self._is_kf = cur, self._c2w, True
            self._aligner.set_pose(np.eye(4, dtype=np.float32))
            self._keyframes.append(self._row)
        else:
            self._spare = cur.pyramid

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
        return 0                                           # no loop closing: the map is never re-anchored

    def get_keyframe_points(self):
        return list(self._keyframes)

    def shutdown(self) -> None:
        self._aligner = self._kf = self._spare = None
        self.closed = True
