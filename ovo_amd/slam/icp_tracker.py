"""A live tracker behind the seam `WrapperORBSLAM` calls (slam/orbslam.py): geometry-only pose from depth, multi-scale projective point-to-plane
ICP of every frame against a reference model (csrc/icp.hip).  The reference gets the same capability from Open3D's RGB-D
odometry in its Gaussian-SLAM back end (ovo/submodules/gaussian_slam/entities/visual_odometer.py); here the alignment runs on the GPU with the
pose device-resident, and the host reads one pinned result block per frame.

The seven methods follow `ReplayTracker`'s conventions: a trajectory / keyframe row is 13 f32 -- the frame's time stamp, then the top three rows
of its pose (camera to the FIRST frame's camera; `WrapperORBSLAM` puts `world_ref` in front).

`process_image_rgbd` is the one frame loop: prepare the frame, queue one alignment and wait for it, LOST or a pose, the
row, the keyframe decision, buffers handed back.  What a frame is aligned to is a reference model (slam/icp_reference.py), which answers only
what differs between the two:

`model="keyframe"`: the last keyframe's depth image (`KeyframeReference`).
`model="tsdf"`: frame to MODEL (`TsdfReference`) -- every tracked frame is fused into a dense TSDF volume
(utils/tsdf_utils.py, csrc/tsdf.hip), and a frame is aligned to the volume's ray-cast depth image from the last good pose.

`model="tsdf", tsdf_align="volume"`: frame to the volume ITSELF (`VolumeReference`) -- the signed distance where a pixel's
vertex falls is the residual and its gradient the normal (`ovo_icp_align_volume`); nothing is ray-cast and no model image prepared in the frame loop.

`close_loops=True` adds loop detection, verification and correction on keyframes (`LoopCloser`, slam/loop_closer.py): the
new keyframe is aligned against the old keyframes its own pose estimate puts nearby -- all of them in the launches of one alignment
(`ovo_icp_align_batch`) -- the ones that pass become edges of a pose graph (slam/pose_graph.py), and when the optimised graph moves a keyframe
the tracker replaces the keyframe rows and the big-change index goes up, which is what `WrapperORBSLAM.map` re-anchors its map on."""
from __future__ import annotations

from typing import Any, List, Optional

import numpy as np
import torch

from ..utils import icp_utils as U
from ..utils.tsdf_utils import MAX_HISTORY
from .icp_reference import KeyframeReference, TsdfReference, VolumeReference
from .keyframe_store import KeyframeStore
from .loop_closer import LoopCloser
from .relocaliser import Relocaliser


class IcpTracker:
    OK = U.OK
    LOST = U.LOST

    def __init__(self, K, levels: int = 3, iters=(10, 5, 4), dist_th: float = 0.1, normal_th_deg: float = 30.0, max_depth: float = 10.0,
                 depth_jump: float = 0.1, min_pairs_frac: float = 0.05, min_pivot_ratio: float = 1e-6, kf_translation: float = 0.15,
                 kf_rotation_deg: float = 10.0, kf_min_overlap: float = 0.5, device="cuda", close_loops: bool = False, loop_min_gap: int = 10,
                 loop_radius: float = 0.5, loop_angle_deg: float = 30.0, loop_max_candidates: int = 8, loop_iters=None, loop_dist_th: float = 0.2,
                 loop_min_overlap: float = 0.3, loop_max_rms: float = 0.02, loop_max_correction=(0.3, 10.0), loop_min_shift=(0.01, 0.2),
                 loop_max_keyframes: int = 256, model: str = "keyframe", tsdf_dims=(512, 512, 512), tsdf_voxel: float = 0.02, tsdf_origin=None,
                 tsdf_trunc=None, tsdf_max_weight: float = 64, tsdf_near: float = 0.05, tsdf_far=None, tsdf_history: int = 0,
                 tsdf_color: bool = False, tsdf_labels: bool = False, relocalise: bool = False, fern_count: int = 256, fern_seed: int = 0,
                 fern_tau=(0.3, None), reloc_max_candidates: int = 4, reloc_max_dissimilarity: float = 0.3, reloc_iters=None, reloc_dist_th: float = 0.2,
                 reloc_min_overlap: float = 0.3, reloc_max_rms: float = 0.02, reloc_max_keyframes: int = 256, loop_candidates: str = "pose",
                 loop_max_dissimilarity: float = 0.3, tsdf_align: str = "raycast") -> None:
        """No GPU work happens here: buffers are made with the first frame.  The loop_* parameters are read and checked by `LoopCloser`, the
        tsdf_* parameters by `TsdfReference`, whichever mode is chosen.

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
        model="tsdf" with close_loops=True and tsdf_history=0 raises ValueError: a corrected trajectory would need the volume fused again, and
        without the frames it cannot be.

        tsdf_history > 0 (model="tsdf" only, at most 4096): the last tsdf_history fused depth images stay
        on the device (`history`, a `TsdfHistory`: 1.12 MB a frame at 456 x 616), each with the keyframe it hangs on and its pose relative to it, and
        close_loops=True is allowed: the keyframes' own depth pyramids are verified against each other as in keyframe mode, the odometry edge is the
        keyframe-to-keyframe transform, and after an applied closure the volume is fused again from the history at the corrected poses
        (`TsdfVolume.refuse`: one memset, then one `ovo_tsdf_integrate` call per kept frame) and ray-cast at the corrected pose, all queued behind that frame's one extra
        wait.  A frame older than the history is no longer in the model after a re-fusion.  A LOST frame adds nothing to the history.

        tsdf_color (model="tsdf" only): the volume also fuses the colour image of every tracked frame (1 GB more at 512^3,
        0.84 MB a frame more in the history), `render_model` shows the model in colour and `extract_mesh(colors=True)` puts it on the mesh.
        Colour takes no part in the alignment: the model image stays the depth-only ray cast, and poses are bit-identical with it on or off.

        tsdf_labels (model="tsdf" only): a label array beside the volume (1 GB more at 512^3, 1.12 MB a frame more in the
        history).  The frame loop never touches it: `fuse_labels(ins)` votes a keyframe's instance image (`OVO.instance_image`) into it,
        `render_model(labels=True)` and `extract_mesh(labels=True)` read it back, `volume.remap_labels(OVO.last_instance_table)` follows the map's
        merges.  Poses, the volume and the model image are bit-identical with it on or off.

        tsdf_align (model="tsdf" only): "raycast" (the default: all of the above) or "volume" -- a frame is aligned to the
        volume itself (`ovo_icp_align_volume`): per pixel the trilinear F at its vertex, times trunc, is the point-to-plane residual and the
        normalised gradient of F the plane normal.  The first frame is fused and nothing is cast; the device pose is the frame's pose in the volume's
        frame (the first camera's), carried from frame to frame: c2w = T with no product, an OK frame is fused at it, a LOST one restores it.
        `model_depth` stays None; keyframes are decided on inv(kf_c2w) @ c2w and the pairs against the volume.  A re-fusion after a loop closure
        and a relocalisation set the device pose to the corrected / found pose.  tsdf_color, tsdf_labels, tsdf_history, close_loops, relocalise,
        `extract_mesh`, `sample_model` and `render_model` work as with "raycast".  Limit: the residual exists only where |F| < 1, within
        tsdf_trunc of the surface -- a start pose further off than that pairs nothing and is LOST, where "raycast" with its dist_th reaches further.
        Anything else raises ValueError, and so does "volume" with model="keyframe".

        relocalise: every frame's fern code -- fern_count ferns (a multiple of 8) of 4 depth tests over the coarsest pyramid
        level, pixels and thresholds drawn from fern_seed, thresholds uniform in fern_tau metres (None: max_depth / 2) -- is searched against the
        keyframes' codes, queued in front of the frame's alignment: no extra wait.  A frame whose alignment is LOST is then verified, from the
        identity, against the reloc_max_candidates (<= 16) most similar kept keyframes within reloc_max_dissimilarity (a fraction of the ferns) in
        ONE `ovo_icp_align_batch` call with reloc_iters (default: iters) and reloc_dist_th -- one extra host wait, on such a frame only.
        model="keyframe": against the kept pyramids of the last reloc_max_keyframes keyframes (one store with the loop closer's: with both on it
        holds the larger of the two counts); model="tsdf": against the model ray-cast at the candidates' keyframe poses.  An entry passes when it is
        OK, has pairs >= reloc_min_overlap * pixels and rms <= reloc_max_rms; the winner k has the most pairs, then the smaller rms, then the lower
        index.  The frame is then OK at X_k @ T (an f64 product rounded once; X_k the graph's pose with close_loops, else the keyframe row), is no
        keyframe, and is neither fused nor added to the history; `last_reloc` records the attempt.  model="keyframe": keyframe k is the reference
        again and the next keyframe's odometry edge hangs on k; model="tsdf": the model image is cast at the new pose.  Without a winner the frame is
        LOST as ever.  The fern_* and reloc_* defaults are JUDGEMENT, not measurement.  Limits: the codes see depth only, and an alignment of
        views that overlap little can be OK at a wrong pose (a box sliding along its walls) -- the gates do not detect that.

        loop_candidates (close_loops only): "pose" (by the pose estimate, as above), "fern" (by appearance: the kept keyframes k <= n -
        loop_min_gap within loop_max_dissimilarity of the new keyframe's code, in (distance, k) order, each with the identity as its guess) or
        "both" (by pose first, then by appearance into the slots left).  The verification batch, its one wait and the acceptance are the same."""
        self.K = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float32)[:3, :3].copy()
        self.levels, self.iters = int(levels), tuple(int(i) for i in iters)
        if not 1 <= self.levels <= U.MAX_LEVELS or len(self.iters) != self.levels:
            raise ValueError(f"IcpTracker: levels must be 1 .. {U.MAX_LEVELS} with one entry of iters per level, coarse to fine")
        self.dist_th, self.normal_th_deg, self.max_depth, self.depth_jump = float(dist_th), float(normal_th_deg), float(max_depth), float(depth_jump)
        self.min_pairs_frac, self.min_pivot_ratio = float(min_pairs_frac), float(min_pivot_ratio)
        self.kf_translation, self.kf_rotation_deg, self.kf_min_overlap = float(kf_translation), float(kf_rotation_deg), float(kf_min_overlap)
        self.close_loops = bool(close_loops)
        self.relocalise = bool(relocalise)
        self._ferns = Relocaliser(self.iters, self.normal_th_deg, self.min_pivot_ratio, self.max_depth, fern_count, fern_seed, fern_tau,
                                  reloc_max_candidates, reloc_max_dissimilarity, reloc_iters, reloc_dist_th, reloc_min_overlap, reloc_max_rms,
                                  reloc_max_keyframes)
        self._store = KeyframeStore(max(int(loop_max_keyframes), self._ferns.max_keyframes) if self.relocalise else int(loop_max_keyframes))
        self._loops = LoopCloser(self.iters, self.normal_th_deg, self.min_pivot_ratio, loop_min_gap, loop_radius, loop_angle_deg, loop_max_candidates,
                                 loop_iters, loop_dist_th, loop_min_overlap, loop_max_rms, loop_max_correction, loop_min_shift, loop_max_keyframes,
                                 loop_candidates, loop_max_dissimilarity, self._ferns.fern_count, self._store)
        self._loop_ferns = self.close_loops and self._loops.candidates != "pose"
        self._use_ferns = self.relocalise or self._loop_ferns      # False: no fern call is ever made
        self._ref_kf = 0                                   # the keyframe the frames are aligned against (model="keyframe": not the newest after a relocalisation)
        self.loop_iters = self._loops.iters
        self.model = str(model)
        if self.model not in ("keyframe", "tsdf"):
            raise ValueError(f"IcpTracker: model must be 'keyframe' or 'tsdf' (got {model!r})")
        self.tsdf_history = int(tsdf_history)
        if not 0 <= self.tsdf_history <= MAX_HISTORY:
            raise ValueError(f"IcpTracker: tsdf_history must be 0 .. {MAX_HISTORY} frames (got {tsdf_history})")
        if self.tsdf_history > 0 and self.model != "tsdf":
            raise ValueError("IcpTracker: tsdf_history keeps the frames of a fused volume and needs model='tsdf'")
        if self.model == "tsdf" and self.close_loops and self.tsdf_history == 0:
            raise ValueError("IcpTracker: model='tsdf' with close_loops=True is not built: a corrected trajectory would need the volume fused again")
        # (read in either mode, as the loop parameters are: tsdf_trunc and tsdf_far are the tracker's attributes whatever the model)
        self.tsdf_color = bool(tsdf_color)
        if self.tsdf_color and self.model != "tsdf":
            raise ValueError("IcpTracker: tsdf_color fuses colour into the volume and needs model='tsdf'")
        self.tsdf_labels = bool(tsdf_labels)
        if self.tsdf_labels and self.model != "tsdf":
            raise ValueError("IcpTracker: tsdf_labels votes instance labels into the volume and needs model='tsdf'")
        self.tsdf_align = str(tsdf_align)
        if self.tsdf_align not in ("raycast", "volume"):
            raise ValueError(f"IcpTracker: tsdf_align must be 'raycast' or 'volume' (got {tsdf_align!r})")
        if self.tsdf_align == "volume" and self.model != "tsdf":
            raise ValueError("IcpTracker: tsdf_align='volume' aligns to the fused volume and needs model='tsdf'")
        tsdf = (VolumeReference if self.tsdf_align == "volume" else TsdfReference)(self._prepare, self.K, self.max_depth, tsdf_dims, tsdf_voxel, tsdf_origin, tsdf_trunc, tsdf_max_weight, tsdf_near, tsdf_far,
                             history=self.tsdf_history, color=self.tsdf_color, **({"labels": True} if self.tsdf_labels else {}))
        self.tsdf_trunc, self.tsdf_far = tsdf.trunc, tsdf.far
        self._ref = tsdf if self.model == "tsdf" else KeyframeReference(self._prepare)
        self.device = device
        self._aligner: Optional[U.Aligner] = None
        self._kf_c2w = np.eye(4, dtype=np.float32)
        self._c2w = np.eye(4, dtype=np.float32)            # the pose of the last good frame
        self._row = None
        self._state = self.LOST
        self._is_kf = False
        self._keyframes: List[np.ndarray] = []
        self.last: Any = None                              # the last alignment's result (None for the first frame)
        self.closed = False

    volume = property(lambda self: getattr(self._ref, "volume", None))             # model="tsdf": the TsdfVolume, made with the first frame
    model_depth = property(lambda self: getattr(self._ref, "model_depth", None))   # model="tsdf": the last ray-cast image, what the next frame is aligned to
    history = property(lambda self: getattr(self._ref, "history", None))           # tsdf_history > 0: the TsdfHistory, made with the first frame
    loop_edges = property(lambda self: self._loops.loop_edges)                     # close_loops: see LoopCloser
    last_loop = property(lambda self: self._loops.last_loop)
    last_reloc = property(lambda self: self._ferns.last_reloc)                     # relocalise: the last attempt, see Relocaliser.verify
    loop_poses = property(lambda self: self._loops.poses)                          # close_loops: the graph's keyframe poses in f64, what `history.poses` takes

    def _row_of(self, t, c2w: np.ndarray) -> np.ndarray:
        return np.concatenate([np.asarray([t], dtype=np.float32), np.asarray(c2w, dtype=np.float32)[:3].reshape(12)])

    def _depth(self, depth) -> torch.Tensor:
        if not isinstance(depth, torch.Tensor):
            depth = torch.from_numpy(np.ascontiguousarray(np.asarray(depth, dtype=np.float32)))
        return depth.to(device=self.device, dtype=torch.float32).contiguous()

    def _rgb(self, rgb, depth: torch.Tensor) -> dict:
        """tsdf_color: {"rgb": the frame's colour image u8[h, w, 3] on the device}; else {} -- the image takes no part and is not looked at."""
        if not self.tsdf_color:
            return {}
        if isinstance(rgb, np.ndarray) and rgb.dtype == np.uint8:
            rgb = torch.from_numpy(np.ascontiguousarray(rgb))
        if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or tuple(rgb.shape) != (int(depth.shape[0]), int(depth.shape[1]), 3):
            got = f"{rgb.dtype} {tuple(rgb.shape)}" if isinstance(rgb, (torch.Tensor, np.ndarray)) else type(rgb).__name__
            raise ValueError(f"IcpTracker: tsdf_color needs rgb as a u8 array or tensor [{int(depth.shape[0])}, {int(depth.shape[1])}, 3] (got {got})")
        return {"rgb": rgb.to(device=self.device).contiguous()}

    def _prepare(self, depth: torch.Tensor, out: Optional[torch.Tensor]) -> U.Frame:
        return U.prepare_frame(depth, self.K, self.levels, self.max_depth, self.depth_jump, out=out)

    def process_image_rgbd(self, rgb, depth, t) -> None:
        """Tracks one frame (the colour image takes no part in it; tsdf_color fuses it into the model of a tracked frame); returns when its pose
        is on the host: one host wait per frame, one more on a keyframe whose loop candidates are verified, and with relocalise one more on a LOST
        frame that has keyframes to be verified against."""
        if self.closed:
            raise RuntimeError("IcpTracker: shut down")
        depth, ref = self._depth(depth), self._ref
        color = self._rgb(rgb, depth)
        if self._aligner is None:                          # the first frame: the identity pose, a keyframe
            self._aligner = U.Aligner(depth.device)
            ref.start(depth, self._aligner, t, **color)
            self._state, self._is_kf, self.last = self.OK, True, None
            self._row = self._row_of(t, self._c2w)
            self._keyframes.append(self._row)
            if self._use_ferns:                            # keyframe 0's code, from its own pyramid (model="tsdf" without a history keeps none: made here)
                own = ref.frame if self.model == "keyframe" else ref._kf
                if own is None:
                    own = self._prepare(depth, None)
                    ref.spare = own.pyramid
                self._ferns.encode(own)
                self._ferns.add_keyframe(0)
            return
        cur = self._prepare(depth, ref.spare)
        ref.aim(self._aligner)
        pixels = cur.h * cur.w
        min_pairs = int(np.ceil(self.min_pairs_frac * pixels))
        if self._use_ferns:                                # code and search in front of the alignment: their block is there when the alignment's is
            n = len(self._keyframes)                       # the index this frame would get as a keyframe
            self._ferns.queue(cur, [n - self._loops.min_gap + 1, n] if self._loop_ferns else [n])
        seq = ref.queue(self._aligner, cur, self.iters, self.dist_th, self.normal_th_deg, min_pairs, self.min_pivot_ratio)      # against its frame, or its volume
        self.last = res = self._aligner.wait(seq)
        matches = self._ferns.matches() if self._use_ferns else None
        self._is_kf = False
        if res["state"] != U.OK:
            if self.relocalise and self._relocalise(cur, t, matches[-1], pixels, min_pairs):
                return                                     # found again: OK at a kept keyframe's pose times the verified alignment, no keyframe
            self._state = self.LOST                        # the pose stays that of the last good frame, and the reference as it was
            ref.spare = cur.pyramid
            return
        self._state = self.OK
        self._c2w, relative = ref.compose(self._c2w, self._kf_c2w, res["T"])
        self._row = self._row_of(t, self._c2w)
        if U.keyframe_decision(relative, res["pairs"], pixels, self.kf_translation, self.kf_rotation_deg, self.kf_min_overlap):
            self._kf_c2w, self._is_kf = self._c2w, True
            self._keyframes.append(self._row)
        n = len(self._keyframes) - 1                       # the keyframe this frame hangs on (itself, when it is one)
        old = ref.tracked(cur, depth, self._c2w, self._is_kf, self._aligner, t, n, relative, **color)
        more = {}
        if self._is_kf:
            parent, self._ref_kf = self._ref_kf, n
            if parent != n - 1:                            # after a relocalisation: the outgoing reference is an old keyframe, and the edge hangs on it
                more["parent"] = parent
            if self._use_ferns:
                self._ferns.add_keyframe(n)
            if self._loop_ferns:
                more["fern"] = matches[0]
            if self.relocalise and not self.close_loops and self.model == "keyframe":      # the loop closer's bookkeeping of the pyramids, without it
                self._store.put(parent, old)
                ref.spare = self._store.trim()
        if self._is_kf and self.close_loops:               # `old`'s pyramid is kept: the next frame takes the one that became free, or a new one
            # model="tsdf": `old` and `cur` are the keyframes' own images, and the edge is keyframe to keyframe, not the alignment to the model
            X, ref.spare = self._loops.keyframe(n, old, cur, res, pixels, min_pairs, edge_T=relative if self.model == "tsdf" else None, **more)
            if X is not None:                              # a closure moved the keyframes: their rows, rounded to f32, and this frame's pose
                self._keyframes = [self._row_of(row[0], x) for row, x in zip(self._keyframes, X)]
                self._kf_c2w = self._c2w = X[n].astype(np.float32)
                self._row = self._keyframes[n]
                ref.corrected(X, self._c2w)                # model="tsdf": the volume fused again from its history, the model image cast again

    def _relocalise(self, cur: U.Frame, t, matches, pixels: int, min_pairs: int) -> bool:
        """A LOST frame and its fern matches [(keyframe, distance)]: verifies the kept keyframes it looks like in one batch and, with a winner k,
        takes the pose X_k @ T.  False: no candidate or no winner, and nothing has changed."""
        ref, keyframe_mode = self._ref, self.model == "keyframe"
        kept = (lambda k: k in self._store or k == self._ref_kf) if keyframe_mode else (lambda k: k < len(self._keyframes))
        chosen = self._ferns.choose(matches, kept)
        if not chosen:
            return False
        poses = self._loops.poses if self.close_loops else [np.vstack([row[1:].reshape(3, 4).astype(np.float64), [[0.0, 0.0, 0.0, 1.0]]]) for row in self._keyframes]
        if keyframe_mode:
            refs = [ref.frame if k == self._ref_kf else self._store[k] for k, _ in chosen]
        else:
            refs = ref.cast_at([poses[k] for k, _ in chosen])
        k, res = self._ferns.verify(chosen, refs, cur, pixels, min_pairs)
        if k is None:
            return False
        self._state = self.OK
        self._c2w = (poses[k] @ res["T"].astype(np.float64)).astype(np.float32)      # an f64 product, rounded once
        self._row = self._row_of(t, self._c2w)
        if keyframe_mode:
            if k != self._ref_kf:                          # the outgoing reference is a kept keyframe like any other
                self._store.put(self._ref_kf, ref.frame)
                self._ref_kf = k
                self._store.trim(keep=k)
            self._kf_c2w = poses[k].astype(np.float32)
            ref.relocalised(refs[[c for c, _ in chosen].index(k)], res["T"], cur, self._aligner)
        else:
            ref.relocalised(self._c2w, cur)
        return True

    def fuse_labels(self, ins) -> None:
        """tsdf_labels: votes the instance image ins (i32 [h, w] of the depth's size, an array or a tensor; negative = no label) into the label volume
        with the depth and the pose of the most recent fused frame -- call it after `process_image_rgbd` of a keyframe, once its instances are known.
        With a history the image is kept in that frame's slot and voted again by a re-fusion.  Queued on the current stream; never waits."""
        if self.closed:
            raise RuntimeError("IcpTracker: shut down")
        if not self.tsdf_labels:
            raise ValueError("IcpTracker.fuse_labels: the model holds no labels (build the tracker with model='tsdf', tsdf_labels=True)")
        if self.volume is None or self._ref._last is None:
            raise ValueError("IcpTracker.fuse_labels: no frame fused yet (the volume is made with the first frame)")
        hw = tuple(int(x) for x in self._ref._last[0].shape)
        if isinstance(ins, np.ndarray) and ins.dtype == np.int32:
            ins = torch.from_numpy(np.ascontiguousarray(ins))
        if not isinstance(ins, torch.Tensor) or ins.dtype != torch.int32 or tuple(ins.shape) != hw:
            got = f"{ins.dtype} {tuple(ins.shape)}" if isinstance(ins, (torch.Tensor, np.ndarray)) else type(ins).__name__
            raise ValueError(f"IcpTracker.fuse_labels: ins must be an i32 array or tensor {list(hw)} (got {got})")
        self._ref.fuse_labels(ins.to(device=self.device).contiguous())

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
        return self._loops.big_change                      # goes up when a closure moved the keyframes (always 0 without close_loops)

    def get_keyframe_points(self):
        return list(self._keyframes)

    def extract_mesh(self, **kw):
        """model="tsdf": `TsdfVolume.extract_mesh(**kw)` of the fused model, (vertices f32[V, 3], faces i32[T, 3]) on the device, in the tracker's
        frame (that of the first camera: a world_ref is applied by whoever holds it, e.g. `OVO.semantic_mesh(transform=)`).  With tsdf_color,
        `colors=True` adds rgb u8[V, 3], which `OVO.semantic_mesh(rgb=)` carries into the PLY.  `normals=True` adds vertex normals f32[V, 3] last
        (the volume's gradient), which `OVO.semantic_mesh(normals=)` carries likewise.  With tsdf_labels, `labels=True` adds
        vertex instance ids i32[V] after them, which `OVO.semantic_mesh(instance=)` takes in place of its 5-NN transfer."""
        if self.model != "tsdf":
            raise ValueError("IcpTracker.extract_mesh: model='keyframe' keeps no fused model (build the tracker with model='tsdf')")
        if self.volume is None:
            raise ValueError("IcpTracker.extract_mesh: no frame processed yet (the volume is made with the first frame)")
        return self.volume.extract_mesh(**kw)

    def sample_model(self, points, **kw):
        """model="tsdf": `TsdfVolume.sample(points, **kw)` of the fused model -- what the model says at points f32[n, 3] given in the
        tracker's frame (that of the first camera; `transform=` takes points of another frame there, e.g. inv(world_ref) for world-frame points):
        F f32[n], then what `colors=` / `normals=` / `labels=` ask for.  Reads the volume only: poses, volume and model image stay as they are."""
        if self.model != "tsdf":
            raise ValueError("IcpTracker.sample_model: model='keyframe' keeps no fused model (build the tracker with model='tsdf')")
        if self.volume is None:
            raise ValueError("IcpTracker.sample_model: no frame processed yet (the volume is made with the first frame)")
        if kw.get("labels", False) and not self.tsdf_labels:
            raise ValueError("IcpTracker.sample_model: the model holds no labels (build the tracker with model='tsdf', tsdf_labels=True)")
        return self.volume.sample(points, **kw)

    def render_model(self, c2w=None, normals: bool = False, labels: bool = False):
        """tsdf_color: the fused model seen from `c2w` (None: the last good pose), in the tracker's frame: (depth f32[h, w], rgb u8[h, w, 3]) on
        the device, new tensors; the depth has the bits `model_depth` has at that pose.  Queued on the current stream, not waited for.
        `normals=True` (any model="tsdf" tracker): (depth, normals f32[h, w, 3]), or (depth, rgb, normals) with tsdf_color --
        unit normals in the tracker's frame from the volume's gradient, zeros where there is no surface; `tsdf_utils.shade_normals` makes a picture of them.
        `labels=True` (tsdf_labels) appends the instance image i32[h, w]: an occlusion-correct, hole-free view of the labels, -1 where
        there is no surface or no label -- (depth, ins), (depth, rgb, ins), (depth, normals, ins) or (depth, rgb, normals, ins)."""
        if labels and not self.tsdf_labels:
            raise ValueError("IcpTracker.render_model: the model holds no labels (build the tracker with model='tsdf', tsdf_labels=True)")
        if normals and self.model != "tsdf":
            raise ValueError("IcpTracker.render_model: model='keyframe' keeps no fused model (build the tracker with model='tsdf')")
        if not normals and not labels and not self.tsdf_color:
            raise ValueError("IcpTracker.render_model: the model holds no colour (build the tracker with model='tsdf', tsdf_color=True)")
        if self.volume is None:
            raise ValueError("IcpTracker.render_model: no frame processed yet (the volume is made with the first frame)")
        pose = self._c2w if c2w is None else np.asarray(c2w.detach().cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float32)
        if labels:
            return self._ref.render(pose, normals=bool(normals), labels=True)
        return self._ref.render(pose, normals=True) if normals else self._ref.render(pose)

    def shutdown(self) -> None:
        self._aligner = self._ref = None                   # with the reference go the keyframe's pyramid, or the volume and its image
        self._loops.release()
        self._ferns.release()
        self.closed = True
