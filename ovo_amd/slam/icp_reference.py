"""What `IcpTracker` aligns a frame to: the last keyframe's depth image (`KeyframeReference`, section 15), a fused TSDF
volume ray-cast at the last good pose (`TsdfReference`, section 17), or that volume itself (`VolumeReference`, section 25).  The tracker's frame loop
is the same for all three; a reference answers only what differs, through the same attributes and methods:

    frame                    the prepared `Frame` the next alignment runs against
    spare                    the pyramid buffer the next frame is written into (None: a new one); a LOST frame's own, set by the tracker
    start(depth, aligner, t) the first frame (time stamp t), at the identity pose; `TsdfReference(color=True)` takes rgb= here and in `tracked`
    aim(aligner)             the device start pose before an alignment is queued
    queue(aligner, cur, ...) queues the alignment of `cur` with the tracker's settings: `aligner.queue` against `frame`, or `aligner.queue_volume`
    compose(c2w, kf_c2w, T)  an alignment's result T -> (the frame's pose, the pose relative to the keyframe that `keyframe_decision` takes)
    tracked(cur, depth, c2w, is_kf, aligner, t=None, kf=0, relative=None)   after an OK frame at pose c2w (time stamp t, hanging on keyframe kf at
                             `relative`); returns the outgoing keyframe's `Frame` when there is one
    corrected(X, c2w)        after a loop closure moved the keyframes to X (f64) and this frame to c2w

`prepare(depth, out)` is the tracker's `prepare_frame` with its own intrinsics and thresholds.  The three forms of `compose` ARE the contract
(tests/icp_restatement.py, tests/tsdf_restatement.py, tests/sdf_align_restatement.py): each is kept one operation at a time, and they are not to
be unified."""
from __future__ import annotations

import numpy as np
import torch

from ..utils import icp_utils as U
from ..utils import tsdf_utils

EYE = np.eye(4, dtype=np.float32)


class KeyframeReference:
    """Every frame against the last keyframe's pyramid.  The device pose is carried from frame to frame (keyframe camera <- frame camera) and set
    to the identity at a new keyframe; two pyramid buffers swap roles, unless the caller keeps the outgoing keyframe's and sets `spare` itself."""

    def __init__(self, prepare) -> None:
        self.prepare = prepare
        self.frame = self.spare = None

    def start(self, depth, aligner, t=None) -> None:
        self.frame = self.prepare(depth, None)
        aligner.set_pose(EYE)

    def aim(self, aligner) -> None:
        pass                                               # carried: the last alignment left its result there

    def queue(self, aligner, cur, *settings) -> int:
        return aligner.queue(self.frame, cur, *settings)

    def compose(self, c2w, kf_c2w, T):
        return (kf_c2w @ T).astype(np.float32), T          # an f32 product; the keyframe is decided on T itself

    def tracked(self, cur, depth, c2w, is_kf, aligner, t=None, kf=0, relative=None):
        if not is_kf:
            self.spare = cur.pyramid
            return None
        old, self.frame = self.frame, cur
        aligner.set_pose(EYE)
        self.spare = old.pyramid                           # (stream order: the next prepare is queued behind this frame's alignment)
        return old

    def corrected(self, X, c2w) -> None:
        pass                                               # the keyframe's own image is the model: nothing to rebuild

    def relocalised(self, frame, T, cur, aligner) -> None:
        """A LOST frame `cur` found itself at T against the kept keyframe pyramid `frame`: that keyframe is the reference
        again and T the device pose the next frame starts from; the frame itself is no keyframe, and its buffer takes the next frame."""
        self.frame = frame
        aligner.set_pose(T)
        self.spare = cur.pyramid


class TsdfReference:
    """Every frame, from the identity, against the volume ray-cast at the last good pose: an OK frame is fused at its pose and the model image
    (`model_depth`) is cast again there; a LOST frame fuses nothing and the same image serves the next frame.  tsdf_origin None: the volume is
    centred on the first camera, in the first camera's frame; tsdf_trunc None: 4 voxels; tsdf_far None: max_depth.  1 GB at 512^3.

    history > 0: the last `history` fused depth images are kept (`tsdf_utils.TsdfHistory`), each with the keyframe it hangs
    on and its pose relative to it, and `corrected` fuses the volume again from them after a loop closure.  The keyframes' OWN depth pyramids are
    then kept as `KeyframeReference` keeps them -- `tracked` returns the outgoing one at a keyframe -- because loop verification aligns keyframe
    images, not model images.

    color: the volume and the history are made with color=True and every fused frame brings its colour image; the model
    image the next frame is aligned to stays the depth-only ray cast, so poses do not depend on it.  `render(c2w)` casts depth and colour.

    labels: the volume and the history are made with labels=True.  Nothing in the frame loop votes: `fuse_labels(ins)` votes an
    instance image with the depth and the pose of the most recent fused frame (`_last`), whenever the caller has one -- at keyframes."""

    def __init__(self, prepare, K, max_depth, tsdf_dims, tsdf_voxel, tsdf_origin, tsdf_trunc, tsdf_max_weight, tsdf_near, tsdf_far, history=0,
                 color=False, labels=False) -> None:
        self.prepare, self.K = prepare, K
        self.dims, self.voxel = tuple(int(d) for d in tsdf_dims), float(tsdf_voxel)
        self.origin = tuple(-0.5 * self.voxel * (n - 1) for n in self.dims) if tsdf_origin is None else tuple(float(o) for o in tsdf_origin)
        self.trunc = 4.0 * self.voxel if tsdf_trunc is None else float(tsdf_trunc)
        self.max_weight, self.near = float(tsdf_max_weight), float(tsdf_near)
        self.far = float(max_depth) if tsdf_far is None else float(tsdf_far)
        self.volume = self.model_depth = self.frame = self.spare = self._eye = None
        self.history_capacity, self.history, self._kf = int(history), None, None
        self.color = bool(color)
        self.labels = bool(labels)
        self._more = {"color": True} if self.color else {}     # a plain model is made by the very calls it was made by before there was colour
        if self.labels:
            self._more["labels"] = True
        self._last = None                                  # (depth, c2w, history slot or None) of the most recent fused frame

    def start(self, depth, aligner, t=None, rgb=None) -> None:
        self.volume = tsdf_utils.TsdfVolume(self.dims, self.voxel, self.origin, self.trunc, self.max_weight, device=depth.device, **self._more)
        self._eye = torch.eye(4, dtype=torch.float32, device=depth.device)[:3].reshape(12).contiguous()
        if self.history_capacity > 0:                      # the first keyframe's own pyramid, and history entry 0
            self._kf = self.prepare(depth, None)
            self.history = tsdf_utils.TsdfHistory(self.history_capacity, int(depth.shape[0]), int(depth.shape[1]), device=depth.device, **self._more)
            self._slot = self.history.add(depth, t, 0, np.eye(4), **self._with(rgb))
        self._fuse(depth, EYE, rgb)

    def aim(self, aligner) -> None:
        aligner.T.copy_(self._eye)                         # device to device: no host wait

    def queue(self, aligner, cur, *settings) -> int:
        return aligner.queue(self.frame, cur, *settings)

    def compose(self, c2w, kf_c2w, T):
        c2w = (c2w.astype(np.float64) @ T.astype(np.float64)).astype(np.float32)      # an f64 product, rounded once
        return c2w, U.rigid_inverse(kf_c2w) @ c2w.astype(np.float64)

    def _with(self, rgb) -> dict:
        return {"rgb": rgb} if self.color else {}

    def tracked(self, cur, depth, c2w, is_kf, aligner, t=None, kf=0, relative=None, rgb=None):
        old = None
        if self.history is None or not is_kf:
            self.spare = cur.pyramid                       # (stream order: the next prepare is queued behind this frame's alignment)
        else:                                              # the keyframe's own pyramid is kept; the outgoing one is free unless a LoopCloser keeps it
            old, self._kf = self._kf, cur
            self.spare = old.pyramid
        if self.history is not None:
            self._slot = self.history.add(depth, t, kf, np.eye(4) if is_kf else relative, **self._with(rgb))
        self._fuse(depth, c2w, rgb)
        return old

    def fuse_labels(self, ins) -> None:
        """Votes ins i32[h, w] (device) into the label volume with the depth and the pose of the most recent fused frame, and keeps it in that frame's
        slot of the history, so that a re-fusion votes it again.  Queued, not waited for."""
        depth, c2w, slot = self._last
        if self.history is not None:
            depth = self.history.depths[slot]              # the ring's own copy: the caller's tensor may have moved on
            self.history.set_labels(slot, ins)
        self.volume.integrate_labels(depth, ins, self.K, c2w, self.near, self.far)

    def corrected(self, X, c2w) -> None:
        """The keyframes moved to X: the volume is fused again from the history at X[kf] @ rel, and the model image is cast at the corrected pose.
        All of it is queued; nothing waits."""
        self.volume.refuse(self.history, self.K, self.history.poses(X), self.near, self.far)
        if self._last is not None:
            self._last = (self._last[0], c2w, self._last[2])
        self._cast(c2w)

    def cast_at(self, poses):
        """Relocalisation: the model ray-cast and prepared at each of `poses` (4 x 4), into new buffers -- what a LOST frame is
        verified against.  No history is needed.  Queued, not waited for."""
        return [self.prepare(self.volume.raycast(self.K, self._hw[0], self._hw[1], np.asarray(X, dtype=np.float32), self.near, self.far), None)
                for X in poses]

    def relocalised(self, c2w, cur) -> None:
        """A LOST frame `cur` found itself at c2w: nothing is fused, the model image is cast there for the next frame, and the frame's buffer takes it."""
        self._cast(c2w)
        self.spare = cur.pyramid

    def _fuse(self, depth, c2w, rgb=None) -> None:
        """Fuses a tracked frame at its pose and ray-casts the model there for the next frame: queued, not waited for."""
        self._hw = (int(depth.shape[0]), int(depth.shape[1]))
        self.volume.integrate(depth, self.K, c2w, self.near, self.far, **self._with(rgb))
        self._last = (depth, c2w, getattr(self, "_slot", None))
        self._cast(c2w)

    def render(self, c2w, normals: bool = False, labels: bool = False):
        """(depth f32[h, w], rgb u8[h, w, 3]) of the colour model from c2w, into new tensors: the model image of the frame loop is not touched.
        `normals=True` (any volume): the normal image f32[h, w, 3] comes last, and the rgb only from a colour volume.  `labels=True` (a label volume):
        the instance image i32[h, w] comes after them; rgb from a colour volume, normals when asked for."""
        if labels:
            more = dict(self._more, **({"normals": True} if normals else {}))
            return self.volume.raycast(self.K, self._hw[0], self._hw[1], c2w, self.near, self.far, **more)
        if not normals:
            return self.volume.raycast(self.K, self._hw[0], self._hw[1], c2w, self.near, self.far, color=True)
        return self.volume.raycast(self.K, self._hw[0], self._hw[1], c2w, self.near, self.far, **({"color": True} if self.color else {}), normals=True)

    def _cast(self, c2w) -> None:
        self.model_depth = self.volume.raycast(self.K, self._hw[0], self._hw[1], c2w, self.near, self.far, out=self.model_depth)
        self.frame = self.prepare(self.model_depth, None if self.frame is None else self.frame.pyramid)


class VolumeReference(TsdfReference):
    """Every frame against the volume ITSELF (`ovo_icp_align_volume`): the trilinear F where a pixel's vertex falls, times trunc,
    is the residual and the gradient of F the normal, so nothing is ray-cast in the frame loop, no model image is prepared, and `model_depth` and
    `frame` stay None.  The device pose IS the frame's pose in the volume's frame -- that of the first camera -- and is carried from frame to frame as
    `KeyframeReference` carries its own: an OK alignment leaves c2w there, a LOST one restores it, `aim` does nothing.  Everything else -- fusing, the
    history, colour, labels, `cast_at`, `render` -- is `TsdfReference`'s.  Limit: the residual exists only within trunc of the surface (|F| < 1), so a
    start pose further off than that pairs nothing and is LOST, where the ray-cast form with its dist_th reaches further."""

    def start(self, depth, aligner, t=None, rgb=None) -> None:
        self._aligner = aligner                            # `corrected` and `relocalised` set the device pose and are not handed it
        super().start(depth, aligner, t, rgb)
        aligner.set_pose(EYE)

    def aim(self, aligner) -> None:
        pass                                               # carried: the last alignment left its result there, or restored it

    def queue(self, aligner, cur, *settings) -> int:
        return aligner.queue_volume(self.volume, cur, *settings)

    def compose(self, c2w, kf_c2w, T):
        return T, U.rigid_inverse(kf_c2w) @ T.astype(np.float64)      # c2w = T, no product; the keyframe is decided on inv(kf_c2w) @ c2w in f64

    def corrected(self, X, c2w) -> None:
        super().corrected(X, c2w)                          # the volume fused again from the history
        self._aligner.set_pose(c2w)

    def relocalised(self, c2w, cur) -> None:
        super().relocalised(c2w, cur)
        self._aligner.set_pose(c2w)

    def _cast(self, c2w) -> None:
        pass                                               # the frame loop needs no model image (`cast_at` and `render` cast on demand)
