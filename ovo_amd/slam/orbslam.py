"""The loop-closing SLAM back end around an injected tracker -- reference: ovo/slam/orbslam.py:WrapperORBSLAM.

ORB-SLAM3 itself (a C++ tracker with a vocabulary file) is not part of this package: `tracker=` is any object with the seven methods the
reference calls on its `orbslam.System` (orbslam.py:36-72,120):
    process_image_rgbd(rgb, depth, t) / get_tracking_state() / get_last_trajectory_point() / is_last_frame_kf() /
    get_last_big_change_idx() / get_keyframe_points() / shutdown()
`ReplayTracker` serves them from a recorded run (tests, tools, users without ORB-SLAM).  What IS built here is everything around the tracker:
the keyframe bookkeeping on top of `VanillaMapper` (which rows of the map each keyframe appended) and `update_map` (orbslam.py:68-115) --
after a loop closure / global bundle adjustment every surviving keyframe's slice of the point map moves by `updated_c2w @ inv(old_c2w)`, the
slices of pruned keyframes are dropped and the map is re-packed in the tracker's keyframe order.  The reference does that with a slice, a cat,
an einsum and four appends per keyframe and four `torch.cat` over the whole map; here the host builds a segment table and ONE `ovo_map_reanchor`
launch moves the map into fresh capacity buffers.
"""
from __future__ import annotations

from typing import Any, Dict, List, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from .vanilla_mapper import VanillaMapper


def convert_pose(traj) -> torch.Tensor:
    """The last 12 numbers of a trajectory / keyframe row as a 4 x 4 pose (orbslam.py:9-14), f32 on the host."""
    top = np.asarray(traj, dtype=np.float32).reshape(-1)[-12:].reshape(3, 4)
    return torch.from_numpy(np.concatenate([top, np.asarray([[0, 0, 0, 1]], np.float32)]))


def build_segment_table(kfs: Dict[int, Dict[str, Any]], updated_ids: Sequence[int], head_rows: int = 0) -> Tuple[List[int], np.ndarray, np.ndarray]:
    """The re-packing of orbslam.py:80-107 as a table: for the tracker's keyframes IN ITS ORDER, skipping the ones `kfs` does not know (:84-88),
    (kept ids, seg_src i64[K], seg_dst i64[K + 1]) -- segment k copies rows kfs[id]["pcd_idxs"] to rows [seg_dst[k], seg_dst[k + 1]).
    `head_rows` > 0: a leading segment [0, head_rows) that stays where it is (rows that belong to no keyframe: the map a pipeline was seeded with);
    the keyframes' segments follow it, so the arrays are one entry longer than `kept`."""
    kept = [int(i) for i in updated_ids if int(i) in kfs]
    head = [(0, int(head_rows))] if head_rows > 0 else []
    runs = head + [tuple(kfs[i]["pcd_idxs"]) for i in kept]
    src = np.asarray([a for a, _ in runs], dtype=np.int64).reshape(-1)
    length = np.asarray([b - a for a, b in runs], dtype=np.int64).reshape(-1)
    dst = np.zeros(len(runs) + 1, dtype=np.int64)
    np.cumsum(length, out=dst[1:])
    return kept, src, dst


def map_reanchor(src, out, n_src: int, seg_src: np.ndarray, seg_dst: np.ndarray, seg_T: np.ndarray, ws: torch.Tensor = None) -> int:
    """`ovo_map_reanchor` on the current stream: src / out = (xyz f32[*,3], ids i32[*], ins i32[*], rgb u8[*,3] or None) device tensors, the
    segment table as host arrays.  Returns the rows written (seg_dst[K])."""
    lib = L.load()
    seg_src = np.ascontiguousarray(seg_src, dtype=np.int64)
    seg_dst = np.ascontiguousarray(seg_dst, dtype=np.int64)
    seg_T = np.ascontiguousarray(seg_T, dtype=np.float32).reshape(-1)
    K = int(seg_src.shape[0])
    if seg_dst.shape[0] != K + 1 or seg_T.shape[0] != 12 * K:
        raise L.OvoHipError(f"map_reanchor: {K} segments need seg_dst[{K + 1}] and seg_T[{K}, 12]")
    names = ("xyz", "ids", "ins", "rgb")
    dtypes = (torch.float32, torch.int32, torch.int32, torch.uint8)
    for group in (src, out):
        for t, name, dt in zip(group, names, dtypes):
            if t is not None:
                L.dev(t, dt, name)
    cap_out = min(int(t.shape[0]) for t in out if t is not None)
    if n_src > min(int(t.shape[0]) for t in src if t is not None):
        raise L.OvoHipError("map_reanchor: n_src exceeds the source buffers")
    nb = int(lib.ovo_map_reanchor_workspace_bytes(K))
    if ws is None:
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=out[0].device)
    L.check(lib.ovo_map_reanchor(L.ptr(src[0]), L.ptr(src[1]), L.ptr(src[2]), L.ptr(src[3]), n_src, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]),
                                 L.ptr(out[3]), cap_out, seg_src.ctypes.data, seg_dst.ctypes.data, seg_T.ctypes.data, K, L.ptr(ws), ws.numel(),
                                 L.stream()))
    return int(seg_dst[K])


def dense_repack(src, out, n_src: int, seg_src: np.ndarray, seg_dst: np.ndarray, n_fill: int, empty_cls: int = -1, empty_conf: float = 0.0,
                 src_shards: int = 1, shard: Tuple[int, int, int] = (0, 1, 4096), ws: torch.Tensor = None) -> int:
    """`ovo_dense_repack` on the current stream: everything a pipeline indexes by map row, moved through the segment table `map_reanchor` used.
    src = (acc f32[src_shards * R, D] or [src_shards, R, D], cnt i32, cls i64 or None, conf f32 or None): the old state, shard-major as
    `parallel.allgather` returns it (src_shards = 1: plain point order); out = the same four for THIS rank's shard (rank, count, block) = `shard`;
    rows [seg_dst[K], n_fill) get the empty state.  Returns the rows written (seg_dst[K])."""
    lib = L.load()
    seg_src = np.ascontiguousarray(seg_src, dtype=np.int64)
    seg_dst = np.ascontiguousarray(seg_dst, dtype=np.int64)
    K = int(seg_src.shape[0])
    if seg_dst.shape[0] != K + 1:
        raise L.OvoHipError(f"dense_repack: {K} segments need seg_dst[{K + 1}]")
    names = ("acc", "cnt", "cls", "conf")
    dtypes = (torch.float32, torch.int32, torch.int64, torch.float32)
    for group in (src, out):
        for t, name, dt in zip(group, names, dtypes):
            if t is not None:
                L.dev(t, dt, name)
    D = int(out[0].shape[-1])
    if int(src[0].shape[-1]) != D:
        raise L.OvoHipError("dense_repack: source and output rows differ in width")
    if any(t is not None and t.numel() // (D if i == 0 else 1) % src_shards for i, t in enumerate(src)):
        raise L.OvoHipError("dense_repack: the source arrays do not split into src_shards equal shards")
    src_rows_local = min(int(t.numel()) // (D if i == 0 else 1) for i, t in enumerate(src) if t is not None) // src_shards
    rows_out = min(int(t.shape[0]) for t in out if t is not None)
    nb = int(lib.ovo_dense_repack_workspace_bytes(K))
    if ws is None:
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=out[0].device)
    L.check(lib.ovo_dense_repack(L.ptr(src[0]), L.ptr(src[1]), L.ptr(src[2]), L.ptr(src[3]), D, src_shards, src_rows_local, n_src,
                                 L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), L.ptr(out[3]), rows_out, int(shard[0]), int(shard[1]), int(shard[2]),
                                 n_fill, int(empty_cls), float(empty_conf), seg_src.ctypes.data, seg_dst.ctypes.data, K, L.ptr(ws), ws.numel(),
                                 L.stream()))
    return int(seg_dst[K])


def reanchor_map(m: VanillaMapper, kfs: Dict[int, Dict[str, Any]], updated_keyframes, world_ref: torch.Tensor, head_rows: int = 0,
                 exact_identity: bool = False, ws: torch.Tensor = None):
    """orbslam.py:68-115 with one launch for the whole map, on any `VanillaMapper` `m` whose keyframes appended the rows `kfs` names:
    `updated_keyframes` = the tracker's keyframe rows (id, then the top three rows of the corrected pose) in ITS order.  Every surviving
    keyframe's rows move by `updated_c2w @ inv(old_c2w)`, pruned keyframes' rows are dropped, the map is re-packed in the tracker's order into
    fresh capacity buffers and `m`'s poses become the surviving keyframes' new ones.  `head_rows`: rows [0, head_rows) belong to no keyframe and
    stay in front under the exact identity.  `exact_identity`: a keyframe whose updated pose is bit-equal to its stored pose gets the exact
    identity instead of `P @ inv(P)` (which is the identity only up to the f32 composition error).
    Returns (kept, seg_src, seg_dst, new_kfs): the table it used -- whatever else is indexed by map row is re-packed through the same one -- and
    the surviving keyframes with their new row ranges; the caller stores `new_kfs`.  The stream is synchronised before the old buffers are released."""
    if m._deferred:                                        # they hold the old buffers' addresses (the rule of _reserve), and `settle` would wait for them forever
        raise L.OvoHipError("update_map: deferred map steps outstanding -- launch the round before the map is re-anchored")
    m.settle()
    updated_kfs = [r for r in updated_keyframes if int(r[0]) in kfs]      # unknown keyframes are skipped (:84-88)
    kept, seg_src, seg_dst = build_segment_table(kfs, [int(r[0]) for r in updated_kfs], head_rows)
    h = len(seg_src) - len(kept)                           # 1 with a head segment
    identity = np.eye(4, dtype=np.float32)[:3].reshape(-1)
    seg_T = np.zeros((len(seg_src), 12), dtype=np.float32)
    seg_T[:h] = identity
    poses = []
    for k, (kf_id, updated_kf) in enumerate(zip(kept, updated_kfs)):
        kf_c2w = m._host_pose(kf_id, m.estimated_c2ws[kf_id]).float()
        updated_kf_c2w = world_ref @ convert_pose(np.asarray(updated_kf)[1:13])
        if exact_identity and torch.equal(updated_kf_c2w, kf_c2w):
            seg_T[h + k] = identity
        else:
            transform = updated_kf_c2w @ torch.linalg.inv(kf_c2w)      # the reference's own expression (:93), f32 on the CPU
            seg_T[h + k] = transform[:3].reshape(-1).numpy()
        poses.append(updated_kf_c2w)
    total = int(seg_dst[-1])
    dev, cap = m.device, max(m._cap, total)                # > _cap only when the tracker lists a keyframe twice
    out = (torch.empty((cap, 3), dtype=torch.float32, device=dev), torch.empty((cap,), dtype=torch.int32, device=dev),
           torch.empty((cap,), dtype=torch.int32, device=dev), torch.empty((cap, 3), dtype=torch.uint8, device=dev))
    map_reanchor((m._xyz, m._ids, m._ins, m._rgb), out, m._n_known, seg_src, seg_dst, seg_T, ws)
    torch.cuda.current_stream().synchronize()              # the old buffers are released below, and other streams may read the new ones next
    m._xyz, m._ids, m._ins, m._rgb = out
    m._cap = cap
    m._n = total                                           # nothing in flight: map_ref() hands the host's size over and the device state is re-seeded from it
    new_kfs, new_c2w = {}, {}
    for k, kf_id in enumerate(kept):
        new_kfs[kf_id] = {"id": kfs[kf_id]["id"], "pcd_idxs": (int(seg_dst[h + k]), int(seg_dst[h + k + 1]))}
        new_c2w[kfs[kf_id]["id"]] = poses[k]
    m.estimated_c2ws = new_c2w                             # only the surviving keyframes' poses (:109)
    m._c2w_host = dict(new_c2w)
    return kept, seg_src, seg_dst, new_kfs


class ReplayTracker:
    """A recorded tracker run served through the seven methods `WrapperORBSLAM` calls.  Per frame (in the order frames will be fed):
    `trajectory[i]` 13 numbers (frame id, then the top three rows of the pose), `is_kf[i]`, `states[i]` (default: all OK) and `big_change[i]`
    (default: all 0); `keyframe_points[idx]`: the keyframe rows (13 numbers each) the tracker reports once its big-change index is `idx`."""
    OK = 2                                                 # ORB-SLAM3's TrackingState.OK

    def __init__(self, trajectory, is_kf, states=None, big_change=None, keyframe_points=None) -> None:
        self.trajectory = [np.asarray(r, dtype=np.float32).reshape(13) for r in trajectory]
        n = len(self.trajectory)
        self.is_kf = [bool(v) for v in is_kf]
        self.states = [self.OK] * n if states is None else list(states)
        self.big_change = [0] * n if big_change is None else [int(v) for v in big_change]
        self.keyframe_points = {int(k): [np.asarray(r, dtype=np.float32).reshape(13) for r in v] for k, v in (keyframe_points or {}).items()}
        if not (len(self.is_kf) == len(self.states) == len(self.big_change) == n):
            raise ValueError("ReplayTracker: one trajectory row, keyframe flag, state and big-change index per frame")
        self._i = -1
        self.processed: List[Any] = []                     # the time stamps handed to process_image_rgbd
        self.closed = False

    def process_image_rgbd(self, rgb, depth, t) -> None:
        if self._i + 1 >= len(self.trajectory):
            raise IndexError("ReplayTracker: the recorded run has no more frames")
        self._i += 1
        self.processed.append(t)

    def _cur(self) -> int:
        if self._i < 0:
            raise RuntimeError("ReplayTracker: no frame processed yet")
        return self._i

    def get_tracking_state(self):
        return self.states[self._cur()]

    def get_last_trajectory_point(self):
        return self.trajectory[self._cur()]

    def is_last_frame_kf(self) -> bool:
        return self.is_kf[self._cur()]

    def get_last_big_change_idx(self) -> int:
        return self.big_change[self._cur()]

    def get_keyframe_points(self):
        return self.keyframe_points[self.get_last_big_change_idx()]

    def shutdown(self) -> None:
        self.closed = True


class WrapperORBSLAM(VanillaMapper):
    """Same constructor and methods as the reference class (orbslam.py:17-120) plus `tracker=` / `ok_state=`: tracking succeeded when
    `tracker.get_tracking_state() == ok_state` (default: the tracker's own `OK`, else ORB-SLAM3's TrackingState.OK = 2)."""

    def __init__(self, config: Dict[str, Any], cam_intrinsics: torch.Tensor, world_ref=torch.eye(4), tracker=None, ok_state=None) -> None:
        if tracker is None:
            raise NotImplementedError("WrapperORBSLAM needs tracker=: the ORB-SLAM3 binding is not built here (ReplayTracker serves a recorded run)")
        self.tracker = None                                # __del__ is safe whatever happens below
        super().__init__(config, cam_intrinsics)
        self.close_loops = config.get("slam", {}).get("close_loops", True)
        self.last_big_change_id = 0
        self.map_updated = False
        self.world_ref = torch.as_tensor(world_ref).detach().cpu().float()
        self.kfs = {}
        self.ok_state = ok_state if ok_state is not None else getattr(tracker, "OK", 2)
        self._reanchor_ws = None
        self.tracker = tracker

    def track_camera(self, frame_data: List[Any]) -> None:
        """orbslam.py:39-50; the pose stays on the host (see VanillaMapper.track_camera)."""
        frame_id, rgb_image, depth_image = frame_data[:3]
        self.tracker.process_image_rgbd(rgb_image, depth_image, frame_id)      # blocks until tracking is completed
        tracking_state = self.tracker.get_tracking_state()
        if tracking_state == self.ok_state:
            orb_c2w = self.tracker.get_last_trajectory_point()
            assert int(orb_c2w[0]) == frame_id, "Retrieved wrong frame pose"
            host = self.world_ref @ convert_pose(orb_c2w)
            self._c2w_host[frame_id] = host
            self.estimated_c2ws[frame_id] = host
        else:
            print(f"Tracking state: {tracking_state}!")

    def map(self, frame_data: List[Any], c2w: torch.Tensor) -> None:
        """orbslam.py:52-66."""
        if self.tracker.is_last_frame_kf():
            frame_id = frame_data[0]
            first_p_idx = self._n                          # exact: settles what is in flight
            super().map(frame_data, c2w)
            last_p_idx = self._n
            self.kfs[frame_id] = {"id": frame_id, "pcd_idxs": (first_p_idx, last_p_idx)}
        last_big_change_id = self.tracker.get_last_big_change_idx()
        if self.close_loops and last_big_change_id != self.last_big_change_id:
            self.last_big_change_id = last_big_change_id
            self.update_map()

    def update_map(self) -> None:
        """orbslam.py:68-115 with one launch for the whole map (`reanchor_map`)."""
        rows = self.tracker.get_keyframe_points()
        nb = int(L.load().ovo_map_reanchor_workspace_bytes(sum(int(r[0]) in self.kfs for r in rows)))
        if self._reanchor_ws is None or self._reanchor_ws.numel() < nb:
            self._reanchor_ws = torch.empty(max(nb, 1 << 12), dtype=torch.uint8, device=self.device)
        *_, self.kfs = reanchor_map(self, self.kfs, rows, self.world_ref, head_rows=0, exact_identity=False, ws=self._reanchor_ws)
        self.map_updated = True

    def __del__(self) -> None:
        tracker = getattr(self, "tracker", None)
        if tracker is not None:
            tracker.shutdown()
