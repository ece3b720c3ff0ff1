"""Semantic core of the open-vocabulary map on MI355X: mask <-> 3D-instance tracking, keyframe queue,
descriptor fusion, text query.

Mirror of the reference's `ovo/entities/ovo.py:OVO` -- the "entities update" API `OVOSemMap.run` and
`run_eval.py` call: same constructor, same methods, same return types, same checkpoint
keys.  What changed underneath:

  reference (ovo.py)                                    here
  ----------------------------------------------------  -------------------------------------------------
  :209-222  cull, gather, project, depth-test, seg      ONE pass `ovo_track_project` over the map: writes a
            lookup as ~15 torch ops + 4 compactions      per-point mask id and the [mask x instance] vote table
  :255-280  python loop, >=3 device syncs per mask       `ovo_vote_stats` -> one 16 B/mask D2H, host decisions on
                                                         that table (instance-id allocation order preserved)
  :228-229,:280 clone + two scatters                     `ovo_assign_instances`
  :349,:437 descriptors to CPU, dict of tensors          DescriptorBank rows on the GPU
  :459-460  per-instance torch fusion on CPU             one `ovo_fuse_views` launch per keyframe
  :513-527  re-stack + re-upload on every query          gather from the resident table, `ovo_similarity`
"""
from __future__ import annotations

import contextlib
import time
from collections import deque
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib as L
from ..utils import geometry_utils as G
from .descriptor_bank import DescriptorBank, KeyframeView
from .instance3d import Instance3D
from .token_lookahead import TokenLookahead


def _timed(slot: str):
    """Per-stage wall clock like the reference's `profil` decorator (ovo.py:101-119), active when config['log']."""
    def deco(fn):
        def wrapper(self, *a, **k):
            if not self.config.get("log", False):
                return fn(self, *a, **k)
            torch.cuda.synchronize()
            t0 = time.time()
            out = fn(self, *a, **k)
            torch.cuda.synchronize()
            self._time_cache.append(time.time() - t0)
            return out
        return wrapper
    return deco


class OVO:
    def __init__(self, config: Dict[str, Any], logger=None, scene_name: Optional[str] = None,
                 cam_intrinsics: Optional[torch.Tensor] = None, eval: bool = False, device="cuda",
                 clip_generator=None, mask_generator=None) -> None:
        """Reference: ovo.py:24-69.  `clip_generator` / `mask_generator` may be injected (tests, bench)."""
        if not eval:
            assert cam_intrinsics is not None, "Camera intrinsics required for reconstruction!"
        config.setdefault("sam", {})
        config.setdefault("clip", {})
        config["sam"]["multi_crop"] = config["clip"].get("embed_type", "vanilla") != "vanilla"
        self.cam_intrinsics = cam_intrinsics
        self._K_host = None if cam_intrinsics is None else G._cpu32(cam_intrinsics).contiguous()
        self.config = config
        self.logger = logger
        self.debug_info = config.get("debug_info", False)
        self.device = device
        self.n_top_views = config["clip"].get("k_top_views", 0)
        Instance3D.n_top_kf = self.n_top_views
        Instance3D.set_fusion(config["clip"].get("fusion", "l1_medoid"), config["clip"].get("mv_fuser_ckpt"))
        if "mask_res" in config["sam"] and "mask_res" not in config["clip"]:
            config["clip"]["mask_res"] = config["sam"]["mask_res"]

        if clip_generator is None:
            from .clip_generator import CLIPGenerator
            clip_generator = CLIPGenerator(config["clip"], device=device)
        self.clip_generator = clip_generator
        if not eval and mask_generator is None:
            from .mask_generator import MaskGenerator
            mask_generator = MaskGenerator(config["sam"], scene_name, device=device)
        self.mask_generator = None if eval else mask_generator

        self.bank = DescriptorBank(self.clip_generator.clip_dim, device)
        self.keyframes = {"ins_descriptors": dict(), "frame_id": list(), "ins_maps": list()}
        self.keyframes_queue = deque([])
        self.lookahead: Optional[TokenLookahead] = None   # ViT tokens computed ahead of `_extract_clip` (made by the first prefetch call)
        self._planned_kfs: set = set()                # keyframes whose descriptors are planned (rows decided) but not stored yet
        self.objects: Dict[int, Instance3D] = dict()
        self._time_cache: List[float] = []
        self.next_ins_id = 0
        self.kf_id = 0
        self.last_instance_table: Optional[torch.Tensor] = None     # i32[n_slots]: what the last update_map did to the instance ids (None: nothing)
        self.last_point_seg: Optional[torch.Tensor] = None     # i16[N] mask id per map point of the last keyframe
        self.last_mask_rows: Optional[List[int]] = None
        # (rank, world, block) of the dense accumulators' point shards: the tracking chain then lists the points its masks cover (`ovo_track_step_t.hits`)
        # for `ovo_scatter_accum_query`; None: no list.  `last_hits` = (hits i32[...], pointer of the device-side count) of the last keyframe, or None
        self.hit_shard: Optional[Tuple[int, int, int]] = None
        self.last_hits = None
        # native keyframe chain (`ovo_track_step`): the next instance id also lives on the device; results arrive in pinned blocks
        self._track_pending: deque = deque()
        self._track_ring = None
        self._track_ring_slots = 32                               # FramePipeline sizes it for its rounds (2 x world + margin) before the first keyframe
        self.last_n_points = 0                                    # map size the last tracked keyframe saw
        self._next_ins_dev = None
        self._own_state = None
        # loop-closure thresholds (ovo.py:62-65); update_map itself is a "next" row
        self.th_centroid = config.get("th_centroid", 1.5)
        self.th_cossim = config.get("th_cossim", 0.81)
        self.th_points = config.get("th_points", 0.1)

    # ------------------------------------------------------------------ device moves (ovo.py:72-99)
    def to(self, device: str) -> None:
        return self.cuda() if "cuda" in device else self.cpu()

    def cpu(self) -> None:
        """The reference parks its models on the CPU here; this build's kernels only run on the GPU, so
        the call releases nothing and only records the request."""
        self.device = "cpu"

    def cuda(self) -> None:
        self.device = "cuda"

    # ------------------------------------------------------------------ per-keyframe entry point
    def detect_and_track_objects(self, frame_data, map_data, c2w: torch.Tensor):
        """Reference: ovo.py:121-166.  Returns the updated i32[N] per-point instance ids, or None."""
        frame_id, image = frame_data[:2]
        seg_map, binary_maps = self._get_masks(image, frame_id)
        if len(seg_map) == 0:
            print(f"No mask segmented in {frame_id}!")
            return None
        first_new = self.next_ins_id
        matched, binary_maps, n_matched, updated = self._match_and_track_instances(
            frame_data[1:], map_data, c2w, seg_map, binary_maps)
        self.keyframes_queue.append([matched, binary_maps, image, self.kf_id])
        self.kf_id += 1
        if self.config.get("log", False):
            self.keyframes["frame_id"].append(frame_id)
            if self.logger is not None:
                self.logger.log_ovo_stats({"frame_id": frame_id, "n_obj": [self.next_ins_id - first_new],
                                           "n_matches": n_matched, "t_sam": round(self._time_cache[0], 2),
                                           "t_obj": round(self._time_cache[1], 3)}, print_output=True)
            self._time_cache = []
        return updated

    def detect_and_track_launch(self, frame_data, slam, c2w, stream=None, defer: bool = False) -> Optional[Dict[str, Any]]:
        """`detect_and_track_objects` split in two (MI355X extension): this half gets the masks and QUEUES the tracking chain against
        `slam`'s device-resident map (whose `map_launch` calls may be in flight); `detect_and_track_finish` reads the result block.
        A round of keyframes is queued back to back and finished in order: the host never stalls the device between keyframes.
        Only for keyframes `_native_ok` accepts (the caller checks) and without per-stage logging."""
        frame_id, image = frame_data[:2]
        seg_map, binary_maps = self.mask_generator.get_masks(image, frame_id)
        if len(seg_map) == 0:
            print(f"No mask segmented in {frame_id}!")
            return None
        pend = self.track_launch(frame_data[1:], None, c2w, seg_map, binary_maps, slam=slam, stream=stream, defer=defer)
        pend["frame"] = (frame_id, image)
        return pend

    def detect_and_track_finish(self, pend: Optional[Dict[str, Any]], want_maps: bool = True):
        """`want_maps=False` (a keyframe another rank owns, pipeline.py): the kept binary maps -- read only by the descriptor extraction of the
        keyframe's owner -- are not gathered; the queued keyframe carries None in their place."""
        if pend is None:
            return None
        frame_id, image = pend["frame"]
        matched, binary_maps, n_matched, updated = self.track_finish(pend, want_maps)
        self.keyframes_queue.append([matched, binary_maps, image, self.kf_id])
        self.kf_id += 1
        return updated

    @_timed("t_sam")
    def _get_masks(self, image: np.ndarray, frame_id: int):
        return self.mask_generator.get_masks(image, frame_id)

    # ------------------------------------------------------------------ tracking
    MAX_RESULT_MASKS = 1024     # masks per keyframe a slot of the pinned result ring holds (more: the host-decision path below)

    @_timed("t_obj")
    def _match_and_track_instances(self, frame_data, map_data, c2w, seg_map: torch.Tensor, binary_maps: torch.Tensor):
        """Reference: ovo.py:182-238 (with :240-324 inlined).  One C call queues the whole chain -- cull / project / depth-test / seg
        lookup / votes / decisions / assignment / mask fusion (`ovo_track_step`) -- and one pinned result block comes back."""
        if not self._native_ok(binary_maps):
            return self._match_and_track_instances_host(frame_data, map_data, c2w, seg_map, binary_maps)
        pend = self.track_launch(frame_data, map_data, c2w, seg_map, binary_maps)
        return self.track_finish(pend)

    def _native_ok(self, binary_maps: torch.Tensor) -> bool:
        """The device-side decisions cover the ordinary state; these corners keep the host-decision path: debug exports (point-id lists,
        instance maps), mask sizes the 16-byte kernels cannot take, and a restored checkpoint whose `next_ins_id` restarts below the
        existing ids (the reference's own behaviour, ovo.py:559-575: new ids then overwrite old instances)."""
        n_all = int(binary_maps.shape[0])
        pixels = binary_maps[0].numel() if n_all else 0
        return (not self.debug_info and not self.config.get("host_decisions", False) and 0 < n_all <= self.MAX_RESULT_MASKS and pixels % 16 == 0 and binary_maps.is_contiguous()
                and binary_maps.element_size() == 1 and (not self.objects or self.next_ins_id > max(self.objects)))

    def track_launch(self, frame_data, map_data, c2w, seg_map: torch.Tensor, binary_maps: torch.Tensor, slam=None, stream=None,
                     defer: bool = False) -> Dict[str, Any]:
        """Queue the tracking chain of one keyframe (MI355X extension; no host round trip).  `map_data` as in the reference; with
        `slam` (a VanillaMapper whose `map_launch` calls may still be in flight) the map's size is read on the device and the
        instance ids are assigned in place in the mapper's buffer.  Returns the pending record `track_finish` consumes; several
        keyframes may be queued before the first is finished (they must be finished in order).  `stream`: queue on this torch stream
        instead of the current one (the mapper's `map_launch` calls must use the same one); the chain then starts after everything queued
        on the CURRENT stream so far (its inputs and buffers are allocated here), and `track_finish` makes the current stream wait for it.
        `defer`: do not launch; the `ovo_track_step_t` is left in the record (`pend["step"]`) for the caller's `ovo_round_chain`, who also
        sets `pend["done"]`."""
        lib = L.load()
        h, w = frame_data[1].shape
        if self._track_ring is None:
            self._track_ring = L.PinnedRing(8 + 6 * self.MAX_RESULT_MASKS, np.int32, getattr(self, "_track_ring_slots", 32))
        a = L.TrackStep()
        if slam is not None:
            dev = slam._xyz.device
            a.map = slam.map_ref()
            a.n_upper = slam._n_upper
            ins_view = None
        else:
            points_3d, points_ids, points_ins_ids = map_data
            dev = points_3d.device
            pts = L.dev(points_3d, torch.float32, "points_3d")
            ins_view = L.dev(points_ins_ids.reshape(-1), torch.int32, "points_ins_ids").clone()      # the reference returns a copy (:228)
            if self._own_state is None:
                self._own_state = torch.zeros(4, dtype=torch.int64, device=dev)
            n = pts.shape[0]
            a.map = L.MapRef(pts.data_ptr(), 0, ins_view.data_ptr(), 0, n, self._own_state.data_ptr(), n, 0)
            a.n_upper = n
        if self._next_ins_dev is None:
            self._next_ins_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        if len(self._track_pending) >= self._track_ring.slots - 1:
            raise L.OvoHipError("too many keyframes queued without track_finish")
        depth, a.cam, a.ratio, seg_map, a.hist_cols = self._track_inputs(frame_data, c2w, seg_map, dev)
        a.depth = depth.data_ptr()
        if self.config.get("depth_filter", False):                # filtered in the chain, into a scratch image
            scratch = getattr(self, "_depth_scratch", None)
            if scratch is None or scratch.numel() < h * w or scratch.device != depth.device:
                scratch = self._depth_scratch = torch.empty(h * w, dtype=torch.float32, device=dev)
            a.filter_depth, a.depth_scratch = 1, scratch.data_ptr()
        n_masks = int(binary_maps.shape[0])
        a.seg_map, a.seg_h, a.seg_w = seg_map.data_ptr(), seg_map.shape[0], seg_map.shape[1]
        a.masks, a.n_masks, a.pixels = binary_maps.data_ptr(), n_masks, binary_maps[0].numel()
        a.track_th = int(self.config["track_th"])
        point_seg = torch.empty((max(int(a.n_upper), 1) + 0xfffff) & ~0xfffff, dtype=torch.int16, device=dev)    # 1 Mi-point steps: the allocator re-uses blocks
        a.point_seg = point_seg.data_ptr()
        hits = None
        if self.hit_shard is not None:                            # the list and, behind it, its device-side count (zeroed by the step itself)
            hits = torch.empty(point_seg.numel() + 4, dtype=torch.int32, device=dev)
            a.hits, a.n_hits = hits.data_ptr(), hits[point_seg.numel():].data_ptr()
            a.hit_shard_rank, a.hit_shard_count, a.hit_shard_block = self.hit_shard
        a.ws_bytes = lib.ovo_track_workspace_bytes(n_masks, a.hist_cols)
        ws = getattr(self, "_track_ws", None)
        if ws is None or ws.numel() < a.ws_bytes or ws.device != point_seg.device:
            # grown geometrically (hist_cols rises with every queued keyframe); steps queued or built earlier keep THEIR tensor alive through
            # pend["keep"] -- they hold its raw address, and a freed block could be handed to the next keyframe's masks or depth copy
            grow = max(int(a.ws_bytes), 1 << 20, 2 * (ws.numel() if ws is not None else 0))
            ws = self._track_ws = torch.empty(grow, dtype=torch.uint8, device=dev)
            if stream is not None:
                ws.record_stream(stream)                          # allocated on the current stream, used on the chain stream
        a.ws = ws.data_ptr()
        a.next_ins, a.next_ins_host = self._next_ins_dev.data_ptr(), (self.next_ins_id if not self._track_pending else -1)
        seq, slot = self._track_ring.next()
        a.result_host, a.seq = slot, seq
        done = None
        if defer:
            pass
        elif stream is None:
            L.check(lib.ovo_track_step(L.C.byref(a), L.stream()))
        else:
            ready = torch.cuda.Event()                            # the buffers above were allocated (and the masks produced) on the current
            ready.record()                                        # stream: the chain must not touch them before this point of it
            stream.wait_event(ready)
            L.check(lib.ovo_track_step(L.C.byref(a), L.C.c_void_p(stream.cuda_stream)))
            done = torch.cuda.Event()
            done.record(stream)
        pend = {"seq": seq, "n_masks": n_masks, "point_seg": point_seg, "hits": hits, "binary_maps": binary_maps, "ins": ins_view, "slam": slam,
                "keep": (depth, seg_map, ws), "done": done, "step": a if defer else None}
        self._track_pending.append(pend)
        return pend

    def track_finish(self, pend: Dict[str, Any], want_maps: bool = True):
        """Wait for the keyframe's result block and do the host bookkeeping of ovo.py:255-324 on it (instances, top-k heaps, kept mask
        rows).  Returns what `_match_and_track_instances` returns (`want_maps=False`: None instead of the kept binary maps)."""
        if not self._track_pending or self._track_pending[0] is not pend:
            raise L.OvoHipError("track_finish: keyframes must be finished in the order they were launched")
        res = self._track_ring.wait(pend["seq"])
        self._track_pending.popleft()
        if int(res[6]) != 0:
            raise L.OvoHipError("the round chain aborted on the device (a grid barrier timed out)")
        if pend["done"] is not None:                               # what follows on the current stream reads the chain's outputs, which were
            cur = torch.cuda.current_stream()                      # allocated on the chain's stream: tell the allocator about the second user
            cur.wait_event(pend["done"])
            pend["point_seg"].record_stream(cur)
            if pend["hits"] is not None:
                pend["hits"].record_stream(cur)
            pend["binary_maps"].record_stream(cur)
        kf_id, n_masks = self.kf_id, pend["n_masks"]
        n, n_matched, next_after = int(res[1]), int(res[3]), int(res[4])
        table = res[8:8 + 6 * n_masks].reshape(n_masks, 6).tolist()
        matched_info, _ = self._walk_masks(table, kf_id, next_after)
        binary_maps = pend["binary_maps"]                       # fused in place by the chain (ovo.py:303)
        matched_ins_ids, keep_rows, mask_rows = self._keep_rows(matched_info, kf_id, n_masks, lambda first: table[first][5])
        kept = L.gather_rows(binary_maps, keep_rows) if want_maps else None
        slam = pend["slam"]
        updated = pend["ins"] if slam is None else slam._ins[:n]
        self.last_point_seg, self.last_mask_rows, self.last_n_points = pend["point_seg"][:n], mask_rows, n
        self.last_hits = pend["hits"]
        return matched_ins_ids, kept, n_matched, updated

    def _track_inputs(self, frame_data, c2w, seg_map: torch.Tensor, dev):
        """What tracking one keyframe needs of the frame, on either decision path: (depth f32[h, w] on `dev`, camera struct, Ratio, seg map
        i32 on the device, columns of the vote table).  The pose goes through the host for the frustum set-up (a CPU tensor costs nothing, a
        device tensor one 64-byte D2H)."""
        _, depth_in, ratio = frame_data
        h, w = depth_in.shape
        depth = G.to_device(depth_in, torch.float32, dev)
        near, far = G.depth_range(depth_in)                       # frustum uses the raw depth (:209)
        cam = G.frame_camera(near, far, h, w, G._cpu32(c2w).contiguous(), self._K_host, self.config["match_distance_th"])
        r = L.Ratio(1, float(ratio[0]), float(ratio[1]), int(ratio[2])) if len(ratio) > 0 else L.Ratio(0, 1.0, 1.0, 0)
        # votes table columns: [unassigned | instance 0 .. max id]; ids the queued keyframes may still allocate are covered (restore_dict leaves
        # next_ins_id at 0 like the reference: hence the instances' own maximum)
        queued_masks = sum(p["n_masks"] for p in self._track_pending)
        hist_cols = max(self.next_ins_id + queued_masks, max(self.objects) + 1 if self.objects else 0) + 1
        return depth, cam, r, L.dev(seg_map, torch.int32, "seg_map"), hist_cols

    def _walk_masks(self, table, kf_id: int, device_next: Optional[int] = None):
        """The decisions of ovo.py:255-280 on the per-mask table, in mask order: rows (points, assigned points, their mode instance, mask
        area) from `ovo_vote_stats`, or with the device's own decision behind them (target id of a NEW instance, fused area) from
        `ovo_track_step` -- the ids allocated here must then be the device's, and `device_next` its next free id.
        Returns ({instance: [(mask, area), ...]}, instance per mask or -1)."""
        track_th = self.config["track_th"]
        objects = self.objects
        matched_info: Dict[int, List[Tuple[int, int]]] = {}
        target = [-1] * len(table)
        for m, (n_pts, n_assigned, mode_id, area, *device) in enumerate(table):
            if n_pts <= track_th:
                continue
            if n_assigned > track_th:
                target[m] = mode_id
                objects[mode_id].observe(kf_id, area)
                matched_info.setdefault(mode_id, []).append((m, area))
            elif n_pts - n_assigned > track_th:
                target[m] = new_id = self.next_ins_id
                self.next_ins_id += 1
                if device and device[0] != new_id:
                    raise L.OvoHipError(f"instance ids diverged between host and device ({device[0]} vs {new_id})")
                objects[new_id] = Instance3D(new_id, kf_id=kf_id, points_ids=[], mask_area=area, bank=self.bank)
                matched_info[new_id] = [(m, area)]
        if device_next is not None and device_next != self.next_ins_id:
            raise L.OvoHipError(f"next instance id diverged between host and device ({device_next} vs {self.next_ins_id})")
        return matched_info, target

    def _keep_rows(self, matched_info, kf_id: int, n_masks: int, fused_area):
        """The bookkeeping of ovo.py:299-322 once the masks of one instance are fused into its first mask: `fused_area(first mask)` feeds the
        top-k view heap (:305-309), and an instance keeps a row only while this keyframe is among its top views.  Returns (matched instance
        ids, the mask row each keeps, per ORIGINAL mask index the kept row it contributes to or -1 -- for the dense accumulator)."""
        matched_ins_ids, keep_rows = [], []
        mask_rows = [-1] * n_masks
        for ins_id, hits in matched_info.items():
            first = hits[0][0]
            if len(hits) > 1 and self.n_top_views > 0:
                self.objects[ins_id].add_top_kf(kf_id, int(fused_area(first)))
            if self.n_top_views <= 0 or self.objects[ins_id].is_top_kf(kf_id):
                for m, _ in hits:
                    mask_rows[m] = len(matched_ins_ids)
                matched_ins_ids.append(ins_id)
                keep_rows.append(first)
        return matched_ins_ids, keep_rows, mask_rows

    def _match_and_track_instances_host(self, frame_data, map_data, c2w, seg_map: torch.Tensor, binary_maps: torch.Tensor):
        """The same stage with the decisions of ovo.py:255-280 taken on the host from the vote statistics (one D2H of 16 B per mask):
        debug exports, odd mask sizes, restored checkpoints (`_native_ok`)."""
        kf_id = self.kf_id
        points_3d, points_ids, points_ins_ids = map_data
        dev = points_3d.device
        lib = L.load()
        depth, cam, r, seg_map, hist_cols = self._track_inputs(frame_data, c2w, seg_map, dev)
        if self.config.get("depth_filter", False):
            depth = G.depth_filter(depth)

        pts = L.dev(points_3d, torch.float32, "points_3d")
        ins = L.dev(points_ins_ids.reshape(-1), torch.int32, "points_ins_ids")
        n, n_masks = pts.shape[0], int(binary_maps.shape[0])
        point_seg = torch.empty(n, dtype=torch.int16, device=dev)
        hist = torch.empty((n_masks, hist_cols), dtype=torch.int32, device=dev)
        small = torch.empty(n_masks * 4 + 4, dtype=torch.int32, device=dev)        # stats | {in frustum, matched} as i64
        stats, counters = small[:n_masks * 4], small[n_masks * 4:]
        L.check(lib.ovo_track_project(L.ptr(pts), L.ptr(ins), n, cam, L.ptr(depth), L.ptr(seg_map), seg_map.shape[0],
                                      seg_map.shape[1], r, L.ptr(point_seg), L.ptr(hist), n_masks, hist_cols,
                                      L.ptr(counters), L.stream()))
        L.check(lib.ovo_vote_stats(L.ptr(hist), n_masks, hist_cols, L.ptr(seg_map), seg_map.numel(), L.ptr(stats), L.stream()))
        host = small.cpu()                                           # the one sync of the tracking stage
        n_matched = int(host[n_masks * 4:].view(torch.int64)[1])
        matched_info, target = self._walk_masks(host[:n_masks * 4].view(n_masks, 4).tolist(), kf_id)

        mask_target = torch.tensor(target, dtype=torch.int32).to(dev, non_blocking=True)
        updated = torch.empty_like(ins)
        L.check(lib.ovo_assign_instances(L.ptr(ins), L.ptr(point_seg), n, L.ptr(mask_target), n_masks, L.ptr(updated),
                                         None, L.stream()))
        if self.debug_info:                                        # point-id lists are only exported in debug checkpoints
            pid = points_ids.reshape(-1)
            was_free = ins == -1
            for m, ins_id in enumerate(target):
                if ins_id >= 0:
                    sel = torch.nonzero((point_seg == m) & was_free).reshape(-1)
                    self.objects[ins_id].add_points_ids(pid[sel].reshape(-1, 1).cpu().tolist())

        fused_area = self._fuse_masks_with_same_ins_id(binary_maps, matched_info)
        matched_ins_ids, keep_rows, mask_rows = self._keep_rows(matched_info, kf_id, n_masks, fused_area.__getitem__)
        if binary_maps[0].numel() % 16 == 0 and binary_maps.is_contiguous():
            binary_maps = L.gather_rows(binary_maps, keep_rows)
        else:
            binary_maps = binary_maps.index_select(0, torch.tensor(keep_rows, dtype=torch.int64).to(binary_maps.device, non_blocking=True))
        self.last_point_seg, self.last_mask_rows = point_seg, mask_rows
        self.last_hits = None

        if self.debug_info:
            ins_maps = torch.full(tuple(seg_map.shape), -1, dtype=torch.int32, device=dev)     # == image.shape[:2] (ovo.py:277)
            for row, ins_id in enumerate(matched_ins_ids):
                ins_maps[binary_maps[row]] = ins_id
            self.keyframes["ins_maps"].append(ins_maps.cpu().numpy())
        return matched_ins_ids, binary_maps, n_matched, updated

    @staticmethod
    def instance_image(matched_ins_ids, binary_maps: torch.Tensor, hw=None) -> torch.Tensor:
        """The instance image of a keyframe, i32[H, W] on the masks' device, from what `track_finish` returns: the id of the FIRST kept mask that
        covers the pixel, -1 where none does -- what `TsdfVolume.integrate_labels` / `IcpTracker.fuse_labels` take.  One `ovo_paint_segmap` and one
        gather, no host round trip (the `debug_info` loop that fills `keyframes["ins_maps"]` goes through the host and stays as it is).
        `hw` = (h, w): resampled to that size, nearest neighbour: out[y, x] = image[y * H // h, x * W // w]."""
        if binary_maps.dim() != 3 or binary_maps.dtype not in (torch.bool, torch.uint8) or len(matched_ins_ids) != binary_maps.shape[0]:
            raise ValueError(f"OVO.instance_image: binary_maps must be bool [n, H, W] with one id a mask (got {binary_maps.dtype} {tuple(binary_maps.shape)} "
                             f"for {len(matched_ins_ids)} ids)")
        n, H, W = (int(x) for x in binary_maps.shape)
        dev = binary_maps.device
        if n == 0:
            out = torch.full((H, W), -1, dtype=torch.int32, device=dev)
        else:
            maps = L.dev(binary_maps.view(torch.uint8) if binary_maps.dtype == torch.bool else binary_maps, torch.uint8, "binary_maps")
            seg = torch.empty((H, W), dtype=torch.int32, device=dev)
            L.check(L.load().ovo_paint_segmap(L.ptr(maps), n, H * W, L.ptr(seg), L.stream()))
            ids = torch.tensor([int(i) for i in matched_ins_ids] + [-1], dtype=torch.int32).to(dev, non_blocking=True)
            out = ids[torch.where(seg >= 0, seg, torch.full_like(seg, n)).long()]
        if hw is not None and (int(hw[0]), int(hw[1])) != (H, W):
            h, w = int(hw[0]), int(hw[1])
            ys = (torch.arange(h, device=dev) * H) // h
            xs = (torch.arange(w, device=dev) * W) // w
            out = out[ys[:, None], xs[None, :]]
        return out.contiguous()

    @staticmethod
    def instance_table(n_slots: int, fused: Dict[int, int], removed) -> np.ndarray:
        """What a loop-closure update did to the instance ids, i32[n_slots]: the identity, but a fused instance b -> the a it went into and a removed
        one -> -1.  `TsdfVolume.remap_labels` takes it."""
        table = np.arange(int(n_slots), dtype=np.int32)
        for b_id, a_id in fused.items():
            table[b_id] = a_id
        for r_id in removed:
            table[r_id] = -1
        return table

    def _fuse_masks_with_same_ins_id(self, binary_maps: torch.Tensor, matched_info) -> Dict[int, int]:
        """The ORs of ovo.py:299-306: every further mask of an instance is fused into its first one, in place.  Returns {first mask: fused
        area} when the top-k view heap wants the areas (n_top_views > 0)."""
        lib = L.load()
        pixels = binary_maps[0].numel() if binary_maps.shape[0] else 0
        maps_u8 = binary_maps.view(torch.uint8) if binary_maps.dtype == torch.bool else binary_maps
        pairs = [(hits[0][0], other) for hits in matched_info.values() for other, _ in hits[1:]]
        dst = sorted({d for d, _ in pairs}) if self.n_top_views > 0 else []
        if not pairs:
            return {}
        if pixels % 16 != 0 or not binary_maps.is_contiguous():     # odd image sizes: plain torch
            for d, s in pairs:
                binary_maps[d].logical_or_(binary_maps[s])
            return {d: int(binary_maps[d].sum().item()) for d in dst}
        flat = torch.tensor(pairs, dtype=torch.int32).reshape(-1).to(maps_u8.device, non_blocking=True)
        L.check(lib.ovo_mask_or(L.ptr(maps_u8), pixels, L.ptr(flat), len(pairs), L.stream()))       # all ORs of the keyframe in one launch
        if not dst:
            return {}
        rows = torch.tensor(dst, dtype=torch.int32).to(maps_u8.device, non_blocking=True)
        area = torch.empty(len(dst), dtype=torch.int32, device=maps_u8.device)
        L.check(lib.ovo_mask_area(L.ptr(maps_u8), pixels, L.ptr(rows), len(dst), L.ptr(area), L.stream()))
        return dict(zip(dst, area.tolist()))

    # ------------------------------------------------------------------ descriptors
    def compute_semantic_info(self) -> None:
        if len(self.keyframes_queue) > self.config.get("kf_queue_delay", 0):
            self._compute_semantic_info()

    def complete_semantic_info(self) -> None:
        while len(self.keyframes_queue) > 0:
            self._compute_semantic_info()

    def _compute_semantic_info(self) -> None:
        """Reference: ovo.py:334-364 = plan (which descriptors, which instances re-fuse from which keyframes) -> extract -> apply."""
        plan = self._plan_semantic_info()
        if plan is None:
            return
        clip_embeds = self._extract_clip(plan["image"], plan["binary_maps"])
        self._apply_semantic_plan(plan, clip_embeds)
        if self.config.get("log", False) and self.logger is not None:
            self.logger.log_ovo_stats({"frame_id": self.keyframes["frame_id"][plan["kf_id"]],
                                       "t_clip": round(self._time_cache[0], 2), "t_up": round(self._time_cache[1], 3)},
                                      print_output=True)
        self._time_cache = []

    def _plan_semantic_info(self) -> Optional[Dict[str, Any]]:
        """The host half of ovo.py:334-364 / :440-461 for the oldest queued keyframe, decided NOW from the instances' state: which masks
        get a descriptor (top-k view filter, :342-349) and which instances re-fuse from which keyframes' descriptors (`to_update`, the
        top-k heap / keyframe list: instance3d.py:157-189).  Nothing here needs the descriptors themselves, so a frame-sharded run
        (pipeline.py) plans every keyframe on every rank right after tracking it and applies the descriptors --
        computed by the rank that owns the frame -- later, in keyframe order, with exactly the result of the one-process order."""
        matched_ins_ids, binary_maps, image, kf_id = self.keyframes_queue.popleft()
        if len(matched_ins_ids) == 0:
            self.discard_prefetched(image)
            return None
        if self.n_top_views > 0:
            rows = [j for j, i in enumerate(matched_ins_ids) if self.objects[i].is_top_kf(kf_id)]
            if not rows:
                self.discard_prefetched(image)
                return None
            if len(rows) != len(matched_ins_ids):
                matched_ins_ids = [matched_ins_ids[j] for j in rows]
                if binary_maps is not None:                      # (None: a keyframe whose descriptors another rank extracts)
                    binary_maps = binary_maps[torch.tensor(rows, device=binary_maps.device)]
        self._planned_kfs.add(kf_id)
        updates = self._planned_updates(matched_ins_ids)
        return {"kf_id": kf_id, "matched_ins_ids": matched_ins_ids, "binary_maps": binary_maps, "image": image, "updates": updates}

    def _planned_updates(self, matched_ins_ids) -> List[tuple]:
        """(instance, keyframes to fuse from, in the reference's stacking order[, views already summed]) for every matched instance that is due
        (instance3d.py:157-178); only keyframes whose descriptors exist or are planned count.
        avg_pooling (the configured fusion, ovo.yaml:50) is kept as a RUNNING SUM per instance: the tuple then names only the views that are new
        since the instance's last fusion plus the number already in the sum (0 = start over: first fusion, a summed view evicted from the top-k
        heap, or a full re-fusion in between) -- the mean of all views, without walking an instance's whole view list (which grows with the
        sequence at k_top_views = 10000) on every keyframe it is seen in."""
        known = self._planned_kfs.union(self.keyframes["ins_descriptors"])
        incremental = Instance3D.mv_fusion == "avg_pooling" and not self.config.get("full_refusion", False)
        updates = []
        for ins_id in matched_ins_ids:
            obj = self.objects[ins_id]
            if not obj.to_update:
                continue
            if not incremental:
                views = [kf for kf in obj.fusion_views() if kf in known]
                if views:
                    updates.append((ins_id, views))
                    obj.to_update = False
                continue
            if obj._needs_full:
                views = [kf for kf in obj.fusion_views() if kf in known]
                if not views:
                    continue
                obj._inc_kfs, before = set(views), 0
                obj._pending_kfs = [kf for kf in obj._pending_kfs if kf not in obj._inc_kfs]
                obj._needs_full = False
            else:
                in_views = obj.is_top_kf if obj.n_top_kf > 0 else obj.kfs_ids.__contains__
                views = [kf for kf in obj._pending_kfs if kf in known and kf not in obj._inc_kfs and in_views(kf)]
                obj._pending_kfs = [kf for kf in obj._pending_kfs if kf not in known and in_views(kf)]
                before = len(obj._inc_kfs)
                obj._inc_kfs.update(views)
            obj.to_update = False
            if views:
                updates.append((ins_id, views, before))
        return updates

    def _apply_semantic_plan(self, plan: Dict[str, Any], clip_embeds: torch.Tensor) -> None:
        """The device half: store the keyframe's descriptors, then re-fuse the planned instances in ONE launch (ovo.py:440-461)."""
        kf_id, matched_ins_ids = plan["kf_id"], plan["matched_ins_ids"]
        self.last_clip_embeds, self.last_clip_ins_ids, self.last_clip_kf = clip_embeds, matched_ins_ids, kf_id
        self._store_and_fuse(clip_embeds, matched_ins_ids, kf_id, plan["updates"])

    def _apply_semantic_plans(self, items) -> None:
        """`_apply_semantic_plan` for the keyframes of one multi-GPU round, in keyframe order (MI355X extension): every keyframe's descriptors are
        stored as they are, but the running-sum fusions of the whole round go down as ONE launch -- an instance seen in several keyframes of
        the round gets their rows added in keyframe order, the additions a keyframe-by-keyframe replay would do (nothing reads the instance
        table between the keyframes of a round).  A plan with a full re-fusion (a view left a top-k heap) or a restarted sum sends the round
        through the one-by-one path."""
        items = list(items)
        if len(items) <= 1 or any(len(u) == 2 for p, _ in items for u in p["updates"]):
            for plan, clip in items:
                self._apply_semantic_plan(plan, clip)
            return
        merged: Dict[int, list] = {}
        desc = self.keyframes["ins_descriptors"]
        for plan, clip in items:
            kf_id, matched = plan["kf_id"], plan["matched_ins_ids"]
            self.last_clip_embeds, self.last_clip_ins_ids, self.last_clip_kf = clip, matched, kf_id
            rows = self.bank.append(clip)
            desc[kf_id] = KeyframeView(self.bank, {i: rows[j] for j, i in enumerate(matched) if i != -1})
            self._planned_kfs.discard(kf_id)
            for ins_id, kfs, before in plan["updates"]:
                new = [desc[kf]._rows[ins_id] for kf in kfs]
                cur = merged.get(ins_id)
                if cur is None:
                    merged[ins_id] = [new, before]
                elif before == cur[1] + len(cur[0]):
                    cur[0].extend(new)
                else:                                              # the sum restarts inside the round: keep the order, launch what is pending
                    self.bank.fuse_add([(i, r, b) for i, (r, b) in merged.items()])
                    merged = {ins_id: [new, before]}
        self.bank.fuse_add([(i, r, b) for i, (r, b) in merged.items()])

    def _lookahead(self) -> Optional[TokenLookahead]:
        """The look-ahead object (made on first use); None when the configured embed type has no mask-independent half."""
        tr = getattr(self.clip_generator, "textregion", None)
        if tr is not None and self.lookahead is None:
            self.lookahead = TokenLookahead(tr, self.bank.device)
        return self.lookahead

    def prefetch_image_features(self, image, image_ready=None) -> bool:
        """MI355X extension (no counterpart in the reference): start the ViT forward of `image`'s TextRegion crops NOW on the look-ahead's
        side stream (token_lookahead.py), so that it overlaps the tracking stage (whose host decisions wait on a device->host copy) and the
        SAM2 encoder.  The matching `_extract_clip(image, ...)` call (same image object) picks the tokens up and only pools; any other image
        takes the ordinary path and drops them.  Returns False when the configured embed type has no such half."""
        la = self._lookahead()
        return la is not None and la.encode_one(image, image_ready)

    def prefetch_image_features_batch(self, images, ready=(), stream=None) -> bool:
        """`prefetch_image_features` for SEVERAL keyframes' images in ONE ViT forward (`TokenLookahead.encode`); every `_extract_clip(image, ...)`
        of one of these image objects then only pools its slice."""
        la = self._lookahead()
        return la is not None and la.encode(images, ready, stream)

    def discard_prefetched(self, image) -> None:
        """A keyframe that never reaches `_extract_clip` gives its look-ahead tokens up."""
        if self.lookahead is not None:
            self.lookahead.discard(image)

    @_timed("t_clip")
    def _extract_clip(self, image: np.ndarray, binary_maps: torch.Tensor) -> torch.Tensor:
        """Reference: ovo.py:427-437 -- but the descriptors stay on the GPU."""
        if binary_maps is None:                                   # (pipeline.py: a keyframe another rank owns is tracked with want_maps=False)
            raise L.OvoHipError("_extract_clip: this keyframe's binary maps were not kept (track_finish(want_maps=False)): only its owner pools it")
        la = self.lookahead
        feats = la.take(image) if la is not None else None
        if feats is not None:                                    # tokens from a look-ahead forward: only pool
            tr = self.clip_generator.textregion
            tr._crops(*image.shape[:2])                          # the tiling state of THIS image
            out = tr.pe_value_with_sam2_attn(tr.get_features_mask(binary_maps), feats) if binary_maps.shape[0] > 0 else \
                torch.empty((0, tr.out_dim), dtype=torch.float32, device=feats.device)
            la.release(image)
            return out
        if isinstance(image, torch.Tensor):                      # already resident: HWC u8 -> CHW
            img = image.to(self.bank.device).permute(2, 0, 1).contiguous()
        else:
            img = torch.from_numpy(np.ascontiguousarray(image.transpose((2, 0, 1)))).to(self.bank.device, non_blocking=True)
        with la.workspace() if la is not None else contextlib.nullcontext():      # the encoder's workspace is the look-ahead's too
            return self.clip_generator.extract_clip(img, binary_maps, self.config.get("return_all_clips", False))

    @_timed("t_up")
    def _store_and_fuse(self, clip_embeds: torch.Tensor, matched_ins_ids: List[int], kf_id: int, updates) -> None:
        rows = self.bank.append(clip_embeds)
        self.keyframes["ins_descriptors"][kf_id] = KeyframeView(
            self.bank, {i: rows[j] for j, i in enumerate(matched_ins_ids) if i != -1})
        self._planned_kfs.discard(kf_id)
        desc = self.keyframes["ins_descriptors"]
        full = [(u[0], [desc[kf]._rows[u[0]] for kf in u[1]]) for u in updates if len(u) == 2]
        add = [(u[0], [desc[kf]._rows[u[0]] for kf in u[1]], u[2]) for u in updates if len(u) == 3]
        self.bank.fuse(full, Instance3D.mv_fusion)
        self.bank.fuse_add(add)

    def _update_matched_objects_clip(self, clip_embeds: torch.Tensor, matched_ins_ids: List[int], kf_id: int) -> None:
        """Reference: ovo.py:440-461; all touched instances are fused in one launch."""
        self._planned_kfs.add(kf_id)
        self._store_and_fuse(clip_embeds, matched_ins_ids, kf_id, self._planned_updates(matched_ins_ids))

    def update_objects_clip(self, force_update: bool = False) -> None:
        for obj in self.objects.values():
            obj.update_clip(self.keyframes["ins_descriptors"], force_update=force_update)

    def update_map(self, map_data, kfs, same_instance=None):
        """Loop-closure semantic update.  Reference: ovo.py:366-424 with instance_utils.py:5-35.
        `same_instance(id1, id2) -> bool` (optional, not in the reference's signature) replaces the geometric pair predicate of
        instance_utils.py:5-24 -- the seam the golden fixture `loopclose.npz` (case "table") pins the control flow through.

        Same steps and the same greedy merge order; what changed underneath: one pass over the map gives every instance's
        point count and centroid (`ovo_instance_moments`, replacing `unique()` + a boolean slice per instance); the
        pair predicate is static during the merge loop (it only reads centroids, point sets and descriptors taken BEFORE
        any merge), so centroid distances and descriptor cosines are evaluated for all pairs at once, the nearest-neighbour
        test (`(dists < th).mean()` over an Open3D KD-tree in the reference) runs for the surviving pairs in one launch
        (`ovo_near_fraction`), and the per-merge relabelling of the map becomes one `ovo_remap_instances` pass.

        `self.last_instance_table` records what happened to the ids (`instance_table`: i32[n_slots] on the map's device, fused b -> a, removed -> -1),
        or None when nothing changed: a label volume follows with `TsdfVolume.remap_labels(ovo.last_instance_table)`."""
        lib = L.load()
        self.last_instance_table = None
        self.complete_semantic_info()
        points_3d, _, points_ins_ids = map_data
        for i, kf in enumerate(self.keyframes["frame_id"]):           # 0.1 keyframes the SLAM back end deleted
            if kf not in kfs:
                if kf in self.keyframes["ins_descriptors"]:
                    self.keyframes["ins_descriptors"].pop(kf)
                self.keyframes["frame_id"][i] = "Deleted"
        if not self.objects:
            return points_ins_ids
        pts = L.dev(points_3d, torch.float32, "points_3d")
        ins = L.dev(points_ins_ids.reshape(-1), torch.int32, "points_ins_ids")
        dev, n = pts.device, pts.shape[0]
        n_slots = max(self.objects) + 1
        sums = torch.empty((n_slots, 3), dtype=torch.float64, device=dev)
        cnt = torch.empty(n_slots, dtype=torch.int32, device=dev)
        L.check(lib.ovo_instance_moments(L.ptr(pts), L.ptr(ins), n, n_slots, L.ptr(sums), L.ptr(cnt), L.stream()))
        cnt_h, sums_h = cnt.cpu().numpy(), sums.cpu().numpy()
        # 1. instances that lost all their points
        objects_list = [o for i, o in self.objects.items() if cnt_h[i] > 0]
        n_removed = len(self.objects) - len(objects_list)
        ids = [o.id for o in objects_list]
        N = len(ids)
        # 2. pair predicate for all i < j (static during the merge loop)
        same = np.zeros((N, N), bool)
        if N > 1 and same_instance is not None:
            for i in range(N):
                for j in range(i + 1, N):
                    same[i, j] = bool(same_instance(ids[i], ids[j]))
        elif N > 1:
            self._adopt_loose_features()                               # checkpoint-restored descriptors move into the table first
            has = np.asarray([self.bank.has_feature(i) for i in ids])  # the reference reads clip_feature only for pairs that pass the
            cen = (sums_h[ids] / cnt_h[ids, None]).astype(np.float32)  # centroid test; an instance without one can never merge here
            dist = np.sqrt(((cen[:, None, :] - cen[None, :, :]) ** 2).sum(-1, dtype=np.float32))
            with_f = [i for i, h in zip(ids, has) if h]
            cos = np.zeros((N, N), np.float32)
            if len(with_f) > 1:
                feats = self.bank.gather(with_f)                       # rows = clip_feature[0]
                unit = torch.empty_like(feats)
                L.check(lib.ovo_l2_normalize_rows(L.ptr(feats), len(with_f), feats.shape[1], L.ptr(unit), L.stream()))
                from ..utils import clip_utils
                sel = np.nonzero(has)[0]
                cos[np.ix_(sel, sel)] = clip_utils.similarity(unit, unit)[0].cpu().numpy()
            both = has[:, None] & has[None, :]
            iu, ju = np.nonzero(np.triu(np.ones((N, N), bool), 1) & both & ~(dist > np.float32(self.th_centroid)) & ~(cos < np.float32(self.th_cossim)))
            if len(iu):
                # group the map by instance: CSR over instance ids.  A stable sort puts the unassigned points (id -1) first -- their
                # number is the offset of instance 0 -- and ids beyond the table last, where no row of the CSR reaches them
                order = torch.argsort(ins, stable=True)
                grouped = pts.index_select(0, order).contiguous()
                off = np.zeros(n_slots + 1, np.int64)
                off[1:] = np.cumsum(cnt_h)
                off += int((ins < 0).sum().item())
                d_off = torch.from_numpy(off).to(dev)
                slots = np.asarray(ids, np.int32)
                pairs = torch.from_numpy(np.stack([slots[iu], slots[ju]], 1).astype(np.int32)).to(dev)
                near = torch.empty(len(iu), dtype=torch.int32, device=dev)
                for s in range(0, len(iu), 65535):                     # grid.y limit
                    e = min(s + 65535, len(iu))
                    L.check(lib.ovo_near_fraction(L.ptr(grouped), L.ptr(d_off), pairs[s:e].data_ptr(), e - s, int(cnt_h[slots[iu[s:e]]].max()),
                                                  float(self.th_points), near[s:e].data_ptr(), L.stream()))
                p_dist = near.cpu().numpy().astype(np.float64) / cnt_h[slots[iu]]
                ok = (p_dist > 0.5) | ((cos[iu, ju] > np.float32(0.9)) & (p_dist > 0.2))
                same[iu[ok], ju[ok]] = True
        # greedy merge in the reference's order
        objects: Dict[int, Instance3D] = {}
        fused: Dict[int, int] = {}
        for i, a in enumerate(objects_list):
            if a.id in fused:
                continue
            for j in range(i + 1, N):
                b = objects_list[j]
                if b.id in fused or not same[i, j]:
                    continue
                a.add_points_ids(b.points_ids)                         # instance_utils.fuse_instances
                for kf in b.kfs_ids:
                    a.add_keyframes(kf)
                for area, kf_id in b.top_kf:
                    a.add_top_kf(kf_id, area)
                fused[b.id] = a.id
            objects[a.id] = a
        print(f"Semantic Map update: removed {n_removed}, fused {len(fused)} instances")
        if fused or n_removed:
            removed = [i for i in self.objects if cnt_h[i] <= 0]
            self.last_instance_table = torch.from_numpy(self.instance_table(n_slots, fused, removed)).to(dev)
        if fused:
            table = np.arange(n_slots, dtype=np.int32)
            for b_id, a_id in fused.items():
                table[b_id] = a_id
            d_table = torch.from_numpy(table).to(dev)
            L.check(lib.ovo_remap_instances(L.ptr(ins), n, L.ptr(d_table), n_slots, L.stream()))      # `ins` views the caller's tensor: in place
        # 3. descriptors of merged instances move to the surviving id
        for id2, id1 in fused.items():
            for kf in self.objects[id2].kfs_ids:
                view = self.keyframes["ins_descriptors"].get(kf)
                if view is None or id2 not in view:
                    continue
                view[id1] = view.pop(id2)
        self.objects = objects
        self.update_objects_clip()                                     # 4.
        return points_ins_ids

    # ------------------------------------------------------------------ query (ovo.py:473-527)
    @torch.no_grad()
    def get_objs_clips(self) -> torch.Tensor:
        """f32[N_instances, D] on the GPU, rows in `self.objects` order."""
        self._adopt_loose_features()
        return self.bank.gather(self.objects.keys())

    def _adopt_loose_features(self) -> None:
        """Descriptors that live outside the resident table (restored from a checkpoint, or never fused) move into it."""
        loose = [o for o in self.objects.values() if o._own_feature is not None or not self.bank.has_feature(o.id)]
        for obj in loose:
            if obj._own_feature is not None:                   # restored from a checkpoint: adopt into the table
                feat, kf = obj._own_feature, obj._own_feature_kf
                self.bank.set_feature(obj.id, feat)
                obj._bank, obj._own_feature = self.bank, None
                self.bank.medoid_of[self.bank.slot_of[obj.id]] = kf
            else:                                              # "this should never happen" (ovo.py:523)
                obj._bank, obj.to_update = self.bank, True
                obj.update_clip(self.keyframes["ins_descriptors"])

    @torch.no_grad()
    def query(self, queries: List[str], templates=['{}'], ensemble: bool = False) -> torch.Tensor:
        assert len(self.objects) > 0, "No 3D instances to query!"
        return self.clip_generator.get_embed_txt_similarity(self.get_objs_clips(), queries, templates=templates)

    @torch.no_grad()
    def classify_instances(self, classes: List[str], template="This is a photo of a {}", th: float = 0):
        """Reference: ovo.py:473-492; argmax / threshold fused into the similarity kernel's epilogue."""
        assert len(self.objects) > 0, "No 3D instances to query!"
        cls, conf = self.clip_generator.classify(self.get_objs_clips(), classes, templates=template, th=th)
        return {"classes": cls.cpu().numpy(), "conf": conf.cpu().numpy()}

    # ------------------------------------------------------------------ view rendering (no reference counterpart but its GUI: visualizer.py:165-181)
    def _instance_tables(self, device, *columns):
        """Per-instance values (rows in `self.objects` order, as `get_objs_clips` returns them) as tables on `device` indexed by instance id;
        ids without an entry hold -1 (integer columns) / 0 (float columns)."""
        ids = torch.tensor(list(self.objects), dtype=torch.int64, device=device)
        n_slots = max(self.objects) + 1 if self.objects else 0
        tables = []
        for col in columns:
            col = torch.as_tensor(col).to(device)
            t = torch.zeros(n_slots, dtype=torch.float32, device=device) if col.is_floating_point() \
                else torch.full((n_slots,), -1, dtype=torch.int64, device=device)
            t[ids] = col.to(t.dtype)
            tables.append(t)
        return tables

    @torch.no_grad()
    def render_view(self, map_data, c2w, hw, K=None, radius: int = 1, near: float = 0.05, far: float = float("inf"), colors=None,
                    classes: Optional[List[str]] = None, template="This is a photo of a {}", th: float = 0.0,
                    query: Optional[str] = None, context=(), query_th: float = 0.0, boxes=None, box_width: float = 1.0, oriented: bool = False,
                    depth_slack: float = 0.02) -> Dict[str, torch.Tensor]:
        """The map seen from the pose `c2w` as images of `hw` = (h, w) pixels (utils/render_utils.py: a z-buffered splat of the points, a point
        covering (2 radius + 1)^2 pixels, depths in [near, far]).  `map_data`: what `slam.get_map()` returns; `K`: the view's intrinsics (default:
        the ones this OVO was built with).  Always returns
          "row"   i32[h,w]  the visible map row per pixel, -1 where no point lands        "depth"  f32[h,w]  its camera-frame depth, 0 there
          "ins"   i32[h,w]  its instance id, -1 where there is no point or it is unassigned
        and, when asked for,
          "rgb"   u8[h,w,3]            `colors` given: the mapper's `pcd_colors`, black where no point lands
          "cls" i64 / "conf" f32       `classes` given: `classify_instances(classes, template, th)` of the pixel's instance (-1 / 0 without one)
          "heat"  f32[h,w]             `query` given: column 0 of `self.query([query] + list(context))` of the pixel's instance, instances with
                                       heat <= query_th written as 0 -- the `heat > th` picture of the reference's `_update_query_vis`.
          "box" i32[h,w] / "box_depth" f32[h,w]   `boxes` given: the 12 edges of the instances' boxes (`instance_boxes`; `oriented`: the PCA-aligned
                                       ones), `2 box_width` pixels wide -- the instance id of the nearest visible edge (-1: none) and its depth (0).
                                       `boxes`: "all", "query" (the instances whose heat is > query_th; needs `query=`) or a list of instance ids;
                                       instances without points have no box.  An edge is hidden where it lies more than `depth_slack` behind
                                       the view's own "depth", so a box hugging its object's surface shows through the splat."""
        from ..utils import render_utils as R
        K = self._K_host if K is None else K
        if K is None:
            raise ValueError("render_view: no intrinsics (pass K=, or build OVO with cam_intrinsics)")
        view = R.make_view(c2w, K, int(hw[0]), int(hw[1]), radius=radius, near=near, far=far)
        pcd, point_ins = map_data[0], map_data[2].reshape(-1)
        row, depth = R.render_rows(pcd, view)
        out = {"row": row, "depth": depth}
        ins_cls = ins_conf = None
        if classes is not None:
            info = self.classify_instances(classes, template=template, th=th)
            ins_cls, ins_conf = self._instance_tables(row.device, info["classes"].astype(np.int64), info["conf"].astype(np.float32))
        res = R.resolve(row, point_ins=point_ins, point_rgb=colors, ins_cls=ins_cls, ins_val=ins_conf, fill_cls=-1, fill_val=0.0)
        out["ins"] = res["ins"]
        if colors is not None:
            out["rgb"] = res["rgb"]
        if classes is not None:
            out["cls"], out["conf"] = res["ins_cls"], res["val"]
        if boxes is not None and isinstance(boxes, str) and boxes not in ("all", "query"):
            raise ValueError(f"render_view: boxes={boxes!r} (\"all\", \"query\" or a list of instance ids)")
        if isinstance(boxes, str) and boxes == "query" and query is None:
            raise ValueError("render_view: boxes=\"query\" needs query=")
        sim = None
        if query is not None:
            sim = self.query([query] + list(context))[:, 0].float()
            heat = torch.where(sim > query_th, sim, torch.zeros_like(sim))           # (NaN -- an instance without a descriptor -- is not > th)
            table, = self._instance_tables(row.device, heat)
            out["heat"] = R.resolve(row, point_ins=point_ins, ins_val=table, fill_val=0.0)["val"]
        if boxes is not None:
            from ..utils import instance_geometry as IG
            geo = self.instance_boxes(map_data, oriented=oriented)
            ids = geo["ids"]
            if isinstance(boxes, str):
                want = torch.ones_like(ids, dtype=torch.bool) if boxes == "all" else (sim > query_th).to(ids.device)
            else:
                want = torch.isin(ids, torch.as_tensor(list(boxes), dtype=torch.int64, device=ids.device))
            keep = want & (geo["count"] > 0)
            corners = IG.box_corners(geo["min"][keep], geo["max"][keep], geo["R"][keep] if oriented else None)
            out["box"], out["box_depth"] = R.render_boxes(corners, ids[keep].to(torch.int32), view, half_width=box_width, scene_depth=depth,
                                                          depth_slack=depth_slack)
        return out

    # ------------------------------------------------------------------ a labelled surface (no reference counterpart: it shows its result in a window)
    @torch.no_grad()
    def semantic_mesh(self, map_data, vertices: torch.Tensor, faces: torch.Tensor, transform=None, classes: Optional[List[str]] = None,
                      template="This is a photo of a {}", th: float = 0.0, max_dist: Optional[float] = None, rgb=None, normals=None,
                      instance=None) -> Dict[str, Any]:
        """The map's labels on a mesh (e.g. `IcpTracker.extract_mesh()`), ready for `mesh_utils.write_ply(path, **out)`:
          "vertices" f32[V,3]  `vertices` moved by the 4 x 4 `transform` (mesh frame -> map frame, e.g. the tracker's world_ref), in f32
          "faces"    i32[T,3]  as given
          "instance" i32[V]    the most frequent instance id among the vertex's 5 nearest ASSIGNED map points (`mesh_utils.label_mesh`), -1 where
                               the nearest of them is farther than `max_dist`, or when the map has fewer than 5 assigned points; or `instance`
                               when given (the volume's own labels, `extract_mesh(labels=True)`: an i32 tensor [V], else ValueError), as it is
          "cls"      i32[V]    `classes` given: `classify_instances(classes, template, th)` of that instance, -1 without one; else None
          "rgb"      u8[V,3]   `rgb` when given (the scene's appearance, e.g. `extract_mesh(colors=True)`: u8[V,3], one row a vertex, else
                               ValueError); otherwise `mesh_utils.label_colors` of the class when `classes` is given, else of the instance
          "normals"  f32[V,3]  only when `normals` is given (e.g. `extract_mesh(normals=True)`: an f32 tensor [V,3], else ValueError): its rows rotated
                               by transform[:3, :3] in f32.  The transform is assumed rigid, so they are not normalised again."""
        from ..utils import mesh_utils as M
        pcd, point_ins = map_data[0], map_data[2].reshape(-1)
        v = vertices.to(torch.float32)
        if rgb is not None and not (isinstance(rgb, torch.Tensor) and rgb.dtype == torch.uint8 and tuple(rgb.shape) == (v.shape[0], 3)):
            got = f"{rgb.dtype} {tuple(rgb.shape)}" if isinstance(rgb, torch.Tensor) else type(rgb).__name__
            raise ValueError(f"OVO.semantic_mesh: rgb must be a u8 tensor [{v.shape[0]}, 3], one row a vertex (got {got})")
        if normals is not None and not (isinstance(normals, torch.Tensor) and normals.dtype == torch.float32 and tuple(normals.shape) == (v.shape[0], 3)):
            got = f"{normals.dtype} {tuple(normals.shape)}" if isinstance(normals, torch.Tensor) else type(normals).__name__
            raise ValueError(f"OVO.semantic_mesh: normals must be an f32 tensor [{v.shape[0]}, 3], one row a vertex (got {got})")
        if instance is not None and not (isinstance(instance, torch.Tensor) and instance.dtype == torch.int32 and tuple(instance.shape) == (v.shape[0],)):
            got = f"{instance.dtype} {tuple(instance.shape)}" if isinstance(instance, torch.Tensor) else type(instance).__name__
            raise ValueError(f"OVO.semantic_mesh: instance must be an i32 tensor [{v.shape[0]}], one id a vertex (got {got})")
        if transform is not None:
            m = torch.as_tensor(np.asarray(transform.detach().cpu() if isinstance(transform, torch.Tensor) else transform, dtype=np.float32)).to(v.device)
            v = v @ m[:3, :3].t() + m[:3, 3]
            if normals is not None:
                normals = (normals @ m[:3, :3].t()).contiguous()
        v = v.contiguous()
        assigned = point_ins >= 0
        if instance is not None:
            pass                                               # the volume's labels: nothing is transferred from the point map
        elif int(assigned.sum()) >= 5:
            instance = M.label_mesh(v, pcd[assigned].contiguous(), point_ins[assigned], max_dist=max_dist)
        else:
            instance = torch.full((v.shape[0],), -1, dtype=torch.int32, device=v.device)
        cls = None
        if classes is not None:
            info = self.classify_instances(classes, template=template, th=th)
            table, = self._instance_tables(v.device, info["classes"].astype(np.int64))
            table = torch.cat([table, table.new_full((1,), -1)])      # the last row answers for "no instance" and for ids the table does not reach
            known = (instance >= 0) & (instance < table.numel() - 1)
            cls = table[torch.where(known, instance.long(), torch.full_like(instance, table.numel() - 1).long())].to(torch.int32)
        if rgb is None:
            rgb = torch.from_numpy(M.label_colors(instance if cls is None else cls)).to(v.device)
        out = {"vertices": v, "faces": faces, "instance": instance, "cls": cls, "rgb": rgb}
        if normals is not None:
            out["normals"] = normals
        return out

    # ------------------------------------------------------------------ where the instances are (the viewer's boxes: vis_utils.py:72-87)
    @torch.no_grad()
    def instance_boxes(self, map_data, oriented: bool = False) -> Dict[str, torch.Tensor]:
        """The box of every instance, rows in `self.objects` order (the row order of `get_objs_clips`), on the map's device: "ids" i64[N], "count"
        i32[N] map points of the instance, "center" f32[N,3] (the middle of the box), "min" / "max" f32[N,3] and, with `oriented`, "R" f32[N,3,3] --
        rows the PCA axes of the instance's points (`instance_geometry.pca_axes`); "min" / "max" are then extents along them and "center" is back
        in the world -- and "extent" f32[N,3] = max - min.  An instance without points has count 0 and NaN boxes.  One pass over the map
        (`ovo_instance_geometry`), two when oriented."""
        from ..utils import instance_geometry as IG
        pcd, point_ins = map_data[0], map_data[2].reshape(-1)
        dev = pcd.device
        ids = torch.tensor(list(self.objects), dtype=torch.int64, device=dev)
        if not self.objects:
            empty = torch.zeros((0, 3), dtype=torch.float32, device=dev)
            out = {"ids": ids, "count": torch.zeros(0, dtype=torch.int32, device=dev), "center": empty, "min": empty.clone(), "max": empty.clone()}
            if oriented:
                out.update(R=torch.zeros((0, 3, 3), dtype=torch.float32, device=dev), extent=empty.clone())
            return out
        n_slots = max(self.objects) + 1
        if oriented:
            g = IG.instance_geometry(pcd, point_ins, n_slots, oriented=True)
            lo, hi, R = g["min_o"][ids], g["max_o"][ids], g["R"][ids]
        else:
            g = IG.geometry_pass(pcd, point_ins, n_slots, moments=False)
            lo, hi, R = g["min"][ids], g["max"][ids], None
        count = g["count"][ids]
        nan = torch.full_like(lo, float("nan"))
        has = (count > 0)[:, None]
        lo, hi = torch.where(has, lo, nan), torch.where(has, hi, nan)
        mid = (lo + hi) * 0.5
        out = {"ids": ids, "count": count, "center": mid if R is None else (mid[:, :, None] * R).sum(1), "min": lo, "max": hi}
        if oriented:
            out.update(R=R, extent=hi - lo)
        return out

    @torch.no_grad()
    def locate(self, map_data, queries: List[str], templates=['{}'], top_k: int = 5, th: float = 0.0, oriented: bool = False):
        """"Where is the X?": per query a list of at most `top_k` dicts {"ins_id", "score", "center", "min", "max", "n_points"} (+ "R", "extent" with
        `oriented`; boxes as `instance_boxes` returns them, as numpy) of the instances whose `self.query(queries, templates)` score is > th, by
        descending score, ties to the smaller id.  An instance without a descriptor (NaN score) or without map points is never listed."""
        sim = self.query(list(queries), templates=templates).float().cpu().numpy()
        geo = {k: v.cpu().numpy() for k, v in self.instance_boxes(map_data, oriented=oriented).items()}
        ids, found = geo["ids"], []
        for q in range(len(queries)):
            score = sim[:, q]
            with np.errstate(invalid="ignore"):
                ok = np.nonzero((score > th) & (geo["count"] > 0))[0]               # (NaN is not > th)
            ok = ok[np.lexsort((ids[ok], -score[ok]))][:max(int(top_k), 0)]
            hits = []
            for r in ok:
                hit = {"ins_id": int(ids[r]), "score": float(score[r]), "center": geo["center"][r], "min": geo["min"][r], "max": geo["max"][r],
                       "n_points": int(geo["count"][r])}
                if oriented:
                    hit.update(R=geo["R"][r], extent=geo["extent"][r])
                hits.append(hit)
            found.append(hits)
        return found

    # ------------------------------------------------------------------ checkpoint (ovo.py:529-575)
    def capture_dict(self, debug_info: bool) -> Dict[str, Any]:
        scene = {"ins_3d_ids": np.asarray(list(self.objects.keys()))}
        for obj in self.objects.values():
            scene.update(obj.export(debug_info))
        if debug_info:
            scene["frame_id"] = np.array(self.keyframes["frame_id"])
            scene["ins_map"] = np.array(self.keyframes["ins_maps"])
            for kf_id, view in self.keyframes["ins_descriptors"].items():
                for ins_id, desc in view.items():
                    scene[f"kf_{kf_id}_ins3d_{ins_id}_clips"] = desc.cpu().numpy()
        return scene

    def restore_dict(self, scene_dict: Dict[str, Any], debug_info: bool = False) -> None:
        for i in scene_dict["ins_3d_ids"]:
            obj = Instance3D(int(i), bank=None)
            obj.restore(scene_dict, debug_info)
            self.objects[obj.id] = obj
        if debug_info:
            self.keyframes["frame_id"] = list(scene_dict["frame_id"])
            n_kf = len(self.keyframes["frame_id"])
            self.keyframes["ins_maps"] = [x.squeeze() for x in np.split(scene_dict["ins_map"], n_kf)] if n_kf else []
            for k in range(n_kf):
                rows = {}
                for ins_id in self.objects:
                    desc = scene_dict.get(f"kf_{k}_ins3d_{ins_id}_clips")
                    if desc is not None:
                        rows[ins_id] = self.bank.append(torch.as_tensor(desc).reshape(1, -1))[0]
                self.keyframes["ins_descriptors"][k] = KeyframeView(self.bank, rows)
            self.kf_id = n_kf
