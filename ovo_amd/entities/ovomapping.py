"""The per-sequence driver around the hot path (reference: ovo/entities/ovomapping.py:29-243) -- the caller that feeds
`VanillaMapper` and `OVO` one frame at a time, writes the logger files and the `ovo_map.ckpt` checkpoint, and can resume from
one.  Same class name, constructor, methods, cadence rules (`track_every` / `map_every` / `segment_every`), skip rules (no
pose, no valid depth) and files on disk.

What is different, on purpose:
  * the dataset is injected (`dataset=`): the loaders of ovo/entities/datasets.py parse third-party sequence formats through
    imageio / OpenCV and are out of scope; anything indexable that returns the reference's frame tuple
    `(frame_id, image HxWx3 u8, depth HxW f32, c2w 4x4[, full-resolution image])` and carries `intrinsics`, `height`, `width`
    (+ `dataset_config`, `crop_edge` when colour and depth resolutions differ) works;
  * the `vanilla` back end, and the `orbslam*` wrapper around an INJECTED tracker (`tracker=`, `ok_state=`: slam/orbslam.py; the ORB-SLAM
    binding itself and Gaussian-SLAM are out of scope), and `rgbd_icp`: the same wrapper around the package's own depth tracker
    (slam/icp_tracker.py); there is no Open3D visualiser process (`vis.stream` must be false);
  * no autocast context: the kernels choose their own arithmetic (bf16 MFMA operands, fp32 accumulation);
  * when a frame is segmented, the mask-independent half of the next segmented frame's feature extraction is not started
    early here (a dataset may be a live camera); `ovo_amd.pipeline.FramePipeline` is the throughput-oriented driver that does;
  * opt-in: with config["semantic"]["volume_labels"] and a back end whose tracker was built with tsdf_labels
    (`rgbd_icp`: config["slam"]["icp"]), every segmented keyframe's instance image is voted into the tracker's TSDF volume, the volume follows
    the merges of `OVO.update_map`, and config["slam"]["save_mesh"] writes `semantic_mesh.ply`.  Without both, `run` makes the calls it made before.
"""
from __future__ import annotations

import gc
import os
import time
from pathlib import Path
from typing import Any, Dict, Optional

import numpy as np
import torch

from ..slam.vanilla_mapper import VanillaMapper
from ..utils import io_utils
from .logger import Logger
from .ovo import OVO


def get_slam_backbone(config: Dict[str, Any], dataset, cam_intrinsics: torch.Tensor, tracker=None, ok_state=None) -> VanillaMapper:
    """Reference: ovomapping.py:18-27.  `tracker` / `ok_state`: the injected tracker of the "orbslam*" back ends (slam/orbslam.py)."""
    backbone = config["slam"].get("slam_module", "vanilla")
    if backbone.startswith("orbslam") and tracker is not None:
        from ..slam.orbslam import WrapperORBSLAM
        return WrapperORBSLAM(config, cam_intrinsics, world_ref=torch.from_numpy(dataset[0][3]), tracker=tracker, ok_state=ok_state)      # :23-25
    if backbone == "rgbd_icp":                             # the package's own tracker behind the same seam (slam/icp_tracker.py)
        from ..slam.icp_tracker import IcpTracker
        from ..slam.orbslam import WrapperORBSLAM
        if tracker is None:
            tracker = IcpTracker(cam_intrinsics, device=config.get("device", "cuda"), **config["slam"].get("icp", {}))
        first = np.asarray(dataset[0][3], dtype=np.float32) if len(dataset[0]) > 3 and dataset[0][3] is not None else None
        world_ref = torch.from_numpy(first.copy()) if first is not None and first.shape == (4, 4) and np.isfinite(first).all() else torch.eye(4)
        return WrapperORBSLAM(config, cam_intrinsics, world_ref=world_ref, tracker=tracker, ok_state=ok_state)
    if backbone != "vanilla":
        raise NotImplementedError(f"slam_module {backbone!r}: only the ground-truth-pose 'vanilla' mapper is built here, the 'orbslam*' wrapper "
                                  "around an injected tracker= and 'rgbd_icp' (Gaussian-SLAM and the ORB-SLAM binding itself are out of scope, SURVEY.md §2)")
    return VanillaMapper(config, cam_intrinsics)


def _sync() -> None:
    if torch.cuda.is_available():
        torch.cuda.synchronize()


class OVOSemMap:
    def __init__(self, config: Dict[str, Any], output_path: str, dataset=None, ovo: Optional[OVO] = None, tracker=None, ok_state=None) -> None:
        self._setup_output_path(output_path)
        io_utils.save_dict_to_yaml(config, "config.yaml", directory=self.output_path)
        config["output_path"] = str(self.output_path)
        self.config = config
        self.device = config.get("device", "cuda")
        self.dataset_name = config.get("dataset_name")
        vis = config.get("vis", {})
        if vis.get("stream", False):
            raise NotImplementedError("vis.stream: the Open3D visualiser process is out of scope (SURVEY.md §2)")
        self.stream = self.show_stream = False
        self.map_every = config.get("mapping", {}).get("map_every", 10)
        self.segment_every = config["semantic"].get("segment_every", 10)
        tracking = config.get("tracking")
        self.track_every = 1 if tracking is None else tracking.get("track_every", 1)

        self.logger = Logger(self.output_path, os.getpid(), config.get("use_wandb", False))
        if dataset is None:
            raise NotImplementedError("pass dataset=: the reference's dataset loaders (ovo/entities/datasets.py) are out of scope")
        self.dataset = dataset
        cam_intrinsics = torch.tensor(np.asarray(dataset.intrinsics, dtype=np.float32), device=self.device)
        config["semantic"]["debug_info"] = config.get("debug_info", False)
        scene = config.get("data", {}).get("scene_name")
        self.ovo = ovo if ovo is not None else OVO(config["semantic"], self.logger, scene, cam_intrinsics, device=self.device)
        if self.ovo.logger is None:
            self.ovo.logger = self.logger
        sam = config["semantic"].get("sam", {})
        if (sam.get("precomputed", False) or sam.get("precompute", False)) and self.ovo.mask_generator is not None:
            self.ovo.mask_generator.precompute(self.dataset, self.segment_every)
        self.slam_backbone = get_slam_backbone(config, self.dataset, cam_intrinsics, tracker=tracker, ok_state=ok_state)

        self.first_frame = 0
        if config.get("restore_map", False):
            self.restore_representation()
            self.first_frame = list(self.slam_backbone.estimated_c2ws.keys())[-1] + 1

    def _setup_output_path(self, output_path: str) -> None:
        self.output_path = Path(output_path)
        self.output_path.mkdir(exist_ok=True, parents=True)

    # ------------------------------------------------------------------ checkpoint (ovomapping.py:81-116)
    def save_representation(self) -> None:
        ckpt = {"map_params": self.slam_backbone.get_map_dict(),
                "ovo_map_params": self.ovo.capture_dict(debug_info=self.config.get("debug", False))}
        io_utils.save_dict_to_ckpt(ckpt, "ovo_map.ckpt", directory=self.output_path)
        if self.config["slam"].get("save_estimated_cam", False):
            with open(self.output_path / "estimated_c2w.npy", "wb") as f:
                torch.save(self.slam_backbone.get_cam_dict(), f)
        tracker = self._label_tracker()
        if self.config["slam"].get("save_mesh", False) and tracker is not None and tracker.volume is not None:
            self._save_semantic_mesh(tracker)

    # ------------------------------------------------------------------ the labelled volume beside the map (no reference counterpart)
    def _label_tracker(self):
        """The back end's tracker when its fused model takes the map's instance labels -- config["semantic"]["volume_labels"] and a tracker built with
        tsdf_labels (`config["slam"]["icp"]`), both -- else None, and `run` makes exactly the calls it makes without the key."""
        if not self.config["semantic"].get("volume_labels", False):
            return None
        tracker = getattr(self.slam_backbone, "tracker", None)
        return tracker if getattr(tracker, "tsdf_labels", False) else None

    def _fuse_labels(self, tracker, depth) -> None:
        """Votes the keyframe just queued into the tracker's label volume: its instance image at the depth's size.  A frame the tracker did not fuse
        (LOST, or none yet) is skipped: `fuse_labels` would vote with the depth and pose of an earlier frame."""
        ok = getattr(self.slam_backbone, "ok_state", getattr(tracker, "OK", None))
        if tracker.volume is None or tracker.get_tracking_state() != ok:
            return
        matched, binary_maps = self.ovo.keyframes_queue[-1][:2]
        if binary_maps is None:
            return
        tracker.fuse_labels(self.ovo.instance_image(matched, binary_maps, hw=tuple(int(x) for x in depth.shape)))

    def _save_semantic_mesh(self, tracker) -> None:
        """<output_path>/semantic_mesh.ply: the fused model's surface with the volume's own instance labels, its normals and (tsdf_color) its colour,
        moved into the map's frame by the back end's world_ref."""
        from ..utils import mesh_utils
        color = bool(getattr(tracker, "tsdf_color", False))
        out = list(tracker.extract_mesh(labels=True, normals=True, colors=color))
        vertices, faces = out[:2]
        rgb = out[2] if color else None
        normals, instance = out[-2], out[-1]
        mesh = self.ovo.semantic_mesh(self.slam_backbone.get_map(), vertices, faces, instance=instance, normals=normals, rgb=rgb,
                                      transform=self.slam_backbone.world_ref)
        mesh_utils.write_ply(self.output_path / "semantic_mesh.ply", **mesh)

    def restore_representation(self) -> None:
        ckpt_path = self.output_path / "ovo_map.ckpt"
        assert ckpt_path.exists(), f"Missing required checkpoint to restore: {ckpt_path}"
        ckpt = torch.load(ckpt_path, map_location=self.device, weights_only=False)
        self.ovo.restore_dict(ckpt["ovo_map_params"], debug_info=self.config.get("debug", False))
        self.slam_backbone.set_map_dict(ckpt["map_params"])
        c2w_path = self.output_path / "estimated_c2w.npy"
        if c2w_path.exists():
            self.slam_backbone.set_cam_dict(torch.load(c2w_path, weights_only=False))
        else:
            print(f"Missing cameras positions to restore: {c2w_path}\nRestoring without cameras positions!")

    # ------------------------------------------------------------------ main loop (ovomapping.py:120-243)
    def _due(self, frame_id: int) -> bool:
        return (self.track_every == 1 or frame_id % self.track_every == 0 or frame_id % self.map_every == 0
                or frame_id % self.segment_every == 0)

    def _segment(self, frame_id: int, frame_data, c2w) -> None:
        image = frame_data[-1] if len(frame_data) == 5 else frame_data[1]
        ds = self.dataset
        if ds.height != image.shape[0] or ds.width != image.shape[1]:      # colour at a higher resolution than depth
            ratio = (image.shape[0] / ds.dataset_config["H"], image.shape[1] / ds.dataset_config["W"], ds.crop_edge)
        else:
            ratio = ()
        scene_data = [frame_id, image, frame_data[2], ratio]
        tracker = self._label_tracker()
        queued = len(self.ovo.keyframes_queue) if tracker is not None else 0
        updated = self.ovo.detect_and_track_objects(scene_data, self.slam_backbone.get_map(), c2w)
        if updated is not None:
            self.slam_backbone.update_pcd_obj_ids(updated)
        if tracker is not None and len(self.ovo.keyframes_queue) > queued:      # before compute_semantic_info consumes the queue
            self._fuse_labels(tracker, frame_data[2])
        self.ovo.compute_semantic_info()
        self.logger.log_memory_usage(frame_id)

    def run(self) -> None:
        spf = []
        _sync()
        t_start = time.time()
        for frame_id in range(self.first_frame, len(self.dataset)):
            if not self._due(frame_id):
                continue
            frame_data = self.dataset[frame_id]
            self.slam_backbone.track_camera(frame_data)
            c2w = self.slam_backbone.get_c2w(frame_id)
            depth = frame_data[2]
            if c2w is None or not bool((depth > 0).any()):
                continue
            t_lc = 0.0
            if frame_id % self.map_every == 0:
                self.slam_backbone.map(frame_data, c2w)
                if getattr(self.slam_backbone, "map_updated", False):       # set by back ends with loop closure (orbslam.py:68-115)
                    _sync()
                    t0 = time.time()
                    updated = self.ovo.update_map(self.slam_backbone.get_map(), self.slam_backbone.get_kfs())
                    if updated is not None:
                        self.slam_backbone.update_pcd_obj_ids(updated)
                    tracker = self._label_tracker()
                    if tracker is not None and tracker.volume is not None and self.ovo.last_instance_table is not None:
                        tracker.volume.remap_labels(self.ovo.last_instance_table)      # the volume follows the merges and removals of the update
                    self.slam_backbone.map_updated = False
                    _sync()
                    t_lc = time.time() - t0
                    print(f"Sem LC update took {t_lc};")
            t_sem = 0.0
            if frame_id % self.segment_every == 0:
                t0 = time.time()
                with torch.no_grad():       # (upstream writes `inference_mode() and autocast(...)`, which enters only the autocast)
                    self._segment(frame_id, frame_data, c2w)
                t_sem = time.time() - t0
            if t_sem + t_lc > 0:
                spf.append(t_sem + t_lc)
            if frame_id % 50 == 0:
                gc.collect()
        self.ovo.complete_semantic_info()
        _sync()
        fps = len(self.dataset) / self.segment_every / max(time.time() - t_start, 1e-9)

        self.logger.log_fps(fps)
        self.logger.log_spf(spf)
        self.logger.log_max_memory_usage()
        self.logger.write_stats()
        self.logger.print_final_stats()
        self.save_representation()
        self.ovo.cpu()
