"""What colour in the TSDF volume costs: every colour entry point against its colourless counterpart in ONE job, on section 17's
workload -- `synthetic.render_depth` / `render_rgb` frames at 456 x 616 (scale 1.0) into a dim^3 volume of 2 cm voxels, the frustum box for far = 5 m.

    python tools/tsdf_color_bench.py [--runs 9] [--scale 1.0] [--dim 512] [--out profiles/tsdf_color_bench.txt]

  integrate       `ovo_tsdf_integrate_color` against `ovo_tsdf_integrate`, one frame into its frustum box: device-event time of REP calls / REP
  raycast         `ovo_tsdf_raycast_color` against `ovo_tsdf_raycast`, one image
  extract_mesh    `TsdfVolume.extract_mesh(colors=True)` against `extract_mesh()` over the whole volume: device-event time around the call, its one host
                  wait for (V, T) and its allocations included
  tracker         wall-clock milliseconds per frame of `IcpTracker(model="tsdf")` over a short sequence with `tsdf_color` on and off (each frame ends
                  with the tracker's one host wait; the colour image is on the device already)
Each pair alternates for RUNS rounds after a warm-up; medians, with the smallest and largest.  Before anything is timed the two forms are compared:
(F, W), the ray-cast depth and the mesh must be bit-equal with colour on and off.  None of the figures is a pass mark.  Writes one JSON line to --out
and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ovo_amd import synthetic as syn
from ovo_amd.slam.icp_tracker import IcpTracker
from ovo_amd.utils import icp_utils as U
from ovo_amd.utils import tsdf_utils as TU
from tsdf_bench import BASE, FAR, NEAR, REP, TRUNC, VOXEL, XI, copy_gbs, timed


def track(color, K, depths, rgbs, dim, dev):
    """A fresh tracker over the frames (device tensors): (rows, states, wall-clock ms per frame behind the first)."""
    tracker = IcpTracker(K, device=dev, model="tsdf", tsdf_dims=(dim, dim, dim), tsdf_voxel=VOXEL, tsdf_far=FAR, kf_min_overlap=0.1, tsdf_color=color)
    rows, states, ms = [], [], []
    for k, (d, c) in enumerate(zip(depths, rgbs)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tracker.process_image_rgbd(c, d, k)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        rows.append(tracker.get_last_trajectory_point().copy())
        states.append(tracker.get_tracking_state())
    tracker.shutdown()
    return rows, states, ms[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tsdf_color_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tsdf_color_bench needs a GPU"
    assert args.runs >= 7, "the median of at least 7 runs"
    dev = torch.device("cuda", 0)
    med = statistics.median
    stream_gbs = copy_gbs(dev)
    K, (h, w) = syn.scannet_intrinsics(args.scale), syn.scannet_depth_hw(args.scale)
    dim = args.dim
    origin = [0.2 - 0.5 * VOXEL * (dim - 1), -0.5 * VOXEL * (dim - 1), 0.2 - 0.5 * VOXEL * (dim - 1)]      # around the room's centre, world frame
    poses = [(BASE @ U.se3_exp(tuple(k * x for x in XI))).astype(np.float32) for k in range(3)]
    depths = [torch.from_numpy(syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.0)).to(dev) for i, p in enumerate(poses)]
    rgbs = [torch.from_numpy(syn.render_rgb(h, w, i)).to(dev) for i in range(len(poses))]
    plain = TU.TsdfVolume((dim, dim, dim), VOXEL, origin, TRUNC, 64, device=dev)
    color = TU.TsdfVolume((dim, dim, dim), VOXEL, origin, TRUNC, 64, device=dev, color=True)
    boxes = [plain.frustum_box(K, h, w, p, NEAR, FAR) for p in poses]
    dz = TRUNC / 2

    # ---- colour changes nothing it shares with the colourless form: compared before anything is timed
    for d, c, p, b in zip(depths, rgbs, poses, boxes):
        plain.integrate(d, K, p, NEAR, FAR, box=b)
        color.integrate(d, K, p, NEAR, FAR, box=b, rgb=c)
    depth_p = plain.raycast(K, h, w, poses[1], NEAR, FAR, dz)
    depth_c, image = color.raycast(K, h, w, poses[1], NEAR, FAR, dz, color=True)
    vp, fp = plain.extract_mesh()
    vc, fc, cc = color.extract_mesh(colors=True)
    torch.cuda.synchronize()
    assert torch.equal(plain.vol.view(torch.int32), color.vol.view(torch.int32)) and torch.equal(depth_p.view(torch.int32), depth_c.view(torch.int32))
    assert torch.equal(vp.view(torch.int32), vc.view(torch.int32)) and torch.equal(fp, fc) and tuple(cc.shape) == (vp.shape[0], 3)
    hits, updated = int((depth_c > 0).sum()), int((color.vol[..., 1] > 0).sum())
    assert bool(image[depth_c > 0].any()) and not bool(image[depth_c == 0].any()) and bool(((color.vol[..., 1] > 0) == color.col[..., :3].any(-1)).all())

    box = boxes[1]
    box_voxels = int(np.prod([hi - lo for lo, hi in zip(*box)]))
    out_d, out_c = torch.empty((h, w), dtype=torch.float32, device=dev), torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    pairs = {"integrate": (lambda: plain.integrate(depths[1], K, poses[1], NEAR, FAR, box=box),
                           lambda: color.integrate(depths[1], K, poses[1], NEAR, FAR, box=box, rgb=rgbs[1]), REP),
             "raycast": (lambda: plain.raycast(K, h, w, poses[1], NEAR, FAR, dz, out=out_d),
                         lambda: color.raycast(K, h, w, poses[1], NEAR, FAR, dz, out=out_d, color=True, out_rgb=out_c), REP),
             "extract_mesh": (lambda: plain.extract_mesh(), lambda: color.extract_mesh(colors=True), 1)}
    ms = {}
    for name, (off, on, rep) in pairs.items():
        for _ in range(2):                                          # warm-up of every shape the timed window uses
            off(), on()
        ms[name], ms[name + "_color"] = [], []
        for _ in range(args.runs):                                  # alternating
            ms[name].append(timed(off, rep))
            ms[name + "_color"].append(timed(on, rep))

    # ---- a tracker frame, colour off and on alternating
    n_seq = 6
    seq_poses = [(BASE @ U.se3_exp(tuple(k * x for x in XI))).astype(np.float32) for k in range(n_seq)]
    seq = [torch.from_numpy(syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.0)).to(dev) for i, p in enumerate(seq_poses)]
    seq_rgb = [torch.from_numpy(syn.render_rgb(h, w, i)).to(dev) for i in range(n_seq)]
    del plain, color
    torch.cuda.empty_cache()
    frame_ms, rows = {False: [], True: []}, {}
    for c in (False, True):
        track(c, K, seq, seq_rgb, dim, dev)                         # warm-up
    for _ in range(args.runs):
        for c in (False, True):
            rows[c], states, per = track(c, K, seq, seq_rgb, dim, dev)
            assert all(s == U.OK for s in states), (c, states)
            frame_ms[c].append(med(per))
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(rows[False], rows[True]))      # poses: the same bits

    figures = lambda v: {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out = {"tool": "tsdf_color_bench", "runs": args.runs, "rep": REP, "image": [h, w], "volume": [dim] * 3, "voxel": VOXEL, "trunc": TRUNC, "far": FAR, "dz": dz,
           "stream_copy_gbs": round(stream_gbs, 1), "box": [list(box[0]), list(box[1])], "box_voxels": box_voxels, "updated_voxels_3_frames": updated,
           "hits": hits, "mesh": {"vertices": int(vp.shape[0]), "triangles": int(fp.shape[0])},
           "ms": {k: figures(v) for k, v in ms.items()},
           "color_over_plain": {k: round(med(ms[k + "_color"]) / med(ms[k]), 3) for k in pairs},
           "tracker_frame_ms": {"plain": figures(frame_ms[False]), "color": figures(frame_ms[True])},
           "tracker_color_over_plain": round(med(frame_ms[True]) / med(frame_ms[False]), 3)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
