"""What aligning a frame to the TSDF volume itself costs and gives: `ovo_icp_align_volume` against `ovo_icp_align` on the same frame,
and a tracker frame with `tsdf_align="volume"` against `tsdf_align="raycast"` (the yardstick: `model="tsdf"` as it was) and `model="keyframe"`.

    python tools/sdf_align_bench.py [--runs 9] [--scale 1.0] [--dim 512] [--drift] [--basin] [--out profiles/sdf_align_bench.txt]

One job, a warm-up, RUNS alternating runs, medians and ranges, device events for the kernels.  456 x 616 frames of `synthetic.render_depth`, a dim^3 volume of
2 cm voxels, the settings of tools/tsdf_bench.py.
  iteration_ms   one Gauss-Newton step on level 0 (reduce pass + solve) of each form: the device-event time of an alignment of 40 steps minus that of one of 8,
                 over 32 -- init, publish, the host's wait and the launch of the first kernel cancel.  The solve is the same kernel in both, so the difference of the two is the
                 difference of the reduce passes.  Both start at the true pose and must end OK.
  gather bytes   what a pixel gathers besides its own 32 bytes: 32 (one reference pixel) against 64 (eight voxels as four 16-byte pairs)
  tracker        wall-clock milliseconds per frame of IcpTracker over a short sequence (each frame ends with the tracker's one host wait), the three modes
                 alternating, medians of RUNS
  --drift        tools/tsdf_bench.py's closed loop of 64 frames with noise 0.004 in all three modes: the final and the largest distance to the ground truth
  --basin        one frame aligned from start poses pushed off the truth along the camera's x axis and about its y axis: per mode the largest offset of the
                 list from which it, and every smaller one, still ends OK within 1 mm of the pose it reaches from the truth itself with the same iterations
None of these is a pass mark.  Writes one JSON line to --out and prints it."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tsdf_bench import BASE, FAR, NEAR, TRUNC, VOXEL, XI, loop_pose, pose_distance, rot, row_pose, timed

from ovo_amd import synthetic as syn
from ovo_amd.slam.icp_tracker import IcpTracker
from ovo_amd.utils import icp_utils as U
from ovo_amd.utils import tsdf_utils as TU

MODES = {"volume": dict(model="tsdf", tsdf_align="volume"), "raycast": dict(model="tsdf"), "keyframe": {}}
SETTINGS = (0.1, 30.0, 1, 1e-6)                                     # dist_th, normal_th_deg, min_pairs, min_pivot_ratio
OFFSETS_M = [0.01, 0.02, 0.03, 0.05, 0.075, 0.1, 0.15, 0.2, 0.3]
OFFSETS_DEG = [0.5, 1.0, 2.0, 3.0, 5.0, 7.5, 10.0, 15.0]


def track(mode, K, depths, dim, dev):
    """A fresh tracker over `depths` (device tensors): (rows, states, wall-clock ms per frame behind the first)."""
    kw = dict(MODES[mode], **(dict(tsdf_dims=(dim, dim, dim), tsdf_voxel=VOXEL, tsdf_far=FAR, kf_min_overlap=0.1) if mode != "keyframe" else {}))
    tracker = IcpTracker(K, device=dev, **kw)
    rows, states, ms = [], [], []
    for k, d in enumerate(depths):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tracker.process_image_rgbd(None, d, k)
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
    ap.add_argument("--drift", action="store_true")
    ap.add_argument("--basin", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sdf_align_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sdf_align_bench needs a GPU"
    assert args.runs >= 7, "the median of at least 7 runs"
    dev = torch.device("cuda", 0)
    med = statistics.median
    K, (h, w) = syn.scannet_intrinsics(args.scale), syn.scannet_depth_hw(args.scale)
    dim = args.dim
    origin = [0.2 - 0.5 * VOXEL * (dim - 1), -0.5 * VOXEL * (dim - 1), 0.2 - 0.5 * VOXEL * (dim - 1)]      # around the room's centre, world frame
    poses = [(BASE @ U.se3_exp(tuple(k * x for x in XI))).astype(np.float32) for k in range(3)]
    depths = [torch.from_numpy(syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.0)).to(dev) for i, p in enumerate(poses)]

    # ---- the model: two frames fused; the third is aligned to it -- to the volume, to its ray cast at the second pose, and to the second frame itself
    volume = TU.TsdfVolume((dim, dim, dim), VOXEL, origin, TRUNC, 64, device=dev)
    for d, p in zip(depths[:2], poses[:2]):
        volume.integrate(d, K, p, NEAR, FAR)
    prep = lambda d: U.prepare_frame(d, K, 3, 10.0, 0.1)
    cur, model, kf = prep(depths[2]), prep(volume.raycast(K, h, w, poses[1], NEAR, FAR)), prep(depths[1])
    rel = U.rigid_inverse(poses[1]) @ poses[2].astype(np.float64)      # reference camera <- current camera, the truth
    aligner = U.Aligner(dev)

    def run(mode, iters, offset=np.eye(4)):
        """One alignment from the truth times `offset` (in the current camera's frame): queued only; `aligner.wait(seq)` gives the result."""
        if mode == "volume":
            aligner.set_pose(poses[2].astype(np.float64) @ offset)
            return aligner.queue_volume(volume, cur, iters, *SETTINGS)
        aligner.set_pose(rel @ offset)
        return aligner.queue(model if mode == "raycast" else kf, cur, iters, *SETTINGS)

    step = {}
    for mode in ("volume", "raycast"):
        for iters in ((0, 0, 8), (0, 0, 40)):                       # warm-up, and both must stay OK to the end: a LOST alignment's later steps do nothing
            res = aligner.wait(run(mode, iters))
            assert res["state"] == U.OK and res["iterations"] == iters[2], (mode, res["state"], res["iterations"])
        step[mode] = {"pairs": res["pairs"], "ms": []}
    for _ in range(args.runs):                                      # alternating
        for mode in ("volume", "raycast"):
            short, long_ = (timed(lambda: aligner.wait(run(mode, its))) for its in ((0, 0, 8), (0, 0, 40)))
            step[mode]["ms"].append((long_ - short) / 32)
    out = {"tool": "sdf_align_bench", "runs": args.runs, "image": [h, w], "volume": [dim] * 3, "voxel": VOXEL, "trunc": TRUNC, "far": FAR,
           "iteration_ms": {m: round(med(s["ms"]), 5) for m, s in step.items()},
           "iteration_ms_min_max": {m: [round(min(s["ms"]), 5), round(max(s["ms"]), 5)] for m, s in step.items()},
           "reduce_difference_ms": round(med(step["volume"]["ms"]) - med(step["raycast"]["ms"]), 5),
           "pairs_level0": {m: s["pairs"] for m, s in step.items()}, "pixels": h * w, "gather_bytes_per_pixel": {"volume": 64, "raycast": 32}}

    if args.basin:
        basin = {}
        for mode in MODES:
            home = aligner.wait(run(mode, (10, 5, 4)))
            assert home["state"] == U.OK, mode
            reach = {}
            for name, offsets, make in (("translation_m", OFFSETS_M, lambda x: U.se3_exp((0, 0, 0, x, 0, 0))), ("rotation_deg", OFFSETS_DEG, lambda a: rot(1, math.radians(a)))):
                reach[name] = 0.0
                for x in offsets:
                    res = aligner.wait(run(mode, (10, 5, 4), make(x)))
                    if res["state"] != U.OK or pose_distance(res["T"], home["T"])[0] > 1e-3:
                        break
                    reach[name] = x
            basin[mode] = dict(reach, home_to_truth_mm=round(pose_distance(home["T"], poses[2] if mode == "volume" else rel)[0] * 1e3, 3), pairs=home["pairs"])
        out["basin"] = dict(basin, offsets_m=OFFSETS_M, offsets_deg=OFFSETS_DEG)

    # ---- a tracker frame, the three modes alternating
    del volume, cur, model, kf
    torch.cuda.empty_cache()
    seq_poses = [(BASE @ U.se3_exp(tuple(k * x for x in XI))).astype(np.float32) for k in range(6)]
    seq = [torch.from_numpy(syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.0)).to(dev) for i, p in enumerate(seq_poses)]
    frame_ms, worst = {m: [] for m in MODES}, {}
    for mode in MODES:
        track(mode, K, seq, dim, dev)                               # warm-up
    for _ in range(args.runs):
        for mode in MODES:
            rows, states, per = track(mode, K, seq, dim, dev)
            assert all(s == U.OK for s in states), (mode, states)
            frame_ms[mode].append(med(per))
            worst[mode] = round(max(pose_distance(seq_poses[0].astype(np.float64) @ row_pose(r), g)[0] for r, g in zip(rows, seq_poses)) * 1e3, 3)
    out["tracker_frame_ms"] = {m: round(med(v), 4) for m, v in frame_ms.items()}
    out["tracker_frame_ms_min_max"] = {m: [round(min(v), 4), round(max(v), 4)] for m, v in frame_ms.items()}
    out["tracker_largest_error_mm"] = worst

    if args.drift:
        n = 64
        gt = [loop_pose(k, n) for k in range(n + 1)]                # frame n is frame 0 again
        noisy = [torch.from_numpy(syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.004)).to(dev) for i, p in enumerate(gt)]
        drift = {}
        for mode in MODES:
            rows, states, _ = track(mode, K, noisy, dim, dev)
            err = [pose_distance(gt[0].astype(np.float64) @ row_pose(r), g) for r, g in zip(rows, gt)]
            drift[mode] = {"frames": n + 1, "lost": int(sum(s != U.OK for s in states)), "final_mm": round(err[-1][0] * 1e3, 3), "final_deg": round(err[-1][1], 4),
                           "largest_mm": round(max(e[0] for e in err) * 1e3, 3), "largest_deg": round(max(e[1] for e in err), 4)}
        out["drift_noise_0.004"] = drift
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
