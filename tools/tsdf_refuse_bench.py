"""Re-fusing a TSDF volume from N kept frames and what a loop closure costs a frame of
`IcpTracker(model="tsdf", tsdf_history=N)`.

    python tools/tsdf_refuse_bench.py [--runs 7] [--n 64,1024] [--history 256,1024] [--scale 1.0] [--dim 512] [--drift] [--out profiles/tsdf_refuse_bench.txt]

Section 17's workload: 456 x 616 frames of `synthetic.render_depth`, a 512^3 volume of 2 cm voxels, trunc 0.08, far 5 m.  The trajectory is a closed
loop of 64 poses walked N / 64 times; frame n is image n % 64 from pose n % 64.
  refuse_ms[N]     device-event time of reset + N x `ovo_tsdf_integrate`, each over its own frustum box (what `TsdfVolume.refuse` queues): median and
                   range of RUNS after a warm-up
  closing_frame    a tracker whose history holds H frames: wall-clock ms of what an applied closure adds to its frame (`TsdfReference.corrected`:
                   reset, re-fusion, ray cast, prepare, then one wait so that it can be timed -- the tracker itself does not wait) against the
                   median ordinary frame of the same tracker
  --drift          section 17's noisy closed loop (65 frames, noise 0.004): model="tsdf" alone against model="tsdf" with close_loops and a history
None of these is a pass mark.  Writes one JSON line to --out and prints it."""
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tsdf_bench import FAR, NEAR, TRUNC, VOXEL, loop_pose, pose_distance, row_pose, timed  # noqa: E402

LOOP = 64


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--n", default="64,1024")
    ap.add_argument("--history", default="256,1024")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--drift", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tsdf_refuse_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tsdf_refuse_bench needs a GPU"
    assert args.runs >= 5, "the median of at least 5 runs"
    dev = torch.device("cuda", 0)
    K, (h, w) = syn.scannet_intrinsics(args.scale), syn.scannet_depth_hw(args.scale)
    dim = args.dim
    origin = [0.2 - 0.5 * VOXEL * (dim - 1), -0.5 * VOXEL * (dim - 1), 0.2 - 0.5 * VOXEL * (dim - 1)]      # around the room's centre, world frame
    loop = [loop_pose(k, LOOP) for k in range(LOOP)]
    stack = torch.from_numpy(np.stack([syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.0) for i, p in enumerate(loop)])).to(dev)
    volume = TU.TsdfVolume((dim, dim, dim), VOXEL, origin, TRUNC, 64, device=dev)
    loop_boxes = [volume.frustum_box(K, h, w, p, NEAR, FAR) for p in loop]
    out = {"tool": "tsdf_refuse_bench", "runs": args.runs, "image": [h, w], "volume": [dim] * 3, "voxel": VOXEL, "trunc": TRUNC, "far": FAR, "refuse_ms": {}}

    for n in (int(x) for x in args.n.split(",") if x):
        slots = [i % LOOP for i in range(n)]

        def sequential():
            volume.reset()
            for s_ in slots:
                volume.integrate(stack[s_], K, loop[s_], NEAR, FAR, box=loop_boxes[s_])

        sequential()                                                # warm-up
        torch.cuda.synchronize()
        updated = int((volume.vol[..., 1] > 0).sum())
        ms = [timed(sequential) for _ in range(args.runs)]
        reset_ms = statistics.median([timed(volume.reset) for _ in range(args.runs)])
        out["refuse_ms"][str(n)] = {"box_voxels_sum": int(sum(np.prod([b - a for a, b in zip(*loop_boxes[s_])]) for s_ in slots)), "updated_voxels": updated,
                                    "reset_ms": round(reset_ms, 4), **stats(ms), "us_per_frame": round(1e3 * statistics.median(ms) / n, 2)}
    del volume
    torch.cuda.empty_cache()

    # ---- what a closure adds to a tracker's frame
    out["closing_frame"] = {}
    kw = dict(model="tsdf", tsdf_dims=(dim, dim, dim), tsdf_voxel=VOXEL, tsdf_far=FAR, kf_min_overlap=0.1)
    for H in (int(x) for x in args.history.split(",") if x):
        tracker = IcpTracker(K, device=dev, tsdf_history=H, **kw)
        frame_ms = []
        for k in range(H):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tracker.process_image_rgbd(None, stack[k % LOOP], k)
            torch.cuda.synchronize()
            frame_ms.append((time.perf_counter() - t0) * 1e3)
            assert tracker.get_tracking_state() == U.OK, k
        X = [row_pose(r) for r in tracker.get_keyframe_points()]    # the keyframes where they are: the work of a correction without the change
        ref, c2w = tracker._ref, tracker._c2w
        ref.corrected(X, c2w)                                       # warm-up
        torch.cuda.synchronize()
        extra = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            ref.corrected(X, c2w)
            torch.cuda.synchronize()
            extra.append((time.perf_counter() - t0) * 1e3)
        out["closing_frame"][str(H)] = {"history": len(tracker.history), "keyframes": len(X), "ordinary_frame_ms": stats(frame_ms[1:]),
                                        "closure_adds_ms": stats(extra)}
        tracker.shutdown()
        del tracker, ref
        torch.cuda.empty_cache()

    if args.drift:
        n = LOOP
        gt = [loop_pose(k, n) for k in range(n + 1)]                # frame n is frame 0 again
        noisy = [torch.from_numpy(syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.004)).to(dev) for i, p in enumerate(gt)]
        drift = {}
        for name, extra_kw in (("tsdf", {}), ("tsdf_loops_history", dict(close_loops=True, tsdf_history=n + 1, kf_translation=0.05)),
                               # (noisy keyframe images pair 16 .. 24 % of their pixels, under the default loop_min_overlap 0.3: a run with the gate at 0.1)
                               ("tsdf_loops_history_overlap_0.1", dict(close_loops=True, tsdf_history=n + 1, kf_translation=0.05, loop_min_overlap=0.1))):
            tracker = IcpTracker(K, device=dev, **kw, **extra_kw)
            rows, lost = [], 0
            for k, d in enumerate(noisy):
                tracker.process_image_rgbd(None, d, k)
                rows.append(tracker.get_last_trajectory_point().copy())
                lost += tracker.get_tracking_state() != U.OK
            err = [pose_distance(gt[0].astype(np.float64) @ row_pose(r), g) for r, g in zip(rows, gt)]
            drift[name] = {"frames": n + 1, "lost": int(lost), "keyframes": len(tracker.get_keyframe_points()), "closures_applied": tracker.get_last_big_change_idx(),
                           "loop_edges": len(tracker.loop_edges), "final_mm": round(err[-1][0] * 1e3, 3), "final_deg": round(err[-1][1], 4),
                           "largest_mm": round(max(e[0] for e in err) * 1e3, 3), "largest_deg": round(max(e[1] for e in err), 4)}
            last = tracker.last_loop                                # the last keyframe's verification: what the gates saw
            if last is not None:
                drift[name]["last_loop"] = {"n": last["n"], "candidates": len(last["candidates"]), "accepted": len(last["accepted"]),
                                            "results": [{"state": int(r["state"]), "pairs_frac": round(r["pairs"] / (h * w), 3), "rms": round(float(r["rms"]), 4)}
                                                        for r in last["results"]]}
            tracker.shutdown()
            del tracker
            torch.cuda.empty_cache()
        out["drift_noise_0.004"] = drift
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
