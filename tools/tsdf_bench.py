"""The fused model's two kernels and the tracker that uses them: `ovo_tsdf_integrate` / `ovo_tsdf_raycast` (csrc/tsdf.hip) against the same
algorithms written in torch on the same GPU, and a tracker frame in `model="tsdf"` mode against `model="keyframe"` mode.

    python tools/tsdf_bench.py [--runs 9] [--scale 1.0] [--dim 512] [--drift] [--out profiles/tsdf_bench.txt]

There is no path on the parent commit to compare with, so torch restatements are the yardstick: dense tensor operations over the frustum box
(integrate) and over all pixels for every step of the march (ray cast).  Frames: `synthetic.render_depth` at 456 x 616 (scale 1.0), a dim^3 volume
of 2 cm voxels around the room, the frustum box for far = 5 m.  Results are compared before anything is timed (asserted: at most one voxel or pixel in a thousand differs, by a decision on a rounding boundary).
  integrate_ms   device-event time of REP calls / REP, median of RUNS after a warm-up, alternating with the torch form; gbs = 16 B x voxels of the
                 box over that time (a voxel read and written once), against the stream-copy rate measured in THIS job
  raycast_ms     likewise; a ray stops at its hit
  tracker        wall-clock milliseconds per frame of IcpTracker over a short sequence (each frame ends with the tracker's one host wait), the two
                 modes alternating, medians of RUNS
  --drift        a closed loop of 64 frames with noise 0.004 in both modes: the final and the largest distance to the ground truth
None of these is a pass mark.  Writes one JSON line to --out and prints it."""
import argparse
import json
import math
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

REP = 5
VOXEL, TRUNC, NEAR, FAR = 0.02, 0.08, 0.05, 5.0
XI = (0.01, -0.02, 0.015, 0.02, 0.01, -0.015)


def copy_gbs(dev):
    n = 1 << 26                                                    # 256 MiB of f32
    a, b = torch.ones(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.copy_(a)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(10):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 10 * 2 * 4 * n / (e0.elapsed_time(e1) * 1e-3) / 1e9


def rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    m = np.eye(4)
    i, j = ((1, 2), (2, 0))[axis]                                   # axis 0: x, 1: y
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


BASE = rot(1, 0.75) @ rot(0, 0.45)


def timed(fn, rep=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(rep):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / rep


# ---- the same algorithms in torch ----
def t_integrate(vol, volume, depth, K, c2w, box):
    (x0, y0, z0), (x1, y1, z1) = box
    dev = vol.device
    ax = [volume.origin[a] + volume.voxel * torch.arange(lo, hi, device=dev, dtype=torch.float32) for a, (lo, hi) in enumerate(((x0, x1), (y0, y1), (z0, z1)))]
    Z, Y, X = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    m = torch.from_numpy(TU.rigid_inverse_f32(c2w)).to(dev)
    P = [m[r, 0] * X + m[r, 1] * Y + m[r, 2] * Z + m[r, 3] for r in range(3)]
    h, w = depth.shape
    u, v = torch.round(float(K[0, 0]) * P[0] / P[2] + float(K[0, 2])), torch.round(float(K[1, 1]) * P[1] / P[2] + float(K[1, 2]))
    inside = (P[2] > 0) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
    at = torch.where(inside, v * w + u, torch.zeros_like(u)).long()
    d = depth.reshape(-1)[at]
    sdf = d - P[2]
    upd = inside & torch.isfinite(d) & (d >= NEAR) & (d <= FAR) & ~(sdf < -volume.trunc)
    f = torch.clamp(sdf / volume.trunc, max=1.0)
    sub = vol[z0:z1, y0:y1, x0:x1]
    F, W = sub[..., 0], sub[..., 1]
    W1 = W + 1
    sub[..., 0] = torch.where(upd, (F * W + f) / W1, F)
    sub[..., 1] = torch.where(upd, torch.clamp(W1, max=volume.max_weight), W)


def t_raycast(vol, volume, K, h, w, c2w, dz):
    dev = vol.device
    nx, ny, nz = volume.dims
    F, seen = vol[..., 0].reshape(-1), (vol[..., 1] > 0).reshape(-1)
    c = torch.from_numpy(np.asarray(c2w, dtype=np.float32)).to(dev)
    dcx = ((torch.arange(w, device=dev, dtype=torch.float32) - float(K[0, 2])) / float(K[0, 0]))[None, :].expand(h, w)
    dcy = ((torch.arange(h, device=dev, dtype=torch.float32) - float(K[1, 2])) / float(K[1, 1]))[:, None].expand(h, w)
    dw = [c[r, 0] * dcx + c[r, 1] * dcy + c[r, 2] for r in range(3)]
    depth = torch.zeros((h, w), device=dev)
    active = torch.ones((h, w), dtype=torch.bool, device=dev)
    valid_prev = torch.zeros_like(active)
    f_prev = torch.zeros((h, w), device=dev)
    n = (nx, ny, nz)
    for k in range(TU.march_steps(NEAR, FAR, dz) + 1):              # (every step over all pixels: no host wait to ask whether any ray is left)
        zk = NEAR + k * dz
        g = [((c[a, 3] + zk * dw[a]) - volume.origin[a]) / volume.voxel for a in range(3)]
        b = [torch.floor(x) for x in g]
        t = [x - y for x, y in zip(g, b)]
        inr = active.clone()
        for a in range(3):
            inr &= (b[a] >= 0) & (b[a] <= n[a] - 2)
        bl = [torch.where(inr, x, torch.zeros_like(x)).long() for x in b]      # (whole numbers before the index is formed: 512^3 is beyond f32's integers)
        base = (bl[2] * ny + bl[1]) * nx + bl[0]
        corner = lambda dk, dj, di: base + (dk * ny + dj) * nx + di
        val = inr
        for dk in (0, 1):
            for dj in (0, 1):
                for di in (0, 1):
                    val = val & seen[corner(dk, dj, di)]
        lerp = lambda p, q, s: p + s * (q - p)
        cf = lambda dk, dj, di: F[corner(dk, dj, di)]
        f = lerp(lerp(lerp(cf(0, 0, 0), cf(0, 0, 1), t[0]), lerp(cf(0, 1, 0), cf(0, 1, 1), t[0]), t[1]),
                 lerp(lerp(cf(1, 0, 0), cf(1, 0, 1), t[0]), lerp(cf(1, 1, 0), cf(1, 1, 1), t[0]), t[1]), t[2])
        hit = val & valid_prev & (f_prev > 0) & (f <= 0)
        back = val & valid_prev & (f_prev <= 0) & (f > 0)
        depth = torch.where(hit, (NEAR + (k - 1) * dz) + dz * (f_prev / (f_prev - f)), depth)
        active = active & ~(hit | back)
        f_prev = torch.where(val, f, f_prev)
        valid_prev = val
    return depth


def pose_distance(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    r = a[:3, :3].T @ b[:3, :3]
    s = 0.5 * math.sqrt(sum((r[i, j] - r[j, i]) ** 2 for i, j in ((2, 1), (0, 2), (1, 0))))
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), math.degrees(math.atan2(s, (np.trace(r) - 1) * 0.5))


def loop_pose(k, n):
    """Frame k of a closed loop of n frames around BASE: at most 2.5 cm and 0.7 degrees a frame at n = 64."""
    a = 2 * math.pi * k / n
    return (BASE @ U.se3_exp((0.06 * math.sin(a), 0.12 * (1 - math.cos(a)), 0.04 * math.sin(2 * a), 0.25 * math.sin(a), 0.1 * (1 - math.cos(a)),
                              0.2 * math.sin(2 * a)))).astype(np.float32)


def track(mode, K, depths, dim, dev):
    """A fresh tracker over `depths` (device tensors): (rows, states, wall-clock ms per frame behind the first)."""
    kw = dict(model="tsdf", tsdf_dims=(dim, dim, dim), tsdf_voxel=VOXEL, tsdf_far=FAR, kf_min_overlap=0.1) if mode == "tsdf" else {}
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


def row_pose(row):
    return np.concatenate([np.asarray(row, np.float64)[1:].reshape(3, 4), [[0, 0, 0, 1]]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--drift", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tsdf_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tsdf_bench needs a GPU"
    assert args.runs >= 7, "the median of at least 7 runs"
    dev = torch.device("cuda", 0)
    med = statistics.median
    stream_gbs = copy_gbs(dev)
    K, (h, w) = syn.scannet_intrinsics(args.scale), syn.scannet_depth_hw(args.scale)
    dim = args.dim
    origin = [0.2 - 0.5 * VOXEL * (dim - 1), -0.5 * VOXEL * (dim - 1), 0.2 - 0.5 * VOXEL * (dim - 1)]      # around the room's centre, world frame
    poses = [(BASE @ U.se3_exp(tuple(k * x for x in XI))).astype(np.float32) for k in range(3)]
    depths = [torch.from_numpy(syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.0)).to(dev) for i, p in enumerate(poses)]
    volume, other = (TU.TsdfVolume((dim, dim, dim), VOXEL, origin, TRUNC, 64, device=dev) for _ in range(2))
    boxes = [volume.frustum_box(K, h, w, p, NEAR, FAR) for p in poses]
    dz = TRUNC / 2

    # ---- the two forms agree before anything is timed
    for d, p, b in zip(depths, poses, boxes):
        volume.integrate(d, K, p, NEAR, FAR, box=b)
        t_integrate(other.vol, other, d, K, p, b)
    torch.cuda.synchronize()
    dW = int((volume.vol[..., 1] != other.vol[..., 1]).sum())      # (a voxel on a pixel-rounding boundary may take the neighbouring pixel's depth in one form)
    dF = int(((volume.vol[..., 0] - other.vol[..., 0]).abs() > 1e-4).sum())
    got, want = volume.raycast(K, h, w, poses[1], NEAR, FAR, dz), t_raycast(volume.vol, volume, K, h, w, poses[1], dz)
    torch.cuda.synchronize()
    differ = int(((got > 0) != (want > 0)).sum())
    both = (got > 0) & (want > 0)
    dD = int(((got - want)[both].abs() > 1e-4).sum())
    hits = int((got > 0).sum())
    updated = int((volume.vol[..., 1] > 0).sum())
    assert dW <= 1e-3 * updated and dF <= 1e-3 * updated and differ <= 1e-3 * h * w and dD <= 1e-3 * h * w, (dW, dF, differ, dD)

    box = boxes[1]
    box_voxels = int(np.prod([hi - lo for lo, hi in zip(*box)]))
    out_img = torch.empty((h, w), dtype=torch.float32, device=dev)
    hip_int = lambda: volume.integrate(depths[1], K, poses[1], NEAR, FAR, box=box)
    torch_int = lambda: t_integrate(other.vol, other, depths[1], K, poses[1], box)
    hip_ray = lambda: volume.raycast(K, h, w, poses[1], NEAR, FAR, dz, out=out_img)
    torch_ray = lambda: t_raycast(volume.vol, volume, K, h, w, poses[1], dz)
    for _ in range(2):                                              # warm-up of every shape the timed window uses
        hip_int(), torch_int(), hip_ray(), torch_ray()
    ms = {k: [] for k in ("integrate", "torch_integrate", "raycast", "torch_raycast")}
    for _ in range(args.runs):                                      # alternating
        ms["integrate"].append(timed(hip_int, REP))
        ms["torch_integrate"].append(timed(torch_int))
        ms["raycast"].append(timed(hip_ray, REP))
        ms["torch_raycast"].append(timed(torch_ray))
    del other
    integ_gbs = 16 * box_voxels / (med(ms["integrate"]) * 1e-3) / 1e9

    # ---- a tracker frame, the two modes alternating
    n_seq = 6
    seq_poses = [(BASE @ U.se3_exp(tuple(k * x for x in XI))).astype(np.float32) for k in range(n_seq)]
    seq = [torch.from_numpy(syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.0)).to(dev) for i, p in enumerate(seq_poses)]
    del volume
    torch.cuda.empty_cache()
    frame_ms = {"tsdf": [], "keyframe": []}
    for mode in ("tsdf", "keyframe"):
        track(mode, K, seq, dim, dev)                               # warm-up
    for _ in range(args.runs):
        for mode in ("tsdf", "keyframe"):
            _, states, per = track(mode, K, seq, dim, dev)
            assert all(s == U.OK for s in states), (mode, states)
            frame_ms[mode].append(med(per))

    out = {"tool": "tsdf_bench", "runs": args.runs, "rep": REP, "image": [h, w], "volume": [dim] * 3, "voxel": VOXEL, "trunc": TRUNC, "far": FAR, "dz": dz,
           "stream_copy_gbs": round(stream_gbs, 1), "box": [list(box[0]), list(box[1])], "box_voxels": box_voxels, "updated_voxels_3_frames": updated,
           "hip_vs_torch": {"voxels_weight_differs": dW, "voxels_F_differs_1e-4": dF, "px_hit_differs": differ, "px_depth_differs_1e-4": dD, "hits": hits},
           "integrate_ms": round(med(ms["integrate"]), 4), "integrate_ms_min_max": [round(min(ms["integrate"]), 4), round(max(ms["integrate"]), 4)],
           "integrate_gbs": round(integ_gbs, 1), "integrate_frac_of_copy": round(integ_gbs / stream_gbs, 4),
           "torch_integrate_ms": round(med(ms["torch_integrate"]), 3), "integrate_ratio": round(med(ms["torch_integrate"]) / med(ms["integrate"]), 1),
           "raycast_ms": round(med(ms["raycast"]), 4), "raycast_ms_min_max": [round(min(ms["raycast"]), 4), round(max(ms["raycast"]), 4)],
           "march_steps": TU.march_steps(NEAR, FAR, dz) + 1,
           "torch_raycast_ms": round(med(ms["torch_raycast"]), 3), "raycast_ratio": round(med(ms["torch_raycast"]) / med(ms["raycast"]), 1),
           "tracker_frame_ms": {m: round(med(v), 4) for m, v in frame_ms.items()},
           "tracker_frame_ms_min_max": {m: [round(min(v), 4), round(max(v), 4)] for m, v in frame_ms.items()}}

    if args.drift:
        n = 64
        gt = [loop_pose(k, n) for k in range(n + 1)]                # frame n is frame 0 again
        noisy = [torch.from_numpy(syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.004)).to(dev) for i, p in enumerate(gt)]
        drift = {}
        for mode in ("tsdf", "keyframe"):
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
