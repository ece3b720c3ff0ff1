"""The loop-closing map update on one box: `ovo_map_reanchor` (one launch, out of place) against the reference's algorithm restated in torch on the
same GPU (orbslam.py:80-114: per keyframe a slice, a cat with a ones column, an einsum and four appends, then four torch.cat over the whole map).

    python tools/reanchor_bench.py [--sizes 1000000x200,1000000x1000,5000000x200,5000000x1000] [--runs 9]

There is no path on the parent commit to compare with, so the restatement is the yardstick.  Per size (points x keyframes; keyframes of random
lengths, listed in a shuffled order, every tenth one pruned):
  hip_ms      device-event time of REP back-to-back ovo_map_reanchor calls (table check + staging copy + kernel each) / REP, median of RUNS after a
              warm-up
  torch_ms    host clock around the restatement ending in a synchronise (it is launch-bound: its cost is on the host), median of RUNS, alternating
              with the HIP runs
  ratio       torch_ms / hip_ms
  gbs, frac_of_copy   23 B read + 23 B written per output row over hip_ms, and that rate over the stream-copy rate measured in THIS job the way
              bench.py's roofline leg measures it (torch copy of f32, 2 x 4 B per element)
Results of the two are compared (integers exactly, xyz to 1e-4) before anything is timed.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ovo_amd.slam.orbslam import map_reanchor

REP = 10


def rigid(rng, max_angle, max_t):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-max_angle, max_angle)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    T[:3, 3] = rng.uniform(-max_t, max_t, 3)
    return T.astype(np.float32)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000x200,1000000x1000,5000000x200,5000000x1000")
    ap.add_argument("--runs", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "reanchor_bench needs a GPU"
    dev = torch.device("cuda", 0)
    stream_gbs = copy_gbs(dev)
    rows = []
    for size in args.sizes.split(","):
        n, kf = (int(x) for x in size.split("x"))
        rng = np.random.default_rng(n + kf)
        cuts = np.sort(rng.integers(0, n + 1, kf - 1))
        starts = np.concatenate([[0], cuts]).astype(np.int64)
        lens = np.diff(np.concatenate([starts, [n]])).astype(np.int64)
        order = rng.permutation(kf)
        order = order[order % 10 != 3]                                            # every tenth keyframe pruned
        seg_src = starts[order]
        seg_dst = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.int64)
        T = np.stack([rigid(rng, 0.05, 0.3) for _ in order])
        seg_T = np.ascontiguousarray(T[:, :3].reshape(len(order), 12))
        total = int(seg_dst[-1])
        xyz = torch.from_numpy(rng.uniform(-8, 8, (n, 3)).astype(np.float32)).to(dev)
        ids = torch.arange(n, dtype=torch.int32, device=dev)
        ins = torch.from_numpy(rng.integers(-1, 500, n).astype(np.int32)).to(dev)
        rgb = torch.from_numpy(rng.integers(0, 256, (n, 3)).astype(np.uint8)).to(dev)
        out = (torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 3), dtype=torch.uint8, device=dev))
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        T_dev = [torch.from_numpy(t).to(dev) for t in T]
        ranges = [(int(s), int(s + l)) for s, l in zip(seg_src, lens[order])]
        ids2, ins2 = ids.unsqueeze(1), ins.unsqueeze(1)

        def hip():
            map_reanchor((xyz, ids, ins, rgb), out, n, seg_src, seg_dst, seg_T, ws)

        def reference():                                                          # orbslam.py:80-114
            new_pcd, new_ids, new_ins, new_rgb = [], [], [], []
            for (a, b), t in zip(ranges, T_dev):
                new_pcd.append(torch.einsum("mn,bn->bm", t, torch.cat([xyz[a:b], torch.ones((b - a, 1), device=dev)], dim=1))[:, :3])
                new_ids.append(ids2[a:b])
                new_ins.append(ins2[a:b])
                new_rgb.append(rgb[a:b])
            return torch.cat(new_pcd, dim=0), torch.cat(new_ids, dim=0), torch.cat(new_ins, dim=0), torch.cat(new_rgb, dim=0)

        hip()
        ref = reference()
        torch.cuda.synchronize()
        assert ref[0].shape[0] == total
        assert torch.equal(out[1][:total], ref[1][:, 0]) and torch.equal(out[2][:total], ref[2][:, 0]) and torch.equal(out[3][:total], ref[3])
        max_diff = float((out[0][:total] - ref[0]).abs().max())
        assert max_diff < 1e-4, max_diff
        del ref
        hip_ms, torch_ms = [], []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.runs):                                                # alternating
            torch.cuda.synchronize()
            e0.record()
            for _ in range(REP):
                hip()
            e1.record()
            torch.cuda.synchronize()
            hip_ms.append(e0.elapsed_time(e1) / REP)
            t = time.perf_counter()
            r = reference()
            torch.cuda.synchronize()
            torch_ms.append(1e3 * (time.perf_counter() - t))
            del r
        h, t = statistics.median(hip_ms), statistics.median(torch_ms)
        gbs = 46.0 * total / (h * 1e-3) / 1e9
        rows.append({"points": n, "keyframes": kf, "segments": len(order), "rows_out": total, "hip_ms": round(h, 4), "hip_ms_min_max": [round(min(hip_ms), 4), round(max(hip_ms), 4)],
                     "torch_ms": round(t, 3), "torch_ms_min_max": [round(min(torch_ms), 3), round(max(torch_ms), 3)], "ratio": round(t / h, 1),
                     "gbs": round(gbs, 1), "frac_of_copy": round(gbs / stream_gbs, 3), "max_abs_diff_vs_torch": max_diff})
    print(json.dumps({"tool": "reanchor_bench", "runs": args.runs, "stream_copy_gbs": round(stream_gbs, 1), "bytes_per_row": 46, "sizes": rows}))


if __name__ == "__main__":
    main()
