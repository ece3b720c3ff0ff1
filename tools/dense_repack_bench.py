"""The dense re-pack of a loop closure on one box: `ovo_dense_repack` (one launch, out of place) against two yardsticks on the same GPU in the same job.

    python tools/dense_repack_bench.py [--points 1000000] [--dim 1024] [--keyframes 300] [--runs 9]

The bench's shape: 1 M points, D = 1024, a table of a few hundred segments -- keyframes of random lengths, listed in a shuffled order, every tenth one
pruned; one process (src_shards = shard_count = 1), n_fill = the rows written.  All three move acc f32[*, D], cnt i32, cls i64 and conf f32 of the
surviving rows: bytes = rows_out x (4 D + 16), read once and written once.
  hip     device-event time of REP back-to-back `dense_repack` calls (argument checks + staging copy of the table + kernel each) / REP
  torch   (a) the composition the reference's style implies (orbslam.py:80-114: per keyframe a slice appended to a list per array, then one torch.cat
          per array), host clock around it ending in a synchronise -- its cost may be on the host
  copy    (b) a plain `copy_` of the same number of rows of the four arrays, device events: the ceiling (nothing is gathered)
Median of RUNS after a warm-up, the three alternating; the kernel's result is compared with (a) bit for bit before anything is timed.  Prints a table and
one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ovo_amd.slam.orbslam import dense_repack

REP = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--keyframes", type=int, default=300)
    ap.add_argument("--runs", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dense_repack_bench needs a GPU"
    dev = torch.device("cuda", 0)
    n, D, kf = args.points, args.dim, args.keyframes
    rng = np.random.default_rng(n + kf)
    cuts = np.sort(rng.integers(0, n + 1, kf - 1))
    starts = np.concatenate([[0], cuts]).astype(np.int64)
    lens = np.diff(np.concatenate([starts, [n]])).astype(np.int64)
    order = rng.permutation(kf)
    order = order[order % 10 != 3]                                                # every tenth keyframe pruned
    seg_src = starts[order]
    seg_dst = np.concatenate([[0], np.cumsum(lens[order])]).astype(np.int64)
    total = int(seg_dst[-1])
    gen = torch.Generator(device=dev).manual_seed(1)
    src = [torch.randn((n, D), dtype=torch.float32, device=dev, generator=gen), torch.randint(0, 1000, (n,), dtype=torch.int32, device=dev, generator=gen),
           torch.randint(-1, 10, (n,), dtype=torch.int64, device=dev, generator=gen), torch.rand((n,), dtype=torch.float32, device=dev, generator=gen)]
    out = [torch.empty_like(t[:total]) for t in src]
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    ranges = [(int(s), int(s + l)) for s, l in zip(seg_src, lens[order])]

    def hip():
        dense_repack(src, out, n, seg_src, seg_dst, total, ws=ws)

    def composition():
        return [torch.cat([t[a:b] for a, b in ranges], dim=0) for t in src]

    def copy():
        for o, t in zip(out, src):
            o.copy_(t[:total])

    hip()
    ref = composition()
    torch.cuda.synchronize()
    assert ref[0].shape[0] == total
    for o, r in zip(out, ref):
        assert torch.equal(o.view(torch.int32) if o.dtype == torch.float32 else o, r.view(torch.int32) if r.dtype == torch.float32 else r)
    del ref
    copy()
    torch.cuda.synchronize()
    ms = {"hip": [], "torch": [], "copy": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.runs):                                                    # alternating
        for name, fn in (("hip", hip), ("copy", copy)):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(REP):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / REP)
        t = time.perf_counter()
        r = composition()
        torch.cuda.synchronize()
        ms["torch"].append(1e3 * (time.perf_counter() - t))
        del r
    moved = 2.0 * total * (4 * D + 16)
    res = {"tool": "dense_repack_bench", "points": n, "dim": D, "keyframes": kf, "segments": len(order), "rows_out": total, "bytes_moved": int(moved),
           "runs": args.runs}
    print(f"{n} points x D {D}, {len(order)} segments of {kf} keyframes, {total} rows out, {moved / 1e9:.3f} GB moved (read + written)")
    print(f"{'':34s}{'ms (median)':>12s}{'min':>9s}{'max':>9s}{'GB/s':>9s}")
    for name, label in (("hip", "ovo_dense_repack, one launch"), ("torch", "(a) slices + torch.cat per array"), ("copy", "(b) copy_ of the same bytes")):
        m = statistics.median(ms[name])
        print(f"{label:34s}{m:12.3f}{min(ms[name]):9.3f}{max(ms[name]):9.3f}{moved / (m * 1e-3) / 1e9:9.1f}")
        res[name + "_ms"], res[name + "_ms_min_max"], res[name + "_gbs"] = round(m, 4), [round(min(ms[name]), 4), round(max(ms[name]), 4)], round(moved / (m * 1e-3) / 1e9, 1)
    res["torch_over_hip"] = round(res["torch_ms"] / res["hip_ms"], 2)
    res["hip_frac_of_copy"] = round(res["hip_gbs"] / res["copy_gbs"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
