"""Loop-closure verification: `ovo_icp_align_batch` with m references against m back-to-back `ovo_icp_align` calls, and the pose graph's host time.

    python tools/loop_bench.py [--runs 9]

Frames: `synthetic.render_depth` at 456 x 616, 3 levels, 10 / 5 / 4 iterations; the current frame is the two-wall pose moved by motion A of the
tests, reference j is the view from which the current frame is (0.5 + j / 16) x motion A away, every alignment started at the identity.  Before
anything is timed every entry of the 16-batch is compared with its single call (asserted: the same bits) and must be OK.
  batch_ms[m]       device-event time of REP batch calls of m entries / REP, median of RUNS after a warm-up
  sequential_ms[m]  the same for m `ovo_icp_align` calls queued back to back -- own pose row, own result block, ONE wait at the end, so no host wait
                    sits between them -- alternating with the batch runs
  graph_ms[n]       `pose_graph.optimise` on the host: a chain of n keyframes with a loop edge back by n / 2 every tenth keyframe, 2 cm / 1 deg
                    of drift per step in the start poses; median of 3 runs (1 run at n = 1000)
Prints one JSON line."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ovo_amd import _lib as L
from ovo_amd import synthetic as syn
from ovo_amd.slam import pose_graph
from ovo_amd.utils import icp_utils as U

REP = 5
LEVELS, ITERS = 3, (10, 5, 4)
DIST_TH, NORMAL_DEG, MAX_DEPTH, JUMP = 0.1, 30.0, 10.0, 0.1
XI_A = np.array((0.01, -0.02, 0.015, 0.02, 0.01, -0.015))
SIZES = (1, 4, 8, 16)


def rot(axis, a):
    c, s = math.cos(a), math.sin(a)
    m = np.eye(4)
    i, j = ((1, 2), (2, 0))[axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def timed(fn, rep):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(rep):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / rep


def graph_case(n, rng):
    truth = [np.eye(4)]
    for k in range(1, n):
        truth.append(truth[-1] @ U.se3_exp((0.0, 0.05, 0.0, 0.1, 0.0, 0.02)))
    weight = np.diag([4e4, 4e4, 4e4, 1e4, 1e4, 1e4])
    noisy = lambda i, j: U.se3_exp(rng.normal(size=6) * 1e-3) @ U.rigid_inverse(truth[i]) @ truth[j]
    edges = [(k - 1, k, noisy(k - 1, k), weight) for k in range(1, n)]
    edges += [(k - n // 2, k, noisy(k - n // 2, k), weight) for k in range(n // 2, n, 10)]
    start = [np.eye(4)]
    for k in range(1, n):
        start.append(start[-1] @ U.rigid_inverse(truth[k - 1]) @ truth[k] @ U.se3_exp((0.0, math.radians(1.0) / 10, 0.0, 0.002, 0.0, 0.0)))
    return start, edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loop_bench needs a GPU"
    assert args.runs >= 7, "the median of at least 7 runs"
    dev = torch.device("cuda", 0)
    lib = L.load()
    K, (h, w) = syn.scannet_intrinsics(1.0), syn.scannet_depth_hw(1.0)
    base = rot(1, 0.75) @ rot(0, 0.45)
    c1 = (base @ U.se3_exp(XI_A)).astype(np.float32)
    depth = lambda pose, seed: torch.from_numpy(syn.render_depth(pose, K, h, w, seed, invalid_frac=0.05, noise=0.0)).to(dev)
    cur = U.prepare_frame(depth(c1, 1), K, LEVELS, MAX_DEPTH, JUMP)
    refs = [U.prepare_frame(depth((c1.astype(np.float64) @ U.rigid_inverse(U.se3_exp((0.5 + j / 16) * XI_A))).astype(np.float32), 2 + j), K, LEVELS, MAX_DEPTH, JUMP)
            for j in range(U.MAX_BATCH)]
    min_pairs = int(math.ceil(0.05 * h * w))
    eye = torch.from_numpy(np.tile(np.eye(4, dtype=np.float32)[:3].reshape(12), (U.MAX_BATCH, 1))).to(dev)
    T = torch.empty_like(eye)
    ws = torch.empty(int(lib.ovo_icp_align_batch_workspace_bytes(U.MAX_BATCH)), dtype=torch.uint8, device=dev)
    host = L.PinnedRing(U.RESULT_WORDS * U.MAX_BATCH, np.int64, slots=1)
    desc = U.align_desc(ITERS, DIST_TH, NORMAL_DEG, min_pairs, 1e-6, 1)
    table = (C.c_void_p * U.MAX_BATCH)(*[r.pyramid.data_ptr() for r in refs])

    def batch(m):
        T.copy_(eye)
        L.check(lib.ovo_icp_align_batch(C.cast(table, C.c_void_p), C.byref(cur.desc), L.ptr(cur.pyramid), C.byref(cur.desc), C.byref(desc), m, L.ptr(T),
                                        C.c_void_p(host.base), L.ptr(ws), ws.numel(), L.stream()))

    def sequential(m):
        T.copy_(eye)
        for k in range(m):
            L.check(lib.ovo_icp_align(L.ptr(refs[k].pyramid), C.byref(cur.desc), L.ptr(cur.pyramid), C.byref(cur.desc), C.byref(desc),
                                      C.c_void_p(T.data_ptr() + 48 * k), C.c_void_p(host.base + 8 * U.RESULT_WORDS * k), L.ptr(ws), ws.numel(), L.stream()))

    def outcome(fn):
        host.view[:] = 0
        fn(U.MAX_BATCH)
        torch.cuda.synchronize()
        return T.cpu().numpy().view(np.int32).copy(), np.array(host.view[0]).reshape(U.MAX_BATCH, U.RESULT_WORDS)

    (Tb, Bb), (Ts, Bs) = outcome(batch), outcome(sequential)
    assert np.array_equal(Tb, Ts) and np.array_equal(Bb, Bs), "the batch and the single calls differ"
    results = [U.decode_result(b) for b in Bb]
    assert all(r["state"] == U.OK and r["iterations"] == sum(ITERS) for r in results)
    for m in SIZES:                                                  # warm-up
        batch(m), sequential(m)
    batch_ms, seq_ms = {m: [] for m in SIZES}, {m: [] for m in SIZES}
    for _ in range(args.runs):                                      # alternating
        for m in SIZES:
            batch_ms[m].append(timed(lambda: batch(m), REP))
            seq_ms[m].append(timed(lambda: sequential(m), REP))
    med = statistics.median
    rng = np.random.default_rng(0)
    graph = {}
    for n in (10, 100, 1000):
        start, edges = graph_case(n, rng)
        times = []
        for _ in range(1 if n == 1000 else 3):
            t0 = time.perf_counter()
            _, info = pose_graph.optimise(start, edges)
            times.append((time.perf_counter() - t0) * 1e3)
        assert info["improved"]
        graph[n] = {"ms": round(med(times), 2), "edges": len(edges), "steps": info["steps"], "cost0": info["cost0"], "cost": info["cost"],
                    "solver": "dense" if n <= pose_graph.DENSE_NODES else "sparse"}
    out = {"tool": "loop_bench", "runs": args.runs, "rep": REP, "image": [h, w], "levels": LEVELS, "iters": list(ITERS), "launches_per_call": 2 + 2 * sum(ITERS),
           "pair_fraction": [round(r["pairs"] / (h * w), 3) for r in results],
           "batch_ms": {m: round(med(batch_ms[m]), 4) for m in SIZES}, "batch_ms_min_max": {m: [round(min(batch_ms[m]), 4), round(max(batch_ms[m]), 4)] for m in SIZES},
           "sequential_ms": {m: round(med(seq_ms[m]), 4) for m in SIZES},
           "sequential_ms_min_max": {m: [round(min(seq_ms[m]), 4), round(max(seq_ms[m]), 4)] for m in SIZES},
           "sequential_over_batch": {m: round(med(seq_ms[m]) / med(batch_ms[m]), 2) for m in SIZES}, "graph": graph}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
