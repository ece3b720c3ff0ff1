"""The ICP tracker's frame: `ovo_icp_prepare` + `ovo_icp_align` (csrc/icp.hip) against the same algorithm written in torch on the same GPU.

    python tools/icp_bench.py [--runs 9] [--scale 1.0]

There is no path on the parent commit to compare with, so the torch restatement is the yardstick: dense tensor operations over the whole level
(masks instead of compaction, so it never waits for the host), f32 per pixel, the 6 x 6 system in f64, Cholesky and the SE(3) update on the
device.  Frames: `synthetic.render_depth` at 456 x 616 (scale 1.0), the two-wall pose and motion A of the tests, 3 levels, 10 / 5 / 4 iterations.
The two final poses are compared before anything is timed (asserted: 1e-5 m, 1e-4 deg -- torch's products are not the kernel's operation order).
  frame_ms      device-event time of REP x (prepare + align, result block read) / REP, median of RUNS after a warm-up; prepare_ms, align_ms likewise
  torch_ms      the restatement's prepare + align, median of RUNS, alternating with the HIP runs
  per level     align with that level's iterations only: ms per iteration (one reduce + one solve launch), the level's share of align_ms, and
                bytes per iteration (32 B per current pixel + 32 B gathered per pixel with a valid normal) over that time, against the
                stream-copy rate measured in THIS job (torch copy of f32, 2 x 4 B per element)
  fixed_ms      align_ms minus the levels' times: the init and publish launches and what the queue adds between 40 small launches
Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ovo_amd import synthetic as syn
from ovo_amd.utils import icp_utils as U

REP = 5
LEVELS, ITERS = 3, (10, 5, 4)
DIST_TH, NORMAL_DEG, MAX_DEPTH, JUMP = 0.1, 30.0, 10.0, 0.1


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


# ---- the restatement in torch ----
def t_valid(d):
    return torch.isfinite(d) & (d > 0) & (d <= MAX_DEPTH)


def t_prepare(depth, intr):
    out = []
    d = depth
    for l in range(LEVELS):
        if l:
            h2, w2 = d.shape[0] >> 1, d.shape[1] >> 1
            b = torch.stack([d[0:2 * h2:2, 0:2 * w2:2], d[0:2 * h2:2, 1:2 * w2:2], d[1:2 * h2:2, 0:2 * w2:2], d[1:2 * h2:2, 1:2 * w2:2]])
            m = t_valid(b)
            lo = torch.where(m, b, torch.full_like(b, float("inf"))).amin(0)
            take = m & (b - lo <= JUMP)
            cnt = take.sum(0).float()
            d = torch.where(cnt > 0, torch.where(take, b, torch.zeros_like(b)).sum(0) / cnt.clamp(min=1), torch.zeros_like(cnt))
        fx, fy, cx, cy = (float(x) for x in intr[l])
        h, w = d.shape
        ok = t_valid(d)
        dd = torch.where(ok, d, torch.zeros_like(d))
        u = torch.arange(w, device=d.device, dtype=torch.float32)[None, :]
        v = torch.arange(h, device=d.device, dtype=torch.float32)[:, None]
        V = torch.stack([(u - cx) * dd / fx, (v - cy) * dd / fy, dd], -1)
        c, xl, xr, yu, yd = V[1:-1, 1:-1], V[1:-1, :-2], V[1:-1, 2:], V[:-2, 1:-1], V[2:, 1:-1]
        nok = ok[1:-1, 1:-1] & ok[1:-1, :-2] & ok[1:-1, 2:] & ok[:-2, 1:-1] & ok[2:, 1:-1]
        for nb in (xl, xr, yu, yd):
            nok = nok & ((nb[..., 2] - c[..., 2]).abs() <= JUMP)
        n = torch.linalg.cross(xr - xl, yd - yu)
        length = n.norm(dim=-1)
        nok = nok & (length > 0)
        n = n / length.clamp(min=1e-30)[..., None]
        n = torch.where(((n * c).sum(-1) > 0)[..., None], -n, n)
        N = torch.zeros_like(V)
        N[1:-1, 1:-1] = torch.where(nok[..., None], n, torch.zeros_like(n))
        nm = torch.zeros_like(ok)
        nm[1:-1, 1:-1] = nok
        out.append((V.reshape(-1, 3), N.reshape(-1, 3), nm.reshape(-1), (h, w), (fx, fy, cx, cy)))
    return out


def t_exp(xi):
    w, v = xi[:3], xi[3:]
    th2 = (w * w).sum()
    th = th2.sqrt().clamp(min=1e-12)
    a, b, c = torch.sin(th) / th, (1 - torch.cos(th)) / th2.clamp(min=1e-24), (th - torch.sin(th)) / (th2 * th).clamp(min=1e-36)
    z = torch.zeros((), dtype=xi.dtype, device=xi.device)
    k = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device)
    out = torch.eye(4, dtype=xi.dtype, device=xi.device)
    out[:3, :3] = eye + a * k + b * (k @ k)
    out[:3, 3] = (eye + b * k + c * (k @ k)) @ v
    return out


def t_align(ref, cur, T, iters=ITERS):
    cos_th = math.cos(math.radians(NORMAL_DEG))
    for k, n_it in enumerate(iters):
        l = LEVELS - 1 - k
        Vr, Nr, mr, (h, w), (fx, fy, cx, cy) = ref[l]
        Vc, Nc, mc, _, _ = cur[l]
        for _ in range(n_it):
            T32 = T.float()
            P = Vc @ T32[:3, :3].t() + T32[:3, 3]
            N = Nc @ T32[:3, :3].t()
            z = P[:, 2]
            u, v = torch.round(fx * P[:, 0] / z + cx), torch.round(fy * P[:, 1] / z + cy)
            ok = mc & (z > 0) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
            at = torch.where(ok, v * w + u, torch.zeros_like(u)).long()
            q, nq = Vr[at], Nr[at]
            d = P - q
            keep = ok & mr[at] & ((d * d).sum(-1) <= DIST_TH * DIST_TH) & ((N * nq).sum(-1) >= cos_th)
            r = (nq * d).sum(-1)
            J = torch.cat([torch.linalg.cross(P, nq), nq], -1)
            wgt = keep.double()
            J64 = J.double() * wgt[:, None]
            A, b = J64.t() @ J64, J64.t() @ (r.double() * wgt)
            Lm, _ = torch.linalg.cholesky_ex(A)
            xi = torch.cholesky_solve(-b[:, None], Lm)[:, 0]
            T = (t_exp(xi) @ T).float().double()
    return T


def pose_distance(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    r = a[:3, :3].T @ b[:3, :3]
    s = 0.5 * math.sqrt(sum((r[i, j] - r[j, i]) ** 2 for i, j in ((2, 1), (0, 2), (1, 0))))
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), math.degrees(math.atan2(s, (np.trace(r) - 1) * 0.5))


def timed(fn, rep=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(rep):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "icp_bench needs a GPU"
    assert args.runs >= 7, "the median of at least 7 runs"
    dev = torch.device("cuda", 0)
    stream_gbs = copy_gbs(dev)
    K, (h, w) = syn.scannet_intrinsics(args.scale), syn.scannet_depth_hw(args.scale)
    base = rot(1, 0.75) @ rot(0, 0.45)
    c0, c1 = base.astype(np.float32), (base @ U.se3_exp((0.01, -0.02, 0.015, 0.02, 0.01, -0.015))).astype(np.float32)
    truth = np.linalg.inv(c0.astype(np.float64)) @ c1.astype(np.float64)
    d0 = torch.from_numpy(syn.render_depth(c0, K, h, w, 0, invalid_frac=0.05, noise=0.0)).to(dev)
    d1 = torch.from_numpy(syn.render_depth(c1, K, h, w, 1, invalid_frac=0.05, noise=0.0)).to(dev)
    intr = U.level_intrinsics(K, LEVELS)
    min_pairs = int(math.ceil(0.05 * h * w))
    aligner = U.Aligner(dev)
    eye = np.eye(4, dtype=np.float32)
    bufs = [torch.empty(int(U.L.load().ovo_icp_pyramid_bytes(h, w, LEVELS)), dtype=torch.uint8, device=dev) for _ in range(2)]
    ref = U.prepare_frame(d0, K, LEVELS, MAX_DEPTH, JUMP, out=bufs[0])
    eye_dev = torch.from_numpy(eye[:3].reshape(12).copy()).to(dev)

    def hip_prepare():
        return U.prepare_frame(d1, K, LEVELS, MAX_DEPTH, JUMP, out=bufs[1])

    def hip_align(cur, iters=ITERS):
        aligner.T.copy_(eye_dev)
        return aligner.wait(aligner.queue(ref, cur, iters, DIST_TH, NORMAL_DEG, min_pairs, 1e-6))

    def hip_frame():
        return hip_align(hip_prepare())

    def torch_frame():
        return t_align(t_ref, t_prepare(d1, intr), torch.eye(4, dtype=torch.float64, device=dev))

    t_ref = t_prepare(d0, intr)
    res = hip_frame()
    T_torch = torch_frame().cpu().numpy()
    assert res["state"] == U.OK and res["iterations"] == sum(ITERS)
    dt, dr = pose_distance(res["T"], T_torch)
    tt, tr = pose_distance(res["T"], truth)
    assert dt <= 1e-5 and dr <= 1e-4, f"the two results differ by {dt} m, {dr} deg"
    cur = hip_prepare()
    normals = [int((cur.level(l)[..., 7].view(torch.int32) & 1).sum()) for l in range(LEVELS)]
    for _ in range(2):                                              # warm-up of every shape the timed window uses
        hip_frame(), torch_frame()
        for k in range(LEVELS):
            hip_align(cur, tuple(ITERS[j] if j == k else 0 for j in range(LEVELS)))
    frame_ms, prep_ms, align_ms, torch_ms = [], [], [], []
    level_ms = [[] for _ in range(LEVELS)]
    for _ in range(args.runs):                                      # alternating
        frame_ms.append(timed(hip_frame, REP))
        torch_ms.append(timed(torch_frame))
        prep_ms.append(timed(hip_prepare, REP))
        align_ms.append(timed(lambda: hip_align(cur), REP))
        for k in range(LEVELS):
            level_ms[k].append(timed(lambda: hip_align(cur, tuple(ITERS[j] if j == k else 0 for j in range(LEVELS))), REP))
    med = statistics.median
    single = [med(level_ms[k]) for k in range(LEVELS)]
    # a one-level call carries the fixed part too: with s_k = fixed + t_k and align = fixed + sum t_k, fixed = (sum s_k - align) / (LEVELS - 1)
    fixed = (sum(single) - med(align_ms)) / (LEVELS - 1)
    levels = []
    for k in range(LEVELS):
        l = LEVELS - 1 - k
        hl, wl = h >> l, w >> l
        per_iter = (single[k] - fixed) / ITERS[k]
        nbytes = 32 * hl * wl + 32 * normals[l]
        levels.append({"level": l, "size": [hl, wl], "iters": ITERS[k], "ms_per_iteration": round(per_iter, 5), "share_of_align": round((single[k] - fixed) / med(align_ms), 3),
                       "bytes_per_iteration": nbytes, "gbs": round(nbytes / (per_iter * 1e-3) / 1e9, 1), "frac_of_copy": round(nbytes / (per_iter * 1e-3) / 1e9 / stream_gbs, 4)})
    out = {"tool": "icp_bench", "runs": args.runs, "rep": REP, "image": [h, w], "levels": LEVELS, "iters": list(ITERS), "launches_per_frame": 2 * LEVELS + 2 + 2 * sum(ITERS),
           "stream_copy_gbs": round(stream_gbs, 1), "pairs": res["pairs"], "pair_fraction": round(res["pairs"] / (h * w), 3),
           "hip_vs_torch_pose": [dt, dr], "hip_vs_truth_pose": [tt, tr],
           "frame_ms": round(med(frame_ms), 4), "frame_ms_min_max": [round(min(frame_ms), 4), round(max(frame_ms), 4)],
           "prepare_ms": round(med(prep_ms), 4), "align_ms": round(med(align_ms), 4), "fixed_ms": round(fixed, 4),
           "torch_ms": round(med(torch_ms), 3), "torch_ms_min_max": [round(min(torch_ms), 3), round(max(torch_ms), 3)],
           "ratio": round(med(torch_ms) / med(frame_ms), 1), "per_level": levels}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
