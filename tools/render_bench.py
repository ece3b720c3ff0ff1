"""The view renderer's one pass over the map: `ovo_render_points` (fill + splat + decode) against the same algorithm restated in torch on the same
GPU (the matrix products, then `scatter_reduce_(..., "amin")` on int64 keys, one pass per footprint offset).

    python tools/render_bench.py [--sizes 1000000,5000000,10000000] [--radii 0,1,2] [--runs 9]

There is no path on the parent commit to compare with, so the restatement is the yardstick.  Per map size (`synthetic.padded_map`), view (480 x 640:
`inside` = a pose of the synthetic trajectory, in the room; `outside` = pulled back until the whole map is in view) and radius:
  hip_ms      device-event time of REP back-to-back `render_rows` calls / REP, median of RUNS after a warm-up
  torch_ms    device-event time of one restatement, median of RUNS, alternating with the HIP runs
  ratio       torch_ms / hip_ms
  gbs, frac_of_copy   12 B read per map row over hip_ms, and that rate over the stream-copy rate measured in THIS job the way bench.py's roofline leg
              measures it (torch copy of f32, 2 x 4 B per element)
The two results are compared before anything is timed.  torch's matrix products are not the kernel's FMA chains, so a point's pixel can differ (its
share is reported: `points_other_pixel`, against `ovo_project_points`); pixels within the footprint of such a point are left out (`pixels_left_out`).
On every other pixel both sides take the minimum over the same candidates of two depth functions that differ by rounding only, so the two depth
images must agree to that rounding (asserted: 1e-5 m at these depths) and emptiness must agree; `pixels_other_row` is the share of those pixels where
the rounding picked another of two nearly equal candidates.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ovo_amd import synthetic as syn
from ovo_amd.utils import geometry_utils as G, render_utils as R

REP = 10
H, W = 480, 640
I64_MAX = torch.iinfo(torch.int64).max


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


def torch_project(xyz, w2c, K):
    cam = torch.addmm(w2c[:3, 3], xyz, w2c[:3, :3].t())
    pix = cam @ K.t()
    return cam[:, 2].contiguous(), torch.round(pix[:, 0] / pix[:, 2]).long(), torch.round(pix[:, 1] / pix[:, 2]).long()


def torch_render(xyz, w2c, K, radius, near, far):
    zc, u, v = torch_project(xyz, w2c, K)
    ok = (zc >= near) & (zc <= far) & (u >= -radius) & (u < W + radius) & (v >= -radius) & (v < H + radius)
    keys = (zc.view(torch.int32).long() << 32) | torch.arange(xyz.shape[0], device=xyz.device)
    keys, u, v = keys[ok], u[ok], v[ok]
    img = torch.full((H * W,), I64_MAX, dtype=torch.int64, device=xyz.device)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            x, y = u + dx, v + dy
            inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            img.scatter_reduce_(0, (y * W + x)[inside], keys[inside], "amin")
    hit = img != I64_MAX
    row = torch.where(hit, img & 0xFFFFFFFF, torch.full_like(img, -1)).int().reshape(H, W)
    depth = torch.where(hit, img >> 32, torch.zeros_like(img)).int().view(torch.float32).reshape(H, W)
    return row, depth


def compare(xyz, view, w2c, K, radius, hip, ref):
    """What the docstring says: shares, and the assertion on the comparable pixels."""
    _, ut, vt = torch_project(xyz, w2c, K)
    uv = G.project_3d_points(xyz, K, w2c).long()
    other = (uv[:, 0] != ut) | (uv[:, 1] != vt)
    left_out = torch.zeros((H, W), dtype=torch.bool, device=xyz.device)
    r = radius + 1                                                  # either pixel of such a point, and both footprints
    for u, v in ((uv[other, 0], uv[other, 1]), (ut[other], vt[other])):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                x, y = u + dx, v + dy
                inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
                left_out[y[inside], x[inside]] = True
    keep = ~left_out
    assert torch.equal((hip[0] >= 0)[keep], (ref[0] >= 0)[keep]), "filled pixels differ"
    diff = float((hip[1] - ref[1]).abs()[keep].max()) if bool(keep.any()) else 0.0
    assert diff <= 1e-5, f"depth images differ by {diff}"
    return {"points_other_pixel": float(other.float().mean()), "pixels_left_out": float(left_out.float().mean()),
            "pixels_other_row": float((hip[0] != ref[0])[keep].float().mean()), "max_depth_diff": diff, "filled": float((hip[0] >= 0).float().mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,5000000,10000000")
    ap.add_argument("--radii", default="0,1,2")
    ap.add_argument("--runs", type=int, default=9)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "render_bench needs a GPU"
    dev = torch.device("cuda", 0)
    stream_gbs = copy_gbs(dev)
    K_host = syn.scannet_intrinsics(1.0)
    outside = np.eye(4, dtype=np.float32)
    outside[:3, 3] = (0.2, 0.0, -12.0)                              # the room (synthetic.ROOM_MIN / ROOM_MAX) 9.8 .. 14.6 m ahead, all of it inside the image
    poses = {"inside": syn.pose(2), "outside": outside}
    K = torch.from_numpy(K_host).to(dev)
    rows = []
    for n in (int(s) for s in args.sizes.split(",")):
        xyz = torch.from_numpy(syn.padded_map(n, frames=4, scale=1.0, seed=0)).to(dev)
        for name, c2w in poses.items():
            for radius in (int(s) for s in args.radii.split(",")):
                view = R.make_view(c2w, K_host, H, W, radius=radius)
                w2c = torch.tensor(list(view.w2c), dtype=torch.float32, device=dev).reshape(4, 4)
                near, far = float(view.near), float(view.far)
                hip = R.render_rows(xyz, view)
                ref = torch_render(xyz, w2c, K, radius, near, far)
                torch.cuda.synchronize()
                cmp = compare(xyz, view, w2c, K, radius, hip, ref)
                del ref, hip
                hip_ms, torch_ms = [], []
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(args.runs):                          # alternating
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(REP):
                        R.render_rows(xyz, view)
                    e1.record()
                    torch.cuda.synchronize()
                    hip_ms.append(e0.elapsed_time(e1) / REP)
                    e0.record()
                    torch_render(xyz, w2c, K, radius, near, far)
                    e1.record()
                    torch.cuda.synchronize()
                    torch_ms.append(e0.elapsed_time(e1))
                h, t = statistics.median(hip_ms), statistics.median(torch_ms)
                gbs = 12.0 * n / (h * 1e-3) / 1e9
                rows.append({"points": n, "view": name, "radius": radius, "hip_ms": round(h, 4), "hip_ms_min_max": [round(min(hip_ms), 4), round(max(hip_ms), 4)],
                             "torch_ms": round(t, 3), "torch_ms_min_max": [round(min(torch_ms), 3), round(max(torch_ms), 3)], "ratio": round(t / h, 1),
                             "gbs": round(gbs, 1), "frac_of_copy": round(gbs / stream_gbs, 3), **{k: round(v, 6) for k, v in cmp.items()}})
                print(f"[render_bench] {n} points, {name}, radius {radius}: hip {h:.4f} ms, torch {t:.3f} ms", file=sys.stderr, flush=True)
        del xyz
    print(json.dumps({"tool": "render_bench", "runs": args.runs, "rep": REP, "image": [H, W], "stream_copy_gbs": round(stream_gbs, 1), "bytes_per_row": 12,
                      "cases": rows}))


if __name__ == "__main__":
    main()
