"""What surface normals from the TSDF volume cost: every call that can return them against the same call without them in ONE
job, on section 17's workload -- `synthetic.render_depth` / `render_rgb` frames at 456 x 616 (scale 1.0) into a dim^3 volume of 2 cm voxels, far = 5 m.

    python tools/tsdf_normal_bench.py [--runs 9] [--scale 1.0] [--dim 512] [--out profiles/tsdf_normal_bench.txt]

  raycast         `ovo_tsdf_raycast_normals` (col NULL) against `ovo_tsdf_raycast`, one image: device-event time of REP calls / REP
  raycast_color   `ovo_tsdf_raycast_normals` with the colour volume against `ovo_tsdf_raycast_color`
  extract_mesh    `TsdfVolume.extract_mesh(normals=True)` against `extract_mesh()` over the whole volume: device-event time around the call, its one host
                  wait for (V, T) and its allocations included
  render          `IcpTracker.render_model(normals=True)`, and the same followed by `shade_normals`, against the plain ray cast of the tracker's volume
                  from the same pose (new tensors in all three)
Each group alternates for RUNS rounds after a warm-up; medians, with the smallest and largest, and each figure's ratio to the normal-free call of its
group.  Before anything is timed the forms are compared: the depth, the rgb and the mesh must be bit-equal with normals on and off.  None of the figures
is a pass mark.  Not measured: a tracker frame (nothing in the frame loop asks for normals), volumes other than dim^3, other image sizes.  Writes one
JSON line to --out and prints it."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ovo_amd import synthetic as syn
from ovo_amd.slam.icp_tracker import IcpTracker
from ovo_amd.utils import icp_utils as U
from ovo_amd.utils import tsdf_utils as TU
from tsdf_bench import BASE, FAR, NEAR, REP, TRUNC, VOXEL, XI, copy_gbs, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tsdf_normal_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tsdf_normal_bench needs a GPU"
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
    vol = TU.TsdfVolume((dim, dim, dim), VOXEL, origin, TRUNC, 64, device=dev, color=True)
    plain = TU.TsdfVolume((dim, dim, dim), VOXEL, origin, TRUNC, 64, device=dev)
    for d, c, p in zip(depths, rgbs, poses):
        vol.integrate(d, K, p, NEAR, FAR, rgb=c)
        plain.integrate(d, K, p, NEAR, FAR)
    dz = TRUNC / 2
    view = (K, h, w, poses[1], NEAR, FAR, dz)

    # ---- normals change nothing they share with the normal-free forms: compared before anything is timed
    bits = lambda t: t.view(torch.int32)
    d0 = plain.raycast(*view)
    d1, n1 = plain.raycast(*view, normals=True)
    d2, c2 = vol.raycast(*view, color=True)
    d3, c3, n3 = vol.raycast(*view, color=True, normals=True)
    v0, f0 = plain.extract_mesh()
    v1, f1, vn = plain.extract_mesh(normals=True)
    v2, f2, cc, vn2 = vol.extract_mesh(colors=True, normals=True)
    torch.cuda.synchronize()
    assert all(torch.equal(bits(d0), bits(x)) for x in (d1, d2, d3)) and torch.equal(c2, c3) and torch.equal(bits(n1), bits(n3))
    assert torch.equal(bits(v0), bits(v1)) and torch.equal(f0, f1) and torch.equal(bits(v0), bits(v2)) and torch.equal(bits(vn), bits(vn2))
    hit = d0 > 0
    lengths = n1[hit].double().norm(dim=1)
    unit = int(((lengths - 1).abs() < 1e-6).sum())
    assert not bool(bits(n1[~hit]).any()) and unit > 0.99 * int(hit.sum()) and tuple(vn.shape) == (v0.shape[0], 3)

    out_d, out_c = torch.empty((h, w), dtype=torch.float32, device=dev), torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    out_n = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
    tracker = IcpTracker(K, device=dev, model="tsdf", tsdf_dims=(dim, dim, dim), tsdf_voxel=VOXEL, tsdf_far=FAR, kf_min_overlap=0.1)
    for k, d in enumerate(depths):
        tracker.process_image_rgbd(None, d, k)
    assert tracker.get_tracking_state() == U.OK
    tv, tpose = tracker.volume, tracker.get_last_trajectory_point()[1:].reshape(3, 4)
    tpose = np.vstack([tpose, [0, 0, 0, 1]]).astype(np.float32)

    def shaded():
        d, n = tracker.render_model(normals=True)
        return TU.shade_normals(n, K, tpose)

    assert torch.equal(bits(tracker.render_model(normals=True)[0]), bits(tracker.model_depth)) and bool(shaded()[tracker.model_depth > 0].any())
    # a group: the normal-free call first, then the forms measured against it
    groups = {"raycast": ([("plain", lambda: plain.raycast(*view, out=out_d)),
                           ("normals", lambda: plain.raycast(*view, out=out_d, normals=True, out_normals=out_n))], REP),
              "raycast_color": ([("plain", lambda: vol.raycast(*view, out=out_d, color=True, out_rgb=out_c)),
                                 ("normals", lambda: vol.raycast(*view, out=out_d, color=True, out_rgb=out_c, normals=True, out_normals=out_n))], REP),
              "extract_mesh": ([("plain", lambda: plain.extract_mesh()), ("normals", lambda: plain.extract_mesh(normals=True))], 1),
              "render": ([("plain", lambda: tv.raycast(K, h, w, tpose, NEAR, FAR)), ("normals", lambda: tracker.render_model(normals=True)),
                          ("normals_shaded", shaded)], REP)}
    ms = {}
    for name, (forms, rep) in groups.items():
        for _ in range(2):                                          # warm-up of every shape the timed window uses
            for _, fn in forms:
                fn()
        ms[name] = {form: [] for form, _ in forms}
        for _ in range(args.runs):                                  # alternating
            for form, fn in forms:
                ms[name][form].append(timed(fn, rep))
    tracker.shutdown()

    figures = lambda v: {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out = {"tool": "tsdf_normal_bench", "runs": args.runs, "rep": REP, "image": [h, w], "volume": [dim] * 3, "voxel": VOXEL, "trunc": TRUNC, "far": FAR, "dz": dz,
           "stream_copy_gbs": round(stream_gbs, 1), "hits": int(hit.sum()), "unit_normals": unit,
           "mesh": {"vertices": int(v0.shape[0]), "triangles": int(f0.shape[0]), "zero_normals": int((~(vn != 0).any(1)).sum())},
           "ms": {g: {form: figures(v) for form, v in forms.items()} for g, forms in ms.items()},
           "over_plain": {g: {form: round(med(v) / med(forms["plain"]), 3) for form, v in forms.items() if form != "plain"} for g, forms in ms.items()}}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
