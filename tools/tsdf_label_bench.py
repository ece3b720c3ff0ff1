"""What instance labels in the TSDF volume cost: every label entry point against the call it runs beside, in ONE job, on section
17's workload -- `synthetic.render_depth` frames at 456 x 616 (scale 1.0) into a dim^3 volume of 2 cm voxels, the frustum box for far = 5 m.  The
instance images label a pixel by the 1 m cell of the room its surface point lies in (12 ids), so the frames agree about a surface as a map's keyframes do.

    python tools/tsdf_label_bench.py [--runs 9] [--scale 1.0] [--dim 512] [--out profiles/tsdf_label_bench.txt]

  vote            `ovo_tsdf_integrate_labels` against `ovo_tsdf_integrate`, one frame over the same frustum box: device-event time of REP calls / REP
  raycast         `ovo_tsdf_raycast_labels` (depth and labels, one launch) against `ovo_tsdf_raycast`, one image
  extract_mesh    `TsdfVolume.extract_mesh(labels=True)` against `extract_mesh()` over the whole volume: device-event time around the call, its one host
                  wait for (V, T) and its allocations included
  remap           `ovo_tsdf_labels_remap` over the whole label array (a table that merges two instances and removes one) against a plain device copy of
                  the array
  semantic_mesh   `OVO.semantic_mesh(instance=)` with the volume's own labels against the 5-NN transfer from a point map (every 4th pixel of the three
                  frames, back-projected) on the same mesh
Each pair alternates for RUNS rounds after a warm-up; medians, with the smallest and largest.  Before anything is timed the outputs are compared: the
ray-cast depth and the mesh must be bit-equal with labels on and off, a second vote of the same frames must reproduce the label array, and the remap must
leave no merged-away id.  None of the figures is a pass mark.  Writes one JSON line to --out and prints it."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ovo_amd import synthetic as syn
from ovo_amd.entities.ovo import OVO
from ovo_amd.utils import icp_utils as U
from ovo_amd.utils import tsdf_utils as TU
from tsdf_bench import BASE, FAR, NEAR, REP, TRUNC, VOXEL, XI, copy_gbs, timed


def world_points(d, p, K):
    """(points f32 [h, w, 3] in the world, valid mask) of a depth image seen from p."""
    h, w = d.shape
    v, u = torch.meshgrid(torch.arange(h, device=d.device), torch.arange(w, device=d.device), indexing="ij")
    ok = torch.isfinite(d) & (d > NEAR) & (d < FAR)
    z = torch.where(ok, d, torch.zeros_like(d))
    cam = torch.stack([(u - float(K[0, 2])) / float(K[0, 0]) * z, (v - float(K[1, 2])) / float(K[1, 1]) * z, z], -1)
    m = torch.from_numpy(p).to(d.device)
    return cam @ m[:3, :3].t() + m[:3, 3], ok


def instance_image(d, p, K):
    """i32 [h, w]: the id of the 1 m cell of the world the pixel's surface point lies in, 0 .. 11; -1 without a valid depth."""
    x, ok = world_points(d, p, K)
    c = torch.floor(x + 0.013).to(torch.int64)               # (off the walls' own coordinates)
    ids = torch.remainder(c[..., 0], 3) + 3 * torch.remainder(c[..., 1], 2) + 6 * torch.remainder(c[..., 2], 2)
    return torch.where(ok, ids, torch.full_like(ids, -1)).to(torch.int32).contiguous()


def point_map(depths, images, poses, K, step=4):
    """A sparse map as the keyframes make one: every `step`-th pixel with a valid depth, back-projected, with its pixel's instance id."""
    pts, ids = [], []
    for d, ins, p in zip(depths, images, poses):
        h, w = d.shape
        v, u = torch.meshgrid(torch.arange(0, h, step, device=d.device), torch.arange(0, w, step, device=d.device), indexing="ij")
        z = d[v, u]
        ok = torch.isfinite(z) & (z > NEAR) & (z < FAR)
        cam = torch.stack([(u - float(K[0, 2])) / float(K[0, 0]) * z, (v - float(K[1, 2])) / float(K[1, 1]) * z, z], -1)[ok]
        m = torch.from_numpy(p).to(d.device)
        pts.append(cam @ m[:3, :3].t() + m[:3, 3])
        ids.append(ins[v, u][ok])
    return torch.cat(pts).to(torch.float32).contiguous(), torch.cat(ids).to(torch.int32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tsdf_label_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tsdf_label_bench needs a GPU"
    assert args.runs >= 7, "the median of at least 7 runs"
    dev = torch.device("cuda", 0)
    med = statistics.median
    stream_gbs = copy_gbs(dev)
    K, (h, w) = syn.scannet_intrinsics(args.scale), syn.scannet_depth_hw(args.scale)
    dim = args.dim
    origin = [0.2 - 0.5 * VOXEL * (dim - 1), -0.5 * VOXEL * (dim - 1), 0.2 - 0.5 * VOXEL * (dim - 1)]      # around the room's centre, world frame
    poses = [(BASE @ U.se3_exp(tuple(k * x for x in XI))).astype(np.float32) for k in range(3)]
    depths = [torch.from_numpy(syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.0)).to(dev) for i, p in enumerate(poses)]
    images = [instance_image(d, p, K) for d, p in zip(depths, poses)]
    plain = TU.TsdfVolume((dim, dim, dim), VOXEL, origin, TRUNC, 64, device=dev)
    labelled = TU.TsdfVolume((dim, dim, dim), VOXEL, origin, TRUNC, 64, device=dev, labels=True)
    boxes = [plain.frustum_box(K, h, w, p, NEAR, FAR) for p in poses]
    dz = TRUNC / 2

    # ---- labels change nothing they share with the plain form: compared before anything is timed
    for d, ins, p, b in zip(depths, images, poses, boxes):
        plain.integrate(d, K, p, NEAR, FAR, box=b)
        labelled.integrate(d, K, p, NEAR, FAR, box=b)
        labelled.integrate_labels(d, ins, K, p, NEAR, FAR, box=b)
    first = labelled.lab.clone()
    labelled.lab.zero_()
    for d, ins, p, b in zip(depths, images, poses, boxes):
        labelled.integrate_labels(d, ins, K, p, NEAR, FAR, box=b)
    depth_p = plain.raycast(K, h, w, poses[1], NEAR, FAR, dz)
    depth_l, image = labelled.raycast(K, h, w, poses[1], NEAR, FAR, dz, labels=True)
    vp, fp = plain.extract_mesh()
    vl, fl, il = labelled.extract_mesh(labels=True)
    torch.cuda.synchronize()
    assert torch.equal(first, labelled.lab) and torch.equal(plain.vol.view(torch.int32), labelled.vol.view(torch.int32))
    assert torch.equal(depth_p.view(torch.int32), depth_l.view(torch.int32)) and bool((image[depth_l == 0] == -1).all()) and bool((image >= 0).any())
    assert torch.equal(vp.view(torch.int32), vl.view(torch.int32)) and torch.equal(fp, fl) and tuple(il.shape) == (vp.shape[0],)
    hits, voted = int((depth_l > 0).sum()), int((labelled.lab[..., 0] > 0).sum())
    table = torch.from_numpy(OVO.instance_table(12, {4: 1}, [7])).to(dev)
    keep = labelled.lab.clone()
    labelled.remap_labels(table)
    torch.cuda.synchronize()
    assert not bool(((labelled.lab[..., 0] == 5) | (labelled.lab[..., 0] == 8)).any()) and bool((keep[..., 0] == 5).any())
    del first
    labelled.lab.copy_(keep)
    pts, ids = point_map(depths, images, poses, K)
    ovo = object.__new__(OVO)
    map_data = (pts, None, ids.reshape(-1, 1))
    knn = ovo.semantic_mesh(map_data, vl, fl)["instance"]
    torch.cuda.synchronize()
    agree = float((knn == il)[(knn >= 0) & (il >= 0)].float().mean())

    box = boxes[1]
    box_voxels = int(np.prod([hi - lo for lo, hi in zip(*box)]))
    out_d, out_i = torch.empty((h, w), dtype=torch.float32, device=dev), torch.empty((h, w), dtype=torch.int32, device=dev)
    spare = torch.empty_like(labelled.lab)

    def remap():                                                    # the same work every time: from the voted array
        labelled.remap_labels(table)

    pairs = {"vote": (lambda: plain.integrate(depths[1], K, poses[1], NEAR, FAR, box=box),
                      lambda: labelled.integrate_labels(depths[1], images[1], K, poses[1], NEAR, FAR, box=box), REP),
             "raycast": (lambda: plain.raycast(K, h, w, poses[1], NEAR, FAR, dz, out=out_d),
                         lambda: labelled.raycast(K, h, w, poses[1], NEAR, FAR, dz, out=out_d, labels=True, out_ins=out_i), REP),
             "extract_mesh": (lambda: plain.extract_mesh(), lambda: labelled.extract_mesh(labels=True), 1),
             "remap": (lambda: spare.copy_(keep), remap, 1),
             "semantic_mesh": (lambda: ovo.semantic_mesh(map_data, vl, fl), lambda: ovo.semantic_mesh(map_data, vl, fl, instance=il), 1)}
    ms = {}
    for name, (off, on, rep) in pairs.items():
        for _ in range(2):                                          # warm-up of every shape the timed window uses
            off(), on()
        ms[name], ms[name + "_labels"] = [], []
        for _ in range(args.runs):                                  # alternating
            if name == "remap":
                labelled.lab.copy_(keep)                            # (outside the timed window: a remapped array has nothing left to change)
            ms[name].append(timed(off, rep))
            ms[name + "_labels"].append(timed(on, rep))

    figures = lambda v: {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out = {"tool": "tsdf_label_bench", "runs": args.runs, "rep": REP, "image": [h, w], "volume": [dim] * 3, "voxel": VOXEL, "trunc": TRUNC, "far": FAR, "dz": dz,
           "stream_copy_gbs": round(stream_gbs, 1), "box": [list(box[0]), list(box[1])], "box_voxels": box_voxels, "labelled_voxels_3_frames": voted,
           "hits": hits, "mesh": {"vertices": int(vp.shape[0]), "triangles": int(fp.shape[0])}, "map_points": int(pts.shape[0]),
           "knn_agrees_with_volume_where_both_label": round(agree, 4),
           "unlabelled_vertices": {"knn": int((knn < 0).sum()), "volume": int((il < 0).sum())},
           "ms": {k: figures(v) for k, v in ms.items()},
           "baselines": {"vote": "ovo_tsdf_integrate", "raycast": "ovo_tsdf_raycast", "extract_mesh": "extract_mesh()", "remap": "device copy of the label array",
                         "semantic_mesh": "5-NN transfer"},
           "labels_over_baseline": {k: round(med(ms[k + "_labels"]) / med(ms[k]), 3) for k in pairs}}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
