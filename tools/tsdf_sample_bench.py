"""What reading the TSDF volume at arbitrary points costs: every form of `ovo_tsdf_sample_points` against the same gather written
in torch, and the label forms against the 5-NN transfer they can stand in for, in ONE job, on section 22's workload -- `synthetic.render_depth` frames at
456 x 616 (scale 1.0) fused with colour and labels into a dim^3 volume of 2 cm voxels.

    python tools/tsdf_sample_bench.py [--runs 9] [--scale 1.0] [--dim 512] [--out profiles/tsdf_sample_bench.txt]

  point sets      "mesh": the vertices of `extract_mesh()`, each moved by up to one voxel on every axis (points near the surface, in the mesh's order,
                  which follows the volume's memory); "uniform": 2^20 points uniform in the volume's box (mostly unseen space, no locality at all)
  forms           F only; + normals; + colour; + labels (nearest); + labels (vote); all outputs (vote).  Device-event time of REP calls / REP through
                  `TsdfVolume.sample`, output allocations included
  torch           the same gather in torch -- index arithmetic, eight `vol[...]` gathers, the blends, the selects -- for F, colour and the nearest
                  label.  No torch form of the gradient or of the vote is written: those two are reported against the sampler's own F-only form
  5-NN            `eval_utils.match_labels_to_vtx` from a point map (every 4th pixel of the three frames, back-projected) onto the same points, against
                  `eval_utils.match_volume_to_vtx` in both label modes; and the share of points on which they agree where both give a label
Each pair alternates for RUNS rounds after a warm-up; medians, with the smallest and largest, beside the job's own stream-copy figure.  Before anything
is timed the sampler's outputs are compared with the torch form's.  None of the figures is a pass mark.  Writes one JSON line to --out and prints it."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ovo_amd import synthetic as syn
from ovo_amd.utils import eval_utils as E
from ovo_amd.utils import icp_utils as U
from ovo_amd.utils import tsdf_utils as TU
from tsdf_bench import BASE, FAR, NEAR, REP, TRUNC, VOXEL, XI, copy_gbs, timed
from tsdf_label_bench import instance_image, point_map


def t_sample(volume, points, colors=False, labels=False, min_count=1):
    """`TsdfVolume.sample(points, colors=, labels=, label_mode="nearest")` in torch: (F, rgb, ins), the ones not asked for None."""
    nx, ny, nz = volume.dims
    org = torch.tensor(volume.origin, dtype=torch.float32, device=points.device)
    g = (points - org) / torch.tensor(volume.voxel, dtype=torch.float32, device=points.device)      # (a tensor: torch turns a division by a Python number into a product)
    bf = torch.floor(g)
    t = g - bf
    top = torch.tensor([nx - 2, ny - 2, nz - 2], dtype=torch.float32, device=points.device)
    inside = ((bf >= 0) & (bf <= top)).all(1)
    b = torch.where(inside[:, None], bf, torch.zeros_like(bf)).long()
    at = (b[:, 2] * ny + b[:, 1]) * nx + b[:, 0]
    offs = [dx + nx * dy + nx * ny * dz for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]          # corner x + 2 y + 4 z
    lerp = lambda p, q, s: p + s * (q - p)
    blend = lambda v: lerp(lerp(lerp(v[0], v[1], t[:, 0]), lerp(v[2], v[3], t[:, 0]), t[:, 1]), lerp(lerp(v[4], v[5], t[:, 0]), lerp(v[6], v[7], t[:, 0]), t[:, 1]), t[:, 2])
    flat = volume.vol.view(-1, 2)
    corners = [flat[at + o] for o in offs]
    seen = inside
    for c in corners:
        seen = seen & (c[:, 1] > 0)
    F = torch.where(seen, blend([c[:, 0] for c in corners]), torch.full_like(t[:, 0], 2.0))
    rgb = ins = None
    if colors:
        cflat = volume.col.view(-1, 4)
        q = [(cflat[at + o][:, :3].to(torch.int32) & 0xffff).to(torch.float32) for o in offs]
        pre = torch.stack([blend([c[:, ch] for c in q]) for ch in range(3)], 1)
        rgb = torch.where(seen[:, None], torch.round(torch.clamp(pre / 256.0, 0.0, 255.0)), torch.zeros_like(pre)).to(torch.uint8)
    if labels:
        near = (t >= 0.5).long()
        e = volume.lab.view(-1, 2)[at + near[:, 0] + nx * near[:, 1] + nx * ny * near[:, 2]]
        ins = torch.where(seen & (e[:, 0] > 0) & (e[:, 1] >= min_count), e[:, 0] - 1, torch.full_like(e[:, 0], -1))
    return F, rgb, ins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tsdf_sample_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tsdf_sample_bench needs a GPU"
    assert args.runs >= 7, "the median of at least 7 runs"
    dev = torch.device("cuda", 0)
    med = statistics.median
    stream_gbs = copy_gbs(dev)
    K, (h, w) = syn.scannet_intrinsics(args.scale), syn.scannet_depth_hw(args.scale)
    dim = args.dim
    origin = [0.2 - 0.5 * VOXEL * (dim - 1), -0.5 * VOXEL * (dim - 1), 0.2 - 0.5 * VOXEL * (dim - 1)]      # around the room's centre, world frame
    poses = [(BASE @ U.se3_exp(tuple(k * x for x in XI))).astype(np.float32) for k in range(3)]
    depths = [torch.from_numpy(syn.render_depth(p, K, h, w, i, invalid_frac=0.05, noise=0.0)).to(dev) for i, p in enumerate(poses)]
    colours = [torch.from_numpy(syn.render_rgb(h, w, i)).to(dev) for i in range(3)]
    images = [instance_image(d, p, K) for d, p in zip(depths, poses)]
    volume = TU.TsdfVolume((dim, dim, dim), VOXEL, origin, TRUNC, 64, device=dev, color=True, labels=True)
    for d, c, ins, p in zip(depths, colours, images, poses):
        box = volume.integrate(d, K, p, NEAR, FAR, rgb=c)
        volume.integrate_labels(d, ins, K, p, NEAR, FAR, box=box)
    verts, faces = volume.extract_mesh()
    gen = torch.Generator(device=dev)
    gen.manual_seed(23)
    lo, ext = torch.tensor(origin, dtype=torch.float32, device=dev), VOXEL * (dim - 1)
    sets = {"mesh": (verts + VOXEL * (2 * torch.rand(verts.shape, generator=gen, device=dev) - 1)).contiguous(),
            "uniform": (lo + ext * torch.rand((1 << 20, 3), generator=gen, device=dev)).contiguous()}
    map_pts, map_ids = point_map(depths, images, poses, K)

    # ---- the sampler against the torch form, before anything is timed
    checks = {}
    for name, pts in sets.items():
        F, rgb, nrm, ins = volume.sample(pts, colors=True, normals=True, labels=True)
        vote = volume.sample(pts, labels=True, label_mode="vote")[1]
        tF, trgb, tins = t_sample(volume, pts, colors=True, labels=True)
        torch.cuda.synchronize()
        seen = F < 2
        assert torch.equal(seen, tF < 2), "the sampler and the torch form disagree about which points are seen"
        dF, dc, dl = float((F - tF).abs().max()), int((rgb.int() - trgb.int()).abs().max()), int((ins != tins).sum())
        # (equal bits are the tests' business, against numpy; here a gross check that both forms compute the same thing -- the figures go into the result)
        assert dF < 1e-4 and dc <= 1 and dl <= 1e-3 * len(pts), f"{name}: the sampler against the torch form: |F| {dF}, colour levels {dc}, {dl} labels differ"
        length = nrm.norm(dim=1)
        assert bool(((length - 1).abs() < 1e-5)[length > 0].all()) and not bool(nrm[~seen].any()) and bool((ins[~seen] == -1).all()), f"{name}: normals or unseen points"
        checks[name] = {"points": int(pts.shape[0]), "seen": int(seen.sum()), "labelled_nearest": int((ins >= 0).sum()), "labelled_vote": int((vote >= 0).sum()),
                        "max_abs_F_minus_torch": dF, "rgb_levels_off_by_one": int((rgb != trgb).any(1).sum()), "labels_differ_from_torch": dl,
                        "vote_differs_from_nearest": int((vote != ins).sum())}

    forms = {"F": {}, "normals": {"normals": True}, "colour": {"colors": True}, "labels_nearest": {"labels": True}, "labels_vote": {"labels": True, "label_mode": "vote"},
             "all_vote": {"normals": True, "colors": True, "labels": True, "label_mode": "vote"}}
    torch_forms = {"F": {}, "colour": {"colors": True}, "labels_nearest": {"labels": True}}
    ms, ratios, agree = {}, {}, {}
    figures = lambda v: {"median": round(med(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    for name, pts in sets.items():
        for form, kw in forms.items():
            on = lambda: volume.sample(pts, **kw)
            off = (lambda: t_sample(volume, pts, **torch_forms[form])) if form in torch_forms else (lambda: volume.sample(pts))
            for _ in range(2):                                      # warm-up of every shape the timed window uses
                off(), on()
            a, b = [], []
            for _ in range(args.runs):                              # alternating
                a.append(timed(off, REP))
                b.append(timed(on, REP))
            ms[f"{name}/{form}"] = figures(b)
            ms[f"{name}/{form}/{'torch' if form in torch_forms else 'F_only'}"] = figures(a)
            ratios[f"{name}/{form}"] = {"over": "torch form" if form in torch_forms else "the sampler's F-only form", "ratio": round(med(b) / med(a), 4)}
        # the label transfer: the volume against the map
        knn = lambda: E.match_labels_to_vtx(map_ids, map_pts, pts, device_out=True)
        vol_vote = lambda: E.match_volume_to_vtx(volume, pts, label_mode="vote", device_out=True)
        vol_near = lambda: E.match_volume_to_vtx(volume, pts, label_mode="nearest", device_out=True)
        for _ in range(2):
            knn(), vol_vote(), vol_near()
        a, b, c = [], [], []
        for _ in range(args.runs):
            a.append(timed(knn))
            b.append(timed(vol_vote))
            c.append(timed(vol_near))
        ms[f"{name}/match_labels_to_vtx"], ms[f"{name}/match_volume_to_vtx/vote"], ms[f"{name}/match_volume_to_vtx/nearest"] = figures(a), figures(b), figures(c)
        ratios[f"{name}/match_volume_to_vtx/vote"] = {"over": "match_labels_to_vtx", "ratio": round(med(b) / med(a), 4)}
        ratios[f"{name}/match_volume_to_vtx/nearest"] = {"over": "match_labels_to_vtx", "ratio": round(med(c) / med(a), 4)}
        k5, vv, vn = knn()[0], vol_vote()[0], vol_near()[0]
        both = lambda x: (x >= 0) & (k5 >= 0)
        agree[name] = {"vote_agrees_with_5nn_where_both_label": round(float((vv == k5)[both(vv)].float().mean()), 4), "both_label_vote": int(both(vv).sum()),
                       "nearest_agrees_with_5nn_where_both_label": round(float((vn == k5)[both(vn)].float().mean()), 4), "both_label_nearest": int(both(vn).sum()),
                       "vote_agrees_with_nearest": round(float((vv == vn).float().mean()), 4), "volume_gives_no_label": int((vv < 0).sum())}

    out = {"tool": "tsdf_sample_bench", "runs": args.runs, "rep": REP, "image": [h, w], "volume": [dim] * 3, "voxel": VOXEL, "trunc": TRUNC, "far": FAR,
           "stream_copy_gbs": round(stream_gbs, 1), "mesh": {"vertices": int(verts.shape[0]), "triangles": int(faces.shape[0])}, "map_points": int(map_pts.shape[0]),
           "checks": checks, "ms": ms, "ratios": ratios, "agreement": agree}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
