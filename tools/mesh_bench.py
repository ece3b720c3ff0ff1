"""The mesh extractor (`ovo_tsdf_mesh_plan` + `ovo_tsdf_mesh_emit`, csrc/mesh.hip) against the same algorithm written in torch on the same GPU.

    python tools/mesh_bench.py [--runs 9] [--dim 512] [--out profiles/mesh_bench.txt]

The workload is tools/tsdf_bench.py's: three 456 x 616 frames of `synthetic.render_depth` fused into a dim^3 volume of 2 cm voxels around the room.
There is no path on the parent commit to compare with, so a torch restatement is the yardstick: dense tensor operations classify every cell, the
cells the surface passes through are listed with `nonzero`, their triangles come from a 256-entry table built from tools/gen_mesh_table.py, the
used slots are marked with an indexed store and numbered with one `cumsum`.  The two results are compared before anything is timed (faces equal,
vertices bit-equal: asserted).
  extract_ms   device-event time of `TsdfVolume.extract_mesh()` -- workspace and outputs allocated, plan, the host wait for (V, T), emit -- median
               of RUNS after a warm-up, alternating with the torch form
  plan_ms / emit_ms   the two calls alone on a workspace and outputs allocated once
  volume_gbs   8 B x voxels of the volume over extract_ms and over plan_ms + emit_ms, against the stream-copy rate measured in THIS job
None of these is a pass mark.  Writes one JSON line to --out and prints it."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import gen_mesh_table as G
from tsdf_bench import BASE, FAR, NEAR, TRUNC, VOXEL, XI, copy_gbs, timed

from ovo_amd import _lib as L
from ovo_amd import synthetic as syn
from ovo_amd.utils import icp_utils as U
from ovo_amd.utils import tsdf_utils as TU


def cube_table():
    """codes i64[256, 12, 3]: the triangles of a cell by its corner mask, tetrahedron by tetrahedron; a vertex is owner corner | slot << 3, -1 = none."""
    tab = G.table()
    codes = np.full((256, 12, 3), -1, dtype=np.int64)
    for in8 in range(256):
        k = 0
        for n in range(6):
            c = G.tet_corners(n)
            m = sum(((in8 >> (p[0] + 2 * p[1] + 4 * p[2])) & 1) << r for r, p in enumerate(c))
            for tri in tab[n][m]:
                codes[in8, k] = [corner | slot << 3 for corner, slot in tri]
                k += 1
    return codes


def t_extract(vol, volume, codes):
    dev = vol.device
    F, W = vol[..., 0], vol[..., 1]
    nz, ny, nx = F.shape
    obs = (W >= 1.0) & (F.abs() <= 1.0)
    ins = obs & (F < 0)
    cv = lambda a, c: a[(c >> 2):nz - 1 + (c >> 2), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]
    valid = cv(obs, 0)
    in8 = cv(ins, 0).to(torch.int16)
    for c in range(1, 8):
        valid = valid & cv(obs, c)
        in8 = in8 | (cv(ins, c).to(torch.int16) << c)
    surf = valid & (in8 != 0) & (in8 != 255)
    cells = surf.nonzero()                                           # (z, y, x), in linear order
    tri = codes[in8[surf].long()]                                    # [n, 12, 3]
    lin = (cells[:, 0] * ny + cells[:, 1]) * nx + cells[:, 2]
    corner, slot = tri & 7, tri >> 3
    owner = lin[:, None, None] + (corner & 1) + ((corner >> 1) & 1) * nx + (corner >> 2) * (nx * ny)
    key = (owner * 7 + slot)[tri >= 0]                               # cell, then tetrahedron, then triangle, then vertex
    used = torch.zeros(nz * ny * nx * 7, dtype=torch.bool, device=dev)
    used[key] = True
    index = torch.cumsum(used, 0, dtype=torch.int32) - 1
    faces = index[key].view(-1, 3)
    kv = used.nonzero()[:, 0]
    own, s = kv // 7, kv % 7
    d = torch.tensor(G.SLOTS, dtype=torch.int64, device=dev)[s]
    p = torch.stack([own % nx, (own // nx) % ny, own // (nx * ny)], 1)
    Ff = F.reshape(-1)
    Fp, Fq = Ff[own], Ff[own + d[:, 0] + d[:, 1] * nx + d[:, 2] * (nx * ny)]
    t = Fp / (Fp - Fq)
    g = p.to(torch.float32) + t[:, None] * d.to(torch.float32)
    org = torch.tensor(volume.origin, dtype=torch.float32, device=dev)
    return org + torch.tensor(volume.voxel, dtype=torch.float32, device=dev) * g, faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mesh_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_bench needs a GPU"
    assert args.runs >= 7, "the median of at least 7 runs"
    dev = torch.device("cuda", 0)
    med = statistics.median
    stream_gbs = copy_gbs(dev)
    K, (h, w) = syn.scannet_intrinsics(1.0), syn.scannet_depth_hw(1.0)
    dim = args.dim
    origin = [0.2 - 0.5 * VOXEL * (dim - 1), -0.5 * VOXEL * (dim - 1), 0.2 - 0.5 * VOXEL * (dim - 1)]
    volume = TU.TsdfVolume((dim, dim, dim), VOXEL, origin, TRUNC, 64, device=dev)
    for i in range(3):
        pose = (BASE @ U.se3_exp(tuple(i * x for x in XI))).astype(np.float32)
        volume.integrate(torch.from_numpy(syn.render_depth(pose, K, h, w, i, invalid_frac=0.05, noise=0.0)).to(dev), K, pose, NEAR, FAR)
    codes = torch.from_numpy(cube_table()).to(dev)

    # ---- the two forms agree before anything is timed
    v, f = volume.extract_mesh()
    tv, tf = t_extract(volume.vol, volume, codes)
    torch.cuda.synchronize()
    V, T = int(v.shape[0]), int(f.shape[0])
    assert tuple(tv.shape) == (V, 3) and tuple(tf.shape) == (T, 3) and V > 0 and torch.equal(tf, f), (V, T, tuple(tv.shape), tuple(tf.shape))
    assert torch.equal(tv.view(torch.int32), v.view(torch.int32)), float((tv - v).abs().max())
    del tv, tf

    lib = L.load()
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(dim, dim, dim)
    nbytes = int(lib.ovo_tsdf_mesh_workspace_bytes(C.byref(volume.desc), lo, hi))
    ws, counts = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
    plan = lambda: L.check(lib.ovo_tsdf_mesh_plan(L.ptr(volume.vol), C.byref(volume.desc), lo, hi, 1.0, L.ptr(ws), nbytes, L.ptr(counts), L.stream()))
    emit = lambda: L.check(lib.ovo_tsdf_mesh_emit(L.ptr(volume.vol), C.byref(volume.desc), lo, hi, 1.0, L.ptr(ws), nbytes, L.ptr(v), L.ptr(f), V, T, L.stream()))
    hip = lambda: volume.extract_mesh()
    ref = lambda: t_extract(volume.vol, volume, codes)
    for _ in range(2):                                              # warm-up of every shape the timed window uses
        hip(), ref(), plan(), emit()
    ms = {k: [] for k in ("extract", "torch", "plan", "emit")}
    for _ in range(args.runs):                                      # alternating
        ms["extract"].append(timed(hip))
        ms["torch"].append(timed(ref))
        ms["plan"].append(timed(plan))
        ms["emit"].append(timed(emit))
    vol_bytes = 8 * dim ** 3
    gbs = lambda t: vol_bytes / (t * 1e-3) / 1e9
    kernels = med(ms["plan"]) + med(ms["emit"])
    out = {"tool": "mesh_bench", "runs": args.runs, "volume": [dim] * 3, "voxel": VOXEL, "trunc": TRUNC, "image": [h, w], "frames_fused": 3,
           "vertices": V, "triangles": T, "workspace_mib": round(nbytes / 2 ** 20, 1), "stream_copy_gbs": round(stream_gbs, 1),
           "hip_vs_torch": {"faces_equal": True, "vertices_bit_equal": True},
           "extract_ms": round(med(ms["extract"]), 4), "extract_ms_min_max": [round(min(ms["extract"]), 4), round(max(ms["extract"]), 4)],
           "plan_ms": round(med(ms["plan"]), 4), "plan_ms_min_max": [round(min(ms["plan"]), 4), round(max(ms["plan"]), 4)],
           "emit_ms": round(med(ms["emit"]), 4), "emit_ms_min_max": [round(min(ms["emit"]), 4), round(max(ms["emit"]), 4)],
           "torch_ms": round(med(ms["torch"]), 3), "torch_ms_min_max": [round(min(ms["torch"]), 3), round(max(ms["torch"]), 3)],
           "ratio_torch_over_extract": round(med(ms["torch"]) / med(ms["extract"]), 1),
           "volume_gbs_extract": round(gbs(med(ms["extract"])), 1), "volume_gbs_plan_emit": round(gbs(kernels), 1),
           "frac_of_copy_extract": round(gbs(med(ms["extract"])) / stream_gbs, 4), "frac_of_copy_plan_emit": round(gbs(kernels) / stream_gbs, 4)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
