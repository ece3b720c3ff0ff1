"""The evaluation step on one box: the device path of utils/eval_utils.py against what the reference executes on the CPU (scipy cKDTree.query(k=5) +
torch.mode; a Python loop over all vertices for the confusion matrix), same seeded scenes (synthetic.eval_scene), warm, median of RUNS runs.

    python tools/eval_bench.py [--sizes 1000000x500000,50000x20000] [--runs 5]

Device times are host clocks around work that ends in a synchronise / a copy to the host:
  transfer_dev_ms   map and mesh already on the GPU -> grid build + query + mode + the labels copied back to the host
  transfer_host_ms  the same from host arrays (adds the upload of points, labels and vertices)
  grid_ms / query_ms   the two halves of transfer_dev_ms on their own (each ends in a synchronise)
  confusion_dev_ms  update_confmat on V (gt, prediction) pairs from host arrays, C = 51, into a host matrix
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ovo_amd import synthetic as syn
from ovo_amd.utils import eval_utils as E


def median_ms(fn, runs, warm=1):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000x500000,50000x20000")
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eval_bench needs a GPU"
    assert args.runs >= 5
    from scipy.spatial import cKDTree
    dev = torch.device("cuda", 0)
    rows = []
    for size in args.sizes.split(","):
        n, v = (int(x) for x in size.split("x"))
        pts, ids, vtx = syn.eval_scene(n, v, 200, 0)
        keep = ids > -1
        pts, ids = pts[keep], ids[keep]
        ids_t = torch.from_numpy(ids)
        out = {}

        def reference():
            _, idx = cKDTree(pts).query(vtx, k=5)
            out["ref"] = torch.mode(ids_t[idx]).values

        pts_d, vtx_d, ids_d = torch.from_numpy(pts).to(dev), torch.from_numpy(vtx).to(dev), ids_t.to(torch.int32).to(dev)

        def transfer_dev():
            out["dev"] = E.PointGrid(pts_d).query(vtx_d, ids_d)[2].cpu()

        def transfer_host():
            out["host"] = E.knn5_labels(pts, vtx, ids, want_d2=False)[2].cpu()

        grid = E.PointGrid(pts_d)
        row = dict(points=int(len(pts)), vertices=v, cells=grid.cells, cell_edge_m=round(grid.grid.h, 5),
                   points_per_occupied_cell=round(len(pts) / int((grid.counts > 0).sum()), 2))
        row["candidates_per_vertex"] = round(grid.query(vtx_d, ids_d, count_visited=True)[3] / v, 1)
        row["transfer_dev_ms"] = round(median_ms(transfer_dev, args.runs, warm=2), 3)
        row["transfer_host_ms"] = round(median_ms(transfer_host, args.runs), 3)
        row["grid_ms"] = round(median_ms(lambda: E.PointGrid(pts_d), args.runs), 3)
        row["query_ms"] = round(median_ms(lambda: grid.query(vtx_d, ids_d), args.runs), 3)
        row["reference_kdtree_mode_ms"] = round(median_ms(reference, args.runs, warm=1), 1)
        assert torch.equal(out["dev"].long(), out["ref"]) and torch.equal(out["host"].long(), out["ref"]), "device labels differ from the KD-tree's"
        row["transfer_speedup"] = round(row["reference_kdtree_mode_ms"] / row["transfer_dev_ms"], 1)

        g = np.random.default_rng(1)
        C = 51
        gt = g.integers(-1, C, v)
        pr = np.where(g.random(v) < 0.6, np.clip(gt, 0, C - 1), g.integers(0, C, v))
        ignore = [-1]
        conf_dev, conf_ref = np.zeros((C, C), dtype=np.ulonglong), np.zeros((C, C), dtype=np.ulonglong)

        def confusion_reference():                                  # the per-vertex loop of the reference's update_confmat
            conf_ref[:] = 0
            for a, b in zip(gt, pr):
                if a in ignore:
                    continue
                conf_ref[a][b] += 1

        def confusion_dev():
            conf_dev[:] = 0
            E.update_confmat(conf_dev, gt, pr, ignore)

        row["confusion_dev_ms"] = round(median_ms(confusion_dev, args.runs), 3)
        row["confusion_reference_loop_ms"] = round(median_ms(confusion_reference, args.runs, warm=0), 1)
        assert np.array_equal(conf_dev, conf_ref)
        rows.append(row)
    print(json.dumps({"bench": "eval_transfer", "runs": args.runs, "device": torch.cuda.get_device_name(0), "sizes": rows}))


if __name__ == "__main__":
    main()
