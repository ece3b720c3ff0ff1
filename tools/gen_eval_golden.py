"""Fixtures of the evaluation step: tests/golden/eval_*.npz = seeded synthetic inputs + what the REFERENCE's ovo/utils/eval_utils.py returns for them.

    python tools/gen_eval_golden.py --reference /path/to/OVO [--out tests/golden]

Runs on the CPU.  The reference module imports seaborn (not needed for anything stored here): it is stubbed in sys.modules, and the two plot
functions are replaced by no-ops in this process.  Data only: nothing of the reference's text is copied.

Every scene written is checked for exact ties: no mesh vertex may have its 5th and 6th nearest map point at equal f64 squared distance (the
reference leaves that case to the KD-tree's traversal order); the smallest gap is stored next to the scene.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from gen_golden import save_parts          # noqa: E402
from ovo_amd import synthetic as syn       # noqa: E402

# the shipped evaluation configs in miniature: (name, classes, ignore): ScanNet20 ignores the unmapped -1, Replica ignores id 51 of 51 classes,
# and a set where -1 is NOT ignored, so it wraps into the last row
CONFUSION_CASES = (("c21_ignore_m1", 21, [-1]), ("c51_ignore_51", 51, [51]), ("c21_wrap_m1", 21, []), ("c200_ignore_two", 200, [0, 7]))


def d2_f64(a, b):
    dx, dy, dz = (a[..., k].astype(np.float64) - b[..., k].astype(np.float64) for k in range(3))
    return dx * dx + dy * dy + dz * dz


def gap56(points, vtx):
    """Smallest difference between the 6th and 5th squared distance over all vertices (f64 on the f64 conversion of the inputs)."""
    from scipy.spatial import cKDTree
    _, idx = cKDTree(points.astype(np.float64)).query(vtx.astype(np.float64), k=6)
    d2 = np.sort(d2_f64(vtx[:, None, :], points[idx]), axis=1)
    return float((d2[:, 5] - d2[:, 4]).min())


def gen_match(out, E):
    for name, n, v, ins, seed in (("room_a", 24000, 9000, 60, 11), ("room_b", 6000, 2501, 25, 12)):
        pts, ids, vtx = syn.eval_scene(n, v, ins, seed)
        arrays = dict(points=pts, ids=ids, vtx=vtx)
        for tag, filt in (("filter", True), ("nofilter", False)):
            used = pts[ids > -1] if filt else pts
            gap = gap56(used, vtx)
            assert gap > 0.0, f"{name}/{tag}: a vertex has its 5th and 6th neighbour at equal distance"
            labels, masks, matched = E.match_labels_to_vtx(torch.from_numpy(ids), torch.from_numpy(pts), torch.from_numpy(vtx), filt)
            arrays.update({f"{tag}_labels": labels.numpy(), f"{tag}_masks": np.packbits(masks.numpy(), axis=-1), f"{tag}_ids": matched.numpy(),
                           f"{tag}_gap56": np.float64(gap)})
            print(f"  {name}/{tag}: {len(used)} points, {v} vertices, {len(matched)} ids, smallest 5th/6th gap {gap:.3e} m^2")
        for p in save_parts(os.path.join(out, f"eval_match_{name}.npz"), arrays):
            print(f"  wrote {p} ({os.path.getsize(p)/1024:.1f} KiB)")


def gen_confusion(out, E):
    g = np.random.default_rng(5)
    arrays = {}
    for name, C, ignore in CONFUSION_CASES:
        n = 20000
        gt = g.integers(-1, C, n)
        if C in ignore:                                              # Replica: the id one past the last class marks "no class"
            gt[g.random(n) < 0.1] = C
        pr = np.where(g.random(n) < 0.6, np.clip(gt, 0, C - 1), g.integers(0, C, n))
        conf = np.zeros((C, C), dtype=np.ulonglong)
        E.update_confmat(conf, gt, pr, ignore)
        arrays.update({f"{name}_gt": gt.astype(np.int64), f"{name}_pr": pr.astype(np.int64), f"{name}_ignore": np.array(ignore, dtype=np.int64),
                       f"{name}_confusion": conf})
    for p in save_parts(os.path.join(out, "eval_confusion.npz"), arrays):
        print(f"  wrote {p} ({os.path.getsize(p)/1024:.1f} KiB)")


def gen_host(out, E):
    """get_iou / iou_acc_from_confmat on matrices with empty classes (NaN entries), and process_txt on a file with trailing blanks."""
    g = np.random.default_rng(9)
    arrays = {}
    for name, C, ignore in (("m21", 21, [0, 20]), ("m51", 51, []), ("m7", 7, [3])):
        conf = g.integers(0, 400, (C, C)).astype(np.ulonglong)
        conf[np.arange(C), np.arange(C)] += g.integers(0, 5000, C).astype(np.ulonglong)
        empty = g.choice(C, 3, replace=False)
        conf[empty, :] = 0
        conf[:, empty[:2]] = 0                                      # two classes never occur at all (NaN), one is only predicted
        arrays[f"{name}_confusion"], arrays[f"{name}_ignore"] = conf, np.array(ignore, dtype=np.int64)
        arrays[f"{name}_get_iou"] = np.array([E.get_iou(i, conf) for i in range(C)], dtype=np.float64)
        for tag, mask_nan in (("masknan", True), ("keepnan", False)):
            iou, iou_ok, w, acc, acc_ok = E.iou_acc_from_confmat(conf, C, ignore, mask_nan)
            arrays.update({f"{name}_{tag}_iou": iou, f"{name}_{tag}_iou_ok": iou_ok, f"{name}_{tag}_w": w, f"{name}_{tag}_acc": acc, f"{name}_{tag}_acc_ok": acc_ok})
    text = "3\n 14 \n-1\t\n\n27   \n5"
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "labels.txt")
        with open(path, "w") as f:
            f.write(text)
        lines = E.process_txt(path)
    arrays["txt_bytes"] = np.frombuffer(text.encode(), dtype=np.uint8)
    arrays["txt_lines"] = np.array(lines)
    for p in save_parts(os.path.join(out, "eval_host.npz"), arrays):
        print(f"  wrote {p} ({os.path.getsize(p)/1024:.1f} KiB)")


def e2e_case(name):
    """Label files of two scenes and the dataset description, from seeds (tests rebuild the same files through io_utils.write_labels)."""
    g = np.random.default_rng({"scannet": 21, "replica": 22}[name])
    if name == "scannet":                                            # raw gt ids go through map_to_reduced; unmapped ones become -1, which is ignored
        valid = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
        info = dict(num_classes=21, ignore=[-1], map_to_reduced={v: i for i, v in enumerate(valid)}, background_reduced_ids=[0, 1, 20],
                    class_names=[str(i) for i in range(41)], class_names_reduced=[f"class{i:02d}" for i in range(21)])
        raw = np.array(valid + [13, 40])
        C = 21
    else:                                                            # 51 classes, no mapping, id 51 = "no class" is ignored
        info = dict(num_classes=51, ignore=[51], class_names=[f"name{i:02d}" for i in range(51)], background_ids=[0, 1, 2])
        raw = np.arange(0, 52)
        C = 51
    scenes = {}
    for scene, n in (("scene_a", 7000), ("scene_b", 4100)):
        gt = raw[g.integers(0, len(raw) - 6, n)] if name == "replica" else raw[g.integers(0, len(raw), n)]     # replica: the last classes stay empty (NaN)
        if name == "replica":
            gt[g.random(n) < 0.05] = 51
            pr = np.where(g.random(n) < 0.55, np.clip(gt, 0, C - 1), g.integers(0, C, n))
        else:
            to_reduced = np.vectorize(lambda v: info["map_to_reduced"].get(v, 0))(gt)
            pr = np.where(g.random(n) < 0.55, to_reduced, g.integers(0, C - 1, n))
        scenes[scene] = (gt.astype(np.int64), pr.astype(np.int64))
    return info, scenes


def gen_e2e(out, E, IO):
    import copy
    arrays = {}
    for name in ("scannet", "replica"):
        info, scenes = e2e_case(name)
        # the dataset description as JSON text (keys of map_to_reduced become strings: the test turns them back into ints)
        arrays[f"{name}_info_json"] = np.frombuffer(json.dumps(info).encode(), dtype=np.uint8)
        arrays[f"{name}_scenes"] = np.array(list(scenes))
        for bg in (False, True):
            tag = f"{name}_{'bg' if bg else 'all'}"
            with tempfile.TemporaryDirectory() as tmp:
                pred, gt = os.path.join(tmp, "pred"), os.path.join(tmp, "gt")
                os.makedirs(pred), os.makedirs(gt)
                for scene, (g_ids, p_ids) in scenes.items():
                    IO.write_labels(os.path.join(gt, scene + ".txt"), g_ids)
                    IO.write_labels(os.path.join(pred, scene + ".txt"), p_ids)
                    arrays[f"{name}_{scene}_gt"], arrays[f"{name}_{scene}_pr"] = g_ids, p_ids
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    metrics, conf = E.eval_semantics(pred, gt, list(scenes), copy.deepcopy(info), True, bg, True, True)
                with open(os.path.join(pred, "statistics.txt"), "rb") as f:
                    arrays[f"{tag}_statistics"] = np.frombuffer(f.read(), dtype=np.uint8)
            arrays[f"{tag}_stdout"] = np.frombuffer(buf.getvalue().encode(), dtype=np.uint8)
            arrays[f"{tag}_metric_names"] = np.array(list(metrics))
            arrays[f"{tag}_metric_values"] = np.array([float(v) for v in metrics.values()], dtype=np.float64)
            arrays[f"{tag}_confusion"] = conf
            print(f"  {tag}: {dict(metrics)}")
    for p in save_parts(os.path.join(out, "eval_e2e.npz"), arrays):
        print(f"  wrote {p} ({os.path.getsize(p)/1024:.1f} KiB)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference (tberriel/OVO)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, args.reference)
    torch.set_num_threads(1)
    from ovo.utils import eval_utils as E
    E.plot_metrics = lambda *a, **k: None
    E.plot_confmat = lambda *a, **k: None
    from ovo_amd.utils import io_utils as IO
    print("torch", torch.__version__, "numpy", np.__version__)
    gen_match(args.out, E)
    gen_confusion(args.out, E)
    gen_host(args.out, E)
    gen_e2e(args.out, E, IO)


if __name__ == "__main__":
    main()
