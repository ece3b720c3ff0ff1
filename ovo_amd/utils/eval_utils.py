"""Offline evaluation of a finished map against a labelled ground-truth mesh, on MI355X.

Host-side mirror of the reference's `ovo/utils/eval_utils.py` (same function names, positional arguments and return types)
over libovo_hip.so (csrc/evalknn.hip):

 * `match_labels_to_vtx` (eval_utils.py:13-41): the reference's KD-tree query + `torch.mode` becomes a uniform grid over the
   map points and one lane per mesh vertex (`ovo_knn5_labels`: exact 5 nearest in f64, mode with ties to the smallest label);
 * `update_confmat` (:108-112): the Python loop over all vertices becomes one histogram launch (`ovo_confusion`);
 * `get_iou`, `iou_acc_from_confmat`, `process_txt` and the bookkeeping of `eval_semantics` work on a C x C matrix and stay
   host numpy -- the same expressions on the same integers, so every figure and `statistics.txt` match the reference exactly.

Not built: `plot_metrics`, `plot_confmat` (matplotlib / seaborn figures; `eval_semantics(verbose=True)` says so in one line) and
`eval_scannetpp_semantic`.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import sys
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import _lib as L
from . import geometry_utils as G

K_NN = 5
MAX_DIM = 1024                  # OVO_EVAL_MAX_DIM
MAX_IGNORE = 64                 # OVO_EVAL_MAX_IGNORE
_TARGET_PER_CELL = 4.0          # points per OCCUPIED cell the cell edge aims for


def _device(*arrays) -> torch.device:
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    if not torch.cuda.is_available():
        raise L.OvoHipError("eval_utils needs a GPU; ovo_amd has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _to_dev(arr, dtype: torch.dtype, device) -> torch.Tensor:
    if isinstance(arr, torch.Tensor) or dtype in (torch.float32, torch.int32):
        return G.to_device(arr, dtype, device)
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64)).to(device, non_blocking=True)


# ---- uniform grid over the map points ----------------------------------------------------------------------------
def _grid_for(lo: np.ndarray, hi: np.ndarray, h: float, max_cells: int) -> Tuple[L.EvalGrid, int]:
    """The grid of cell edge >= h that respects the per-axis and total cell caps.  dim = floor((hi - lo) * (1 / h)) + 1 in f64, the
    expression the kernels use for a point's cell, so every point falls inside."""
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    while True:
        inv_h = 1.0 / h
        dim = [int(math.floor(e * inv_h)) + 1 for e in ext]
        if max(dim) <= MAX_DIM and dim[0] * dim[1] * dim[2] <= max_cells:
            break
        h *= 1.25
    g = L.EvalGrid()
    g.lo[:] = [float(v) for v in lo]
    g.dim[:] = dim
    g.h = h
    return g, dim[0] * dim[1] * dim[2]


class PointGrid:
    """Map points sorted into a uniform grid: `records` f32[n,4] (x, y, z, bits of the original row), `cell_start` i32[cells + 1]."""

    def __init__(self, points: torch.Tensor, h: Optional[float] = None):
        pts = L.dev(points, torch.float32, "points")
        n = pts.shape[0]
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"points must be [N, 3] (got {tuple(pts.shape)})")
        if n < K_NN:
            raise ValueError(f"{K_NN}-nearest-neighbour label transfer needs at least {K_NN} points (got {n})")
        # (a reduction over dim 0 of an [n, 3] tensor runs on three columns' worth of threads: 300 us each at 850 k points; over the rows of the transpose, 20 us)
        box = torch.stack(torch.aminmax(pts.t().contiguous(), dim=1)).cpu().numpy()
        lo, hi = box[0], box[1]
        if not np.isfinite(box).all():
            raise ValueError("points must be finite")
        # cells <= 2 n (+ a floor for tiny maps): cell_start stays at most half the size of the 16-byte records
        max_cells = max(2 * n, 4096)
        self.points, self.n = pts, n
        if h is not None:
            self._build(*_grid_for(lo, hi, float(h), 1 << 30))
            return
        # first guess: the points fill the box's volume, _TARGET_PER_CELL per cell.  Points on surfaces occupy far fewer cells than that, so
        # the occupancy is measured and the edge shrunk as for a surface (points per cell ~ h^2), at most twice
        ext = np.maximum(hi.astype(np.float64) - lo.astype(np.float64), 0.0)
        top = float(ext.max())
        ext = np.maximum(ext, 1e-3 * top) if top > 0 else np.ones(3)
        h0 = float((ext.prod() * _TARGET_PER_CELL / n) ** (1.0 / 3.0))
        for attempt in range(3):
            grid, cells = _grid_for(lo, hi, h0, max_cells)
            self._build(grid, cells)
            per_cell = n / max(int((self.counts > 0).sum().item()), 1)
            if attempt == 2 or per_cell <= 2.0 * _TARGET_PER_CELL:
                break
            h_next = grid.h * math.sqrt(_TARGET_PER_CELL / per_cell)
            if _grid_for(lo, hi, h_next, max_cells)[0].h >= grid.h * 0.95:       # the caps leave no room to shrink
                break
            h0 = h_next

    def _build(self, grid: L.EvalGrid, cells: int) -> None:
        lib, pts, n = L.load(), self.points, self.n
        keys = torch.empty(n, dtype=torch.int32, device=pts.device)
        L.check(lib.ovo_eval_cell_keys(L.ptr(pts), n, C.byref(grid), L.ptr(keys), L.stream()))
        sorted_keys, order = torch.sort(keys)
        self.counts = torch.bincount(sorted_keys, minlength=cells)
        self.cell_start = torch.zeros(cells + 1, dtype=torch.int32, device=pts.device)
        self.cell_start[1:] = torch.cumsum(self.counts, 0)
        self.records = torch.empty((n, 4), dtype=torch.float32, device=pts.device)
        L.check(lib.ovo_eval_grid_records(L.ptr(pts), L.ptr(order), n, L.ptr(self.records), L.stream()))
        self.grid, self.cells = grid, cells

    def query(self, vtx: torch.Tensor, labels: Optional[torch.Tensor] = None, want_d2: bool = False, count_visited: bool = False):
        """(nn_idx i32[V,5], nn_d2 f64[V,5] or None, label i32[V] or None, visited candidates or None) for vertices f32[V,3]."""
        lib = L.load()
        vtx = L.dev(vtx, torch.float32, "mesh_vtx")
        if vtx.dim() != 2 or vtx.shape[1] != 3:
            raise ValueError(f"mesh_vtx must be [V, 3] (got {tuple(vtx.shape)})")
        V, dev = vtx.shape[0], vtx.device
        if labels is not None:
            labels = L.dev(labels, torch.int32, "labels")
            if labels.shape != (self.n,):
                raise ValueError("one label per point")
        nn_idx = torch.empty((V, K_NN), dtype=torch.int32, device=dev)
        nn_d2 = torch.empty((V, K_NN), dtype=torch.float64, device=dev) if want_d2 else None
        label = torch.empty(V, dtype=torch.int32, device=dev) if labels is not None else None
        visited = torch.zeros(1, dtype=torch.int64, device=dev) if count_visited else None
        order = None
        if V > 64:                                                # lanes of a wave walk the same cells
            vkeys = torch.empty(V, dtype=torch.int32, device=dev)
            L.check(lib.ovo_eval_cell_keys(L.ptr(vtx), V, C.byref(self.grid), L.ptr(vkeys), L.stream()))
            order = torch.sort(vkeys)[1]
        L.check(lib.ovo_knn5_labels(L.ptr(self.records), L.ptr(self.cell_start), self.n, C.byref(self.grid), L.ptr(vtx), L.ptr(order), V,
                                    L.ptr(labels), L.ptr(nn_idx), L.ptr(nn_d2), L.ptr(label), L.ptr(visited), L.stream()))
        return nn_idx, nn_d2, label, (int(visited.item()) if count_visited else None)


def knn5_labels(points, vtx, labels=None, h: Optional[float] = None, want_d2: bool = True, count_visited: bool = False):
    """The 5 nearest `points` rows of every `vtx` row (and the mode of their labels): the device half of `match_labels_to_vtx`, for
    tests and tools.  `h` overrides the grid's cell edge."""
    dev = _device(points, vtx)
    pts = _to_dev(points, torch.float32, dev)
    lab = None if labels is None else _to_dev(labels, torch.int32, dev)
    return PointGrid(pts, h).query(_to_dev(vtx, torch.float32, dev), lab, want_d2, count_visited)


def match_labels_to_vtx(points_3d_labels, points_3d, mesh_vtx, filter_unasigned: bool = True, tree: str = "kd", verbose=False, *,
                        device_out: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Reference: eval_utils.py:13-41.  Every mesh vertex takes the most frequent label among its 5 nearest map points (both clouds in
    one frame).  Returns (mesh_labels int64 [V], mesh_instances_masks bool [n, V], matched_instances_ids int64 [n]) on the CPU like the
    reference, or on the GPU with `device_out=True`.  `tree` is accepted for compatibility: both of the reference's trees are exact, and so
    is the grid.  Coordinates are taken as f32 (what the map and the mesh loaders hold)."""
    dev = _device(points_3d_labels, points_3d, mesh_vtx)
    labels64 = _to_dev(points_3d_labels, torch.int64, dev).reshape(-1)
    pts = _to_dev(points_3d, torch.float32, dev)
    vtx = _to_dev(mesh_vtx, torch.float32, dev)
    if filter_unasigned:
        assigned = labels64 > -1
        if verbose:
            print(f"Assigned points {assigned.sum().cpu()}, {assigned.float().mean().cpu()*100:.1f}")
        labels64, pts = labels64[assigned], pts[assigned].contiguous()
        assert len(labels64), "All points are unassigned"
    if len(labels64) < K_NN:
        raise ValueError(f"{K_NN}-nearest-neighbour label transfer needs at least {K_NN} usable points (got {len(labels64)})")
    if len(labels64) and (int(labels64.max()) > 2**31 - 1 or int(labels64.min()) < -2**31):
        raise ValueError("labels must fit 32 bits")
    _, _, label, _ = PointGrid(pts).query(vtx, labels64.to(torch.int32))
    mesh_labels = label.to(torch.int64)
    # not every instance of the map reaches a mesh vertex: the masks are keyed by id, one row per id that did
    matched_instances_ids = torch.unique(mesh_labels)
    if not filter_unasigned:
        matched_instances_ids = matched_instances_ids[matched_instances_ids >= 0]
    mesh_instances_masks = mesh_labels[None, :] == matched_instances_ids[:, None]
    if device_out:
        return mesh_labels, mesh_instances_masks, matched_instances_ids
    return mesh_labels.cpu(), mesh_instances_masks.cpu(), matched_instances_ids.cpu()


def match_volume_to_vtx(volume, mesh_vtx, transform=None, min_count: int = 1, label_mode: str = "vote", max_dist: Optional[float] = None, fallback=None,
                        device_out: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`match_labels_to_vtx`'s triple from a labelled TSDF volume (`TsdfVolume(labels=True)`) instead of the sparse map: every mesh
    vertex takes the volume's instance at its own position (`volume.sample(..., labels=True, label_mode=, min_count=)`; `transform`: 4 x 4 from the
    mesh's frame into the volume's, `tsdf_utils.transform_points`).  A vertex is -1 where the sampler answers -1, where the volume has not seen
    all eight voxels around it, and, with `max_dist` (metres), where |F| * trunc > max_dist.  `fallback=(points_3d_labels, points_3d)` fills
    exactly the -1 vertices from `match_labels_to_vtx` of the map: the volume answers where it has seen something, the 5-NN transfer elsewhere.
    -1 is never a row of the masks.  No mirror in the reference: its evaluation has the 5-NN transfer only."""
    vtx = mesh_vtx
    if not (isinstance(vtx, torch.Tensor) and vtx.dtype == torch.float32 and vtx.device == volume.vol.device and vtx.is_contiguous()):
        vtx = _to_dev(mesh_vtx, torch.float32, volume.vol.device)
    F, ins = volume.sample(vtx, transform=transform, labels=True, min_count=min_count, label_mode=label_mode)
    mesh_labels = ins.to(torch.int64)
    drop = F > 1.0                                         # 2.0: not seen (the sampler answers -1 there already)
    if max_dist is not None:
        drop = drop | (F.abs() * float(volume.trunc) > float(max_dist))
    mesh_labels = torch.where(drop, torch.full_like(mesh_labels, -1), mesh_labels)
    if fallback is not None:
        missing = mesh_labels < 0
        if bool(missing.any()):
            filled = match_labels_to_vtx(fallback[0], fallback[1], vtx[missing].contiguous(), device_out=True)[0]
            mesh_labels = mesh_labels.clone()
            mesh_labels[missing] = filled.to(mesh_labels.device)
    matched_instances_ids = torch.unique(mesh_labels)
    matched_instances_ids = matched_instances_ids[matched_instances_ids >= 0]
    mesh_instances_masks = mesh_labels[None, :] == matched_instances_ids[:, None]
    if device_out:
        return mesh_labels, mesh_instances_masks, matched_instances_ids
    return mesh_labels.cpu(), mesh_instances_masks.cpu(), matched_instances_ids.cpu()


# ---- confusion matrix ---------------------------------------------------------------------------------------------
def confusion_counts(gt_ids: torch.Tensor, pr_ids: torch.Tensor, num_classes: int, ignore) -> torch.Tensor:
    """u64-valued counts (int64 tensor [C, C] on the GPU) of the (gt, pr) pairs whose gt is not in `ignore`; IndexError where numpy's
    `confusion[gt][pr]` would raise one."""
    gt, pr = L.dev(gt_ids, torch.int64, "gt_ids"), L.dev(pr_ids, torch.int64, "pr_ids")
    n = min(gt.numel(), pr.numel())                                # zip() stops at the shorter one
    ig = [int(v) for v in ignore]
    if len(ig) > MAX_IGNORE:
        raise ValueError(f"at most {MAX_IGNORE} ignored ids")
    out = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=gt.device)
    bad = torch.zeros(1, dtype=torch.int32, device=gt.device)
    ig_arr = (C.c_int64 * max(len(ig), 1))(*ig)
    L.check(L.load().ovo_confusion(L.ptr(gt), L.ptr(pr), n, num_classes, ig_arr, len(ig), L.ptr(out), L.ptr(bad), L.stream()))
    if int(bad.item()):
        raise IndexError(f"label id out of bounds for a confusion matrix with {num_classes} classes")
    return out


def update_confmat(confusion: np.ndarray, gt_ids, pr_ids, ignore) -> None:
    """Reference: eval_utils.py:108-112.  `confusion[gt][pr] += 1` for every vertex whose gt id is not ignored, in place on the caller's
    numpy matrix; an id that numpy would refuse raises IndexError before anything is added."""
    dev = _device(gt_ids, pr_ids)
    counts = confusion_counts(_to_dev(gt_ids, torch.int64, dev).reshape(-1), _to_dev(pr_ids, torch.int64, dev).reshape(-1), confusion.shape[0], ignore)
    confusion += counts.cpu().numpy().astype(confusion.dtype)


def process_txt(filename) -> List[str]:
    """Reference: eval_utils.py:82-86: the lines of a text file without trailing white space."""
    with open(filename) as f:
        return [line.rstrip() for line in f.readlines()]


def evaluate_scan(pr_file, gt_file, confusion: np.ndarray, map_gt_ids: Optional[Dict[int, int]] = None, ignore: List = []) -> None:
    """Reference: eval_utils.py:88-106.  One scene's label files into its confusion matrix; gt ids absent from `map_gt_ids` map to -1
    (and are remembered in the dictionary, as the reference does)."""
    pr_ids = np.array(process_txt(pr_file), dtype=np.int64)
    gt_ids = np.array(process_txt(gt_file)).astype(np.int64)
    if map_gt_ids is not None:
        assert isinstance(map_gt_ids, dict), "map_gt_ids must be either None or a dictionary which keys map gt label idxs to new idxs"
        for i in np.unique(gt_ids):
            if i not in map_gt_ids.keys():
                map_gt_ids[i] = -1
        gt_ids = np.vectorize(map_gt_ids.get)(gt_ids)
    if not pr_ids.shape == gt_ids.shape:
        print(f'number of predicted values does not match number of vertices. pred: {pr_ids.shape}; gt: {gt_ids.shape};{pr_file}')
    update_confmat(confusion, gt_ids, pr_ids, ignore)


def get_iou(label_id: int, confusion: np.ndarray) -> Tuple[float, float]:
    """Reference: eval_utils.py:114-124.  (IoU, accuracy) of one class; (nan, nan) for a class that never occurs."""
    tp = np.longlong(confusion[label_id, label_id])
    fn = np.longlong(confusion[label_id, :].sum()) - tp
    fp = np.longlong(confusion[:, label_id].sum()) - tp
    denom = float(tp + fp + fn)
    if denom == 0:
        return (float('nan'), float('nan'))
    return (tp / denom, tp / max(float(tp + fn), 1e-6))


def iou_acc_from_confmat(confmat: np.ndarray, num_classes: int, ignore: List[int], mask_nan: bool = True, verbose: bool = False, labels: List[str] = None):
    """Reference: eval_utils.py:127-156.  Per kept class: IoU, accuracy and weight (row sum = tp + fn), and the masks of the valid entries."""
    if verbose:
        print('\n classes \t IoU \t Acc')
        print('----------------------------')
    ious, accs, weights = [], [], []
    for i in range(num_classes):
        if i in ignore:
            continue
        iou, acc = get_iou(i, confmat)
        ious.append(iou)
        accs.append(acc)
        weights.append(confmat[i].sum())
        if verbose:
            print('{0:<14s}: {1:>5.2%}   {2:>6.2%}'.format(labels[i], iou, acc))
    iou_values, acc_values, weights_values = np.array(ious), np.array(accs), np.array(weights)
    if mask_nan:
        return iou_values, ~np.isnan(iou_values), weights_values, acc_values, ~np.isnan(acc_values)
    return iou_values, np.ones_like(iou_values, dtype=bool), weights_values, acc_values, np.ones_like(acc_values, dtype=bool)


def _means(iou, iou_ok, w, acc, acc_ok):
    """mIoU, mAcc, frequency-weighted mIoU and mAcc (the four figures eval_semantics prints and returns)."""
    return (np.mean(iou[iou_ok]), np.mean(acc[acc_ok]), np.sum(iou[iou_ok] * w[iou_ok]) / w[iou_ok].sum(), np.sum(acc[acc_ok] * w[acc_ok]) / w[acc_ok].sum())


def eval_semantics(output_path, gt_path, scenes: List[str], dataset_info: Dict[str, Any], mask_nan: bool = True, ignore_background: bool = False,
                   verbose: bool = True, return_metrics=False):
    """Reference: eval_utils.py:158-245.  `<output_path>/<scene>.txt` against `<gt_path>/<scene>.txt` for every scene: per-scene and overall
    mIoU / mAcc / f-mIoU / f-mAcc, head / comm / tail thirds, `statistics.txt` (verbose only).  Returns (metrics dict, confusion) with
    `return_metrics`, else (mIoU, confusion); confusion is the sum over the scenes."""
    num_classes = dataset_info["num_classes"]
    map_to_reduced = dataset_info.get("map_to_reduced", None)
    labels = dataset_info["class_names"] if map_to_reduced is None else dataset_info["class_names_reduced"]
    ignore = dataset_info.get("ignore", []).copy()
    if ignore_background:
        key = "background_reduced_ids" if map_to_reduced else "background_ids"
        background = dataset_info.get(key, None) if map_to_reduced else dataset_info[key]
        assert background, "To ignore background a list of idxs corresponding to background ids id required!"
        ignore.extend(background)

    pr_files = [Path(output_path) / f'{scene}.txt' for scene in scenes]
    gt_files = [Path(gt_path) / f'{scene}.txt' for scene in scenes]
    confusion = np.zeros([len(scenes), num_classes, num_classes], dtype=np.ulonglong)
    if verbose:
        print('evaluating', len(pr_files), 'scans...')
    for i in range(len(pr_files)):
        evaluate_scan(pr_files[i], gt_files[i], confusion[i], map_to_reduced, ignore)
        if verbose:
            sys.stdout.write("\rscans processed: {}".format(i + 1))
            sys.stdout.flush()

    for i in range(len(scenes)):
        per_scene = iou_acc_from_confmat(confusion[i], num_classes, ignore, mask_nan, False, labels)
        if verbose:
            miou, macc, fiou, facc = _means(*per_scene)
            print(f"Scene: {scenes[i]}")
            print(f'mIoU: \t {miou:.2%}; mAcc: \t {macc:.2%}\n ')
            print(f'f-mIoU: \t {fiou:.2%}; f-mAcc: \t {facc:.2%}\n')
    confusion = confusion.sum(0)
    iou_values, iou_valid_mask, weights_values, acc_values, acc_valid_mask = iou_acc_from_confmat(confusion, num_classes, ignore, mask_nan, verbose, labels)
    miou, macc, fiou, facc = _means(iou_values, iou_valid_mask, weights_values, acc_values, acc_valid_mask)
    metrics = {"iou": round(miou, 3), "acc": round(macc, 3), "fiou": round(fiou, 3), "facc": round(facc, 3)}
    thirds = len(iou_values) // 3
    for k, split in enumerate(("head", "comm", "tail")):
        part = slice(thirds * k, thirds * (k + 1))
        metrics[f"iou_{split}"] = round(np.mean(iou_values[part][iou_valid_mask[part]]), 3)
        metrics[f"acc_{split}"] = round(np.mean(acc_values[part][acc_valid_mask[part]]), 3)

    if verbose:
        print(f"\nmIoU: \t {metrics['iou']:.2%}; mAcc: \t {metrics['acc']:.2%}\n ")
        print(f"f-mIoU: \t {metrics['fiou']:.2%}; f-mAcc: \t {metrics['facc']:.2%}\n")
        print()
        if iou_values.shape[0] == 51:
            for split in ("head", "comm", "tail"):
                print(f'{split}: \t {metrics[f"iou_{split}"]:.2%}')
                print(f'{split}: \t {metrics[f"acc_{split}"]:.2%}')
                print('---')
        output_path = Path(output_path)
        with open(output_path / "statistics.txt", "w") as f:
            f.write("label, acc, iou, \n")
            kept = [i for i in range(len(labels)) if i not in ignore]
            for count, i in enumerate(kept):
                f.write(f"{labels[i]}, {acc_values[count]}, {iou_values[count]}, \n")
        print("plot_iou_acc.png / confmat.png: not drawn (plot_metrics and plot_confmat are not part of ovo_amd)")
    if return_metrics:
        return metrics, confusion
    return miou, confusion
