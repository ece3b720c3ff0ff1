"""Where every instance is: per-instance point count, centroid, axis-aligned extent and covariance of the map in one pass over libovo_hip.so
(csrc/insgeo.hip; include/ovo_hip.h: ovo_instance_geometry has the contract), PCA-aligned boxes from a second pass, and the box corners that
`render_utils.render_boxes` draws -- the boxes of the reference's viewer (ovo/utils/vis_utils.py:72-87).  No CPU path for the passes; the
3 x 3 eigenproblems of the oriented boxes are the host's (`pca_axes`, numpy)."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib as L


def geometry_pass(points_3d: torch.Tensor, points_ins_ids: torch.Tensor, n_slots: int, axes: Optional[torch.Tensor] = None, *, count: bool = True,
                  box: bool = True, moments: bool = True) -> Dict[str, torch.Tensor]:
    """One `ovo_instance_geometry` launch on the current stream: {"count" i32[n_slots], "min" / "max" f32[n_slots,3], "sums" f64[n_slots,3],
    "prods" f64[n_slots,6]}, whichever of the three groups is asked for.  `axes` f32[n_slots,3,3]: min / max along each slot's own three rows."""
    pts = L.dev(points_3d, torch.float32, "points_3d")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise L.OvoHipError(f"points_3d must be [n, 3] (got {tuple(pts.shape)})")
    ins = L.dev(points_ins_ids.reshape(-1), torch.int32, "points_ins_ids")
    if ins.shape[0] != pts.shape[0] or ins.device != pts.device:
        raise L.OvoHipError(f"points_ins_ids: {ins.shape[0]} ids on {ins.device} for {pts.shape[0]} points on {pts.device}")
    n_slots, dev = int(n_slots), pts.device
    if axes is not None:
        axes = L.dev(axes, torch.float32, "axes")
        if tuple(axes.shape) != (n_slots, 3, 3) or axes.device != dev:
            raise L.OvoHipError(f"axes must be [{n_slots}, 3, 3] on {dev} (got {tuple(axes.shape)} on {axes.device})")
    out = {}
    if count:
        out["count"] = torch.empty(max(n_slots, 0), dtype=torch.int32, device=dev)
    if box:
        out["min"], out["max"] = (torch.empty((max(n_slots, 0), 3), dtype=torch.float32, device=dev) for _ in range(2))
    if moments:
        out["sums"] = torch.empty((max(n_slots, 0), 3), dtype=torch.float64, device=dev)
        out["prods"] = torch.empty((max(n_slots, 0), 6), dtype=torch.float64, device=dev)
    L.check(L.load().ovo_instance_geometry(L.ptr(pts), L.ptr(ins), pts.shape[0], n_slots, L.ptr(axes), L.ptr(out.get("count")), L.ptr(out.get("min")),
                                           L.ptr(out.get("max")), L.ptr(out.get("sums")), L.ptr(out.get("prods")), L.stream()))
    return out


def covariance(count, sums, prods):
    """cov f64[n_slots,3,3] = E[p p^T] - E[p] E[p]^T from the pass's moments (numpy or torch, f64); NaN for an empty slot."""
    n = count.to(torch.float64) if isinstance(count, torch.Tensor) else np.asarray(count, np.float64)
    mean = sums / n[:, None]
    second = prods[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3) / n[:, None, None]
    return second - mean[:, :, None] * mean[:, None, :]


def pca_axes(cov: np.ndarray, count: np.ndarray) -> np.ndarray:
    """R f32[n_slots,3,3], the rows of R[s] the principal axes of slot s (`numpy.linalg.eigh` of the f64 covariance): eigenvalues descending, each
    axis with its largest-magnitude component positive, the third flipped if needed so that det R = +1.  The identity where count < 3 or the
    covariance is not finite."""
    cov, count = np.asarray(cov, np.float64), np.asarray(count)
    R = np.tile(np.eye(3), (cov.shape[0], 1, 1))
    for s in range(cov.shape[0]):
        if count[s] < 3 or not np.isfinite(cov[s]).all():
            continue
        w, v = np.linalg.eigh(cov[s])
        ax = v[:, np.argsort(-w, kind="stable")].T                   # rows: axes by descending eigenvalue
        for k in range(3):
            if ax[k, np.argmax(np.abs(ax[k]))] < 0:
                ax[k] = -ax[k]
        if np.linalg.det(ax) < 0:
            ax[2] = -ax[2]
        R[s] = ax
    return R.astype(np.float32)


def instance_geometry(points_3d: torch.Tensor, points_ins_ids: torch.Tensor, n_slots: int, oriented: bool = False) -> Dict[str, torch.Tensor]:
    """Per instance slot in [0, n_slots), on the map's device: "count" i32, "centroid" f32[.,3] (sums / count), "min" / "max" f32[.,3] (+inf / -inf
    for an empty slot), "cov" f64[.,3,3] (NaN for an empty slot).  Rows with an id outside the slots or a non-finite coordinate count nowhere.
    `oriented`: also "R" f32[.,3,3] (`pca_axes`) and "min_o" / "max_o" f32[.,3], the extent along R's rows -- one pass for the moments, the
    eigenproblems on the host, a second pass with `axes=R`."""
    g = geometry_pass(points_3d, points_ins_ids, n_slots)
    cov = covariance(g["count"], g["sums"], g["prods"])
    out = {"count": g["count"], "centroid": (g["sums"] / g["count"].to(torch.float64)[:, None]).float(), "min": g["min"], "max": g["max"], "cov": cov}
    if oriented:
        R = torch.from_numpy(pca_axes(cov.cpu().numpy(), g["count"].cpu().numpy())).to(cov.device)
        o = geometry_pass(points_3d, points_ins_ids, n_slots, axes=R, count=False, moments=False)
        out.update(R=R, min_o=o["min"], max_o=o["max"])
    return out


def box_corners(lo, hi, R=None) -> torch.Tensor:
    """f32[m,8,3]: corner c takes hi on axis k iff bit k of c is set (the order `ovo_render_boxes` reads).  `R` f32[m,3,3]: lo / hi are extents
    along R's rows and the corners go back to the world, p = R^T c."""
    lo, hi = torch.as_tensor(lo, dtype=torch.float32), torch.as_tensor(hi, dtype=torch.float32)
    bits = torch.tensor([[(c >> k) & 1 for k in range(3)] for c in range(8)], dtype=torch.bool, device=lo.device)
    corners = torch.where(bits[None], hi[:, None, :], lo[:, None, :])
    if R is not None:
        corners = (corners[:, :, :, None] * torch.as_tensor(R, dtype=torch.float32).to(lo.device)[:, None, :, :]).sum(2)
    return corners.contiguous()
