"""-m gpu: the evaluation step (utils/eval_utils.py over csrc/evalknn.hip): 5-NN label transfer, confusion matrix, mIoU.

 1. reference golden (tests/golden/eval_match_*.npz, written by the reference's own match_labels_to_vtx): labels, masks, ids equal;
 2. against scipy's KD-tree on seeded scenes from 1 k points to 1 M x 500 k: neighbour lists equal as ordered lists, squared distances `==`
    numpy's f64 value of the same expression, labels equal to CPU torch.mode.  Every scene first asserts on the host that no vertex has
    two of its first six neighbours at equal distance, so no vertex is left out of the comparison;
 3. mode ties go to the smallest label;  4. confusion matrix (golden, np.add.at, IndexError);  5. eval_semantics end to end;  6. determinism.
"""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden, unpack

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _d2(vtx, pts):
    dx, dy, dz = (vtx[..., k].astype(np.float64) - pts[..., k].astype(np.float64) for k in range(3))
    return dx * dx + dy * dy + dz * dz


# ---- 1. reference golden -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", (True, False))
@pytest.mark.parametrize("scene", ("room_a", "room_b"))
def test_match_labels_to_vtx_matches_reference(scene, filt):
    from ovo_amd.utils import eval_utils as E
    d = golden(f"eval_match_{scene}")
    tag = "filter" if filt else "nofilter"
    assert float(d[f"{tag}_gap56"]) > 0.0
    labels, masks, ids = E.match_labels_to_vtx(torch.from_numpy(d["ids"]), torch.from_numpy(d["points"]), torch.from_numpy(d["vtx"]), filt)
    V = d["vtx"].shape[0]
    assert not labels.is_cuda and labels.dtype == torch.int64 and masks.dtype == torch.bool and ids.dtype == torch.int64
    assert torch.equal(labels, torch.from_numpy(d[f"{tag}_labels"]))
    assert torch.equal(ids, torch.from_numpy(d[f"{tag}_ids"]))
    assert torch.equal(masks, torch.from_numpy(unpack(d[f"{tag}_masks"], V)))
    if not filt:
        assert (d[f"{tag}_labels"] < 0).any() and (d[f"{tag}_ids"] >= 0).all()      # the negative-id tail is exercised


def test_match_labels_accepts_numpy_and_device_tensors():
    from ovo_amd.utils import eval_utils as E
    d = golden("eval_match_room_b")
    want = torch.from_numpy(d["filter_labels"])
    a = E.match_labels_to_vtx(d["ids"][:, None], d["points"], d["vtx"], True, "ball")                 # numpy, [n, 1] labels, the other tree name
    b = E.match_labels_to_vtx(torch.from_numpy(d["ids"]).to(DEV), torch.from_numpy(d["points"]).to(DEV), torch.from_numpy(d["vtx"]).to(DEV), device_out=True)
    assert torch.equal(a[0], want) and all(t.is_cuda for t in b) and torch.equal(b[0].cpu(), want)
    assert torch.equal(b[1].cpu(), a[1]) and torch.equal(b[2].cpu(), a[2])


def test_fewer_than_five_usable_points_is_a_value_error():
    from ovo_amd.utils import eval_utils as E
    pts = np.random.default_rng(0).random((9, 3)).astype(np.float32)
    ids = np.array([0, 1, -1, -1, 2, -1, 3, -1, -1])
    with pytest.raises(ValueError):
        E.match_labels_to_vtx(ids, pts, pts[:3])
    assert E.match_labels_to_vtx(ids, pts, pts[:3], False)[0].shape == (3,)


# ---- 2. against scipy ------------------------------------------------------------------------------------------------
def _room(n, v, ins, seed):
    from ovo_amd import synthetic as syn
    pts, ids, vtx = syn.eval_scene(n, v, ins, seed)
    keep = ids > -1
    return pts[keep], ids[keep], vtx, None


def _one_cell(seed=3):
    g = np.random.default_rng(seed)
    return g.random((3000, 3)).astype(np.float32), g.integers(0, 9, 3000), (g.random((333, 3)) * 1.2 - 0.1).astype(np.float32), 100.0     # h = 100 m: grid 1 x 1 x 1


def _far_outside(seed=4):
    pts, ids, vtx, _ = _room(5000, 640, 30, seed)
    g = np.random.default_rng(seed)
    shift = np.array([[50, 0, 0], [-30, -40, 0], [0, 0, 75], [6.5, 4.5, 3.0], [-200, 300, -100]], dtype=np.float32)
    return pts, ids, (vtx + shift[g.integers(0, len(shift), len(vtx))]).astype(np.float32), None


def _five_points(seed=5):
    g = np.random.default_rng(seed)
    return g.random((5, 3)).astype(np.float32), np.array([4, 4, 1, 1, 6]), (g.random((101, 3)) * 3 - 1).astype(np.float32), None


def _two_clusters(seed=6):
    g = np.random.default_rng(seed)
    a, b = g.normal(0, 0.3, (2000, 3)), g.normal(0, 0.3, (1500, 3)) + np.array([80.0, 5.0, -3.0])
    pts = np.concatenate([a, b]).astype(np.float32)
    t = g.random((777, 1))
    vtx = (t * np.array([[80.0, 5.0, -3.0]]) + g.normal(0, 0.5, (777, 3))).astype(np.float32)          # along the empty stretch between them
    return pts, g.integers(0, 40, len(pts)), vtx, None


SCENES = {
    "room_1k": lambda: _room(1000, 701, 20, 1),
    "room_50k": lambda: _room(50000, 20000, 200, 2),
    "one_cell": _one_cell,
    "far_outside": _far_outside,
    "five_points": _five_points,
    "two_clusters": _two_clusters,
    "room_1m": lambda: _room(1000000, 500000, 200, 7),
}
_largest = {}


def _scipy_reference(pts, ids, vtx):
    """(idx [V,5], d2 [V,5], labels [V]) from the KD-tree on the f64 conversion, after asserting that the answer is unique for every vertex."""
    from scipy.spatial import cKDTree
    k = min(6, len(pts))
    _, idx = cKDTree(pts.astype(np.float64)).query(vtx.astype(np.float64), k=k)
    d2 = _d2(vtx[:, None, :], pts[idx])
    gaps = np.diff(d2, axis=1)
    assert (gaps > 0).all(), f"{int((gaps <= 0).any(1).sum())} vertices have neighbours at equal distance: the scene does not pin the answer"
    idx, d2 = idx[:, :5], d2[:, :5]
    return idx, d2, torch.mode(torch.from_numpy(ids.astype(np.int64))[torch.from_numpy(idx)]).values.numpy()


@pytest.mark.parametrize("name", list(SCENES))
def test_knn5_matches_kdtree(name):
    from ovo_amd.utils import eval_utils as E
    pts, ids, vtx, h = SCENES[name]()
    want_idx, want_d2, want_label = _scipy_reference(pts, ids, vtx)
    nn_idx, nn_d2, label, visited = E.knn5_labels(pts, vtx, ids, h=h, want_d2=True, count_visited=True)
    nn_idx, nn_d2, label = nn_idx.cpu().numpy(), nn_d2.cpu().numpy(), label.cpu().numpy()
    print(f"{name}: {len(pts)} points, {len(vtx)} vertices, {visited / len(vtx):.1f} candidates per vertex")
    wrong = (nn_idx != want_idx).any(1)
    assert not wrong.any(), f"{int(wrong.sum())} of {len(vtx)} vertices have another neighbour list"
    assert np.array_equal(nn_d2, want_d2)
    assert np.array_equal(label, want_label)
    if name == "one_cell":
        assert visited == len(pts) * len(vtx)                      # one cell: every vertex looks at every point, once
    if name == "room_1m":
        _largest.update(pts=pts, ids=ids, vtx=vtx, out=(nn_idx, nn_d2, label))


def test_knn5_is_deterministic():
    """6. the largest scene twice: bit-equal neighbour lists, distances and labels (the sort that builds the grid may order a cell's
    points differently from run to run; the result must not depend on it)."""
    from ovo_amd.utils import eval_utils as E
    if not _largest:
        pts, ids, vtx, _ = SCENES["room_1m"]()
        first = E.knn5_labels(pts, vtx, ids)
        _largest.update(pts=pts, ids=ids, vtx=vtx, out=tuple(t.cpu().numpy() for t in first[:3]))
    again = E.knn5_labels(_largest["pts"], _largest["vtx"], _largest["ids"])
    for a, b in zip(_largest["out"], again[:3]):
        assert np.array_equal(a, b.cpu().numpy())


# ---- 3. mode ties ----------------------------------------------------------------------------------------------------
MODE_ROWS = (([5, 5, 2, 2, 9], 2), ([7, 8, 9, 10, 11], 7), ([2, 2, 5, 5, 9], 2), ([9, 3, 3, 9, 1], 3), ([4, 4, 4, 1, 1], 4), ([1, 6, 6, 6, 1], 6),
             ([11, 10, 9, 8, 7], 7), ([3, 3, 3, 3, 3], 3), ([0, 2, 2, 0, 1], 0), ([-1, -1, 3, 3, 7], -1), ([-5, 4, -2, 4, -2], -2), ([-1, -2, -3, -4, -5], -5))


@pytest.mark.parametrize("row,want", MODE_ROWS)
def test_mode_ties_go_to_the_smallest_label(row, want):
    from ovo_amd.utils import eval_utils as E
    assert int(torch.mode(torch.tensor(row)).values) == want       # what the reference's CPU torch.mode does
    pts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0]], dtype=np.float32)       # neighbours of x = -1 come in this order
    vtx = np.array([[-1, 0, 0], [-2, 0.5, 0], [-1.5, 0, 1]], dtype=np.float32)
    nn_idx, _, label, _ = E.knn5_labels(pts, vtx, np.array(row))
    assert np.array_equal(nn_idx.cpu().numpy(), np.tile(np.arange(5), (3, 1)))
    assert label.cpu().tolist() == [want] * 3
    labels, masks, ids = E.match_labels_to_vtx(np.array(row), pts, vtx, False)
    assert labels.tolist() == [want] * 3
    assert ids.tolist() == ([want] if want >= 0 else []) and masks.shape == (len(ids), 3) and bool(masks.all())


# ---- 4. confusion ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("c21_ignore_m1", "c51_ignore_51", "c21_wrap_m1", "c200_ignore_two"))
def test_update_confmat_matches_reference(name):
    from ovo_amd.utils import eval_utils as E
    d = golden("eval_confusion")
    want, ignore = d[f"{name}_confusion"], [int(v) for v in d[f"{name}_ignore"]]
    if name == "c21_wrap_m1":
        assert want[-1].sum() > 0 and (d[f"{name}_gt"] == -1).any()           # the unmapped -1 lands in the last row
    conf = np.zeros_like(want)
    assert conf.dtype == np.ulonglong
    E.update_confmat(conf, d[f"{name}_gt"], d[f"{name}_pr"], ignore)
    assert np.array_equal(conf, want)
    E.update_confmat(conf, list(d[f"{name}_gt"][:100]), list(d[f"{name}_pr"][:100]), ignore)        # in place, on top of what is there; lists as in the reference's signature
    again = np.zeros_like(want)
    E.update_confmat(again, d[f"{name}_gt"][:100], d[f"{name}_pr"][:100], ignore)
    assert np.array_equal(conf, want + again)


@pytest.mark.parametrize("C", (21, 51, 200))
def test_confusion_two_million_pairs(C):
    from ovo_amd.utils import eval_utils as E
    g = np.random.default_rng(C)
    n = 2_000_000
    gt, pr = g.integers(-1, C, n), g.integers(0, C, n)
    pr[g.random(n) < 0.5] = 3                                        # a hot column: many adds to few bins
    ignore = [-1, 2]
    keep = ~np.isin(gt, ignore)
    want = np.zeros((C, C), dtype=np.ulonglong)
    np.add.at(want, (gt[keep], pr[keep]), 1)
    conf = np.zeros((C, C), dtype=np.ulonglong)
    E.update_confmat(conf, gt, pr, ignore)
    assert np.array_equal(conf, want) and int(conf.sum()) == int(keep.sum())


@pytest.mark.parametrize("C,bad_gt,bad_pr", ((21, 21, 0), (21, 0, -22), (51, 5, 51), (200, -201, 3), (200, 7, 1 << 40)))
def test_out_of_range_id_raises_index_error_and_leaves_the_matrix(C, bad_gt, bad_pr):
    from ovo_amd.utils import eval_utils as E
    g = np.random.default_rng(1)
    gt, pr = g.integers(0, C, 5000), g.integers(0, C, 5000)
    gt[4321], pr[4321] = bad_gt, bad_pr
    conf = np.full((C, C), 7, dtype=np.ulonglong)
    with pytest.raises(IndexError):
        E.update_confmat(conf, gt, pr, [])
    assert (conf == 7).all()
    E.update_confmat(conf, gt, pr, [bad_gt])                        # the reference skips an ignored gt before it indexes
    assert int(conf.sum()) == 7 * C * C + 5000 - int((gt == bad_gt).sum())


# ---- 5. end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg", (False, True))
@pytest.mark.parametrize("name", ("scannet", "replica"))
def test_eval_semantics_matches_reference(name, bg, tmp_path):
    from ovo_amd.utils import eval_utils as E, io_utils as IO
    d = golden("eval_e2e")
    tag = f"{name}_{'bg' if bg else 'all'}"
    info = json.loads(d[f"{name}_info_json"].tobytes().decode())
    if "map_to_reduced" in info:
        info["map_to_reduced"] = {int(k): v for k, v in info["map_to_reduced"].items()}
    scenes = [str(s) for s in d[f"{name}_scenes"]]
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    os.makedirs(pred), os.makedirs(gt)
    for s in scenes:
        IO.write_labels(str(gt / f"{s}.txt"), d[f"{name}_{s}_gt"])
        IO.write_labels(str(pred / f"{s}.txt"), d[f"{name}_{s}_pr"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        metrics, conf = E.eval_semantics(str(pred), str(gt), scenes, info, True, bg, True, True)
    assert list(metrics) == [str(k) for k in d[f"{tag}_metric_names"]]
    assert [float(v) for v in metrics.values()] == list(d[f"{tag}_metric_values"])
    assert conf.dtype == d[f"{tag}_confusion"].dtype and np.array_equal(conf, d[f"{tag}_confusion"])
    assert (pred / "statistics.txt").read_bytes() == d[f"{tag}_statistics"].tobytes()
    ours, ref = buf.getvalue(), d[f"{tag}_stdout"].tobytes().decode()
    assert ours.startswith(ref) and ours[len(ref):].count("\n") == 1          # the reference's prints byte for byte, then the one line about the plots
    miou, conf2 = E.eval_semantics(str(pred), str(gt), scenes, info, True, bg, False)      # quiet form: (mIoU, confusion), writes nothing
    assert round(miou, 3) == metrics["iou"] and np.array_equal(conf2, conf)
