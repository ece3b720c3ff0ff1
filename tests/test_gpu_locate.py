"""-m gpu: the public side of the instance boxes -- `OVO.instance_boxes`, `OVO.locate`, `OVO.render_view(boxes=...)` on a small tracked scene (built
like tests/test_gpu_render.py's), and `FramePipeline.instance_boxes` / `.locate` on the pipeline's own map."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_render import _tokenizer

pytestmark = pytest.mark.gpu
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _tracked_scene():
    """(ovo, mapper, poses, (h, w)): three keyframes mapped and tracked; built once, read by every test."""
    from ovo_amd import synthetic as syn
    from ovo_amd.encoders.text import HipTextEncoder, TextSpec
    from ovo_amd.encoders.vit import SPECS as VS, HipViT
    from ovo_amd.entities.clip_generator import CLIPGenerator
    from ovo_amd.entities.ovo import OVO
    from ovo_amd.slam.vanilla_mapper import VanillaMapper
    scale = 0.35
    h, w = syn.scannet_depth_hw(scale)
    K = torch.from_numpy(syn.scannet_intrinsics(scale)).to(DEV)
    vit = HipViT(VS["tiny-pe"], None, device=DEV, seed=1)
    text = HipTextEncoder(TextSpec("tiny", 100, 16, 64, 2, 4, VS["tiny-pe"].out_dim, "gelu"), None, device=DEV, tokenizer=_tokenizer(16))
    clip_cfg = {"embed_type": "TextRegion", "model_card": "PE-tiny-084", "k_top_views": 5, "fusion": "l1_medoid"}

    class Masks:
        def get_masks(self, image, frame_id):
            m = syn.make_masks(h, w, grid=(3, 4), n_blobs=4, seed=frame_id)
            return torch.from_numpy(syn.masks_to_segmap(m)).to(DEV), torch.from_numpy(m).to(DEV)

    cfg = {"match_distance_th": 0.05, "track_th": 40, "depth_filter": False, "log": False, "kf_queue_delay": 1, "clip": clip_cfg, "sam": {}}
    ovo = OVO(cfg, None, None, K, device=DEV, clip_generator=CLIPGenerator(dict(clip_cfg), device=DEV, encoder=vit, text_encoder=text),
              mask_generator=Masks())
    vm = VanillaMapper({"device": DEV, "mapping": {}}, K)
    poses = {}
    for t in range(3):
        fid, rgb, depth, c2w = syn.frame(t, scale=scale, seed=3)
        fd = [fid, rgb, depth, c2w]
        vm.track_camera(fd)
        vm.map(fd, vm.get_c2w(fid))
        updated = ovo.detect_and_track_objects([fid, rgb, depth, ()], vm.get_map(), vm.get_c2w(fid))
        if updated is not None:
            vm.update_pcd_obj_ids(updated)
        ovo.compute_semantic_info()
        poses[fid] = c2w
    ovo.complete_semantic_info()
    assert len(ovo.objects) > 3
    return ovo, vm, poses, (h, w)


def _bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _numpy_boxes(map_data, ids):
    xyz, ins = map_data[0].cpu().numpy(), map_data[2].reshape(-1).cpu().numpy()
    cnt = np.array([(ins == i).sum() for i in ids], np.int32)
    lo = np.array([xyz[ins == i].min(0) if (ins == i).any() else np.full(3, np.nan, np.float32) for i in ids], np.float32)
    hi = np.array([xyz[ins == i].max(0) if (ins == i).any() else np.full(3, np.nan, np.float32) for i in ids], np.float32)
    return cnt, lo, hi


def test_instance_boxes_equal_numpy():
    ovo, vm, _, _ = _tracked_scene()
    ids = list(ovo.objects)
    out = ovo.instance_boxes(vm.get_map())
    assert set(out) == {"ids", "count", "center", "min", "max"} and out["ids"].tolist() == ids
    cnt, lo, hi = _numpy_boxes(vm.get_map(), ids)
    assert (cnt > 0).sum() > 3
    assert np.array_equal(_bits(out["count"]), cnt)
    has = cnt > 0
    assert np.array_equal(_bits(out["min"])[has], lo.view(np.uint32)[has]) and np.array_equal(_bits(out["max"])[has], hi.view(np.uint32)[has])
    assert np.isnan(out["min"].cpu().numpy()[~has]).all() and np.isnan(out["center"].cpu().numpy()[~has]).all()
    assert np.array_equal(_bits(out["center"])[has], ((lo + hi) * np.float32(0.5)).view(np.uint32)[has])
    # an instance that loses its points keeps its row: count 0, a NaN box
    xyz, pid, ins = vm.get_map()
    gone = ids[int(np.argmax(cnt))]
    ins2 = torch.where(ins == gone, torch.full_like(ins, -1), ins)
    lost = ovo.instance_boxes((xyz, pid, ins2))
    r = ids.index(gone)
    assert int(lost["count"][r]) == 0 and bool(torch.isnan(lost["min"][r]).all()) and bool(torch.isnan(lost["max"][r]).all())
    keep = [k for k in range(len(ids)) if k != r]
    assert torch.equal(lost["min"][keep].view(torch.int32), out["min"][keep].view(torch.int32))


def test_oriented_boxes_hold_their_points():
    ovo, vm, _, _ = _tracked_scene()
    ids = list(ovo.objects)
    out = ovo.instance_boxes(vm.get_map(), oriented=True)
    assert set(out) == {"ids", "count", "center", "min", "max", "R", "extent"}
    xyz, ins = vm.get_map()[0].cpu().numpy().astype(np.float64), vm.get_map()[2].reshape(-1).cpu().numpy()
    R, lo, hi = out["R"].cpu().numpy().astype(np.float64), out["min"].cpu().numpy(), out["max"].cpu().numpy()
    checked = 0
    for r, i in enumerate(ids):
        p = xyz[ins == i]
        if len(p) < 3:
            continue
        assert abs(np.linalg.det(R[r]) - 1.0) < 1e-5 and np.abs(R[r] @ R[r].T - np.eye(3)).max() < 1e-5
        c = p @ R[r].T                                              # the extent along the axes, to f32 rounding of the chain
        assert np.abs(c.min(0) - lo[r]).max() < 1e-5 and np.abs(c.max(0) - hi[r]).max() < 1e-5
        var = np.var(c, axis=0)
        assert var[0] >= var[1] * (1 - 1e-6) and var[1] >= var[2] * (1 - 1e-6)              # eigenvalues descend
        assert np.abs(out["center"][r].cpu().numpy() - ((lo[r] + hi[r]) / 2) @ R[r]).max() < 1e-5
        checked += 1
    assert checked > 3


def _crafted_query(ovo, monkeypatch, n_queries=2, seed=0):
    """`ovo.query` replaced by a fixed table f32[N, Q] with a NaN row and a tie: what `locate` sorts is then known exactly."""
    n = len(ovo.objects)
    rng = np.random.default_rng(seed)
    sim = rng.uniform(-0.2, 0.9, (n, n_queries)).astype(np.float32)
    sim[1] = np.nan                                                 # an instance without a descriptor
    sim[3, 0] = sim[2, 0] = np.float32(0.95)                        # a tie at the top: the smaller id first
    table = torch.from_numpy(sim).to(DEV)
    monkeypatch.setattr(ovo, "query", lambda queries, templates=['{}'], ensemble=False: table[:, :len(queries)])
    return sim


def _expected(sim_col, ids, cnt, th, top_k):
    order = sorted((r for r in range(len(ids)) if sim_col[r] > th and cnt[r] > 0), key=lambda r: (-float(sim_col[r]), ids[r]))
    return order[:top_k]


def test_locate_lists_what_a_sort_of_the_query_column_lists(monkeypatch):
    ovo, vm, _, _ = _tracked_scene()
    ids = list(ovo.objects)
    cnt, lo, hi = _numpy_boxes(vm.get_map(), ids)
    # the real text path first: scores are the matching `query` column
    real = ovo.query(["lamp", "floor"]).float().cpu().numpy()
    found = ovo.locate(vm.get_map(), ["lamp", "floor"], top_k=100, th=-2.0)
    for q in range(2):
        rows = _expected(real[:, q], ids, cnt, -2.0, 100)
        assert [hit["ins_id"] for hit in found[q]] == [ids[r] for r in rows] and len(rows) > 3
        assert [np.float32(hit["score"]) for hit in found[q]] == [real[r, q] for r in rows]
    sim = _crafted_query(ovo, monkeypatch)
    for top_k, th in ((5, 0.0), (2, 0.0), (100, 0.5), (100, -1.0), (3, 2.0)):
        found = ovo.locate(vm.get_map(), ["a", "b"], top_k=top_k, th=th)
        assert len(found) == 2
        for q in range(2):
            rows = _expected(sim[:, q], ids, cnt, th, top_k)
            assert [hit["ins_id"] for hit in found[q]] == [ids[r] for r in rows], (top_k, th, q)
            for hit, r in zip(found[q], rows):
                assert set(hit) == {"ins_id", "score", "center", "min", "max", "n_points"} and hit["n_points"] == cnt[r] > 0
                assert np.float32(hit["score"]) == sim[r, q] and hit["score"] > th
                assert np.array_equal(hit["min"].view(np.uint32), lo[r].view(np.uint32)) and np.array_equal(hit["max"].view(np.uint32), hi[r].view(np.uint32))
            assert ids[1] not in [hit["ins_id"] for hit in found[q]]                        # the NaN row
    top = ovo.locate(vm.get_map(), ["a"], top_k=2, th=0.0)[0]
    if cnt[2] > 0 and cnt[3] > 0:
        assert [hit["ins_id"] for hit in top] == sorted([ids[2], ids[3]])                   # the tie goes to the smaller id
    assert ovo.locate(vm.get_map(), ["a"], th=2.0) == [[]]
    hit = ovo.locate(vm.get_map(), ["a"], top_k=1, th=0.0, oriented=True)[0][0]
    assert set(hit) == {"ins_id", "score", "center", "min", "max", "n_points", "R", "extent"} and hit["R"].shape == (3, 3)
    # an instance without points is never listed
    xyz, pid, ins = vm.get_map()
    gone = top[0]["ins_id"]
    ins2 = torch.where(ins == gone, torch.full_like(ins, -1), ins)
    assert gone not in [h["ins_id"] for h in ovo.locate((xyz, pid, ins2), ["a"], top_k=100, th=-1.0)[0]]


def test_render_view_draws_the_boxes():
    ovo, vm, poses, hw = _tracked_scene()
    ids = list(ovo.objects)
    cnt, _, _ = _numpy_boxes(vm.get_map(), ids)
    asked = [ids[r] for r in np.argsort(-cnt)[:3]]
    plain = ovo.render_view(vm.get_map(), poses[1], hw)
    out = ovo.render_view(vm.get_map(), poses[1], hw, boxes=asked, box_width=1.0)
    assert set(out) == set(plain) | {"box", "box_depth"}
    for k in ("row", "depth", "ins"):
        assert torch.equal(out[k].view(torch.int32), plain[k].view(torch.int32)), k
    box = out["box"].cpu().numpy()
    assert out["box"].dtype == torch.int32 and box.shape == tuple(hw) and set(np.unique(box)) <= set(asked) | {-1}
    assert len(set(np.unique(box)) - {-1}) >= 2 and (box >= 0).sum() > 50
    assert torch.equal(out["box_depth"] > 0, out["box"] >= 0)
    # an edge is drawn only where it is not more than the slack behind the splat
    d, bd = out["depth"].cpu().numpy(), out["box_depth"].cpu().numpy()
    seen = box >= 0
    assert ((d[seen] == 0) | (bd[seen] <= d[seen] + np.float32(0.02))).all()
    every = ovo.render_view(vm.get_map(), poses[1], hw, boxes="all", oriented=True)
    assert set(np.unique(every["box"].cpu().numpy())) <= set(ids) | {-1} and int((every["box"] >= 0).sum()) > int(seen.sum())
    sim = ovo.query(["lamp", "floor"])[:, 0].float().cpu()
    th = float(sim[torch.isfinite(sim)].median())
    hot = ovo.render_view(vm.get_map(), poses[1], hw, query="lamp", context=("floor",), query_th=th, boxes="query")
    allowed = {ids[r] for r in range(len(ids)) if bool(sim[r] > th)}
    assert "heat" in hot and set(np.unique(hot["box"].cpu().numpy())) <= allowed | {-1} and 0 < len(allowed) < len(ids)
    with pytest.raises(ValueError):
        ovo.render_view(vm.get_map(), poses[1], hw, boxes="query")
    with pytest.raises(ValueError):
        ovo.render_view(vm.get_map(), poses[1], hw, boxes="some")


def test_pipeline_locate_and_boxes(monkeypatch):
    from ovo_amd import _lib
    from ovo_amd.pipeline import FramePipeline, synthetic_frames
    from test_gpu_multirank import KW
    frames = synthetic_frames(2, DEV, scale=0.35, n_masks_grid=(3, 4), n_blobs=4, start=4)
    pipe = FramePipeline(DEV, **KW)
    for f in frames:
        pipe.step(f)
    assert len(pipe.ovo.objects) > 3
    _crafted_query(pipe.ovo, monkeypatch, seed=1)
    mine = pipe.locate(["a", "b"], top_k=4, th=0.1)
    theirs = pipe.ovo.locate(pipe.slam.get_map(), ["a", "b"], top_k=4, th=0.1)
    assert len(mine) == 2 and sum(len(x) for x in mine) > 2
    for a, b in zip(mine, theirs):
        assert [h["ins_id"] for h in a] == [h["ins_id"] for h in b]
        for x, y in zip(a, b):
            assert x["score"] == y["score"] and x["n_points"] == y["n_points"]
            assert all(np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)) for k in ("center", "min", "max"))
    boxes, direct = pipe.instance_boxes(), pipe.ovo.instance_boxes(pipe.slam.get_map())
    assert all(torch.equal(boxes[k], direct[k]) or k in ("center", "min", "max") for k in boxes) and torch.equal(boxes["count"], direct["count"])
    assert torch.equal(boxes["min"].view(torch.int32), direct["min"].view(torch.int32))
    out = pipe.render_view(frames[1].c2w, dense=False, boxes="all")
    assert "box" in out and int((out["box"] >= 0).sum()) > 20
    # what they refuse, as render_view does
    pipe._queued[99] = None
    for call in (lambda: pipe.locate(["a"]), lambda: pipe.instance_boxes()):
        with pytest.raises(_lib.OvoHipError, match="pre-queued"):
            call()
    pipe._queued.clear()
    pipe.emulate = True
    for call in (lambda: pipe.locate(["a"]), lambda: pipe.instance_boxes()):
        with pytest.raises(_lib.OvoHipError, match="emulate"):
            call()
    pipe.emulate = False
