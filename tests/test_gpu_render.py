"""-m gpu: the view renderer (csrc/render.hip, utils/render_utils.py, OVO.render_view, FramePipeline.render_view) against its CPU restatement
(tests/render_restatement.py).  Every output is compared as raw bits: `row` as i32, `depth` through .view(np.uint32).

1. a general scene (48 x 64, rotated pose, 6000 points: some behind the camera, 60 exact duplicates) at radius 0, 1, 2;
2. edges: n = 0, 1, 63, 65, 6001; a 1 x 1 and a 37 x 53 image; every point on one pixel; depths exactly at near / far; NaN, inf, lw = 0 and a pixel
   beyond the int range; a repeated launch;
3. grid-stride: 300 001 lattice points with the splat's workgroup count capped through the launch heuristic's own knob (OVO_RENDER_GRID_CAP = 8: every
   workgroup loops 37 times) and at the default grid (every workgroup one trip);
4. ovo_render_resolve against numpy fancy indexing;
5. one keyframe mapped on an empty map and rendered from its own pose reproduces the frame;
6. OVO.render_view / FramePipeline.render_view on a small tracked scene."""
import functools

import numpy as np
import pytest
import torch

import render_restatement as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, NEAR, FAR = 48, 64, 0.1, 10.0


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same(got, ref, what=""):
    """(row, depth) of the GPU against (row, depth, ...) of the restatement, bit for bit."""
    row, depth = _bits(got[0]), _bits(got[1])
    assert row.dtype == np.int32 and row.shape == ref[0].shape and depth.shape == ref[1].shape, what
    assert np.array_equal(row, ref[0]), f"{what}: {(row != ref[0]).sum()} row pixels differ"
    assert np.array_equal(depth, _bits(ref[1])), f"{what}: {(depth != _bits(ref[1])).sum()} depth pixels differ"


def _gpu(xyz, view):
    from ovo_amd.utils import render_utils as R
    return R.render_rows(torch.from_numpy(np.array(xyz, dtype=np.float32)).reshape(-1, 3).to(DEV), view)       # (a copy: the shared scene is read-only)


def _w2c(view):
    return np.array(view.w2c, np.float32).reshape(4, 4)


def _manual_view(w2c, K, h, w, radius, near, far):
    from ovo_amd import _lib
    v = _lib.View()
    v.w2c[:] = np.asarray(w2c, np.float32).reshape(-1).tolist()
    v.K[:] = np.asarray(K, np.float32).reshape(-1).tolist()
    v.near, v.far, v.h, v.w, v.radius = near, far, h, w, radius
    return v


@functools.lru_cache(maxsize=None)
def _scene():
    """The general scene, 6001 points (test 1 uses the first 6000), its w2c as `make_view` inverts it, and the exact-chain depths: computed once."""
    from ovo_amd.utils import render_utils as R
    xyz, c2w = RR.general_scene(6001)
    w2c = _w2c(R.make_view(c2w, RR.K_SMALL, H, W))
    zc = RR.depths(xyz, w2c, RR.OG.project(xyz, RR.K_SMALL, w2c))
    for a in (xyz, w2c, zc):
        a.setflags(write=False)
    return xyz, c2w, w2c, zc


# ---------------------------------------------------------------------------------------------------- 1. general scene
@pytest.mark.parametrize("radius", [0, 1, 2])
def test_general_scene(radius):
    from ovo_amd.utils import render_utils as R
    xyz, c2w, w2c, zc = _scene()
    xyz, zc = xyz[:6000], zc[:6000]
    ref = RR.render(xyz, w2c, RR.K_SMALL, H, W, radius, NEAR, FAR, zc=zc)
    if radius == 0:                                                 # the scene is worth rendering: asserted on the reference alone
        filled, multi = (ref[0] >= 0).mean(), (ref[2] >= 2).mean()
        assert filled >= 0.40 and multi >= 0.15, (filled, multi)
        assert ((ref[0] >= 200) & (ref[0] < 260)).sum() > 0 and ((ref[0] >= 260) & (ref[0] < 320)).sum() == 0      # duplicates: the smaller row wins
        m = w2c[2]
        plain = ((m[0] * xyz[:, 0] + m[1] * xyz[:, 1]) + m[2] * xyz[:, 2]) + m[3]
        assert (plain.view(np.uint32) != zc.view(np.uint32)).sum() > 100       # and plain f32 arithmetic would not have been the reference
    view = R.make_view(c2w, RR.K_SMALL, H, W, radius=radius, near=NEAR, far=FAR)
    assert np.array_equal(_w2c(view), w2c)
    got = _gpu(xyz, view)
    _assert_same(got, ref, f"radius {radius}")
    again = _gpu(xyz, view)                                          # a repeated launch: identical bits
    assert torch.equal(got[0], again[0]) and torch.equal(got[1].view(torch.int32), again[1].view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 2. edges
@pytest.mark.parametrize("n", [0, 1, 63, 65, 6001])
def test_tails_of_the_rows_per_wave_loop(n):
    from ovo_amd.utils import render_utils as R
    xyz, c2w, w2c, zc = _scene()
    lo = 0 if n == 6001 else 204                                     # (the first 200 rows are behind the camera; row 204 is in view)
    xyz, zc = xyz[lo:lo + n], zc[lo:lo + n]
    ref = RR.render(xyz, w2c, RR.K_SMALL, H, W, 1, NEAR, FAR, zc=zc)
    assert (ref[0] >= 0).any() == (n > 0)
    _assert_same(_gpu(xyz, R.make_view(c2w, RR.K_SMALL, H, W, radius=1, near=NEAR, far=FAR)), ref, f"n = {n}")
    if n == 0:
        assert (ref[0] == -1).all() and (_bits(ref[1]) == 0).all()


@pytest.mark.parametrize("h,w,radius", [(1, 1, 2), (37, 53, 1), (37, 53, 0)])
def test_image_sizes(h, w, radius):
    from ovo_amd.utils import render_utils as R
    xyz, c2w, w2c, zc = _scene()
    K = RR.K_SMALL.copy()
    if h == 1:
        K[0, 2] = K[1, 2] = 0.0                                      # the optical axis through the only pixel
    ref = RR.render(xyz, w2c, K, h, w, radius, NEAR, FAR, zc=zc)
    assert ref[2].max() > 1
    _assert_same(_gpu(xyz, R.make_view(c2w, K, h, w, radius=radius, near=NEAR, far=FAR)), ref, f"{h} x {w}")


def test_every_point_on_one_pixel():
    """6000 points on the optical axis of an identity pose, distinct depths in a shuffled order, the nearest depth twice: one pixel, 6000 candidates."""
    from ovo_amd.utils import render_utils as R
    rng = np.random.default_rng(3)
    z = (1.0 + np.arange(6000) / 2000.0).astype(np.float32)
    assert len(np.unique(z)) == 6000
    z = rng.permutation(z)
    first = int(np.argmin(z))
    dup = (first + 1234) % 6000
    z[dup] = z[first]
    xyz = np.stack([np.zeros_like(z), np.zeros_like(z), z], axis=1)
    K = np.array([[60, 0, 32], [0, 60, 16], [0, 0, 1]], np.float32)          # a power-of-two principal point: fl(32 z) / z is 32 for every z
    view = R.make_view(np.eye(4, dtype=np.float32), K, H, W, radius=0, near=NEAR, far=FAR)
    ref = RR.render(xyz, _w2c(view), K, H, W, 0, NEAR, FAR)
    assert (ref[0] >= 0).sum() == 1 and ref[2].max() == 6000 and ref[0].max() == min(first, dup) and ref[1].max() == z[first]
    _assert_same(_gpu(xyz, view), ref)


def _special_rows():
    """Rows 0-3 ordinary; then depths exactly at / just outside near and far (identity pose: zc = z), NaN, +-inf, and a pixel beyond the int range."""
    near, far = np.float32(NEAR), np.float32(FAR)
    below, above = np.nextafter(near, np.float32(0)), np.nextafter(far, np.float32(np.inf))
    rows = [(0.0, 0.0, 2.0), (0.2, 0.1, 1.5), (-0.3, 0.2, 3.0), (0.2, 0.1, 2.5),
            (0.01, 0.0, near), (-0.01, 0.0, below), (3.0, 2.0, far), (-3.0, 2.0, above), (-3.0, -2.0, far), (3.0, -2.0, far),
            (np.nan, 0.0, 2.0), (0.0, np.nan, 2.0), (0.0, 0.0, np.nan), (np.inf, 0.0, 2.0), (0.0, -np.inf, 2.0), (0.0, 0.0, np.inf),
            (1.0e12, 0.0, 1.0), (0.0, -1.0e12, 1.0), (3.0e38, 3.0e38, 1.0)]
    return np.array(rows, np.float32)


@pytest.mark.parametrize("radius", [0, 2])
def test_inclusive_depth_bounds_and_dropped_rows(radius):
    from ovo_amd.utils import render_utils as R
    xyz = _special_rows()
    view = R.make_view(np.eye(4, dtype=np.float32), RR.K_SMALL, H, W, radius=radius, near=NEAR, far=FAR)
    ref = RR.render(xyz, _w2c(view), RR.K_SMALL, H, W, radius, NEAR, FAR)
    winners = set(ref[0][ref[0] >= 0].tolist())
    assert {4, 6, 8, 9} <= winners and not winners & {5, 7} and max(winners) <= 9, winners        # at near / far: kept; a ulp outside, NaN, inf, huge: dropped
    _assert_same(_gpu(xyz, view), ref)
    # far = +inf keeps a finite depth however large, and still drops the non-finite rows
    view = R.make_view(np.eye(4, dtype=np.float32), RR.K_SMALL, H, W, radius=radius, near=NEAR)
    ref = RR.render(xyz, _w2c(view), RR.K_SMALL, H, W, radius, NEAR, float("inf"))
    assert 7 in set(ref[0][ref[0] >= 0].tolist())
    _assert_same(_gpu(xyz, view), ref)


def test_zero_homogeneous_coordinate_is_dropped():
    """A projective bottom row (0, 0, 1, -2): lw = z - 2, so a point at z = 2 has lw = 0 and a depth inside [near, far]; the others keep their pixels
    (the division by lw cancels in u and v)."""
    w2c = np.eye(4, dtype=np.float32)
    w2c[3] = (0, 0, 1, -2)
    xyz = np.array([(0.1, 0.1, 1.5), (0.0, 0.0, 2.0), (0.3, -0.2, 2.0), (-0.2, 0.1, 3.0), (0.1, 0.1, 2.5)], np.float32)
    ref = RR.render(xyz, w2c, RR.K_SMALL, H, W, 1, NEAR, FAR)
    assert set(ref[0][ref[0] >= 0].tolist()) == {0, 3, 4}
    _assert_same(_gpu(xyz, _manual_view(w2c, RR.K_SMALL, H, W, 1, NEAR, FAR)), ref)


# ---------------------------------------------------------------------------------------------------- 3. grid-stride
def test_grid_stride_over_a_large_map(monkeypatch):
    n = 300_001
    xyz, w2c = RR.lattice_scene(n)
    ref = RR.render_lattice(xyz, w2c, RR.K_SMALL, H, W, 1, 2.0, 12.0)
    assert (ref[0] >= 0).mean() > 0.9 and ref[2].max() > 100
    view = _manual_view(w2c, RR.K_SMALL, H, W, 1, 2.0, 12.0)
    pts = torch.from_numpy(xyz).to(DEV)
    from ovo_amd.utils import render_utils as R
    _assert_same(R.render_rows(pts, view), ref, "default grid")     # 293 workgroups x 1024 rows: one trip each, a ragged last one
    monkeypatch.setenv("OVO_RENDER_GRID_CAP", "8")                  # the launch heuristic's own cap: 8 workgroups x 1024 rows per trip, 37 trips
    _assert_same(R.render_rows(pts, view), ref, "8 workgroups")


# ---------------------------------------------------------------------------------------------------- 4. resolve
def test_resolve_against_fancy_indexing():
    from ovo_amd.utils import render_utils as R
    rng = np.random.default_rng(9)
    h, w, n, n_slots = 37, 53, 500, 40
    row = rng.integers(0, n, (h, w)).astype(np.int32)
    row[rng.random((h, w)) < 0.3] = -1
    ins = rng.integers(-1, n_slots + 10, n).astype(np.int32)        # -1: unassigned, >= n_slots: no table entry
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    pcls = rng.integers(-5, 1 << 40, n).astype(np.int64)
    pconf = rng.standard_normal(n).astype(np.float32)
    icls = rng.integers(0, 1 << 40, n_slots).astype(np.int64)
    ival = rng.standard_normal(n_slots).astype(np.float32)
    for arr in (pconf, ival):                                       # NaN payloads, -0.0, a denormal: a gather moves bits
        arr.view(np.uint32)[:4] = (0x7FC12345, 0xFFA00001, 0x80000000, 0x00000007)
    hit = row >= 0
    r = np.where(hit, row, 0)
    e_ins = np.where(hit, ins[r], -1).astype(np.int32)
    slot = (e_ins >= 0) & (e_ins < n_slots)
    s = np.where(slot, e_ins, 0)
    bg, fill_cls, fill_val = (7, 200, 31), -3, np.float32(-1.5)
    expect = {"ins": e_ins,
              "rgb": np.where(hit[..., None], rgb[r], np.array(bg, np.uint8)),
              "cls": np.where(hit, pcls[r], fill_cls),
              "conf": np.where(hit, pconf.view(np.uint32)[r], fill_val.view(np.uint32)),
              "ins_cls": np.where(slot, icls[s], fill_cls),
              "val": np.where(slot, ival.view(np.uint32)[s], fill_val.view(np.uint32))}
    assert (e_ins == -1).any() and (e_ins >= n_slots).any() and slot.any() and (~hit).any()
    d = lambda a: torch.from_numpy(a).to(DEV)
    src = {"point_ins": d(ins), "point_rgb": d(rgb), "point_cls": d(pcls), "point_conf": d(pconf), "ins_cls": d(icls), "ins_val": d(ival)}
    key_of = {"point_ins": "ins", "point_rgb": "rgb", "point_cls": "cls", "point_conf": "conf", "ins_cls": "ins_cls", "ins_val": "val"}
    kw = dict(background=bg, fill_cls=fill_cls, fill_val=float(fill_val))

    def check(out, names):
        assert set(out) == {key_of[k] for k in names}
        for k in out:
            assert np.array_equal(_bits(out[k]), expect[k]), k
    drow = d(row)
    for name in src:                                                # every source alone (a per-instance table brings point_ins with it)
        names = [name] + (["point_ins"] if name.startswith("ins_") else [])
        check(R.resolve(drow, **{k: src[k] for k in names}, **kw), names)
    check(R.resolve(drow, **src, **kw), list(src))                  # all together
    # rows at or past the shortest per-point source are empty pixels
    out = R.resolve(drow, point_ins=src["point_ins"][:100])
    assert np.array_equal(_bits(out["ins"]), np.where(hit & (row < 100), ins[np.where(row < 100, r, 0)], -1))
    from ovo_amd import _lib
    with pytest.raises(_lib.OvoHipError):
        R.resolve(drow, ins_val=src["ins_val"])


# ---------------------------------------------------------------------------------------------------- 5. one keyframe, its own pose
@pytest.mark.parametrize("t", [0, 5, 11])
def test_a_keyframe_rendered_from_its_own_pose_reproduces_the_frame(t):
    from ovo_amd import synthetic as syn
    from ovo_amd.slam.vanilla_mapper import VanillaMapper
    from ovo_amd.utils import render_utils as R
    scale = 0.25
    K = syn.scannet_intrinsics(scale)
    h, w = syn.scannet_depth_hw(scale)
    fid, rgb, depth, c2w = syn.frame(t, scale=scale, seed=3)
    vm = VanillaMapper({"device": DEV, "mapping": {}}, torch.from_numpy(K).to(DEV))
    fd = [fid, rgb, depth, c2w]
    vm.track_camera(fd)
    vm.map(fd, vm.get_c2w(fid))
    n = vm.pcd.shape[0]
    assert n > 1000
    view = R.make_view(c2w, K, h, w, radius=0)
    row, zdepth = R.render_rows(vm.pcd, view)
    hit = row >= 0
    assert int(hit.sum()) == n                                      # every point lands on a pixel of its own ...
    assert torch.equal(row[hit], torch.arange(n, dtype=torch.int32, device=row.device))      # ... in append order = row-major pixel order
    img = R.resolve(row, point_rgb=vm.pcd_colors)["rgb"]
    hit_h = hit.cpu().numpy()
    assert np.array_equal(img.cpu().numpy()[hit_h], rgb[hit_h]) and (img.cpu().numpy()[~hit_h] == 0).all()
    xyz = vm.pcd.cpu().numpy()
    ref = RR.render(xyz, _w2c(view), K, h, w, 0, 0.05, float("inf"))
    assert ref[2].max() == 1
    _assert_same((row, zdepth), ref)
    assert np.abs(zdepth.cpu().numpy()[hit_h] - depth[hit_h]).max() < 1e-5       # and the frame's own depth to rounding


# ---------------------------------------------------------------------------------------------------- 6. the public entry points
def _tokenizer(context):
    def tok(texts):
        rows = []
        for s in texts:
            ids = [98] + [1 + (sum(map(ord, w)) % 90) for w in s.split()][: context - 2] + [99]
            rows.append(ids + [0] * (context - len(ids)))
        return torch.tensor(rows)
    return tok


def _lookup(ins_img, ids, values, fill):
    """values (one per instance, in `ids` order) looked up through the instance-id image, with torch."""
    table = {int(i): v for i, v in zip(ids, values)}
    flat = [table.get(int(i), fill) for i in ins_img.reshape(-1).tolist()]
    return torch.tensor(flat, dtype=values.dtype).reshape(ins_img.shape)


def test_ovo_render_view_on_a_tracked_scene():
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

    class Masks:                                                    # the precomputed-mask seam, as in smoke()
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

    classes, template = ["chair", "a wooden table", "lamp", "floor"], "This is a photo of a {}"
    sim = ovo.query(["lamp", "floor"])[:, 0].float().cpu()
    query_th = float(sim[torch.isfinite(sim)].median())            # so that some instances fall under the threshold and some do not
    out = ovo.render_view(vm.get_map(), poses[1], (h, w), radius=1, colors=vm.pcd_colors, classes=classes, template=template, th=-1.0,
                          query="lamp", context=("floor",), query_th=query_th)
    assert set(out) == {"row", "depth", "ins", "rgb", "cls", "conf", "heat"}
    row = out["row"].long()
    hit = row >= 0
    assert float(hit.float().mean()) > 0.5
    safe = row.clamp(min=0)
    point_ins = vm.pcd_obj_ids.reshape(-1)
    ins = torch.where(hit, point_ins[safe], torch.full_like(point_ins[safe], -1))
    assert torch.equal(out["ins"], ins) and int((ins >= 0).sum()) > 100 and len(torch.unique(ins[ins >= 0])) > 3
    assert torch.equal(out["rgb"], torch.where(hit[..., None], vm.pcd_colors[safe], torch.zeros_like(vm.pcd_colors[safe])))
    assert torch.equal(out["depth"] > 0, hit)
    ids = list(ovo.objects)
    info = ovo.classify_instances(classes, template=template, th=-1.0)
    ins_h = ins.cpu()
    assert torch.equal(out["cls"].cpu(), _lookup(ins_h, ids, torch.from_numpy(info["classes"]).long(), -1))
    conf = _lookup(ins_h, ids, torch.from_numpy(info["conf"]).float(), 0.0)
    assert torch.equal(out["conf"].cpu().view(torch.int32), conf.view(torch.int32))
    heat_ins = torch.where(sim > query_th, sim, torch.zeros_like(sim))
    heat = _lookup(ins_h, ids, heat_ins, 0.0)
    assert torch.equal(out["heat"].cpu().view(torch.int32), heat.view(torch.int32))
    assert bool((out["heat"] != 0).any()) and bool(((out["heat"] == 0) & (out["ins"] >= 0)).any())
    # the defaults: row, depth and ins only; the intrinsics OVO was built with
    small = ovo.render_view(vm.get_map(), poses[1], (h, w))
    assert set(small) == {"row", "depth", "ins"} and torch.equal(small["row"], out["row"]) and torch.equal(small["ins"], out["ins"])


def test_pipeline_render_view_reads_the_dense_map():
    from ovo_amd import _lib
    from ovo_amd.pipeline import FramePipeline, synthetic_frames
    from test_gpu_multirank import KW
    frames = synthetic_frames(2, DEV, scale=0.35, n_masks_grid=(3, 4), n_blobs=4, start=4)
    pipe = FramePipeline(DEV, **KW)
    for f in frames:                                                # two rounds (one rank: a round is one keyframe)
        pipe.step(f)
    out = pipe.render_view(frames[1].c2w, dense=True)
    assert {"row", "depth", "ins", "rgb", "dense_cls", "dense_conf"} <= set(out) and out["row"].shape == frames[1].depth.shape
    row = out["row"].long()
    hit = row >= 0
    assert float(hit.float().mean()) > 0.5
    dm = pipe.dense_map
    assert torch.equal(out["dense_cls"][hit], dm.dense_cls[row[hit]]) and len(torch.unique(out["dense_cls"][hit])) > 1
    assert torch.equal(out["dense_conf"][hit].view(torch.int32), dm.dense_conf[row[hit]].view(torch.int32))
    assert bool((out["dense_cls"][~hit] == -1).all()) and bool((out["dense_conf"][~hit] == 0).all())
    assert torch.equal(out["ins"][hit], pipe.slam.pcd_obj_ids.reshape(-1)[row[hit]])
    assert "dense_cls" not in pipe.render_view(frames[1].c2w, hw=(30, 40), dense=False)
    # what it refuses
    pipe._queued[99] = None
    with pytest.raises(_lib.OvoHipError, match="pre-queued"):
        pipe.render_view(frames[1].c2w)
    pipe._queued.clear()
    pipe.world = 2
    with pytest.raises(ValueError, match="DenseMap.gather"):
        pipe.render_view(frames[1].c2w)
    pipe.world = 1
    pipe.emulate = True
    with pytest.raises(_lib.OvoHipError, match="emulate"):
        pipe.render_view(frames[1].c2w)
    pipe.emulate = False
