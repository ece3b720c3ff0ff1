"""-m gpu: SAM2 prompt encoder + mask decoder + automatic mask generator (f1) on MI355X vs the fp32 oracle
(decoder pinned to HuggingFace's implementation; the generator's post-processing is an unpinned restatement)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _inputs(spec, seed=0):
    g = torch.Generator().manual_seed(seed)
    s, c = spec.embed_size, spec.hidden
    emb = torch.randn(s, s, c, generator=g)
    f1 = torch.randn(2 * s, 2 * s, c // 4, generator=g) * 0.5
    f0 = torch.randn(4 * s, 4 * s, c // 8, generator=g) * 0.5
    return emb, f1, f0


@pytest.mark.parametrize("card,n_side", [("sam2_test", 3), ("sam2", 2)])
def test_mask_decoder_vs_oracle(card, n_side):
    from oracle import sam2_decoder as SD
    from ovo_amd.encoders.sam_decoder import SPECS, HipSamDecoder, random_state
    spec = SPECS[card]
    sd = random_state(spec, seed=2)
    dec = HipSamDecoder(spec, sd, device=DEV)
    pts = dec.set_point_grid(n_side)
    emb, f1, f0 = _inputs(spec)
    masks, iou = dec.forward(emb.to(DEV), f1.to(DEV), f0.to(DEV))
    # oracle: NCHW inputs, the same prompt tokens built by its own point embedding
    labels = torch.ones(pts.shape[0], 1, dtype=torch.long)
    sparse = SD.embed_points(sd, pts.float()[:, None, :], labels, spec.image_size)
    np.testing.assert_allclose(dec.tokens0.reshape(pts.shape[0], -1, spec.hidden)[:, 6:].cpu().numpy(), sparse.numpy(), atol=2e-5, rtol=0)
    rm, ri, _ = SD.mask_decoder(sd, emb.permute(2, 0, 1), f1.permute(2, 0, 1), f0.permute(2, 0, 1), sparse, heads=spec.heads, multimask=True)
    assert masks.shape == rm.shape and iou.shape == ri.shape
    m, r = masks.cpu(), rm
    rms = r.pow(2).mean().sqrt().item()
    err = (m - r).abs().max().item()
    cos = torch.nn.functional.cosine_similarity(m.flatten(1), r.flatten(1), dim=1).min().item()
    agree = ((m > 0) == (r > 0)).float().mean().item()
    print(f"{card}: mask logits max err / rms = {err / rms:.3e}, min cosine = {cos:.6f}, sign agreement = {agree:.5f}, "
          f"iou max err = {(iou.cpu() - ri).abs().max().item():.2e}")
    # bf16 GEMM operands through 2 two-way layers + 2 upscaling stages, fp32 accumulation / residuals / LayerNorm
    assert err / rms < 0.08 and cos > 0.9995 and agree > 0.995
    assert (iou.cpu() - ri).abs().max().item() < 2e-2


def test_mask_decoder_unfused_chain_equals_fused_kernels():
    """The chain the decoder takes at hidden widths the fused out-projection + norm kernel does not cover (ovo_sam_proj_ln returns
    OVO_E_UNSUPPORTED: product, then the row pass, over an f32 residual stream) -- forced here at a covered width -- against the fused path:
    same masks up to the bf16 rounding of the per-prompt keys the fused path keeps (and the unfused one does not)."""
    from ovo_amd.encoders.sam_decoder import SPECS, HipSamDecoder, random_state
    spec = SPECS["sam2_test"]
    sd = random_state(spec, seed=7)
    emb, f1, f0 = (t.to(DEV) for t in _inputs(spec, seed=1))
    outs = []
    for unfused in (False, True):
        dec = HipSamDecoder(spec, sd, device=DEV)
        dec.force_unfused = unfused
        dec.set_point_grid(3)
        outs.append(dec.forward(emb, f1, f0))
    (m0, i0), (m1, i1) = outs
    rms = m0.pow(2).mean().sqrt().item()
    assert torch.isfinite(m1).all() and (m0 - m1).abs().max().item() / rms < 0.05
    assert ((m0 > 0) == (m1 > 0)).float().mean().item() > 0.995 and (i0 - i1).abs().max().item() < 1e-2


def test_mask_decoder_batch_invariance():
    """The generator decodes all clicks in one batch where the reference uses batches of 64: a click's masks must not depend
    on which other clicks share its batch (full-size decoder, 64 clicks at once vs 4 x 16)."""
    from ovo_amd.encoders.sam_decoder import SPECS, HipSamDecoder, point_grid
    spec = SPECS["sam2"]
    dec = HipSamDecoder(spec, None, device=DEV, seed=5)
    emb, f1, f0 = (t.to(DEV) for t in _inputs(spec, seed=4))
    pts = point_grid(8) * spec.image_size
    dec.set_points(pts)
    all_m, all_i = dec.forward(emb, f1, f0)
    for b in range(4):
        dec.set_points(pts[16 * b:16 * b + 16])
        m, i = dec.forward(emb, f1, f0)
        scale = all_m[16 * b:16 * b + 16].abs().max().item()
        assert (m - all_m[16 * b:16 * b + 16]).abs().max().item() <= 1e-5 * scale      # same k-order per output element: equal up to fp32 noise
        assert (i - all_i[16 * b:16 * b + 16]).abs().max().item() <= 1e-6


def test_amg_filters_vs_oracle():
    """Stability / area / box statistics and binarisation on the on-the-fly bilinear upsampling == torch's interpolate.
    (One shape, loose bounds; tests/test_gpu_image_kernels.py pins both kernels exactly at the shapes, thresholds and edges this one leaves out.)"""
    from oracle import sam2_amg as OA
    from oracle.features import masks_to_boxes
    from ovo_amd import _lib as L
    g = torch.Generator().manual_seed(3)
    n, h, w, H, W = 23, 64, 64, 150, 200
    logits = torch.randn(n, h, w, generator=g) * 2.0
    logits = torch.nn.functional.avg_pool2d(logits[None], 5, 1, 2)[0] * 4.0       # smooth blobs, like real logit maps
    logits[5] = -3.0                                                              # an empty mask
    logits[6] = 3.0                                                               # a full mask
    d = logits.to(DEV).contiguous()
    stats = torch.empty((n, 7), dtype=torch.int32, device=DEV)
    L.check(L.load().ovo_amg_mask_stats(L.ptr(d), n, h, w, H, W, 0.0, 1.0, L.ptr(stats), L.stream()))
    st = stats.cpu().numpy()
    up = torch.nn.functional.interpolate(logits[None], (H, W), mode="bilinear", align_corners=False)[0]
    for col, thr in ((0, 1.0), (1, -1.0), (2, 0.0)):
        ref = (up > thr).flatten(1).sum(1).numpy()
        assert np.abs(st[:, col] - ref).max() <= 2, (col, st[:, col], ref)        # a value within an ulp of the threshold may flip
    ref_box = masks_to_boxes((up > 0).numpy())
    ok = st[:, 2] > 0
    assert np.abs(st[ok, 3:7] - ref_box[ok]).max() <= 1
    assert st[5, 2] == 0 and tuple(st[5, 3:7]) == (W, H, -1, -1) and st[6, 2] == H * W
    sel = torch.tensor([6, 0, 9, 5], dtype=torch.int32, device=DEV)
    out = torch.empty((4, H, W), dtype=torch.uint8, device=DEV)
    L.check(L.load().ovo_amg_binarize(L.ptr(d), L.ptr(sel), 4, h, w, H, W, 0.0, L.ptr(out), L.stream()))
    ref = (up[[6, 0, 9, 5]] > 0).numpy()
    assert (out.cpu().numpy().astype(bool) != ref).mean() < 1e-5
    # box NMS restatement agrees with the oracle's pairwise loop
    from ovo_amd.entities.sam_amg import box_nms
    rng = np.random.default_rng(1)
    b = rng.uniform(0, 100, (60, 4)).astype(np.float32)
    b[:, 2:] = b[:, :2] + rng.uniform(5, 60, (60, 2)).astype(np.float32)
    s = rng.uniform(0, 1, 60).astype(np.float32)
    assert np.array_equal(box_nms(b, s, 0.4), OA.box_nms(b, s, 0.4))


def test_automatic_mask_generator_end_to_end():
    """Encoder -> all clicks in one decoder batch -> filters -> NMS -> seg map, against the oracle post-processing applied
    to the device's own logits (the decoder itself is covered above)."""
    from oracle import features as OF, sam2_amg as OA
    from ovo_amd import synthetic as syn
    from ovo_amd.entities.mask_generator import MaskGenerator
    cfg = {"sam_encoder": "hiera_test256", "sam_decoder": "sam2_small", "points_per_side": 6, "nms_iou_th": 0.45, "stability_score_th": 0.32,
           "nms_score_th": 0.2, "nms_inner_th": 0.5, "seed": 1}
    mg = MaskGenerator(cfg, None, device=DEV)
    amg = mg.mask_generator
    amg.box_nms_thresh = 1.0                           # random weights give masks with identical boxes: box NMS would eat them all
                                                       # (the NMS itself is checked in test_amg_filters_vs_oracle)
    H, W = 144, 192
    img = syn.render_rgb(H, W, 2)
    amg.generate_device(img)
    logits, iou = amg.last_logits.cpu().numpy(), amg.last_iou.cpu().numpy()
    assert logits.shape == (36, 3, 64, 64)
    # Integer pixel counts may differ by one or two between the kernel and torch (a logit within an ulp of a threshold), so
    # a candidate sitting ON the stability threshold could legitimately flip: put the threshold in the widest gap of the
    # fixture's own scores, then demand identical selections.
    st = np.sort(OA.amg_postprocess(logits, iou, H, W, 0.0, 0.0)["stab_all"])
    st = st[np.isfinite(st) & (st > 0.2) & (st < 0.6)]
    gap = int(np.argmax(np.diff(st)))
    th = float((st[gap] + st[gap + 1]) / 2)
    assert st[gap + 1] - st[gap] > 2e-3 and np.abs(iou.reshape(-1) - 0.45).min() > 1e-4
    amg.stability_score_thresh = th
    seg_map, bmaps = mg.get_masks(img, 0)
    got = amg.generate_device(img)
    ref = OA.amg_postprocess(logits, iou, H, W, pred_iou_thresh=0.45, stability_score_thresh=th, box_nms_thresh=1.0)
    print(f"stability threshold {th:.4f}: {len(ref['index'])} masks kept of {iou.size} candidates")
    assert len(ref["index"]) >= 3, "fixture keeps too few masks to test anything"
    assert np.array_equal(got["point_index"] * 3 + (ref["index"] % 3), ref["index"]) or np.array_equal(
        np.sort(got["point_index"]), np.sort(ref["index"] // 3))
    gm = got["masks"].cpu().numpy().astype(bool)
    assert gm.shape == ref["masks"].shape and (gm != ref["masks"]).mean() < 1e-5
    np.testing.assert_allclose(got["stability_score"], ref["stability_score"], atol=2e-4)
    np.testing.assert_array_equal(got["predicted_iou"], ref["predicted_iou"])
    # the seg map: NMS (a11) + painting in descending stability, against the oracle's own functions on the same masks
    keep = OF.mask_nms(ref["masks"], ref["stability_score"] * ref["predicted_iou"], 0.45, 0.2, 0.5)
    keep = np.sort(np.asarray(keep))
    ref_seg, ref_maps = OF.paint_segmap(ref["masks"][keep], ref["stability_score"][keep])
    assert np.array_equal(seg_map.cpu().numpy(), ref_seg)
    assert np.array_equal(bmaps.cpu().numpy(), ref_maps)
    assert seg_map.dtype == torch.int32 and bmaps.dtype == torch.bool and seg_map.is_cuda


def test_generator_small_region_cleanup():
    """`min_mask_region_area > 0` (segment_utils.py:283,300: the SAM1 default is 100) through the whole generator: the kept masks are what
    `postprocess_small_regions` makes of the masks the same generator keeps with the clean-up off (tests/test_amg_small_regions.py checks
    that function against a flood fill), records stay aligned, no kept mask has an island or a hole below the threshold."""
    from scipy import ndimage
    from ovo_amd import synthetic as syn
    from ovo_amd.entities.mask_generator import MaskGenerator
    from ovo_amd.entities.sam_amg import postprocess_small_regions
    cfg = {"sam_encoder": "hiera_test256", "sam_decoder": "sam2_small", "points_per_side": 6, "nms_iou_th": 0.0, "stability_score_th": 0.0,
           "nms_score_th": 0.2, "nms_inner_th": 0.5, "seed": 1}
    img = syn.render_rgb(144, 192, 2)
    off = MaskGenerator(cfg, None, device=DEV).mask_generator
    on = MaskGenerator(dict(cfg, min_mask_region_area=60), None, device=DEV).mask_generator
    for g in (off, on):
        g.box_nms_thresh, g.pred_iou_thresh = 1.0, -1.0            # random weights give masks with identical boxes: box NMS would eat them all
    a, b = off.generate_device(img), on.generate_device(img)
    assert on.min_mask_region_area == 60 and len(a["masks"]) >= 3
    masks, boxes, keep, changed = postprocess_small_regions(a["masks"].cpu().numpy().astype(bool), a["boxes_xyxy"], 60, 1.0)
    got = b["masks"].cpu().numpy().astype(bool)
    assert got.shape == masks.shape and np.array_equal(got, masks) and np.array_equal(b["boxes_xyxy"], boxes)
    np.testing.assert_array_equal(b["predicted_iou"], a["predicted_iou"][keep])
    np.testing.assert_array_equal(b["point_index"], a["point_index"][keep])
    assert np.array_equal(b["area"][changed], got[changed].reshape(int(changed.sum()), -1).sum(1))
    eight = np.ones((3, 3), bool)
    for m in got:
        for work in (m, ~m):
            lab, n = ndimage.label(work, structure=eight)
            sizes = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
            assert n <= 1 or sizes.min() >= 60 or (work is m and n == 1), sizes
    print(f"small-region clean-up: {len(a['masks'])} -> {len(got)} masks, {int(changed.sum())} changed")


def test_full_size_generator_feeds_tracking_640x480():
    """Row f1 at the benchmark's size: hiera_b+ encoder @1024^2 + the full SAM2 decoder on a 16 x 16 click grid (768 candidates) on a
    640 x 480 frame, generator filters, box NMS, mask NMS and seg-map painting -- against the oracle post-processing of the device's own
    logits -- and then the hand-over the reference makes (mask_generator.py:102-120 -> ovo.py:121-166): the NATIVE masks drive the
    tracker on a point map, whose per-point instance ids must equal the oracle tracker's on the same masks, bit for bit.
    Random-init SAM2 keeps nothing at the reference's thresholds (0.8 / 0.95), so the two score thresholds are placed in gaps of this
    fixture's own score distributions such that >= 16 masks survive; everything else is the reference's setting."""
    from oracle import features as OF, sam2_amg as OA, semantic as OS
    from ovo_amd import synthetic as syn
    from ovo_amd.entities.mask_generator import MaskGenerator
    from ovo_amd.entities.ovo import OVO
    from ovo_amd.slam.vanilla_mapper import VanillaMapper
    cfg = {"sam_encoder": "hiera_b+", "sam_decoder": "sam2", "points_per_side": 16, "nms_iou_th": 0.8, "stability_score_th": 0.95,
           "nms_score_th": 0.0, "nms_inner_th": 0.5, "seed": 2}
    mg = MaskGenerator(cfg, None, device=DEV)
    amg = mg.mask_generator
    amg.box_nms_thresh = 1.0                           # random weights: near-identical boxes (box NMS itself: test_amg_filters_vs_oracle)
    scale = 1.0
    h, w = syn.scannet_depth_hw(scale)
    e = syn.SCANNET["crop_edge"]
    H, W = h + 2 * e, w + 2 * e
    assert (H, W) == (480, 640)
    fid, rgb_lr, depth, c2w = syn.frame(2, scale=scale, seed=9)
    rgb = syn.render_rgb(H, W, 9)
    amg.generate_device(rgb)
    logits, iou = amg.last_logits.cpu().numpy(), amg.last_iou.cpu().numpy()
    assert logits.shape == (256, 3, 256, 256)
    post = OA.amg_postprocess(logits, iou, H, W, 0.0, 0.0)
    # thresholds in gaps of the fixture's own scores: predicted IoU around its median, stability so that >= 16 of those survive
    pi = np.sort(iou.reshape(-1))
    k = len(pi) // 2 + int(np.argmax(np.diff(pi[len(pi) // 2: len(pi) // 2 + 60])))
    th_iou = float((pi[k] + pi[k + 1]) / 2)
    st = np.sort(post["stab_all"][(iou.reshape(-1) > th_iou) & np.isfinite(post["stab_all"])])
    assert len(st) > 40
    cut = len(st) - 24                                 # keep roughly the 24 most stable candidates
    j = cut - 10 + int(np.argmax(np.diff(st[cut - 10: cut + 4])))
    th_st = float((st[j] + st[j + 1]) / 2)
    assert st[j + 1] - st[j] > 1e-4
    amg.pred_iou_thresh, amg.stability_score_thresh = th_iou, th_st
    mg.nms_iou_th, mg.nms_inner_th = 1.01, 0.0         # mask NMS (a11): random-weight masks are near copies of each other; the rule runs
                                                       # (and is compared with the oracle's) but suppresses nothing
    seg_map, bmaps = mg.get_masks(rgb, 0)
    got = amg.generate_device(rgb)
    ref = OA.amg_postprocess(logits, iou, H, W, pred_iou_thresh=th_iou, stability_score_thresh=th_st, box_nms_thresh=1.0)
    print(f"640x480: thresholds iou {th_iou:.4f} / stability {th_st:.4f}: {len(ref['index'])} of {iou.size} candidates kept, {bmaps.shape[0]} after mask NMS")
    assert len(ref["index"]) >= 16
    assert np.array_equal(np.sort(got["point_index"]), np.sort(ref["index"] // 3))
    gm = got["masks"].cpu().numpy().astype(bool)
    assert gm.shape == ref["masks"].shape and (gm != ref["masks"]).mean() < 1e-5
    keep = np.sort(np.asarray(OF.mask_nms(ref["masks"], ref["stability_score"] * ref["predicted_iou"], 1.01, 0.0, 0.0)))
    ref_seg, ref_maps = OF.paint_segmap(ref["masks"][keep], ref["stability_score"][keep])
    if not np.array_equal(gm, ref["masks"]):           # a logit within an ulp of 0 flipped a pixel: compare the hand-over on the device's masks
        keep = np.sort(np.asarray(OF.mask_nms(gm, got["stability_score"] * got["predicted_iou"], 1.01, 0.0, 0.0)))
        ref_seg, ref_maps = OF.paint_segmap(gm[keep], got["stability_score"][keep])
    assert np.array_equal(seg_map.cpu().numpy(), ref_seg) and np.array_equal(bmaps.cpu().numpy(), ref_maps)
    assert bmaps.shape[0] >= 8
    # ---- the native masks drive the tracker (two keyframes), ids bit-exact against the oracle tracker on the same masks
    K = syn.scannet_intrinsics(scale)
    Kd = torch.from_numpy(K).to(DEV)

    class Native:                                      # what OVO._get_masks calls: the generator above, per frame
        def get_masks(self, image, frame_id):
            return mg.get_masks(image, frame_id)

    class Clip:
        clip_dim = 32
    # depth_filter off: the Gaussian high-pass is float arithmetic whose last bit differs between the two sides, and a depth pixel ON its
    # threshold flips one match (the filter has its own test with a tolerance, test_gpu_geometry.py); everything else is integer-exact
    ocfg = {"match_distance_th": 0.05, "track_th": 100, "depth_filter": False, "clip": {"k_top_views": 0, "fusion": "avg_pooling"}, "sam": {}}
    ovo = OVO(ocfg, None, None, Kd, device=DEV, clip_generator=Clip(), mask_generator=Native())
    vm = VanillaMapper({"device": DEV, "mapping": {}}, Kd)
    pm, tr = OS.PointMap(K), OS.SemanticTracker(K, 0.05, 100, False, 0)
    n_inst = 0
    for t in (2, 3):
        fid, rgb_lr, depth, c2w = syn.frame(t, scale=scale, seed=9)
        img = rgb                                      # the thresholds above were placed for THIS image's candidates
        fd = [fid, rgb_lr, depth, c2w]
        vm.track_camera(fd)
        vm.map(fd, vm.get_c2w(fid))
        pm.integrate(rgb_lr, depth, c2w)
        assert np.array_equal(vm.pcd.cpu().numpy(), pm.xyz)
        upd = ovo.detect_and_track_objects([fid, img, depth, (1.0, 1.0, e)], vm.get_map(), vm.get_c2w(fid))
        seg_t, maps_t = mg.get_masks(img, fid)         # the same masks, for the oracle tracker
        matched, _, _, ref_ids = tr.step(depth, (1.0, 1.0, e), pm.xyz, pm.ids, pm.ins, c2w, seg_t.cpu().numpy(), maps_t.cpu().numpy())
        pm.ins = ref_ids
        vm.update_pcd_obj_ids(upd)
        assert np.array_equal(upd.cpu().numpy().reshape(-1), ref_ids.reshape(-1)), f"instance ids differ at frame {t}"
        n_inst = len(ovo.objects)
    print(f"native masks -> {n_inst} instances, {int((pm.ins >= 0).sum())} labelled points")
    assert n_inst >= 1 and int((pm.ins >= 0).sum()) > 1000, "the native masks labelled too few points to mean anything"


@pytest.mark.parametrize("enc_card", ["hiera_l"])
def test_generator_vs_full_fp32_oracle_chain(enc_card):
    """What the encoder's bf16 error (3-4 % of the feature rms at its worst element, test_gpu_hiera.py) does DOWNSTREAM, at the reference's
    default trunk (hiera_l, ovo.yaml:35) and frame size: the whole device chain -- resize, Hiera-L + FPN @1024^2, prompt encoder, mask decoder,
    generator filters, seg map -- against the whole chain in fp32 on the CPU (oracle/hiera.py -> oracle/sam2_decoder.py -> oracle/sam2_amg.py) on
    the same frame, weights and clicks (a 4 x 4 grid: the CPU decoder's cost is per click).  Mask logits agree in sign on > 99 % of the pixels,
    predicted IoUs to 2e-2; with the two score thresholds placed where BOTH chains' score lists have a gap, the two chains keep the same
    candidates, the kept masks overlap (IoU) > 0.97 and the painted seg maps agree on > 97 % of the pixels."""
    from oracle import hiera as OH, sam2_amg as OA, sam2_decoder as SD, vit as OV
    from oracle import features as OF
    from ovo_amd import synthetic as syn
    from ovo_amd.encoders import hiera as EH
    from ovo_amd.encoders.sam_decoder import SPECS as DS, HipSamDecoder, point_grid, random_state as dec_state
    from ovo_amd.entities.sam_amg import HipSam2AutomaticMaskGenerator
    es, ds = EH.SPECS[enc_card], DS["sam2"]
    sd_e, sd_d = EH.random_state(es, seed=3), dec_state(ds, seed=4)
    enc, dec = EH.HipHiera(es, sd_e, device=DEV), HipSamDecoder(ds, sd_d, device=DEV)
    amg = HipSam2AutomaticMaskGenerator(enc, dec, points_per_side=4, pred_iou_thresh=0.0, stability_score_thresh=0.0, box_nms_thresh=1.0)
    H, W = 480, 640
    rgb = syn.render_rgb(H, W, 5)
    amg.generate_device(rgb)
    logits, iou = amg.last_logits.cpu(), amg.last_iou.cpu()
    assert logits.shape == (16, 3, 256, 256)
    # ---- the same chain in fp32 on the CPU
    x = OV.resize_normalize(torch.from_numpy(rgb.transpose(2, 0, 1).copy()), es.image_size, EH.IMAGENET_MEAN, EH.IMAGENET_STD, None, 1 / 255.0)
    f0, f1, f2 = OH.hiera_forward(sd_e, x[None], stages=es.stages, heads=es.heads, window_spec=es.window_spec, global_blocks=es.global_blocks, hi_res=True)
    pts = point_grid(4) * ds.image_size
    sparse = SD.embed_points(sd_d, pts.float()[:, None, :], torch.ones(pts.shape[0], 1, dtype=torch.long), ds.image_size)
    rm, ri, _ = SD.mask_decoder(sd_d, f2[0].permute(2, 0, 1), f1[0].permute(2, 0, 1), f0[0].permute(2, 0, 1), sparse, heads=ds.heads, multimask=True)
    rms = rm.pow(2).mean().sqrt().item()
    agree = ((logits > 0) == (rm > 0)).float().mean().item()
    cos = torch.nn.functional.cosine_similarity(logits.flatten(1), rm.flatten(1), dim=1).min().item()
    d_iou = (iou - ri).abs().max().item()
    print(f"{enc_card} chain: logits max err / rms = {(logits - rm).abs().max().item() / rms:.3e}, min cosine {cos:.5f}, sign agreement {agree:.5f}, iou max err {d_iou:.2e}")
    assert agree > 0.99 and cos > 0.995 and d_iou < 2e-2
    # ---- consequences: selections, masks, seg map
    dev_all = OA.amg_postprocess(logits.numpy(), iou.numpy(), H, W, 0.0, 0.0)
    ref_all = OA.amg_postprocess(rm.numpy(), ri.numpy(), H, W, 0.0, 0.0)

    def joint_gap(a, b, lo_q, hi_q):                     # a threshold both score lists stay clear of (by more than the chains' disagreement)
        v = np.sort(np.concatenate([a[np.isfinite(a)], b[np.isfinite(b)]]))
        v = v[int(lo_q * len(v)): int(hi_q * len(v))]
        k = int(np.argmax(np.diff(v)))
        return float((v[k] + v[k + 1]) / 2), float(v[k + 1] - v[k])
    th_iou, g1 = joint_gap(iou.numpy().reshape(-1), ri.numpy().reshape(-1), 0.3, 0.6)
    th_st, g2 = joint_gap(dev_all["stab_all"], ref_all["stab_all"], 0.2, 0.7)
    dev = OA.amg_postprocess(logits.numpy(), iou.numpy(), H, W, pred_iou_thresh=th_iou, stability_score_thresh=th_st, box_nms_thresh=1.0)
    ref = OA.amg_postprocess(rm.numpy(), ri.numpy(), H, W, pred_iou_thresh=th_iou, stability_score_thresh=th_st, box_nms_thresh=1.0)
    print(f"thresholds iou {th_iou:.4f} (gap {g1:.1e}) / stability {th_st:.4f} (gap {g2:.1e}): device chain keeps {len(dev['index'])}, fp32 chain {len(ref['index'])} of 48")
    assert len(ref["index"]) >= 4, "fixture keeps too few masks to test anything"
    assert sorted(dev["index"].tolist()) == sorted(ref["index"].tolist())
    order_d, order_r = np.argsort(dev["index"]), np.argsort(ref["index"])
    md, mr = dev["masks"][order_d], ref["masks"][order_r]
    inter, union = (md & mr).reshape(len(md), -1).sum(1), (md | mr).reshape(len(md), -1).sum(1)
    ious = inter / np.maximum(union, 1)
    print(f"kept masks: IoU device vs fp32 chain min {ious.min():.4f} mean {ious.mean():.4f}")
    assert ious.min() > 0.97
    seg_d, _ = OF.paint_segmap(md, dev["stability_score"][order_d])
    seg_r, _ = OF.paint_segmap(mr, ref["stability_score"][order_r])
    # (painting order = descending stability; the two chains' scores differ in the 3rd digit, so the ORDER of near-ties may differ: compare coverage)
    same_cover = ((seg_d >= 0) == (seg_r >= 0)).mean()
    print(f"seg map: labelled-pixel agreement {same_cover:.4f}")
    assert same_cover > 0.97
