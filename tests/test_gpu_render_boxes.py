"""-m gpu: `ovo_render_boxes` (csrc/render.hip; include/ovo_hip.h has the contract) against its f64 restatement (tests/box_restatement.py).

The kernel evaluates the restatement's expressions in f32.  A pixel is left out of a comparison only if the REFERENCE says it is a knife edge -- its
f64 distance to some edge within 1e-3 px of half_width, or its two nearest covering boxes within 1e-4 relative in depth -- and at most 4 pixels per
case may be, which is asserted from the reference before the GPU result is looked at.  Everywhere else `out_id` is equal and `out_depth` is within
1e-4 relative (both sides evaluate one short expression on values near 1: some hundred f32 ulps of slack).

The scene: a 48 x 64 view from `render_restatement.general_pose()`, five boxes given in the camera frame and moved to the world -- two in view, one
crossing the near plane, one partly off the image, one behind the camera -- every coordinate jittered by default_rng(3).uniform(-0.03, 0.03) (the
un-jittered boxes put edges at exactly v = 8.5 and v = 42.25, which ties hundreds of pixels at half_width 0.5 and 0.75)."""
import functools

import numpy as np
import pytest
import torch

import box_restatement as BR
import render_restatement as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, NEAR = 48, 64, 0.05
NOMINAL = (((-.6, -.4, 1.4), (.1, .3, 2.2)), ((.2, -.5, 1.), (.9, .1, 1.6)), ((-.3, -.2, -.4), (.3, .25, .8)), ((-2.5, -.3, 1.2), (-.9, .6, 2.)),
           ((-.2, -.2, -2.), (.2, .2, -1.)))
MAX_LEFT_OUT, DEPTH_RTOL = 4, 1e-4


def _to_world(cam_points):
    c2w = RR.general_pose().astype(np.float64)
    return (np.asarray(cam_points, np.float64) @ c2w[:3, :3].T + c2w[:3, 3]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _scene():
    """corners f32[5,8,3] in the world: the five jittered boxes."""
    boxes = np.array(NOMINAL, np.float64) + np.random.default_rng(3).uniform(-0.03, 0.03, (5, 2, 3))
    corners = _to_world(np.stack([BR.corners_of(lo, hi) for lo, hi in boxes]))
    corners.setflags(write=False)
    return corners


def _view(h=H, w=W):
    from ovo_amd.utils import render_utils as R
    return R.make_view(RR.general_pose(), RR.K_SMALL, h, w, near=NEAR)


def _gpu(corners, ids, view, half_width, scene=None, slack=0.0):
    from ovo_amd.utils import render_utils as R
    out_id, out_depth = R.render_boxes(torch.from_numpy(np.array(corners, np.float32)).reshape(-1, 8, 3).to(DEV),
                                       torch.from_numpy(np.asarray(ids, np.int32)).to(DEV), view, half_width=half_width, scene_depth=scene, depth_slack=slack)
    torch.cuda.synchronize()
    return out_id.cpu().numpy(), out_depth.cpu().numpy()


def _reference(corners, ids, view, half_width, scene=None, slack=0.0):
    ref = BR.render(corners, ids, np.array(view.w2c, np.float32).reshape(4, 4), RR.K_SMALL, int(view.h), int(view.w), NEAR, half_width,
                    scene=None if scene is None else scene.cpu().numpy(), slack=slack)
    ref["left_out"] = ref["knife"] | ref["tie"]
    assert int(ref["left_out"].sum()) <= MAX_LEFT_OUT, f"{int(ref['left_out'].sum())} knife-edge pixels: the case does not decide enough"
    return ref


def _compare(got, ref, what=""):
    out_id, out_depth = got
    keep = ~ref["left_out"]
    assert out_id.dtype == np.int32 and out_depth.dtype == np.float32 and out_id.shape == ref["id"].shape
    bad = keep & (out_id != ref["id"])
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ in id, e.g. {np.argwhere(bad)[:5].tolist()}"
    err = np.abs(out_depth.astype(np.float64) - ref["depth"])
    print(f"{what}: {int((ref['id'] >= 0).sum())} covered pixels, {int(ref['left_out'].sum())} left out, "
          f"largest relative depth error {float((err / np.maximum(ref['depth'], 1e-30))[keep].max()):.3e}")
    assert (err[keep] <= DEPTH_RTOL * ref["depth"][keep]).all(), what
    assert (out_depth[out_id == -1] == 0).all() and (out_depth[out_id != -1] > 0).all()


# ---------------------------------------------------------------------------------------------------- the scene
@pytest.mark.parametrize("half_width", [0.5, 1.0, 1.5])
def test_five_boxes(half_width):
    ids = [0, 1, 2, 3, 4]
    view = _view()
    ref = _reference(_scene(), ids, view, half_width)
    assert ref["covered"][4] == 0 and (ref["covered"][:4] > 20).all()                      # behind the camera: nothing; the other four all show
    assert set(np.unique(ref["id"])) == {-1, 0, 1, 2, 3}
    _compare(_gpu(_scene(), ids, view, half_width), ref, f"half_width {half_width}")


def test_box_ids_are_values_not_indices():
    ids = [1000, -5, 7, 7, 123456]
    view = _view()
    ref = _reference(_scene(), ids, view, 1.0)
    assert set(np.unique(ref["id"])) == {-1, -5, 7, 1000}
    _compare(_gpu(_scene(), ids, view, 1.0), ref, "ids")


def test_no_boxes():
    out_id, out_depth = _gpu(np.zeros((0, 8, 3), np.float32), [], _view(), 1.0)
    assert out_id.shape == (H, W) and (out_id == -1).all() and (out_depth == 0).all()


# ---------------------------------------------------------------------------------------------------- occlusion
def test_edges_behind_the_scene_are_hidden():
    """A wall of points at camera z = 1.8 with a hole: edges behind it are hidden, except through the hole and where no point landed."""
    from ovo_amd.utils import render_utils as R
    x, y = np.meshgrid(np.linspace(-1.4, 1.4, 141), np.linspace(-1.1, 1.1, 111))
    wall = np.stack([x.ravel(), y.ravel(), np.full(x.size, 1.8)], 1)
    wall = wall[~((np.abs(wall[:, 0] + 0.35) < 0.25) & (np.abs(wall[:, 1]) < 0.5))]        # the hole, in front of the first box
    view = _view()
    rows_view = R.make_view(RR.general_pose(), RR.K_SMALL, H, W, radius=0, near=NEAR)
    scene = R.render_rows(torch.from_numpy(_to_world(wall)).to(DEV), rows_view)[1]
    sc = scene.cpu().numpy()
    assert 0.05 < (sc == 0).mean() < 0.4 and np.abs(sc[sc > 0] - 1.8).max() < 1e-3
    ids, slack = [0, 1, 2, 3, 4], 0.02
    free = _reference(_scene(), ids, view, 1.0)
    ref = _reference(_scene(), ids, view, 1.0, scene=scene, slack=slack)
    behind = (free["depth"] > 1.8 + slack + 1e-3)
    assert (behind & (sc > 0)).sum() > 30 and (ref["id"][behind & (sc > 0)] != free["id"][behind & (sc > 0)]).all()          # hidden behind the wall ...
    assert (behind & (sc == 0)).sum() > 10 and np.array_equal(ref["id"][sc == 0], free["id"][sc == 0])                        # ... and seen through its holes
    assert (ref["id"] == 1).sum() > 50                                                      # the box in front of the wall is untouched
    _compare(_gpu(_scene(), ids, view, 1.0, scene=scene, slack=slack), ref, "occluded")


# ---------------------------------------------------------------------------------------------------- more than one LDS chunk
def test_forty_small_boxes():
    rng = np.random.default_rng(26)                                 # (a seed whose scene has no knife-edge pixel in the REFERENCE: 480 short edges graze many)
    centre = np.stack([rng.uniform(-0.7, 0.7, 40), rng.uniform(-0.5, 0.5, 40), rng.uniform(1.0, 3.0, 40)], 1)
    half = rng.uniform(0.02, 0.05, (40, 3))
    corners = _to_world(np.stack([BR.corners_of(c - s, c + s) for c, s in zip(centre, half)]))
    ids = (np.arange(40) * 3 + 100).tolist()
    view = _view()
    ref = _reference(corners, ids, view, 0.75)
    assert len(np.unique(ref["id"])) > 30 and (ref["covered"] > 0).all()
    _compare(_gpu(corners, ids, view, 0.75), ref, "40 boxes")


# ---------------------------------------------------------------------------------------------------- image sizes, repeated launch
def _with_corner_box():
    """The five boxes and a small one on the ray through pixel (0, 0)."""
    c = np.array([(0 - 31.5) / 60.0, (0 - 23.5) / 60.0, 1.0]) * 1.5
    return np.concatenate([_scene(), _to_world(BR.corners_of(c - 0.013, c + 0.017)[None])]), [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("h,w", [(1, 1), (37, 53)])
def test_image_sizes(h, w):
    corners, ids = _with_corner_box()
    view = _view(h, w)
    ref = _reference(corners, ids, view, 1.0)
    assert ref["id"][0, 0] == 5
    got = _gpu(corners, ids, view, 1.0)
    assert got[0].shape == (h, w)
    _compare(got, ref, f"{h} x {w}")


def test_repeated_launch_is_bit_identical():
    view = _view()
    a, b = _gpu(_scene(), [0, 1, 2, 3, 4], view, 1.5), _gpu(_scene(), [0, 1, 2, 3, 4], view, 1.5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
