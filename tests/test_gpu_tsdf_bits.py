"""-m gpu: the fused TSDF model gives the bits recorded in tests/golden/tsdf_digests.json (written by tools/gen_tsdf_digests.py with the library as it was
BEFORE a change that must not move any of them; the test compares with the file, never with the code under test).  The other TSDF tests pin integrate,
ray-cast depth and colour and the mesh to the restatements, normals to within 4 d32n of the f64 form; this one pins every output of every kernel form
to yesterday's bits.  The cases are those of test_gpu_tsdf, test_gpu_tsdf_color, test_gpu_tsdf_normal and test_gpu_mesh, imported from them:
  integrate   (F, W) and the colour array after all frames, ovo_tsdf_integrate and ovo_tsdf_integrate_color, the frustum boxes and given boxes over a
              volume that already holds something, each with the default grid and with OVO_TSDF_GRID_CAP=2
  raycast     depth, rgb and normals of all four kernel forms
  mesh        vertices, faces, colours, normals and (V, T), each with the default grid and with OVO_MESH_GRID_CAP=2
and, with the cases of test_gpu_tsdf_labels, test_gpu_tsdf_sample and test_gpu_sdf_align (whose own comparisons leave an undecided set, or a multiple of d32):
  integrate labels   `lab` after the four frames of a vote case, with the default grid and with OVO_TSDF_GRID_CAP=2
  raycast labels     depth and the instance image of ovo_tsdf_raycast_labels
  mesh labels        the label vector at min_count 1 and 3, with the default grid and with OVO_MESH_GRID_CAP=2
  sample             every output of all twelve forms of k_tsdf_sample_points over the 4099 generated points, at every min_count of the case
  align volume       words 1 .. 39 of the result block (everything but the sequence word) and the device pose: one iteration on one level and a whole
                     two-level alignment of the 57 x 77 room case, and the 2x2x2 edge case level by level (its coarsest level is 3 x 3), each with the default
                     grid and with OVO_ICP_GRID_CAP=2
Every case asserts that what it digests is not degenerate (voxels updated, pixels hit, vertices emitted) and that every output was written."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_tsdf as G  # noqa: E402
import test_gpu_tsdf_color as GC  # noqa: E402
import test_gpu_sdf_align as GA  # noqa: E402
import test_gpu_tsdf_labels as GL  # noqa: E402
import test_gpu_tsdf_normal as GN  # noqa: E402
import test_gpu_tsdf_sample as GS  # noqa: E402
import test_tsdf_labels_host as HL  # noqa: E402
import test_tsdf_normal_host as H  # noqa: E402
import test_tsdf_sample_host as HS  # noqa: E402
import tsdf_restatement as T  # noqa: E402

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tsdf_digests.json")

# ovo_tsdf_integrate's three boxes of test_integrate_touches_nothing_outside_its_box and ovo_tsdf_integrate_color's two that differ from them.  98 is even and
# (31, 75) are both odd: that box has half a 16-byte pair at each end of every row; 33 is odd: the V = 1 kernel.
BOXED = [("room57", ((31, 5, 41), (75, 40, 90))), ("33x17x9", ((3, 2, 1), (30, 16, 8))), ("room57", ((60, 0, 50), (61, 40, 60))),
         ("room57", ((31, 5, 41), (76, 40, 90))), ("room57", ((61, 0, 50), (62, 40, 60)))]
INTEGRATE = ["2x2x2", "5x3x2", "33x17x9", "room57"]
MESH = ["5x3x2", "33x17x9", "sphere", "holes", "box", "cell 17", "cell 69"]

CASES = [("integrate", name, None, cap) for name in INTEGRATE for cap in (0, 2)]
CASES += [("integrate", name, box, cap) for name, box in BOXED for cap in (0, 2)]
CASES += [("raycast", name, None, 0) for name in H.RAYCAST_CASES]
CASES += [("mesh", name, None, cap) for name in MESH for cap in (0, 2)]
ALIGN = ["room57 one iteration", "room57 two levels", "2x2x2"]
CASES += [("integrate labels", name, None, cap) for name in INTEGRATE for cap in (0, 2)]
CASES += [("raycast labels", name, None, 0) for name in HL.RAYCASTS]
CASES += [("mesh labels", name, None, cap) for name in MESH for cap in (0, 2)]
CASES += [("sample", name, None, 0) for name in INTEGRATE]
CASES += [("align volume", name, None, cap) for name in ALIGN for cap in (0, 2)]


def case_id(case):
    kind, name, box, cap = case
    return f"{kind} {name}" + ("" if box is None else " box %d-%d" % (box[0][0], box[1][0])) + (f" cap {cap}" if cap else "")


def _digest(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _integrate(name, box):
    sp, frames, rgbs, boxes, *_ = GC.restated(name)
    nx, ny, nz = sp["dims"]
    assert box is not None or len(frames) == 3
    if box is None:
        start, zero_c = None, np.zeros((nz, ny, nx, 4), dtype=np.uint16)
        start_v = np.zeros((nz, ny, nx, 2), dtype=np.float32)
    else:                                                    # a volume that already holds something, as the boxed tests make it
        frames, rgbs, boxes = frames[:1], rgbs[:1], [box]
        rng = np.random.default_rng(5)
        start_v = np.stack([rng.uniform(-1, 1, (nz, ny, nx)), rng.integers(0, 3, (nz, ny, nx))], -1).astype(np.float32)
        zero_c = np.minimum(rng.integers(0, 65536, (nz, ny, nx, 4)), [65280, 65280, 65280, 65535]).astype(np.uint16)
        start = (start_v, zero_c)
    plain, _ = G.run_integration(sp, frames, boxes, None if box is None else start_v)
    vol, col = GC.run_integration(sp, frames, rgbs, boxes, start)
    changed = (G.bits(plain) != G.bits(start_v)).any(-1)
    print(f"  {int(changed.sum())} of {changed.size} voxels updated, {int((col != zero_c).any(-1).sum())} colours changed")
    assert changed.any() and (col[..., :3] != zero_c[..., :3]).any()
    assert np.array_equal(G.bits(vol), G.bits(plain))        # (what test_gpu_tsdf_color asserts: one digest would do, two say which kernel moved)
    return {"plain vol": _digest(plain), "color vol": _digest(vol), "color col": _digest(col)}


def _raycast(name):
    sp, vol32, cam, dz, expect = H.raycast_case(name)
    col = GN.case_colors(name, sp)
    vol, _, _ = GC.color_volume(sp, vol32, col)
    h, w = cam["h"], cam["w"]
    K, c2w = G.cam_args(cam)
    view = (K, h, w, c2w, float(cam["near"]), float(cam["far"]), dz)
    rec = {}
    for form, color, normals in (("plain", False, False), ("color", True, False), ("normals", False, True), ("color normals", True, True)):
        out = torch.full((h, w), -7.0, dtype=torch.float32, device=DEV)
        out_c = torch.full((h, w, 3), 0x7B, dtype=torch.uint8, device=DEV) if color else None
        out_n = torch.full((h, w, 3), -7.0, dtype=torch.float32, device=DEV) if normals else None
        vol.raycast(*view, out=out, color=color, out_rgb=out_c, normals=normals, out_normals=out_n)
        torch.cuda.synchronize()
        hit = out > 0
        assert bool((out >= 0).all()) and (bool(hit.any()) or expect not in ("hits", "plane"))      # every pixel written; a surface is seen where there is one
        rec[form + " depth"] = _digest(out)
        if color:
            assert bool((out_c[~hit] == 0).all()) and bool(out_c[hit].any()) == bool(hit.any())
            rec[form + " rgb"] = _digest(out_c)
        if normals:
            assert bool((out_n[~hit] == 0).all()) and bool((out_n[hit] != 0).any()) == bool(hit.any())
            rec[form + " normals"] = _digest(out_n)
    print(f"  {int(hit.sum())} of {h * w} pixels hit")
    return rec


def _mesh(name):
    sp, vol32, col, box, mw, want_v, _ = GC.mesh_colors_case(name)
    vol, _, _ = GC.color_volume(sp, vol32, col)
    v, f, c, n = vol.extract_mesh(box=box, min_weight=mw, colors=True, normals=True)
    torch.cuda.synchronize()
    print(f"  V {len(v)}, T {len(f)}")
    assert len(v) == len(want_v) >= 1 and len(f) >= 1 and len(c) == len(n) == len(v)
    assert bool(torch.isfinite(v).all()) and int(f.min()) == 0 and int(f.max()) == len(v) - 1 and bool(c.any()) and bool((n != 0).any())
    return {"V": len(v), "T": len(f), "vertices": _digest(v), "faces": _digest(f), "colors": _digest(c), "normals": _digest(n)}


def _integrate_labels(name):
    sp, frames, *_ = HL.vote_case(name)
    lab = GL.run_votes(sp, frames)
    print(f"  {int((lab[..., 0] > 0).sum())} of {lab[..., 0].size} voxels hold a label")
    assert lab.dtype == np.int32 and (lab[..., 0] > 0).any()
    return {"lab": _digest(lab)}


def _raycast_labels(name):
    sp, vol32, lab, cam, dz, expect = HL.raycast_case(name)
    vol, _, _ = GL.label_volume(sp, vol32, lab)
    h, w = cam["h"], cam["w"]
    K, c2w = G.cam_args(cam)
    out = torch.full((h, w), -7.0, dtype=torch.float32, device=DEV)
    out_i = torch.full((h, w), 0x7B7B, dtype=torch.int32, device=DEV)
    vol.raycast(K, h, w, c2w, float(cam["near"]), float(cam["far"]), dz, out=out, labels=True, out_ins=out_i)
    torch.cuda.synchronize()
    hit = out > 0
    print(f"  {int(hit.sum())} of {h * w} pixels hit, {int((out_i >= 0).sum())} labelled")
    assert bool((out >= 0).all()) and bool((out_i != 0x7B7B).all()) and bool((out_i[~hit] == -1).all())      # every pixel written
    assert bool((out_i[hit] >= 0).any()) or expect not in ("hits", "plane")                                  # a labelled pixel where there is a surface
    return {"depth": _digest(out), "ins": _digest(out_i)}


def _mesh_labels(name):
    sp, vol32, lab, box, mw, want1, _ = GL.mesh_labels_case(name)
    run = GL.Run(sp, vol32, lab, box, mw)
    assert run.plan() == len(want1) >= 1
    got1, got3 = run.labels(1).copy(), run.labels(3).copy()
    print(f"  V {run.V}, {int((got1 >= 0).sum())} labelled at min_count 1, {int((got3 >= 0).sum())} at 3")
    assert run.guards() and (got1 >= -1).all() and (name.startswith("cell") or (got1 >= 0).any())      # (a single cell's few vertices may all lack a label)
    return {"V": run.V, "ins min_count 1": _digest(got1), "ins min_count 3": _digest(got3)}


def _sample(name):
    V, points, _, _ = GS.gpu_case(name)
    n = len(points)
    pts, _ = GS.guarded_points(points)
    rec = {}
    for normals in (False, True):
        for colors in (False, True):
            for mode in (None, 0, 1):                        # no labels, the nearest corner, the vote: 2 x 2 x 3 kernel forms
                for mc in HS.MIN_COUNTS[name] if mode is not None else (1,):
                    rc, out = GS.call(V, pts, n, normals, colors, mode is not None, mode or 0, mc)
                    assert rc == 0
                    f, nrm, rgb, ins = out.read()
                    assert (f == 2.0).any() and (f < 2.0).any()      # some point is seen and some is not
                    form = ("normals " if normals else "") + ("colour " if colors else "") + ("" if mode is None else f"{('nearest', 'vote')[mode]} min_count {mc} ")
                    rec[form + "f"] = _digest(f)
                    if normals:
                        rec[form + "normals"] = _digest(nrm)
                    if colors:
                        rec[form + "rgb"] = _digest(rgb)
                    if mode is not None:
                        rec[form + "ins"] = _digest(ins)
    assert V.untouched()
    return rec


def _align_volume(name):
    from ovo_amd.utils import icp_utils as U
    if name == "2x2x2":                                      # the levels one at a time, as test_shapes_at_the_edge runs them: the coarsest is 3 x 3
        sp, vol32, K, depth, T0, levels, _ = GA.edge_case(name)
        assert levels == 2 and tuple(s // 2 for s in depth.shape) == (3, 3)
        runs = [(f"level {level} ", GA.one_level(levels, level), 1) for level in (1, 0)]
    else:
        sp, vol32, K, depth, poses = GA.room_case(0.125)
        assert depth.shape == (57, 77)
        T0 = poses[1]
        levels, runs = (1, [("", (1,), 1)]) if name == "room57 one iteration" else (2, [("", (10, 5), int(np.ceil(0.05 * depth.size)))])
    volume, _ = G.gpu_volume(sp, vol32)
    cur = GA.on_gpu(depth, K, levels)
    aligner = U.Aligner(DEV)
    rec = {}
    for tag, iters, min_pairs in runs:
        aligner.set_pose(T0)
        block = np.array(aligner.ring.wait(aligner.queue_volume(volume, cur, iters, 0.1, 30.0, min_pairs, 1e-6)), dtype=np.int64)
        torch.cuda.synchronize()
        print(f"  {tag}state {int(block[1])}, pairs {int(block[2])}, iterations {int(block[3])}")
        rec[tag + "result"] = _digest(block[1:40])           # state, pairs, iterations, sum r^2, the 29 sums, T; not the sequence word
        rec[tag + "T"] = _digest(aligner.T)
    assert int(block[2]) > 0                                 # (the last run: the finest level)
    return rec


KINDS = {"integrate labels": _integrate_labels, "raycast labels": _raycast_labels, "mesh labels": _mesh_labels, "sample": _sample, "align volume": _align_volume}


def run_case(case):
    kind, name, box, cap = case
    print(case_id(case))
    with pytest.MonkeyPatch.context() as mp:
        if cap:
            mp.setenv("OVO_TSDF_GRID_CAP", str(cap))         # workgroups that loop over everything
            mp.setenv("OVO_MESH_GRID_CAP", str(cap))
            mp.setenv("OVO_ICP_GRID_CAP", str(cap))
        if kind in KINDS:
            return KINDS[kind](name)
        return _integrate(name, box) if kind == "integrate" else (_raycast(name) if kind == "raycast" else _mesh(name))


def test_the_cases_reach_both_integrate_kernels_and_both_row_ends():
    dims = {name: G.integrate_case(name)[0]["dims"] for name in INTEGRATE}
    assert dims["33x17x9"][0] % 2 == 1 and dims["room57"][0] % 2 == 0
    assert any(dims[name][0] % 2 == 0 and box[0][0] % 2 == 1 and box[1][0] % 2 == 1 for name, box in BOXED)
    assert all(dims[name][0] * dims[name][1] * dims[name][2] > 256 * 2 for name in ("33x17x9", "room57"))      # a cap of 2 makes every workgroup loop


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_tsdf_bits(case, golden):
    got, want = run_case(case), golden[case_id(case)]
    assert got == want, sorted(k for k in want if got.get(k) != want[k])
