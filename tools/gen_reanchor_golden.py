"""Golden fixture of the loop-closing map update: `python tools/gen_reanchor_golden.py --reference DIR`.

Imports the reference's ovo/slam/orbslam.py on the CPU (empty stub modules stand in for `orbslam3` and `torchvision`, which nothing here calls),
builds a `WrapperORBSLAM` through `__new__`, fills in a small map of seven keyframes and runs the reference's OWN `update_map` (orbslam.py:68-115)
against a fake `get_keyframe_points`.  Writes the inputs, the reference's outputs and the reference's own rounding error to
tests/golden/loop_reanchor.npz.  Only arrays go to disk.

The scene: keyframes 0, 10, 20, 30, 40, 50, 60 own slices of 257, 1, 300, 64, 513, 0, 129 rows in storage order; the tracker reports
[40, 0, 99, 60, 20, 50, 30] -- 10 was pruned, 99 is unknown to the wrapper, 50 is empty, 30 comes back with its old pose -- and one
non-keyframe pose (frame 5) sits in `estimated_c2ws`, which the reference drops.

`ref_err_ulps`: the reference composes each transform in f32 (a 4 x 4 inverse and two products) and applies it in f32.  The same f32 input poses and
points evaluated in f64 give `out_xyz_f64`; the reference's worst |error| per coordinate, as a multiple of 2^-24 sum_j |T_ij| |p_j| (T the f64
transform, p = (x, y, z, 1)), is what a second implementation is measured against.
"""
import argparse
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np
import torch

KF_IDS = [0, 10, 20, 30, 40, 50, 60]
KF_LEN = [257, 1, 300, 64, 513, 0, 129]
TRACKER_ORDER = [40, 0, 99, 60, 20, 50, 30]
EXTRA_POSE = 5


def rigid(rng, max_angle, max_t):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-max_angle, max_angle)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, rng.uniform(-max_t, max_t, 3)
    return T.astype(np.float32)


def row13(kf_id, pose):
    """A tracker row: the id, then the top three rows of the pose, as the Python floats a binding returns."""
    return [float(kf_id)] + [float(v) for v in pose[:3].reshape(-1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
    a = ap.parse_args()
    for name in ("orbslam3", "torchvision", "torchvision.transforms", "torchvision.transforms.v2"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision.transforms.v2.functional"] = types.ModuleType("torchvision.transforms.v2.functional")
    sys.modules["torchvision.transforms.v2.functional"].gaussian_blur = None
    sys.path.insert(0, a.reference)
    torch.set_num_threads(1)
    from ovo.slam.orbslam import WrapperORBSLAM

    rng = np.random.default_rng(20260)
    n = sum(KF_LEN)
    xyz = rng.uniform(-8, 8, (n, 3)).astype(np.float32)
    ids = np.arange(n, dtype=np.int32).reshape(-1, 1)
    obj_ids = rng.integers(-1, 20, (n, 1)).astype(np.int32)
    colors = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    world_ref = rigid(rng, np.pi, 5.0)
    starts = np.concatenate([[0], np.cumsum(KF_LEN)])
    kf_ranges = np.stack([starts[:-1], starts[1:]], 1).astype(np.int64)

    # the poses the wrapper stored while tracking (world_ref @ convert_pose(row), f32, as orbslam.py:47), one per keyframe + one plain frame
    old_rows = {k: row13(k, rigid(rng, np.pi, 5.0)) for k in KF_IDS + [EXTRA_POSE]}
    W = torch.from_numpy(world_ref)

    def stored(row):
        return W @ torch.cat([torch.tensor(row[-12:]).reshape(3, 4), torch.tensor([[0., 0, 0, 1]])])
    old_pose = {k: stored(r) for k, r in old_rows.items()}
    # what the tracker reports after the loop closure: every pose corrected by a small rigid motion, 30 unchanged, 99 never seen by the wrapper
    updated_rows = []
    for k in TRACKER_ORDER:
        if k == 30:
            updated_rows.append(old_rows[k])
            continue
        base = np.concatenate([np.asarray(old_rows[k][1:], np.float32).reshape(3, 4), [[0, 0, 0, 1]]]).astype(np.float32) if k in old_rows else rigid(rng, np.pi, 5.0)
        updated_rows.append(row13(k, (rigid(rng, 0.2, 0.5).astype(np.float64) @ base.astype(np.float64)).astype(np.float32)))

    m = WrapperORBSLAM.__new__(WrapperORBSLAM)
    m.device, m.world_ref, m.map_updated = "cpu", W, False
    m.pcd, m.pcd_ids, m.pcd_obj_ids, m.pcd_colors = (torch.from_numpy(v.copy()) for v in (xyz, ids, obj_ids, colors))
    m.kfs = {k: {"id": k, "pcd_idxs": (int(r[0]), int(r[1]))} for k, r in zip(KF_IDS, kf_ranges)}
    m.estimated_c2ws = dict(sorted(old_pose.items()))
    m.orbslam = types.SimpleNamespace(get_keyframe_points=lambda: updated_rows, shutdown=lambda: None)
    m.update_map()
    assert m.map_updated

    # the same f32 inputs in f64
    W64 = world_ref.astype(np.float64)
    exp, unit = [], []
    for row in updated_rows:
        k = int(row[0])
        if k not in KF_IDS:
            continue
        U = np.concatenate([np.asarray(row[1:], np.float32).reshape(3, 4), [[0, 0, 0, 1]]]).astype(np.float64)
        T = (W64 @ U) @ np.linalg.inv(old_pose[k].numpy().astype(np.float64))
        s, e = kf_ranges[KF_IDS.index(k)]
        p = np.concatenate([xyz[s:e].astype(np.float64), np.ones((e - s, 1))], 1)
        exp.append(p @ T[:3].T)
        unit.append(2.0 ** -24 * (np.abs(p) @ np.abs(T[:3]).T))
    exp, unit = np.concatenate(exp), np.concatenate(unit)
    out_xyz = m.pcd.numpy()
    assert out_xyz.dtype == np.float32 and out_xyz.shape == exp.shape
    err = np.abs(out_xyz.astype(np.float64) - exp)
    ref_err_ulps = float((err / unit).max())

    new_ids = list(m.kfs)
    arrays = {
        "xyz": xyz, "ids": ids, "obj_ids": obj_ids, "colors": colors, "max_id": np.int64(n), "world_ref": world_ref,
        "kf_ids": np.asarray(KF_IDS, np.int64), "kf_ranges": kf_ranges,
        "pose_keys": np.asarray(sorted(old_pose), np.int64), "pose_values": np.stack([old_pose[k].numpy() for k in sorted(old_pose)]),
        "updated_rows": np.asarray(updated_rows, np.float32),
        "out_xyz": out_xyz, "out_ids": m.pcd_ids.numpy(), "out_obj_ids": m.pcd_obj_ids.numpy(), "out_colors": m.pcd_colors.numpy(),
        "out_kf_ids": np.asarray(new_ids, np.int64), "out_kf_ranges": np.asarray([m.kfs[k]["pcd_idxs"] for k in new_ids], np.int64),
        "out_pose_keys": np.asarray(list(m.estimated_c2ws), np.int64), "out_pose_values": np.stack([v.numpy() for v in m.estimated_c2ws.values()]),
        "out_xyz_f64": exp, "ref_err_ulps": np.float64(ref_err_ulps), "ref_err_abs": np.float64(err.max()),
    }
    assert arrays["updated_rows"].dtype == np.float32 and all(float(np.float32(v)) == v for r in updated_rows for v in r)
    path = os.path.join(a.out, "loop_reanchor.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} {os.path.getsize(path)} bytes; kept {new_ids}, {out_xyz.shape[0]} rows, ref_err_ulps {ref_err_ulps:.3f}, max |err| {err.max():.2e}")


if __name__ == "__main__":
    main()
