"""-m gpu: loop closure in the round pipeline (`FramePipeline.close_loop`), in the configuration of tests/test_gpu_multirank.py.

1. a closure that changes nothing (every keyframe, in order, at its own stored pose) leaves the pipeline where it would have been: three more keyframes
   end in exactly the state of the uninterrupted run -- whatever still named old rows or old buffers after `close_loop` would show here;
2. a real closure (a keyframe pruned, two swapped in the tracker's order, two poses corrected): the dense state equals the numpy re-pack of what
   `gather_dense` returned before, bit for bit, and the empty state behind it; the map's integer columns equal the same gather and its points lie
   within tests/test_gpu_reanchor.py's kernel bound -- |error| <= 4 * 2^-24 * sum_j |T_ij| |p_j| against the f64 evaluation of the same f32 transforms
   (a length-4 f32 dot product in any association, derived there); the pipeline then keeps working: its resident class map equals a full re-query;
3. two ranks on one GPU (gloo, as in test_gpu_multirank.py) equal the one-process run across a closure with the semantic update on;
4. the calls `close_loop` refuses."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_gpu_multirank import KW, _free_port, _state
from test_gpu_reanchor import U24, _rigid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _frames(n):
    """Keyframes 0 .. n - 1.  They are the synthetic sequence from its fifth frame on: the seed map is built from what the first four see, and a keyframe
    that appends (almost) nothing would leave a closure nothing to move -- these append about 2 000 points each (asserted where it matters), so the
    keyframes' row ranges cross the 4096-row shard blocks."""
    import dataclasses
    from ovo_amd.pipeline import synthetic_frames
    return [dataclasses.replace(f, index=i) for i, f in enumerate(synthetic_frames(n, DEV, scale=0.35, n_masks_grid=(3, 4), n_blobs=4, start=4))]


def _row(frame_id, pose):
    return np.concatenate([[np.float32(frame_id)], np.asarray(pose, np.float32)[:3].reshape(-1)]).astype(np.float32)


def _steps(pipe, frames, lo, hi):
    """Keyframes lo .. hi - 1, the look-ahead ending at hi: no round is left pre-queued behind the last one."""
    out = None
    for i in range(lo, hi):
        out = pipe.step(frames[i], frames[i + 1:hi])
    return out


def _assert_states_equal(got, ref):
    for k in ("pcd", "ids", "obj_ids", "colors", "table", "acc", "cnt", "cls", "conf", "sim", "inst_cls"):
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), k
    assert got["objects"] == ref["objects"] and got["next_ins_id"] == ref["next_ins_id"]
    assert got["kfs"] == ref["kfs"] and got["top"] == ref["top"]
    assert got["desc"].keys() == ref["desc"].keys()
    for kf in ref["desc"]:
        assert got["desc"][kf].keys() == ref["desc"][kf].keys()
        for i in ref["desc"][kf]:
            assert torch.equal(torch.nan_to_num(got["desc"][kf][i]), torch.nan_to_num(ref["desc"][kf][i])), (kf, i)


# ------------------------------------------------------------------------------------------------ 1. a closure that changes nothing
@pytest.mark.parametrize("encoder_batch", [1, 2])
def test_a_closure_that_changes_nothing_changes_nothing(encoder_batch):
    from ovo_amd.pipeline import FramePipeline
    frames = _frames(6)
    a = FramePipeline(DEV, encoder_batch=encoder_batch, **KW)
    _steps(a, frames, 0, 6)
    torch.cuda.synchronize()
    ref = _state(a)
    assert len(ref["objects"]) > 5 and (ref["cls"] >= 0).any(), "fixture too small to mean anything"
    kfs_a = {k: dict(v) for k, v in a.kfs.items()}
    del a

    b = FramePipeline(DEV, encoder_batch=encoder_batch, **KW)
    _steps(b, frames, 0, 3)
    assert list(b.kfs) == [0, 1, 2] and all(v["pcd_idxs"][1] - v["pcd_idxs"][0] > 1000 for v in b.kfs.values())
    n_before = b.slam._n
    rows = [_row(k, b.slam._c2w_host[k]) for k in b.kfs]
    res = b.close_loop(rows, semantic_update=False)
    assert res == {"n_points": n_before, "n_dropped": 0, "n_keyframes": 3, "n_pruned_keyframes": 0}
    _steps(b, frames, 3, 6)
    torch.cuda.synchronize()
    assert b.kfs == kfs_a and list(b.kfs) == list(kfs_a)
    _assert_states_equal(_state(b), ref)


# ------------------------------------------------------------------------------------------------ 2. a real closure
def _closure_rows(frames):
    """Keyframe 1 pruned, 3 and 2 swapped in the tracker's order, the poses of 0 and 2 corrected by a small rigid transform (3 keeps its own)."""
    rng = np.random.default_rng(5)
    rows = []
    for t in (0, 3, 2):
        pose = np.asarray(frames[t].c2w, np.float32)
        if t != 3:
            pose = (_rigid(rng, 0.02, 0.05).astype(np.float64) @ pose.astype(np.float64)).astype(np.float32)
        rows.append(_row(t, pose))
    return rows


def test_a_real_closure():
    from ovo_amd.pipeline import FramePipeline
    from ovo_amd.utils import clip_utils
    frames = _frames(6)
    pipe = FramePipeline(DEV, **KW)
    _steps(pipe, frames, 0, 4)
    torch.cuda.synchronize()
    n_old, seed = pipe.slam._n, KW["n_map"]
    old = {k: v["pcd_idxs"] for k, v in pipe.kfs.items()}
    assert list(old) == [0, 1, 2, 3] and old[0][0] == seed and old[3][1] == n_old and all(b - a > 1000 for a, b in old.values())
    dense = [t.cpu().numpy().copy() for t in pipe.gather_dense()]
    pcd, ids, obj, col = (t.cpu().numpy().copy() for t in (pipe.slam.pcd, pipe.slam.pcd_ids, pipe.slam.pcd_obj_ids, pipe.slam.pcd_colors))
    old_pose = {k: pipe.slam._c2w_host[k].clone() for k in old}
    assert dense[1].sum() > 0 and (dense[2] >= 0).any()
    rows = _closure_rows(frames)
    res = pipe.close_loop(rows, same_instance=lambda a, b: False)
    torch.cuda.synchronize()

    order = [0, 3, 2]
    gather = np.concatenate([np.arange(seed)] + [np.arange(*old[k]) for k in order])
    n = gather.shape[0]
    assert res == {"n_points": n, "n_dropped": old[1][1] - old[1][0], "n_keyframes": 3, "n_pruned_keyframes": 1}
    assert pipe.slam._n == n == n_old - (old[1][1] - old[1][0])
    ends = np.cumsum([seed] + [old[k][1] - old[k][0] for k in order])
    assert list(pipe.kfs) == order
    assert [pipe.kfs[k] for k in order] == [{"id": k, "pcd_idxs": (int(a), int(b))} for k, a, b in zip(order, ends[:-1], ends[1:])]
    # the dense state: the re-pack of what was there, bit for bit, then the empty state up to the capacity
    got = [pipe.dense_map.acc, pipe.dense_map.cnt, pipe.dense_map.dense_cls, pipe.dense_map.dense_conf]
    for name, g, d in zip(("acc", "cnt", "cls", "conf"), got, dense):
        g, w = g[:n].cpu().numpy(), d[gather]
        bits = (lambda x: x.view(np.int32)) if g.dtype == np.float32 else (lambda x: x)
        assert np.array_equal(bits(g), bits(w)), name
    cap = pipe.slam._cap
    assert pipe.dense_map.acc.shape[0] == cap > n
    assert not pipe.dense_map.acc[n:].any() and not pipe.dense_map.cnt[n:].any()
    assert (pipe.dense_map.dense_cls[n:] == pipe.dense_map.empty_cls).all() and (pipe.dense_map.dense_conf[n:] == pipe.dense_map.empty_conf).all()
    # the map
    assert np.array_equal(pipe.slam.pcd_ids.cpu().numpy(), ids[gather]) and np.array_equal(pipe.slam.pcd_colors.cpu().numpy(), col[gather])
    assert np.array_equal(pipe.slam.pcd_obj_ids.cpu().numpy(), obj[gather])              # (nothing merges under this predicate)
    T = [np.eye(4)]
    for k, row in zip(order, rows):
        new = torch.from_numpy(np.concatenate([row[1:].reshape(3, 4), [[0, 0, 0, 1]]]).astype(np.float32))
        new = torch.eye(4) @ new
        T.append(np.eye(4) if torch.equal(new, old_pose[k]) else (new @ torch.linalg.inv(old_pose[k])).numpy().astype(np.float64))
        assert torch.equal(pipe.slam._c2w_host[k], new)
    assert np.array_equal(T[2], np.eye(4)) and not np.array_equal(T[1], np.eye(4))      # keyframe 3 kept its pose
    seg_of = np.repeat(np.arange(4), np.diff(np.concatenate([[0], ends])))
    T64 = np.stack(T)[seg_of][:, :3]
    p64 = np.concatenate([pcd[gather].astype(np.float64), np.ones((n, 1))], 1)
    want = np.einsum("nij,nj->ni", T64, p64)
    bound = 4 * U24 * np.einsum("nij,nj->ni", np.abs(T64), np.abs(p64))
    err = np.abs(pipe.slam.pcd.cpu().numpy().astype(np.float64) - want)
    print(f"closure: max |err| {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(pipe.slam.pcd.cpu().numpy()[:seed], pcd[:seed])               # the seed rows stay in front, untouched
    # the pipeline keeps working
    out = _steps(pipe, frames, 4, 6)
    torch.cuda.synchronize()
    grown = sum(pipe.kfs[k]["pcd_idxs"][1] - pipe.kfs[k]["pcd_idxs"][0] for k in (4, 5))
    assert grown > 0 and out["n_points"] == pipe.slam._n == n + grown and pipe.kfs[5]["pcd_idxs"][1] == n + grown
    m = pipe.slam._n
    _, cls, conf = clip_utils.similarity(pipe.dense_map.acc[:m], pipe.texts, cnt=pipe.dense_map.cnt[:m], want_sim=False, want_argmax=True)
    assert torch.equal(cls, pipe.dense_map.dense_cls[:m]) and torch.equal(conf, pipe.dense_map.dense_conf[:m])
    assert torch.equal(out["dense_cls"], pipe.dense_map.dense_cls[:m]) and (cls[n:] >= 0).any()    # the new keyframes' points got classes


# ------------------------------------------------------------------------------------------------ 3. two ranks equal one process
def _worker(rank, world, port, path):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      OVO_FORCE_DEVICE="0", OVO_DIST_BACKEND="gloo")
    from ovo_amd import parallel
    from ovo_amd.pipeline import FramePipeline
    parallel.init_distributed()
    torch.cuda.set_device(0)
    pipe = FramePipeline(DEV, **KW)
    assert pipe.world == world and pipe.rank == rank
    frames = _frames(8)
    for r in range(2):
        pipe.step_round(frames[2 * r:2 * r + 2], frames[2 * r + 2:4])
    res = pipe.close_loop(_closure_rows(frames))
    for r in range(2, 4):
        pipe.step_round(frames[2 * r:2 * r + 2], frames[2 * r + 2:])
    torch.cuda.synchronize()
    state = _state(pipe)                                           # gather_dense is a collective: every rank calls it
    state["closure"], state["pipe_kfs"] = res, pipe.kfs
    if rank == 0:
        torch.save(state, path)
    parallel.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_equal_one_process_across_a_closure():
    from ovo_amd.pipeline import FramePipeline
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "rank0.pt")
        mp.spawn(_worker, args=(2, _free_port(), path), nprocs=2, join=True)
        got = torch.load(path, weights_only=False)
    pipe = FramePipeline(DEV, **KW)
    frames = _frames(8)
    _steps(pipe, frames, 0, 4)
    res = pipe.close_loop(_closure_rows(frames))
    _steps(pipe, frames, 4, 8)
    torch.cuda.synchronize()
    ref = _state(pipe)
    assert len(ref["objects"]) > 5 and ref["cnt"].sum() > 0 and (ref["cls"] >= 0).any(), "fixture too small to mean anything"
    assert got["closure"] == res and res["n_pruned_keyframes"] == 1 and got["pipe_kfs"] == pipe.kfs and list(got["pipe_kfs"]) == list(pipe.kfs)
    _assert_states_equal(got, ref)


# ------------------------------------------------------------------------------------------------ 4. what close_loop refuses
def test_close_loop_refuses_a_pre_queued_round_and_emulation():
    from ovo_amd import _lib
    from ovo_amd.pipeline import FramePipeline
    frames = _frames(3)
    pipe = FramePipeline(DEV, **KW)
    pipe.step(frames[0], frames[1:])                               # the look-ahead pre-queues keyframe 1's chains
    assert pipe._queued
    with pytest.raises(_lib.OvoHipError):
        pipe.close_loop([_row(0, frames[0].c2w)])
    pipe.drain()
    torch.cuda.synchronize()
    emu = FramePipeline(DEV, emulate=(0, 2), **KW)
    with pytest.raises(_lib.OvoHipError):
        emu.close_loop([])
