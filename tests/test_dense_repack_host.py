"""The host side of loop closure in the round pipeline (no GPU): ovo_dense_repack's argument checks -- every one of them before anything is queued --
the segment-table builder with a head segment, and the block-cyclic rule the kernel, `dense_map.shard_rows` and `merge_shards` share."""
import ctypes as C

import numpy as np
import pytest

SRC = (0x1000000, 0x2000000, 0x3000000, 0x4000000)        # acc, cnt, cls, conf: made up, well separated, never dereferenced
OUT = (0x11000000, 0x12000000, 0x13000000, 0x14000000)


def _call(lib, *, D=8, src_shards=1, src_rows_local=100, n_src=100, rows_out=128, shard=(0, 1, 16), n_fill=120, seg_src=(0, 50), seg_dst=(0, 10, 30),
          K=None, src=SRC, out=OUT, ws=0x7000000, ws_bytes=1 << 12):
    """ovo_dense_repack on made-up addresses: a call that passes the checks would reach the device, so every case of the error test has to fail them."""
    s, d = np.asarray(seg_src, np.int64), np.asarray(seg_dst, np.int64)
    K = len(s) if K is None else K
    p = lambda v: C.c_void_p(v) if v else None
    return lib.ovo_dense_repack(p(src[0]), p(src[1]), p(src[2]), p(src[3]), D, src_shards, src_rows_local, n_src, p(out[0]), p(out[1]), p(out[2]), p(out[3]),
                                rows_out, shard[0], shard[1], shard[2], n_fill, -1, 0.0, s.ctypes.data, d.ctypes.data, K, p(ws), ws_bytes, None)


@pytest.mark.parametrize("case, kw", [
    ("seg_dst not from 0", {"seg_dst": (1, 10, 30)}),
    ("decreasing seg_dst", {"seg_dst": (0, 30, 10)}),
    ("negative source row", {"seg_src": (-1, 50)}),
    ("segment past n_src", {"seg_src": (0, 81)}),
    ("segment start past n_src", {"seg_src": (0, 101), "seg_dst": (0, 10, 10)}),
    ("negative K", {"K": -1}),
    ("n_fill < total", {"n_fill": 29}),
    ("negative n_fill", {"n_fill": -1, "seg_src": (), "seg_dst": (0,)}),
    ("source shard too short", {"src_rows_local": 99}),
    ("source shards too short", {"src_shards": 3, "src_rows_local": 35}),      # 100 rows in blocks of 16 over 3 ranks: rank 0 holds 2 blocks + the 4-row rest
    ("no source shard", {"src_shards": 0}),
    ("output shard too short", {"rows_out": 119}),
    ("output shard of rank 1 too short", {"shard": (1, 2, 16), "rows_out": 55}),   # 120 rows: blocks 1, 3, 5 and the 8-row rest of block 7
    ("D == 0", {"D": 0}),
    ("D % 4 != 0", {"D": 6}),
    ("acc misaligned", {"src": (SRC[0] + 4,) + SRC[1:]}),
    ("acc_out misaligned", {"out": (OUT[0] + 8,) + OUT[1:]}),
    ("shard_block not a power of two", {"shard": (0, 1, 24)}),
    ("shard_block == 0", {"shard": (0, 1, 0)}),
    ("shard_rank == shard_count", {"shard": (2, 2, 16)}),
    ("negative shard_rank", {"shard": (-1, 2, 16)}),
    ("shard_count == 0", {"shard": (0, 0, 16)}),
    ("null acc_out", {"out": (0,) + OUT[1:]}),
    ("null cnt_out", {"out": (OUT[0], 0) + OUT[2:]}),
    ("null acc", {"src": (0,) + SRC[1:]}),
    ("null cnt", {"src": (SRC[0], 0) + SRC[2:]}),
    ("cls without conf", {"src": SRC[:3] + (0,)}),
    ("cls_out without conf_out", {"out": OUT[:3] + (0,)}),
    ("cls without cls_out", {"out": OUT[:2] + (0, 0)}),
    ("cls_out without cls", {"src": SRC[:2] + (0, 0)}),
    ("null workspace", {"ws": 0}),
    ("small workspace", {"ws_bytes": 39}),
    ("misaligned workspace", {"ws": 0x7000004}),
    ("in place", {"out": (SRC[0],) + OUT[1:]}),
    ("acc_out inside acc", {"out": (SRC[0] + 3184,) + OUT[1:]}),               # the last 16 bytes of the 100 x 8 x 4 source
    ("cnt_out on the class map", {"out": (OUT[0], SRC[2] + 8) + OUT[2:]}),
    ("conf_out on cnt_out", {"out": OUT[:3] + (OUT[1] + 500,)}),
    ("workspace on a source", {"ws": SRC[3] + 8}),
    ("workspace on an output", {"ws": OUT[2] + 8}),
])
def test_argument_errors_are_reported_before_any_launch(case, kw):
    from ovo_amd import _lib
    lib = _lib.load()
    assert _call(lib, **kw) == -1, case
    assert b"ovo_dense_repack" in lib.ovo_hip_last_error(), case


def test_calls_with_nothing_to_write_and_the_workspace_size():
    from ovo_amd import _lib
    lib = _lib.load()
    assert _call(lib, n_fill=0, seg_src=(), seg_dst=(0,)) == 0                    # nothing below n_fill
    assert _call(lib, n_fill=0, seg_src=(5, 7), seg_dst=(0, 0, 0)) == 0           # K == 2, zero rows
    assert _call(lib, shard=(2, 3, 16), n_fill=30, rows_out=0) == 0               # rows [0, 30) lie in blocks 0 and 1: rank 2 of 3 owns none
    assert lib.ovo_dense_repack_workspace_bytes(0) == 0
    assert lib.ovo_dense_repack_workspace_bytes(7) == 8 * 8 + 8 * 7               # seg_dst i64[K + 1] | seg_src i64[K]


def test_segment_table_with_a_head_segment():
    from ovo_amd.slam.orbslam import build_segment_table
    kfs = {k: {"id": k, "pcd_idxs": r} for k, r in {10: (1000, 1100), 11: (1100, 1100), 12: (1100, 1350), 13: (1350, 1351), 14: (1351, 2000)}.items()}
    order = [13, 99, 10, 14, 10, 11]                                               # 99 unknown, 12 pruned, 10 listed twice, 11 empty
    kept, src, dst = build_segment_table(kfs, order, head_rows=1000)
    assert kept == [13, 10, 14, 10, 11] and src.dtype == dst.dtype == np.int64
    assert src.tolist() == [0, 1350, 1000, 1351, 1000, 1100]
    assert dst.tolist() == [0, 1000, 1001, 1101, 1750, 1850, 1850]
    # without a head the table is the one the back end has always built
    kept0, src0, dst0 = build_segment_table(kfs, order)
    assert kept0 == kept and src0.tolist() == src.tolist()[1:] and dst0.tolist() == (dst[1:] - 1000).tolist()
    assert [a.tolist() for a in build_segment_table(kfs, order, head_rows=0)[1:]] == [src0.tolist(), dst0.tolist()]
    kept, src, dst = build_segment_table(kfs, [], head_rows=7)                     # every keyframe pruned: the seed alone
    assert kept == [] and src.tolist() == [0] and dst.tolist() == [0, 7]
    kept, src, dst = build_segment_table(kfs, [99])
    assert kept == [] and src.shape == (0,) and dst.tolist() == [0]


def _owner(g, B, R):
    """The block-cyclic rule, stated here: global row g lies in block g // B, which rank (g // B) % R holds as its local block (g // B) // R."""
    b = g // B
    return b % R, (b // R) * B + g % B


@pytest.mark.parametrize("B, R", [(16, 1), (16, 2), (16, 3), (4096, 8)])
def test_block_cyclic_rule_agrees_with_the_pipeline(B, R):
    from ovo_amd.entities.dense_map import shard_rows
    sizes = [0, 1, B - 1, B, B + 1, R * B - 1, R * B, R * B + 1, 5 * B, 5 * B + 3, (2 * R + 1) * B, (2 * R + 1) * B + B - 1]
    for n in sizes:
        g = np.arange(n)
        rank, local = _owner(g, B, R)
        for r in range(R):
            mine = local[rank == r]
            want = 0 if mine.size == 0 else int(mine.max()) + 1
            assert np.array_equal(np.sort(mine), np.arange(want))                  # a rank's rows are dense from 0
            assert shard_rows(n, r, R, B) == want, (n, r)
        if R == 1:
            continue
        # merge_shards' order: shards cut to per * B rows, stacked rank-major, [R, per, B] -> [per, R, B] -> the first n rows
        per = -(-(-(-n // B)) // R)
        shards = np.full((R, per * B), -1, np.int64)
        shards[rank, local] = g
        merged = shards.reshape(R, per, B).transpose(1, 0, 2).reshape(per * R * B)[:n]
        assert np.array_equal(merged, g), n
