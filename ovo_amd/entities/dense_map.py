"""The dense per-point state of the keyframe pipeline: per-point descriptor accumulators `acc` / `cnt`, sharded by point over the ranks
(block-cyclic: block b of `block` points lies on rank b % world as its local block b // world), and the RESIDENT class / confidence map
`dense_cls` / `dense_conf` over the same rows.  Everything that knows the shard layout, the touched-row lists or which launches update
the map is here; `FramePipeline` hands it a keyframe's descriptors (`apply`), reads the step's output (`result`), exports (`gather`) and
moves it with the map at a loop closure (`repack`)."""
from __future__ import annotations

import os
from typing import Callable, Tuple

import torch

from .. import _lib as L
from ..slam.orbslam import dense_repack
from ..utils import clip_utils


def shard_rows(n: int, rank: int, world: int, block: int) -> int:
    """Rows of rank `rank`'s shard that hold points of a map with n points (block-cyclic, blocks of `block` points)."""
    if world == 1:
        return n
    full, rem = divmod(n, block)                                   # `full` complete blocks, then one of `rem` points
    mine = (full - rank + world - 1) // world if full > rank else 0          # complete blocks owned by `rank`
    return mine * block + (rem if full % world == rank else 0)


def merge_shards(gathered: torch.Tensor, n: int, block: int) -> torch.Tensor:
    """[R, per * block, ...] -- the ranks' shards, each cut to the same whole number of blocks, stacked rank-major (what an all-gather
    returns) -- as the first n rows in point order: block b = (b // R, b % R).  No arithmetic."""
    R, rows = gathered.shape[:2]
    per = rows // block
    return gathered.reshape(R, per, block, *gathered.shape[2:]).transpose(0, 1).reshape(per * R * block, *gathered.shape[2:])[:n]


class DenseMap:
    def __init__(self, cap: int, D: int, texts: torch.Tensor, shard: Tuple[int, int, int], device, gather: Callable[[torch.Tensor], torch.Tensor]):
        """`cap`: the point map's capacity in rows; `shard` = (rank, world, block); `gather`: the all-gather of one tensor over the ranks
        ([world, ...], rank-major)."""
        self.D, self.texts, self.device, self._gather = D, texts, device, gather
        self.rank, self.world, self.block = shard
        self.rows_local = self._shard_capacity(cap)                # rows of THIS rank's shard
        self.acc = torch.zeros((self.rows_local, D), dtype=torch.float32, device=device)
        self.cnt = torch.zeros(self.rows_local, dtype=torch.int32, device=device)
        # The dense class / confidence map stays RESIDENT: a keyframe changes the accumulators of the points it matched (10-20 % of
        # the map) and only those rows can change class, so the scatter pass emits their indices and the query re-evaluates just
        # them (`ovo_similarity_rows`) -- bit-identical to re-querying all rows (tests/test_gpu_pipeline.py), a fraction of the 5 GB
        # stream.  Initial state = the query of the empty accumulators, computed once here over the whole capacity.
        self.incremental = D % 16 == 0 and not os.environ.get("OVO_DENSE_FULL_QUERY")
        self.dense_cls = self.dense_conf = self.touched = self.n_touched = None
        self.empty_cls, self.empty_conf = -1, 0.0
        self._touch_parity = 0
        if self.incremental:
            _, self.dense_cls, self.dense_conf = clip_utils.similarity(self.acc, texts, cnt=self.cnt, want_sim=False, want_argmax=True)
            # the state of a row without points: what `repack` gives the rows behind the re-packed map
            self.empty_cls, self.empty_conf = int(self.dense_cls[0]), float(self.dense_conf[0])
            self.touched = torch.empty(self.rows_local, dtype=torch.int32, device=device)
            self.n_touched = torch.zeros(2, dtype=torch.int32, device=device)      # two counters, used alternately
        # round 6: the tracking chain lists the points its masks cover and ONE launch accumulates and re-queries them (`ovo_scatter_accum_query`);
        # the scan + apply + query launches remain for keyframes tracked on the host path and for OVO_NO_FUSED_SCATTER=1
        n_text = texts.shape[0]
        self.fused = bool(self.incremental and not os.environ.get("OVO_NO_FUSED_SCATTER") and n_text <= 16 and n_text * D * 4 <= 96 * 1024)

    def _dealt_rows(self, n: int) -> int:
        """The blocks that hold n points, dealt to the ranks, as whole blocks per rank (the last rank's may be short / absent): the rows every
        rank contributes to a gather of the first n points."""
        return -(-(-(-n // self.block)) // self.world) * self.block

    def _shard_capacity(self, cap: int) -> int:
        return self._dealt_rows(cap) if self.world > 1 else cap

    def local_rows(self, n: int) -> int:
        """Rows of this rank's shard that hold points of a map with n points."""
        return shard_rows(n, self.rank, self.world, self.block)

    def apply(self, point_seg: torch.Tensor, rows: torch.Tensor, desc: torch.Tensor, hits) -> None:
        """One keyframe: add descriptor `rows[point_seg[p]]` of `desc` to every point p a kept mask covers (this rank's rows only) and, with the
        resident map, re-evaluate exactly those rows.  `hits`: the tracking pass's list of covered points (None: tracked on the host path)."""
        lib = L.load()
        n_rows = min(point_seg.shape[0], self.rows_local)
        if hits is not None and self.incremental:                  # one launch: accumulate the listed rows and re-evaluate exactly them
            n_list = hits.numel() - 4
            L.check(lib.ovo_scatter_accum_query(L.ptr(hits), hits[n_list:].data_ptr(), n_rows, L.ptr(point_seg),
                                                L.ptr(rows), rows.shape[0], L.ptr(desc), self.D, L.ptr(self.acc), L.ptr(self.cnt), self.rank, self.world,
                                                self.block, L.ptr(self.texts), self.texts.shape[0], 0, 0.0, 0.0, 0.0,
                                                L.ptr(self.dense_cls), L.ptr(self.dense_conf), L.stream()))
            return
        touched, n_cur, n_nxt = None, None, None
        if self.incremental:
            p = self._touch_parity
            self._touch_parity ^= 1
            touched, n_cur, n_nxt = L.ptr(self.touched), self.n_touched[p:].data_ptr(), self.n_touched[p ^ 1:].data_ptr()
        L.check(lib.ovo_scatter_accum_touched(L.ptr(point_seg), point_seg.shape[0], L.ptr(rows), rows.shape[0], L.ptr(desc), self.D,
                                              L.ptr(self.acc), L.ptr(self.cnt), touched, n_cur, n_nxt, self.rank, self.world,
                                              self.block, L.stream()))
        if self.incremental:                                       # only the rows this keyframe changed can change class
            L.check(lib.ovo_similarity_rows(L.ptr(self.acc), 0, touched, n_cur, n_rows, self.D,
                                            L.ptr(self.texts), self.texts.shape[0], L.ptr(self.cnt), 0, 0.0, 0.0, 0.0,
                                            L.ptr(self.dense_cls), L.ptr(self.dense_conf), L.stream()))

    def result(self, n: int):
        """(cls, conf) of this rank's rows of a map with n points."""
        nl = self.local_rows(n)
        if self.incremental:                                       # the resident map, patched by `apply` for the rows the round changed
            return self.dense_cls[:nl], self.dense_conf[:nl]
        _, cls, conf = clip_utils.similarity(self.acc[:nl], self.texts, cnt=self.cnt[:nl], want_sim=False, want_argmax=True)
        return cls, conf                                           # dense query: per-point mean descriptor x texts, every (local) row

    def gather(self, n: int):
        """The whole dense state on every rank, in point order: (acc f32[n, D], cnt i32[n], cls i64[n], conf f32[n]).  The concatenation
        of the shards -- no arithmetic, so it equals the one-process accumulators bit for bit.  A map-sized collective: for export /
        tests, never inside the keyframe loop (queries run on the shards)."""
        state = (self.acc, self.cnt, self.dense_cls, self.dense_conf)
        if self.world == 1:
            return tuple(None if t is None else t[:n] for t in state)
        rows = self._dealt_rows(n)
        return tuple(None if t is None else merge_shards(self._gather(t[:rows].contiguous()), n, self.block) for t in state)

    def repack(self, n_old: int, seg_src, seg_dst, cap: int, ws: torch.Tensor) -> None:
        """Loop closure: move the state of the first `n_old` points through the map's segment table into fresh buffers (one `ovo_dense_repack`
        launch); rows behind the re-packed map get the empty state.  `cap`: the point map's capacity now.  Several ranks: the shards (the rows
        that hold points) are all-gathered and each rank re-packs its own shard straight from the shard-major result -- no merge copy."""
        R, dev, inc = self.world, self.device, self.incremental
        rows_local = max(self.rows_local, self._shard_capacity(cap))          # (the capacity grows only when the tracker lists a keyframe twice)
        src = [self.acc, self.cnt, self.dense_cls, self.dense_conf]
        if R > 1:
            rows = self._dealt_rows(n_old)
            src = [None if t is None else self._gather(t[:rows].contiguous()) for t in src]
        out = [torch.empty((rows_local, self.D), dtype=torch.float32, device=dev), torch.empty(rows_local, dtype=torch.int32, device=dev),
               torch.empty(rows_local, dtype=torch.int64, device=dev) if inc else None,
               torch.empty(rows_local, dtype=torch.float32, device=dev) if inc else None]
        dense_repack(src, out, n_old, seg_src, seg_dst, n_fill=rows_local * R, empty_cls=self.empty_cls, empty_conf=self.empty_conf,
                     src_shards=R, shard=(self.rank, R, self.block), ws=ws)
        torch.cuda.current_stream().synchronize()                  # the old buffers are released below
        del src
        self.acc, self.cnt, self.dense_cls, self.dense_conf = out
        self.rows_local = rows_local
        if inc:
            if self.touched.numel() < rows_local:
                self.touched = torch.empty(rows_local, dtype=torch.int32, device=dev)
            self.n_touched.zero_()                                 # the lists name old rows
            self._touch_parity = 0
