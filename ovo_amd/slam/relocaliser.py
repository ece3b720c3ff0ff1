"""Place recognition for `IcpTracker`: a fern code of every frame (`fern_utils.encode`), the database of the keyframes' codes
and its search (`fern_utils.FernDatabase`), and the verification of a LOST frame against the keyframes it looks like -- all of them in the launches
of one alignment (`ovo_icp_align_batch`).  `IcpTracker(relocalise=True)` uses all of it; `loop_candidates="fern"` / "both" only the codes and the
search.  The tracker tells it of every frame and every new keyframe and applies what it hands back; nothing here reaches into the tracker."""
from __future__ import annotations

from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

from ..utils import fern_utils as F
from ..utils import icp_utils as U

SEARCH_K = F.MAX_K                                         # entries asked of every search: room for matches the host then drops (keyframes no longer kept)
CAPACITY = 1 << 16                                         # keyframes with a code: 8 MB at 256 ferns


class Relocaliser:
    def __init__(self, iters, normal_th_deg: float, min_pivot_ratio: float, max_depth: float, fern_count: int, fern_seed: int, fern_tau,
                 reloc_max_candidates: int, reloc_max_dissimilarity: float, reloc_iters, reloc_dist_th: float, reloc_min_overlap: float,
                 reloc_max_rms: float, reloc_max_keyframes: int) -> None:
        """`iters`, `normal_th_deg`, `min_pivot_ratio` and `max_depth` are the tracker's own; the fern_* and reloc_* parameters are described at
        `IcpTracker`."""
        self.normal_th_deg, self.min_pivot_ratio = normal_th_deg, min_pivot_ratio
        self.fern_count, self.fern_seed = int(fern_count), int(fern_seed)
        lo, hi = fern_tau
        self.fern_tau = (float(lo), 0.5 * float(max_depth) if hi is None else float(hi))
        self.max_candidates, self.max_dissimilarity = int(reloc_max_candidates), float(reloc_max_dissimilarity)
        self.iters = tuple(iters) if reloc_iters is None else tuple(int(i) for i in reloc_iters)
        self.dist_th, self.min_overlap, self.max_rms = float(reloc_dist_th), float(reloc_min_overlap), float(reloc_max_rms)
        self.max_keyframes = int(reloc_max_keyframes)
        if not (8 <= self.fern_count <= F.MAX_FERNS and self.fern_count % 8 == 0):
            raise ValueError(f"IcpTracker: fern_count must be a multiple of 8 in 8 .. {F.MAX_FERNS}")
        if not (np.isfinite(self.fern_tau).all() and 0 <= self.fern_tau[0] <= self.fern_tau[1]):
            raise ValueError("IcpTracker: fern_tau is (lowest, highest) threshold in metres, 0 <= lowest <= highest (None: max_depth / 2)")
        if not (1 <= self.max_candidates <= U.MAX_BATCH and self.max_keyframes >= 1):
            raise ValueError(f"IcpTracker: reloc_max_candidates must be 1 .. {U.MAX_BATCH} and reloc_max_keyframes >= 1")
        if len(self.iters) != len(iters) or min(self.iters) < 0 or sum(self.iters) < 1:
            raise ValueError("IcpTracker: reloc_iters needs one entry per level, coarse to fine, none negative and not all 0")
        if not (0 <= self.max_dissimilarity <= 1 and self.dist_th > 0 and 0 <= self.min_overlap <= 1 and self.max_rms > 0):
            raise ValueError("IcpTracker: reloc_max_dissimilarity and reloc_min_overlap lie in [0, 1], reloc_dist_th and reloc_max_rms must be > 0")
        self.table: Optional[F.FernTable] = None
        self.db: Optional[F.FernDatabase] = None
        self._batch: Optional[U.BatchAligner] = None
        self._code = self._seq = None
        self.last_reloc: Any = None                        # the last attempt: {"candidates", "distances", "results", "passed", "winner"}

    def encode(self, frame: U.Frame) -> None:
        """Queues the frame's code (the table and the database are made with the first frame: the coarsest level's size is known then)."""
        if self.table is None:
            hw = U.level_shapes(frame.h, frame.w, frame.levels)[-1]
            self.table = F.FernTable(self.fern_count, hw, self.fern_seed, self.fern_tau, device=frame.pyramid.device)
            self.db = F.FernDatabase(self.table, CAPACITY, device=frame.pyramid.device)
        self._code = F.encode(frame, self.table, out=self._code)

    def queue(self, frame: U.Frame, limits: Sequence[int]) -> None:
        """The frame's code and its search under `limits` (keyframe counts: a keyframe's row is its index), queued on the current stream."""
        self.encode(frame)
        self._seq = self.db.queue(self._code, [min(max(int(x), 0), self.db.n) for x in limits], SEARCH_K)

    def matches(self) -> List[List[Tuple[int, int]]]:
        """Per limit, [(keyframe, block distance)] in (distance, keyframe) order.  The block was queued in front of the frame's alignment: once that
        has been waited for it is there."""
        return [[(self.db.keyframe_of(r), int(d)) for r, d in zip(rows, dists)] for rows, dists in self.db.wait(self._seq)]

    def add_keyframe(self, n: int) -> None:
        """The code queued last is keyframe n's (a device copy behind the search that read the database)."""
        if self.db.n < self.db.capacity:                   # (beyond the capacity a keyframe has no code and is never a match)
            self.db.set_row_keyframe(self.db.add(self._code), n)

    def choose(self, matches: Sequence[Tuple[int, int]], kept) -> List[Tuple[int, int]]:
        """The keyframes a LOST frame is verified against: the reloc_max_candidates best matches within reloc_max_dissimilarity * M that `kept` holds."""
        return [(k, d) for k, d in matches if d <= self.max_dissimilarity * self.fern_count and kept(k)][:self.max_candidates]

    def verify(self, chosen: Sequence[Tuple[int, int]], refs: Sequence[U.Frame], cur: U.Frame, pixels: int, min_pairs: int):
        """One batch from the identity, one host wait.  Returns (the winner's keyframe, its result) or (None, None): an entry passes when it is OK,
        has pairs >= reloc_min_overlap * pixels and rms <= reloc_max_rms; the winner has the most pairs, then the smaller rms, then the lower index."""
        if self._batch is None:
            self._batch = U.BatchAligner(cur.pyramid.device)
        seq = self._batch.queue(list(refs), cur, [np.eye(4, dtype=np.float32)] * len(refs), self.iters, self.dist_th, self.normal_th_deg, min_pairs,
                                self.min_pivot_ratio)
        results = self._batch.wait(seq)
        passed = [(k, r) for (k, _), r in zip(chosen, results) if accept_reloc(r, pixels, self.min_overlap, self.max_rms)]
        best = min(passed, key=lambda e: (-e[1]["pairs"], e[1]["rms"], e[0])) if passed else (None, None)
        self.last_reloc = {"candidates": [k for k, _ in chosen], "distances": [d for _, d in chosen], "results": results,
                           "passed": [k for k, _ in passed], "winner": best[0]}
        return best

    def release(self) -> None:
        self._batch = self.db = self.table = self._code = None


def accept_reloc(res, pixels: int, min_overlap: float, max_rms: float) -> bool:
    return res["state"] == U.OK and res["pairs"] >= min_overlap * pixels and res["rms"] <= max_rms
