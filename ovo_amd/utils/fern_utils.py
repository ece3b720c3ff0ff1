"""Randomized depth ferns (csrc/fern.hip; Glocker et al., "Real-time RGB-D camera relocalization via randomized ferns"): the index
that says which old keyframe a frame looks like.  `FernTable` is the random tests, `encode` a frame's code (`ovo_fern_encode`, over one level of the
pyramid `icp_utils.prepare_frame` left on the device), `FernDatabase` the stored codes and their search (`ovo_fern_search`): block-wise Hamming distance
to every row and the k nearest rows under up to four row limits, read from a pinned block.  `IcpTracker(relocalise=True)` and
`loop_candidates="fern"` look these up here when they call them."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib as L
from . import icp_utils as U

MAX_FERNS, MAX_ROWS, MAX_K, MAX_LIMITS = 4096, 1 << 20, 16, 4      # ovo_hip.h: OVO_FERN_MAX_*
RESULT_WORDS = 66                                          # ovo_hip.h: 0 sequence | 1 n | 2 + 16 i + e


def draw_table(n_ferns: int, level_hw, seed: int, tau_range) -> Tuple[np.ndarray, np.ndarray]:
    """The table of a seed, in this FIXED order from ONE `numpy.random.default_rng(seed)`: first all 4 M pixel indices, `integers(0, h * w, size=4 M)`
    (uniform over the level, row-major v * w + u), then all 4 M thresholds, `uniform(lo, hi, size=4 M)` rounded to f32.  Entry 4 f + b is test b of
    fern f.  Returns (pix i32[4 M], tau f32[4 M])."""
    m, (h, w), (lo, hi) = int(n_ferns), (int(level_hw[0]), int(level_hw[1])), (float(tau_range[0]), float(tau_range[1]))
    if not (8 <= m <= MAX_FERNS and m % 8 == 0):
        raise ValueError(f"FernTable: n_ferns must be a multiple of 8 in 8 .. {MAX_FERNS} (got {n_ferns})")
    if h < 1 or w < 1 or not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError(f"FernTable: level_hw must be at least 1 x 1 and tau_range finite with lo <= hi (got {level_hw}, {tau_range})")
    rng = np.random.default_rng(int(seed))
    pix = rng.integers(0, h * w, size=4 * m).astype(np.int32)
    tau = rng.uniform(lo, hi, size=4 * m).astype(np.float32)
    return pix, tau


class FernTable:
    """M ferns of 4 depth tests each for a level of level_hw = (h_l, w_l) pixels: `pix` and `tau` (see `draw_table`) on the host and on the device.
    The kernel never range-checks a pixel index: it is checked HERE, when the table is made (also one given as pix=, tau=)."""

    def __init__(self, n_ferns: int, level_hw, seed: int = 0, tau_range=(0.3, 5.0), device="cuda", pix=None, tau=None) -> None:
        self.n_ferns, self.level_hw, self.seed = int(n_ferns), (int(level_hw[0]), int(level_hw[1])), int(seed)
        drawn = draw_table(n_ferns, level_hw, seed, tau_range)
        self.pix = drawn[0] if pix is None else np.ascontiguousarray(pix, dtype=np.int32)
        self.tau = drawn[1] if tau is None else np.ascontiguousarray(tau, dtype=np.float32)
        self.pixels = self.level_hw[0] * self.level_hw[1]
        if self.pix.shape != (4 * self.n_ferns,) or self.tau.shape != (4 * self.n_ferns,):
            raise ValueError(f"FernTable: pix and tau must hold 4 * n_ferns = {4 * self.n_ferns} entries")
        if self.pix.min() < 0 or self.pix.max() >= self.pixels:
            raise ValueError(f"FernTable: a pixel index lies outside the {self.level_hw[0]} x {self.level_hw[1]} level")
        self.words = self.n_ferns // 8
        self.device = torch.device(device)
        self.pix_dev = torch.from_numpy(self.pix).to(self.device)
        self.tau_dev = torch.from_numpy(self.tau).to(self.device)


def encode(frame: U.Frame, table: FernTable, level: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`ovo_fern_encode` on the current stream: the code of `frame` at pyramid level `level` (None: the coarsest) as i32[W] on the device, the bits
    of the contract's u32 words (view it as you like).  One launch, no wait."""
    level = frame.levels - 1 if level is None else int(level)
    if out is None:
        out = torch.empty(table.words, dtype=torch.int32, device=frame.pyramid.device)
    L.dev(out, torch.int32, "code")
    if out.numel() != table.words:
        raise L.OvoHipError(f"encode: the code holds {table.words} words (got {out.numel()})")
    L.check(L.load().ovo_fern_encode(L.ptr(frame.pyramid), C.byref(frame.desc), level, L.ptr(table.pix_dev), L.ptr(table.tau_dev), table.n_ferns,
                                     table.pixels, L.ptr(out), L.stream()))
    return out


def decode_lists(block: np.ndarray, n_limits: int, k: int) -> List[Tuple[np.ndarray, np.ndarray]]:
    """The pinned result block (int64[66]) as [(rows i32, dists i32)] per limit, the -1 entries dropped (a list is as long as it has rows)."""
    block = np.array(block, dtype=np.int64)                # a copy: the slot is reused
    out = []
    for i in range(n_limits):
        keys = block[2 + 16 * i:2 + 16 * i + k]
        keys = keys[keys >= 0]
        out.append(((keys & 0xFFFFFFFF).astype(np.int32), (keys >> 32).astype(np.int32)))
    return out


class FernDatabase:
    """The codes of the keyframes, i32[capacity, W] on the device, the search workspace and a ring of pinned result blocks.  A ROW is a position in
    that array, and rows are never moved: a limit of the search is a row count, so "the keyframes up to m" stays a prefix.  `set_row_keyframe` /
    `keyframe_of` say which keyframe index a row stands for (default: the row itself), so that a store which keeps only some keyframes' pyramids
    can tell a match it still holds from one it dropped.  A code is 4 W bytes: 128 at M = 256."""

    def __init__(self, table: FernTable, capacity: int, device="cuda") -> None:
        self.table, self.capacity, self.device = table, int(capacity), torch.device(device)
        if not 1 <= self.capacity <= MAX_ROWS:
            raise ValueError(f"FernDatabase: capacity must be 1 .. {MAX_ROWS} rows (got {capacity})")
        self.codes = torch.zeros((self.capacity, table.words), dtype=torch.int32, device=self.device)
        # the workspace of any n <= capacity: its size grows with n up to 2^18 rows (256 slabs) and never exceeds that
        self.ws = torch.empty(int(L.load().ovo_fern_search_workspace_bytes(min(self.capacity, 1 << 18), MAX_K)), dtype=torch.uint8, device=self.device)
        self.ring = L.PinnedRing(RESULT_WORDS, np.int64, slots=8)
        self.n = 0
        self._keyframe: Dict[int, int] = {}
        self._pending: Dict[int, Tuple[int, int]] = {}

    def add(self, code: torch.Tensor) -> int:
        """Copies a code (device) into the next row, device to device on the current stream; returns the row."""
        if self.n >= self.capacity:
            raise L.OvoHipError(f"FernDatabase: all {self.capacity} rows are taken")
        self.codes[self.n].copy_(code)
        self.n += 1
        return self.n - 1

    def set_row_keyframe(self, row: int, keyframe: int) -> None:
        self._keyframe[int(row)] = int(keyframe)

    def keyframe_of(self, row: int) -> int:
        return self._keyframe.get(int(row), int(row))

    def queue(self, code: torch.Tensor, limits: Sequence[int], k: int, dist_out: Optional[torch.Tensor] = None) -> int:
        """Queues one search of the first `n` rows on the current stream; returns the sequence number `wait` takes."""
        limits = [int(x) for x in limits]
        if not 1 <= len(limits) <= MAX_LIMITS:
            raise L.OvoHipError(f"FernDatabase: 1 .. {MAX_LIMITS} limits (got {len(limits)})")
        seq, slot = self.ring.next()
        L.check(L.load().ovo_fern_search(L.ptr(code), L.ptr(self.codes), self.n, self.table.words, (C.c_int32 * len(limits))(*limits), len(limits), int(k),
                                         L.ptr(dist_out), C.c_void_p(slot), seq, L.ptr(self.ws), self.ws.numel(), L.stream()))
        self._pending[seq] = (len(limits), int(k))
        return seq

    def wait(self, seq: int) -> List[Tuple[np.ndarray, np.ndarray]]:
        n_limits, k = self._pending.pop(seq)
        return decode_lists(self.ring.wait(seq), n_limits, k)

    def search(self, code: torch.Tensor, limits: Sequence[int], k: int, dist_out: Optional[torch.Tensor] = None):
        return self.wait(self.queue(code, limits, k, dist_out))
