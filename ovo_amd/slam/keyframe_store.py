"""The kept keyframe pyramids of `IcpTracker` (DESIGN.md sections 16 and 24): ONE bounded store, by keyframe index, that both `LoopCloser` (loop
verification) and `Relocaliser` (relocalisation in model="keyframe") draw their references from.  A keyframe enters when the tracker moves on from
it; when the store is full the oldest leaves -- it stays a node of the pose graph and a row of the fern database, but is no longer a candidate --
and its buffer is handed back to take the next frame."""
from __future__ import annotations

from typing import Dict, List, Optional

from ..utils import icp_utils as U


class KeyframeStore:
    def __init__(self, capacity: int) -> None:
        self.capacity = int(capacity)
        self._frames: Dict[int, U.Frame] = {}              # oldest first

    def put(self, k: int, frame: U.Frame) -> None:
        """Keeps keyframe k's pyramid (again, when it is there already: a relocalised tracker moves on from an old keyframe a second time)."""
        self._frames.setdefault(int(k), frame)

    def trim(self, keep: Optional[int] = None):
        """The pyramid buffer of the oldest keyframe when there is one too many, else None.  `keep`: a keyframe that stays whatever its age (the
        one a relocalised tracker is aligning against)."""
        if len(self._frames) <= self.capacity:
            return None
        oldest = next(k for k in self._frames if k != keep)
        return self._frames.pop(oldest).pyramid

    def keys(self) -> List[int]:
        return list(self._frames)

    def __contains__(self, k) -> bool:
        return int(k) in self._frames

    def __getitem__(self, k) -> U.Frame:
        return self._frames[int(k)]

    def __len__(self) -> int:
        return len(self._frames)

    def release(self) -> None:
        self._frames = {}
