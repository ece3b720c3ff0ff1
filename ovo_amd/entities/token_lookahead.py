"""ViT tokens computed ahead of the pooling that reads them (MI355X extension, no counterpart in the reference).

The mask-independent half of `OVO._extract_clip` -- the TextRegion crops' ViT forward (textregion.py:141-142 via :197-199) -- runs for one
or SEVERAL keyframes' images in ONE forward on a side HIP stream, so that it overlaps the tracking stage and the SAM2 encoder.  The reference
defers a keyframe's descriptors by `kf_queue_delay` keyframes anyway (ovo.yaml:53, ovo.py:326-332); B images' crops together make the
encoder GEMMs B times taller (M = B x 2 x 577 for PE-L/14-336 on 640x480), which is what fills 256 CUs.

One object, one set of rules:
  * two token slots, used alternately: batch k+1 is encoded while batch k is pooled; the forward of batch k+2 waits for the last reader of
    batch k (`free`) and is refused while batch k still has unread images (`left`);
  * `take(image)` -> pool -> `release(image)` reads an image's slice (same image OBJECT: the map is keyed by identity); `discard(image)`
    gives it up unread;
  * the encoder's workspace is shared with every forward issued elsewhere: such a forward runs inside `workspace()`, which orders it after the
    newest look-ahead forward and the next look-ahead forward after it.
"""
from __future__ import annotations

import contextlib
import os
from typing import Dict

import torch

from .. import _lib as L
from ..utils.streams import side_stream


class TokenLookahead:
    def __init__(self, textregion, device) -> None:
        self.tr = textregion
        # (a high stream priority for this forward was measured: no effect on MI355X, 167 vs 168 frames/s)
        self.stream = side_stream(device, "OVO_VIT_CUS", int(os.environ.get("OVO_VIT_PRIORITY", "0")))
        self.widest = 0                                           # most images one forward has carried
        self._slots = [dict(batch=None, tokens=None, free=None, left=0) for _ in range(2)]
        self._next = 0                                            # the slots alternate, whatever happens to their images
        self.reset()

    def reset(self) -> None:
        """Forget every pending image; the slots keep their buffers.  Only when nothing of the look-ahead is in flight (after a synchronize)."""
        for slot in self._slots:
            slot["left"], slot["free"] = 0, None
        self._pending: Dict[int, tuple] = {}                      # id(image) -> (image, tokens, done, slot)
        self._single = None                                       # the image of an `encode_one` nobody has read yet
        self._newest = None                                       # `done` of the newest look-ahead forward
        self._outside = None                                      # end of a forward in `workspace()` since then
        self._last_read = None                                    # newest point of a reader's stream: last `release` of a slot, or `_outside`

    def idle(self) -> bool:
        """No image pending and no slot in use: everything encoded was read or discarded."""
        return not self._pending and all(slot["left"] == 0 for slot in self._slots)

    def encode(self, images, ready=(), stream=None) -> bool:
        """One forward for all `images` (HWC u8 frames of one size, on the GPU); False when they are not.  It waits for the slot's last reader
        and for the `ready` events (the images' uploads, when they are still in flight) -- not for the caller's stream, whose queue holds the
        previous keyframes' tails this forward should overlap.  `stream`: measurement runs that fold the forward onto the caller's stream."""
        images = list(images)
        if not images or not all(isinstance(i, torch.Tensor) and i.is_cuda for i in images):
            return False
        slot = self._slots[self._next]
        if slot["left"] > 0:
            raise L.OvoHipError("TokenLookahead.encode: the batch before the previous one still has unconsumed images")
        self._next ^= 1
        tr, dev = self.tr, images[0].device
        h, w = images[0].shape[:2]
        crops = tr.forward_crops(h, w)
        nc, spec = len(crops), tr.vlm.spec
        n = len(images) * nc
        if slot["batch"] is None or slot["batch"].shape[0] < n:
            slot["batch"] = torch.empty((n, 3, spec.image_size, spec.image_size), dtype=torch.float32, device=dev)
            slot["tokens"] = torch.empty((n, spec.tokens, spec.width), dtype=torch.float32, device=dev)
        side = stream if stream is not None else self.stream
        for ev in (slot["free"], self._outside, *ready):
            if ev is not None:
                side.wait_event(ev)
        slot["free"] = self._outside = None
        with torch.cuda.stream(side):
            srcs = [image if image.dtype == torch.uint8 and image.is_contiguous() else image.permute(2, 0, 1).contiguous() for image in images]   # HWC u8: read in place
            tr.vlm.preprocess_batch(srcs, crops, scale=1.0 / 255.0, out=slot["batch"][:n])      # every frame's crops in one launch
            tr.vlm.forward(slot["batch"][:n], tokens=True, out=slot["tokens"][:n])
            done = torch.cuda.Event()
            done.record(side)
        slot["left"] = len(images)
        self._newest = done
        self.widest = max(self.widest, len(images))
        for k, image in enumerate(images):
            self._pending[id(image)] = (image, slot["tokens"][k * nc:(k + 1) * nc], done, slot)
        return True

    def encode_one(self, image, ready=None) -> bool:
        """A look-ahead of one for a caller that names no successor: an earlier one nobody read is dropped, never refused.  The image may have
        been produced on the caller's stream, so the forward is ordered after that stream's newest reader of the look-ahead (past it lies the
        previous keyframe's tail, which the forward overlaps) -- or, before the first reader, after everything queued on it so far."""
        if self._single is not None:
            self.discard(self._single)
        after = self._last_read
        if after is None:
            after = torch.cuda.Event()
            after.record()
        if not self.encode([image], [after, ready]):
            return False
        self._single = image
        return True

    def take(self, image):
        """The tokens of `image`, or None when it was not encoded ahead; the current stream waits for the forward.  Follow the pooling with
        `release(image)`.  A look-ahead of one for ANOTHER image ends here."""
        if self._single is not None and self._single is not image:
            self.discard(self._single)
        hit = self._pending.get(id(image))
        if hit is None or hit[0] is not image:
            return None
        torch.cuda.current_stream().wait_event(hit[2])
        return hit[1]

    def release(self, image) -> None:
        """After the pooling that read `image`'s tokens, on the stream it ran on."""
        hit = self._drop(image)
        if hit is not None:
            slot = hit[3]
            slot["free"] = torch.cuda.Event()                      # (the slot's newest reader; waited for once none of its images is left)
            slot["free"].record()
            if slot["left"] == 0:
                self._last_read = slot["free"]

    def discard(self, image) -> None:
        """A keyframe that gets no descriptor (no mask tracked, or every instance dropped by the top-k view filter) never pools: its share of
        the slot is released here, or the slot would stay "in use" and the forward two groups later would be refused."""
        hit = self._drop(image)
        if hit is not None and hit[3]["free"] is None:             # nobody has read the slot: it is free once the tokens exist
            hit[3]["free"] = hit[2]

    def _drop(self, image):
        hit = self._pending.get(id(image))
        if hit is None or hit[0] is not image:
            return None
        del self._pending[id(image)]
        if image is self._single:
            self._single = None
        hit[3]["left"] -= 1
        return hit

    @contextlib.contextmanager
    def workspace(self):
        """Around an encoder forward issued outside the look-ahead, on the current stream: it uses the same workspace, so it starts after the
        newest look-ahead forward, and the next look-ahead forward starts after it."""
        if self._newest is not None:
            torch.cuda.current_stream().wait_event(self._newest)
        yield
        self._outside = self._last_read = torch.cuda.Event()
        self._outside.record()
