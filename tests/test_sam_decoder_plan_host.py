"""The launch plan of `HipSamDecoder.forward`, on the CPU: which entry points it calls, in which order, with which scalars, strides and descriptor
fields, and which buffer (and byte offset into it) every pointer names -- against tests/golden/sam_decoder_plan.json (written by
tools/gen_sam_decoder_plan.py with the decoder as it was BEFORE a change that must not move a launch; the test compares with the file, never with the
code under test).  Needs neither a GPU nor the built library: `L.load` returns a stand-in that records every call and answers 0, or
OVO_E_UNSUPPORTED for the entry points a case lists; `L.dev` / `L.stream` are pass-throughs; the forward runs over CPU tensors.  Inputs are zeros,
weights `random_state(spec)`: only their addresses matter.  One case per path through the Python: every knob, depth 1 / 2 / 3 (the layer that is
neither first nor last exists from depth 3 on), head dims with and without a dedicated attention kernel, every fused entry point refusing.

Per case the golden holds the sha256 of the canonical JSON of the whole trace, the number of calls and the count per entry point; the traces
themselves are written by `tools/gen_sam_decoder_plan.py --dump DIR` (diff a dump of the tree at hand against one made at the golden's commit)."""
import collections
import ctypes as C
import dataclasses
import hashlib
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_decoder_plan.json")
STREAM = 0x5712EA00                 # what the patched L.stream() hands out: recorded as "stream"
FUSED = ("ovo_sam_linear", "ovo_sam_t2i_attention", "ovo_sam_proj_ln", "ovo_sam_up1_ln", "ovo_sam_up2_masks")


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    card: str = "sam2_test"
    spec: tuple = ()                # (field, value) pairs for dataclasses.replace on SPECS[card]
    multimask: bool = True
    force_unfused: bool = False     # set on the instance after construction
    res16: bool = True              # sam_decoder.RES16, patched before construction
    env: tuple = ()                 # (name, value) pairs, set before construction
    unsupported: tuple = ()         # entry points of the stand-in that answer OVO_E_UNSUPPORTED (plan test only)


CASES = [
    Case("T"),
    Case("T-single_mask", multimask=False),
    Case("T-force_unfused", force_unfused=True),
    Case("T-RES16=0", res16=False),
    Case("T-OVO_Q_PRESCALE=0", env=(("OVO_Q_PRESCALE", "0"),)),
    Case("T-depth3", spec=(("depth", 3),)),
    Case("T-depth1", spec=(("depth", 1),)),
    Case("T-heads8", spec=(("heads", 8),)),                 # head dims 16 / 8: the generic attention in both directions
    Case("sam2_small", card="sam2_small"),
    # no fused instantiation at this width, but the stand-in accepts everything: the Python-side conditions only (head dims 48 / 24)
    Case("T-hidden384-heads8", spec=(("hidden", 384), ("heads", 8))),
] + [Case(f"T-no-{name}", unsupported=(name,)) for name in FUSED] + [Case("T-no-fused", unsupported=FUSED)]
GPU_CASES = CASES[:9]               # tests/test_gpu_sam_decoder_bits.py: the cases the real library runs


def case_spec(case):
    from ovo_amd.encoders.sam_decoder import SPECS
    return dataclasses.replace(SPECS[case.card], **dict(case.spec))


def prompts(spec, n_side=3, n=5):
    """An odd number of clicks: the first five of the 3 x 3 grid."""
    from ovo_amd.encoders.sam_decoder import point_grid
    return point_grid(n_side)[:n] * spec.image_size


def make_decoder(case, mp, state, device, pts=None):
    """HipSamDecoder of a case with its prompts set; `mp` (a pytest MonkeyPatch) carries the case's environment and RES16."""
    from ovo_amd.encoders import sam_decoder as SD
    mp.delenv("OVO_Q_PRESCALE", raising=False)
    for k, v in case.env:
        mp.setenv(k, v)
    mp.setattr(SD, "RES16", case.res16)
    spec = case_spec(case)
    dec = SD.HipSamDecoder(spec, state, device=device)
    if case.force_unfused:
        dec.force_unfused = True
    dec.set_points(prompts(spec) if pts is None else pts)
    return dec


class Recorder:
    """Stands in for the loaded library: every attribute is an entry point that records (name, arguments) and answers 0 or OVO_E_UNSUPPORTED."""

    def __init__(self, unsupported, e_unsupported):
        self.calls, self._unsupported, self._e = [], frozenset(unsupported), e_unsupported

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append([name] + [self._arg(a) for a in args])
            return self._e if name in self._unsupported else 0
        return entry

    @staticmethod
    def _pointer(v):
        return ("ptr", int(v or 0))

    def _arg(self, a):
        if isinstance(a, (int, float)):
            return a
        if isinstance(a, C.c_void_p):
            return self._pointer(a.value)
        s = a._obj                                          # byref(struct): field by field
        return {n: self._pointer(getattr(s, n)) if t is C.c_void_p else getattr(s, n) for n, t in s._fields_}


def _span(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _labelled(calls, named, temps):
    """The trace with every ("ptr", address) replaced by its label: null / stream / "<name>+<byte offset>" / "t<k>+<offset>" (k: order of first
    appearance in the trace) / ext."""
    order = {}

    def label(addr):
        if addr == 0:
            return "null"
        if addr == STREAM:
            return "stream"
        for name, (lo, hi) in named:
            if lo <= addr < hi:
                return f"{name}+{addr - lo}"
        for i, (lo, hi) in enumerate(temps):
            if lo <= addr < hi:
                return f"t{order.setdefault(i, len(order))}+{addr - lo}"
        return "ext"

    def walk(v):
        if isinstance(v, tuple):
            return label(v[1])
        if isinstance(v, dict):
            return {k: walk(x) for k, x in v.items()}
        return v
    return [[c[0]] + [walk(v) for v in c[1:]] for c in calls]


def trace_case(case, mp, pts=None):
    """The labelled trace of one forward of `case`."""
    from ovo_amd import _lib as L
    from ovo_amd.encoders.sam_decoder import random_state
    spec = case_spec(case)
    rec = Recorder(case.unsupported, L.E_UNSUPPORTED)
    mp.setattr(L, "load", lambda: rec)
    mp.setattr(L, "dev", lambda t, dtype, name="tensor": t)
    mp.setattr(L, "stream", lambda: C.c_void_p(STREAM))
    dec = make_decoder(case, mp, random_state(spec), "cpu", pts)
    s, c = spec.embed_size, spec.hidden
    inputs = {"emb": torch.zeros(s, s, c), "f1": torch.zeros(2 * s, 2 * s, c // 4), "f0": torch.zeros(4 * s, 4 * s, c // 8)}
    temps, empty = [], torch.empty

    def keep(*a, **kw):                                     # every temporary stays alive: one address range each
        temps.append(empty(*a, **kw))
        return temps[-1]
    mp.setattr(torch, "empty", keep)
    try:
        out = dec.forward(inputs["emb"], inputs["f1"], inputs["f0"], multimask=case.multimask)
    finally:
        mp.setattr(torch, "empty", empty)
    named = sorted((k, _span(t)) for k, t in list(dec.w.items()) + list(inputs.items()) + [("tokens0", dec.tokens0), ("tok16", dec.tok16)])
    trace = _labelled(rec.calls, named, [_span(t) for t in temps])
    del out
    return trace


def canonical(trace):
    return json.dumps(trace, sort_keys=True, separators=(",", ":"))


def summary(trace):
    return {"sha256": hashlib.sha256(canonical(trace).encode()).hexdigest(), "calls": len(trace),
            "per_entry": dict(sorted(collections.Counter(c[0] for c in trace).items()))}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_forward_launch_plan(case, golden, monkeypatch):
    got, want = summary(trace_case(case, monkeypatch)), golden[case.id]
    print(f"{case.id}: {got['calls']} calls {got['per_entry']}")
    assert got["per_entry"] == want["per_entry"] and got["calls"] == want["calls"]
    assert got["sha256"] == want["sha256"], "same entry points, other arguments, buffers or order: diff `tools/gen_sam_decoder_plan.py --dump` outputs"


def test_harness_counts_the_calls_of_a_four_prompt_forward(monkeypatch):
    """The recorder against call counts taken by hand from the decoder (2 x 2 clicks): a harness that drops or doubles calls shows here, not in a digest."""
    from ovo_amd.encoders.sam_decoder import SPECS, point_grid
    want = {"T": 60, "T-force_unfused": 62, "T-depth3": 78, "T-depth1": 42, "sam2_small": 60}
    by_id = {c.id: c for c in CASES}
    for cid, n in want.items():
        with monkeypatch.context() as mp:
            trace = trace_case(by_id[cid], mp, point_grid(2) * case_spec(by_id[cid]).image_size)
        assert len(trace) == n, (cid, len(trace))
        if cid == "T":
            assert summary(trace)["per_entry"] == {"ovo_attention": 2, "ovo_gemm": 38, "ovo_row_epilogue": 8, "ovo_sam_i2t_attention": 2, "ovo_sam_linear": 3,
                                                   "ovo_sam_proj_ln": 2, "ovo_sam_t2i_attention": 3, "ovo_sam_up1_ln": 1, "ovo_sam_up2_masks": 1}
    four = Case("four", unsupported=("ovo_sam_linear", "ovo_sam_t2i_attention", "ovo_sam_up1_ln", "ovo_sam_up2_masks"))
    with monkeypatch.context() as mp:
        assert len(trace_case(four, mp, point_grid(2) * SPECS["sam2_test"].image_size)) == 68
