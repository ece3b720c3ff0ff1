"""-m gpu: whole `HipSamDecoder.forward` calls give the bits and the launch counts recorded in tests/golden/sam_decoder_digests.json (written by
tools/gen_sam_decoder_digests.py with the decoder as it was BEFORE a change that must not move any of them; the test compares with the file, never with
the code under test).  The cases are those of tests/test_sam_decoder_plan_host.py that the library runs end to end, each one forward over 5 prompts on
a 16 x 16 embedding.  Inputs and weights come from integer arithmetic alone (`values` of test_gpu_stream_bits.py): norm weights near 1, matrices scaled
by fan-in^-1/2, biases and embeddings at 0.05-0.5."""
import ctypes as C
import functools
import hashlib
import json
import os

import pytest
import torch

from test_gpu_stream_bits import values
from test_sam_decoder_plan_host import GPU_CASES as CASES, case_spec, make_decoder

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sam_decoder_digests.json")


@functools.lru_cache(maxsize=None)
def _state(spec):
    """The keys and shapes of random_state(spec), filled from `values`."""
    from ovo_amd.encoders.sam_decoder import random_state
    sd = {}
    for j, (key, t) in enumerate(random_state(spec).items()):
        shape, c = tuple(t.shape), 3000 + 7 * j
        norm = "norm" in key or "output_upscaling.1." in key
        if "gaussian_matrix" in key:
            v = values(shape, c, 1.7)
        elif "embed" in key or "token" in key.rsplit(".", 2)[-2]:   # point / padding / dense embeddings, the output tokens
            v = values(shape, c, 0.1 if key == "no_mem_embed" else 0.5)
        elif norm:
            v = (1 if key.endswith(".weight") else 0) + values(shape, c, 0.1)
        elif key.endswith(".weight"):                                # [out, in] matrices; transposed convolutions [in, out, 2, 2]: fan-in = in
            v = values(shape, c, 1.7) * ((shape[0] if len(shape) == 4 else shape[1]) ** -0.5)
        else:                                                        # biases
            v = values(shape, c, 0.05)
        sd[key] = v
    return sd


@functools.lru_cache(maxsize=None)
def _inputs(s, c):
    return tuple(t.to(DEV) for t in (values((s, s, c), 77, 2.0), values((2 * s, 2 * s, c // 4), 78, 1.0), values((4 * s, 4 * s, c // 8), 79, 1.0)))


def _digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(case):
    """One forward for the bits, a second one under the library's profiler for the launch counts (and the same bits again)."""
    from ovo_amd import _lib as L
    lib = L.load()
    spec = case_spec(case)
    with pytest.MonkeyPatch.context() as mp:
        dec = make_decoder(case, mp, _state(spec), DEV)
        emb, f1, f0 = _inputs(spec.embed_size, spec.hidden)
        out = dec.forward(emb, f1, f0, multimask=case.multimask)
        torch.cuda.synchronize()
        rec = {name: _digest(t) for name, t in zip(("masks", "iou"), out)}
        for name, t in zip(("masks", "iou"), out):           # the inputs are sane: no NaN that would make every path look alike, nothing saturated
            rms = t.double().pow(2).mean().sqrt().item()
            print(f"{case.id} {name} {tuple(t.shape)}: rms {rms:.4g}")
            assert bool(torch.isfinite(t).all()) and 1e-3 < rms < 1e3
        L.check(lib.ovo_profile_start())
        again = dec.forward(emb, f1, f0, multimask=case.multimask)
        ms, work, n = (C.c_double * 9)(), (C.c_double * 9)(), (C.c_int64 * 9)()
        L.check(lib.ovo_profile_stop(ms, work, n, 9))
        assert [_digest(t) for t in again] == [rec["masks"], rec["iou"]], "two forwards of the same input differ"
    rec["launches"] = [int(v) for v in n]
    return rec


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_sam_decoder_forward_bits_and_launches(case, golden):
    got, want = run_case(case), golden[case.id]
    print(f"{case.id}: launches {got['launches']}")
    assert got["launches"] == want["launches"]
    assert (got["masks"], got["iou"]) == (want["masks"], want["iou"])
