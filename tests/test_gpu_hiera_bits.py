"""-m gpu: whole `ovo_hiera_forward` calls give the bits, the workspace size and the launch counts recorded in tests/golden/hiera_digests.json (written
by tools/gen_hiera_digests.py with the library as built BEFORE a change that must not move any of them; the test compares with the file, never with
the code under test).  One case per path through the forward -- the fused form of every step, each of its fall-backs, every knob -- each at the
smallest shape where that path still runs.  Inputs and weights come from integer arithmetic alone (`values` of test_gpu_stream_bits.py): norm weights
near 1, matrices scaled by fan-in^-1/2.  A second group of tests runs the forward in a workspace of exactly `ovo_hiera_workspace_bytes` with guard
bytes behind it."""
import contextlib
import ctypes as C
import dataclasses
import functools
import hashlib
import json
import os

import pytest
import torch

from test_gpu_stream_bits import values

DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hiera_digests.json")
GUARD_BYTES, GUARD = 4096, 0x5A

_B1024 = ("hiera_b+", 1024, 1, True)
# (card, image size, batch, hi_res, environment)
CASES = [
    # 1024 windows >= the fused window attention's 512; stage 2 = exactly 16384 tokens (the streaming kernels' minimum); stage 3 = 64 x 64 under 14 x 14
    # windows (padding windows); the global blocks; the fused neck at both levels
    _B1024 + ({},),
    # 256 windows: three-launch attention, stage-1 QKV through the streaming GEMM with its pooled-q epilogue at the stage change; stage 2 < 16384 rows:
    # k_ln_window, the tiled GEMMs, the two-pass neck at level 1 beside the fused one at level 0
    ("hiera_b+", 512, 1, True, {}),
    # head dim 72 (no fused attention), the K = 192 streaming shapes, window spec (8, 4, 16, 8)
    ("hiera_l", 512, 1, True, {}),
    # width 32: no streaming form at all -- im2col patch path, k_qpool, k_pool_unwindow, k_cast_pad; without hi_res the lateral copies
    ("hiera_test", 256, 2, True, {}),
    ("hiera_test", 256, 2, False, {}),
] + [_B1024 + ({k: "1"},) for k in ("OVO_NO_LN_FOLD", "OVO_HIERA_NO_WINATTN", "OVO_NO_MLP_FUSE", "OVO_HIERA_PROJ_LN", "OVO_HIERA_PATCH_GEMM",
                                    "OVO_HIERA_NECK_TWO_PASS")] + [
    # cfg->q_prescaled == 0 (read when the encoder is built): no fused attention, `scale` passed to ovo_attention
    _B1024 + ({"OVO_Q_PRESCALE": "0"},),
    # the chunked FC1 / FC2 loop needs a hidden block above 200 MB: more than 234 057 rows at width 112, B = 4 is the smallest batch that gets there
    ("hiera_b+", 1024, 4, True, {"OVO_NO_MLP_FUSE": "1", "OVO_HIERA_MLP_CHUNK_MB": "48"}),
]


def case_id(case):
    card, size, batch, hi_res, env = case
    return "-".join([card, str(size), f"B{batch}"] + ([] if hi_res else ["no_hi_res"]) + [f"{k}={v}" for k, v in sorted(env.items())])


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def _state(card):
    """The keys and shapes of random_state(spec), filled from `values`: a state depends on the card alone, not on image size or hi_res."""
    from ovo_amd.encoders.hiera import SPECS, random_state
    sd = {}
    for j, (key, t) in enumerate(random_state(SPECS[card]).items()):
        shape, c = tuple(t.shape), 1000 + 7 * j
        if key.endswith(("norm1.weight", "norm2.weight")):
            v = 1 + values(shape, c, 0.1)
        elif "pos_embed" in key:
            v = values(shape, c, 0.05)
        elif key.endswith(".weight"):                        # matrices and 1 x 1 / 7 x 7 convolutions: [out, fan-in ...]
            v = values(shape, c, 1.7) * (t[0].numel() ** -0.5)
        else:                                                # biases
            v = values(shape, c, 0.05)
        sd[key] = v
    return sd


_ENCODERS = {}


def _encoder(case):
    from ovo_amd.encoders.hiera import SPECS, HipHiera
    card, size, _, hi_res, env = case
    key = (card, size, hi_res, env.get("OVO_Q_PRESCALE"))
    if key not in _ENCODERS:
        spec = dataclasses.replace(SPECS[card], image_size=size, hi_res=hi_res)
        _ENCODERS[key] = HipHiera(spec, _state(card), device=DEV)        # (inside the case's environment: OVO_Q_PRESCALE is read here)
    return _ENCODERS[key]


@functools.lru_cache(maxsize=None)
def _image(size, batch):
    return values((batch, 3, size, size), 77, 2.0).to(DEV)


def _digest(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def run_case(case, ws=None):
    """One forward for the bits, a second one under the library's profiler for the launch counts (and the same bits again).  `ws`: the workspace tensor
    to run in instead of the encoder's own."""
    from ovo_amd import _lib as L
    lib = L.load()
    _, size, batch, _, env = case
    with _environment(env):
        enc = _encoder(case)
        x = _image(size, batch)
        need = int(lib.ovo_hiera_workspace_bytes(C.byref(enc._cfg), batch))
        enc._ws = ws
        try:
            feats = enc.forward(x)
            torch.cuda.synchronize()
            rec = {f"feat{i}": _digest(f) for i, f in enumerate(feats)}
            for i, f in enumerate(feats):                    # the inputs are sane: no NaN that would make every path look alike, nothing saturated
                rms = f.double().pow(2).mean().sqrt().item()
                print(f"{case_id(case)} feat{i} {tuple(f.shape)}: rms {rms:.4g}")
                assert bool(torch.isfinite(f).all()) and 1e-3 < rms < 1e3
            L.check(lib.ovo_profile_start())
            again = enc.forward(x)
            ms, work, n = (C.c_double * 9)(), (C.c_double * 9)(), (C.c_int64 * 9)()
            L.check(lib.ovo_profile_stop(ms, work, n, 9))
            assert [_digest(f) for f in again] == [rec[f"feat{i}"] for i in range(3)], "two forwards of the same input differ"
        finally:
            enc._ws = None                                   # (the B = 4 workspace is gigabytes: not kept beside the cached encoder)
    rec["workspace_bytes"] = need
    rec["launches"] = [int(v) for v in n]
    return rec


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_hiera_forward_bits_workspace_and_launches(case, golden):
    got, want = run_case(case), golden[case_id(case)]
    print(f"{case_id(case)}: workspace {got['workspace_bytes']} bytes, launches {got['launches']}")
    assert got["workspace_bytes"] == want["workspace_bytes"]
    assert got["launches"] == want["launches"]
    assert {k: got[k] for k in ("feat0", "feat1", "feat2")} == {k: want[k] for k in ("feat0", "feat1", "feat2")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES[:3], ids=case_id)
def test_hiera_forward_stays_inside_its_workspace(case, golden):
    """The forward gets `ovo_hiera_workspace_bytes` as ws_bytes (HipHiera.forward passes the size it asked for, not the tensor's) inside a tensor with 4096
    guard bytes behind them: they stay as they were.  The workspace starts as 0x5A bytes instead of whatever the allocator held, and the outputs are the
    golden ones: nothing reads a workspace byte before the forward wrote it."""
    from ovo_amd import _lib as L
    enc = _encoder(case)
    with _environment(case[4]):
        need = int(L.load().ovo_hiera_workspace_bytes(C.byref(enc._cfg), case[2]))
    ws = torch.full((need + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=DEV)
    got = run_case(case, ws)
    assert got["workspace_bytes"] == need == golden[case_id(case)]["workspace_bytes"]
    assert bool((ws[need:] == GUARD).all()), "bytes behind the workspace were written"
    assert {k: got[k] for k in ("feat0", "feat1", "feat2")} == {k: golden[case_id(case)][k] for k in ("feat0", "feat1", "feat2")}
