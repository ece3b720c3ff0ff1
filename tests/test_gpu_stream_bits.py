"""-m gpu: the three row-streaming kernels (k_mlp_stream, k_neck_stream, k_gemm_stream's f32-A form) give the bits recorded in
tests/golden/stream_digests.json -- one sha256 per output tensor, written by tools/gen_stream_digests.py.  The three kernels load their rows with the
same arithmetic (f32 rows -> LayerNorm / cast -> bf16 A fragments) and the first two share loader and two-product core (csrc/stream2.h); whoever moves
that code must not move a bit.  Inputs come from integer arithmetic alone (no library's random stream), weights are rounded to bf16 by torch.  Every output has 64 sentinel
rows behind it."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest
import torch

DEV = "cuda"
ROWS = 16384 + 5            # the smallest stream the kernels accept + a ragged last block; most waves of the last workgroup lie wholly past the end
GUARD = 7.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_digests.json")

MLP = [(112, 128), (224, 256), (96, 128), (192, 192), (144, 192), (288, 320)]                    # (d, k1): the default launch shapes
NECK = [(112, 128, 256, 32), (224, 256, 256, 64)]                                                # (d, k1, hid, n_out): weights resident / chunked
# (K, N, d, mode, window (B, H, W, wh, ww) or None, pool2x2, out dtype)
GEMM = [(K, N, d, mode, None, 0, "bf16") for K, N, d in ((128, 336, 112), (192, 144, 144), (256, 64, 224)) for mode in (1, 2)] + [
    (128, 336, 112, 1, (1, 125, 125, 8, 8), 0, "bf16"),       # 16 x 16 windows of 8 x 8 over a 125 x 125 grid: 16384 product rows, 759 of them padding
    (128, 224, 112, 1, (1, 128, 128, 8, 8), 1, "f32")]        # the stage-change skip path: 2 x 2 max-pool in the epilogue, 4096 rows out
CASES = [("mlp",) + c for c in MLP] + [("neck",) + c for c in NECK] + [("gemm",) + c for c in GEMM]


def case_id(case):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in case)


def values(shape, c, scale=2.0):
    """f32 values in about [-scale, scale): element i is hash(i * 2654435761 + c) / 2^32, all in uint64 arithmetic reduced mod 2^32."""
    n = int(np.prod(shape))
    v = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(c)) & np.uint64(0xFFFFFFFF)
    v = ((v ^ (v >> np.uint64(15))) * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    v = ((v ^ (v >> np.uint64(13))) * np.uint64(3266489917)) & np.uint64(0xFFFFFFFF)
    v = v ^ (v >> np.uint64(16))
    return torch.from_numpy(((v.astype(np.float64) / 2.0 ** 32 - 0.5) * (2.0 * scale)).astype(np.float32).reshape(shape))


def _weight(n, k, d, c):
    """bf16 [n, k]; columns d .. k (the K padding) are zeros"""
    w = torch.zeros(n, k, dtype=torch.bfloat16)
    w[:, :d] = (values((n, d), c) * d ** -0.5).to(torch.bfloat16)
    return w.to(DEV)


def _digest(t):
    t = t.contiguous().cpu()
    return hashlib.sha256((t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy().tobytes()).hexdigest()


def run_case(case):
    """Runs one case; returns (the output rows, the 64 rows behind them)."""
    from ovo_amd import _lib as L
    lib = L.load()
    kind = case[0]
    if kind == "mlp":
        d, k1 = case[1:]
        hid = 4 * d
        x = torch.cat([values((ROWS, d), 1) + 0.5, torch.full((64, d), GUARD)]).to(DEV)
        gamma, beta = (values((d,), 2, 0.5) + 1).to(DEV), values((d,), 3, 0.1).to(DEV)
        w1, w2 = _weight(hid, k1, d, 4), _weight(d, hid, hid, 5)
        b1, b2 = values((hid,), 6, 1.0).to(DEV), values((d,), 7, 1.0).to(DEV)
        L.check(lib.ovo_mlp_f32(x.data_ptr(), ROWS, d, gamma.data_ptr(), beta.data_ptr(), 1e-6, w1.data_ptr(), k1, b1.data_ptr(), hid, w2.data_ptr(), hid,
                                b2.data_ptr(), L.stream()))
        torch.cuda.synchronize()
        return x[:ROWS], x[ROWS:]
    if kind == "neck":
        d, k1, hid, n_out = case[1:]
        x = (values((ROWS, d), 11) + 0.5).to(DEV)
        w1, w2 = _weight(hid, k1, d, 12), _weight(n_out, hid, hid, 13)
        b1, b2 = values((hid,), 14, 1.0).to(DEV), values((n_out,), 15, 1.0).to(DEV)
        out = torch.full((ROWS + 64, n_out), GUARD, device=DEV)
        L.check(lib.ovo_neck_f32(x.data_ptr(), ROWS, d, w1.data_ptr(), k1, b1.data_ptr(), hid, w2.data_ptr(), hid, b2.data_ptr(), out.data_ptr(), n_out,
                                 L.stream()))
        torch.cuda.synchronize()
        return out[:ROWS], out[ROWS:]
    K, N, d, mode, win, pool, dt = case[1:]
    if win is None:
        M, rows_src = ROWS, ROWS
    else:
        B, H, W, wh, ww = win
        M, rows_src = B * -(-H // wh) * -(-W // ww) * wh * ww, B * H * W
        assert M >= 16384
    x = (values((rows_src, d), 21) + 0.5).to(DEV)
    gamma, beta = (values((d,), 22, 0.5) + 1).to(DEV), values((d,), 23, 0.1).to(DEV)
    w, bias = _weight(N, K, d, 24), values((N,), 25, 1.0).to(DEV)
    rows_out = M // 4 if pool else M
    out = torch.full((rows_out + 64, N), GUARD, dtype=torch.float32 if dt == "f32" else torch.bfloat16, device=DEV)
    q = L.gemm_desc(None, w, out, bias=bias, rows=M, ldc=N)
    wd = None
    if win is not None:
        wd = L.Window()
        wd.B, wd.H, wd.W, wd.wh, wd.ww = win
    L.check(lib.ovo_gemm_f32a(C.byref(q), C.byref(wd) if wd is not None else None, x.data_ptr(), d, gamma.data_ptr(), beta.data_ptr(), 1e-6, mode, pool,
                              L.stream()))
    torch.cuda.synchronize()
    return out[:rows_out], out[rows_out:]


def digest_of(case):
    out, behind = run_case(case)
    assert behind.shape[0] == 64 and bool((behind == GUARD).all()), "rows behind the end were written"
    return _digest(out)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stream_kernel_bits(case):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert digest_of(case) == golden[case_id(case)]
