"""-m gpu: MFMA GEMM, fused attention, LayerNorm / embedding / resize kernels and the full ViT forward vs fp32
references (plain torch on the same inputs, and oracle/vit.py pinned against HuggingFace CLIP).

Tolerances: bf16 operands carry 8 mantissa bits; products are accumulated in fp32.  Each check states its bound.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import golden, unpack

pytestmark = pytest.mark.gpu


def _bound(out_dim: int) -> float:
    """north_star's feature bound: |unit-descriptor error| <= 1e-3, flat, for every model the reference can select (out_dim >= 512);
    the reduced test towers (out_dim 64 / 128) have proportionally larger elements, 1/sqrt(out_dim)."""
    return 1e-3 if out_dim >= 512 else 1e-3 * (512 / out_dim) ** 0.5 * 1.5
DEV = "cuda"


def _gemm(a, w, bias=None, add=None, act=0, alpha=1.0, out_dtype=torch.float32):
    from ovo_amd import _lib as L
    return L.gemm(a, w, torch.empty((a.shape[0], w.shape[0]), dtype=out_dtype, device=DEV), bias=bias, add=add, act=act, alpha=alpha)


@pytest.mark.parametrize("m,n,k", [(1154, 3072, 1024), (1154, 1024, 4096), (1154, 1024, 1024), (64, 64, 32), (1, 4, 32),
                                   (130, 132, 96), (4097, 336, 224), (300, 1000, 768), (2, 768, 1024), (65536, 112, 160)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gemm_vs_torch(m, n, k, dtype):
    g = torch.Generator(device="cpu").manual_seed(m * 7 + n * 3 + k)
    a = torch.randn(m, k, generator=g).to(DEV, dtype)
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(DEV, dtype)
    bias = torch.randn(n, generator=g).to(DEV)
    ref = a.float() @ w.float().T + bias                      # same rounded operands, fp32 math
    out = _gemm(a, w, bias)
    # fp32 accumulation in a different order: |err| <= ~1e-5 * sum|a||w| ~ 1e-5 * sqrt(k)
    torch.testing.assert_close(out, ref, atol=2e-4, rtol=2e-4)


# a process of its own: one product, then OVO_GEMM_TILE=64x64 set in its own environment, then the product again; prints the kernel kinds the library's
# profiler counted for each (csrc/common.h: 4..7 = the ring kernels' 128x128 / 128x64 / 64x128 / 64x64 tiles)
_KNOB_CHILD = """
import ctypes as C, os, sys
sys.path.insert(0, sys.argv[1])
import torch
from ovo_amd import _lib as L
lib = L.load()
m, n, k = 1154, 3072, 1024
a = torch.randn(m, k).to("cuda", torch.bfloat16)
w = (torch.randn(n, k) * k ** -0.5).to("cuda", torch.bfloat16)
out = torch.empty(m, n, device="cuda")
def kinds():
    L.check(lib.ovo_profile_start())
    L.check(lib.ovo_gemm(C.byref(L.gemm_desc(a, w, out)), L.stream()))
    ms, work, cnt = (C.c_double * 9)(), (C.c_double * 9)(), (C.c_int64 * 9)()
    L.check(lib.ovo_profile_stop(ms, work, cnt, 9))
    return [i for i in range(9) for _ in range(cnt[i])]
first = kinds()
os.environ["OVO_GEMM_TILE"] = "64x64"
print("KINDS", (first, kinds()))
"""


@pytest.mark.parametrize("dynamic", [False, True])
def test_knobs_are_read_once_unless_dynamic(dynamic):
    """The knob contract (csrc/common.h) seen from outside: a process WITHOUT OVO_KNOBS_DYNAMIC that changes OVO_GEMM_TILE after its first product keeps
    the kernel it had; the same process with OVO_KNOBS_DYNAMIC=1 gets the forced 64 x 64 tile (profiler kind 7) on the second product."""
    import ast
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if not k.startswith("OVO_")}
    if dynamic:
        env["OVO_KNOBS_DYNAMIC"] = "1"
    r = subprocess.run([sys.executable, "-c", _KNOB_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    first, second = ast.literal_eval(r.stdout.split("KINDS", 1)[1].strip())
    assert len(first) == 1 and first[0] != 7, first                 # one launch, and not the tile the knob will ask for
    assert second == ([7] if dynamic else first)


def test_gemm_epilogues_and_padding():
    g = torch.Generator().manual_seed(1)
    m, n, k = 577, 256, 128
    a = torch.randn(m, k + 32, generator=g).to(DEV, torch.bfloat16)[:, :k]            # lda > K
    w = (torch.randn(n, k, generator=g) * 0.1).to(DEV, torch.bfloat16)
    bias, add = torch.randn(n, generator=g).to(DEV), torch.randn(m, n, generator=g).to(DEV)
    z = a.float() @ w.float().T
    for act, fn in ((1, torch.nn.functional.gelu), (2, lambda x: x * torch.sigmoid(1.702 * x)),
                    (5, lambda x: torch.nn.functional.gelu(x, approximate="tanh"))):
        torch.testing.assert_close(_gemm(a, w, bias, act=act), fn(z + bias), atol=3e-4, rtol=3e-4)
    torch.testing.assert_close(_gemm(a, w, bias, add=add, alpha=0.5), 0.5 * z + bias + add, atol=3e-4, rtol=3e-4)
    x = add.clone()                                          # in-place residual: C aliases add
    from ovo_amd import _lib as L
    L.gemm(a, w, x, bias=bias, add=x)
    torch.testing.assert_close(x, add + z + bias, atol=3e-4, rtol=3e-4)
    ob = _gemm(a, w, bias, out_dtype=torch.bfloat16)         # bf16 store = RNE of the fp32 result
    assert torch.equal(ob, _gemm(a, w, bias).to(torch.bfloat16))


@pytest.mark.parametrize("tile", ["256x256", "256x128"])
@pytest.mark.parametrize("m,n,k,dtype", [(4616, 3072, 1024, torch.bfloat16), (1154, 1024, 448, torch.bfloat16), (300, 260, 64, torch.bfloat16),
                                         (2308, 1344, 192, torch.float16), (700, 132, 1792, torch.bfloat16), (257, 516, 128, torch.bfloat16),
                                         (513, 260, 320, torch.bfloat16)])
def test_gemm_pingpong_kernel_vs_ring_kernel_and_torch(monkeypatch, tile, m, n, k, dtype):
    """The 256-row ping-pong kernel (gemm8p.hip, forced through OVO_GEMM_TILE) against the fp32 product of the same rounded operands
    and against the 128-row ring kernel: every output element is accumulated over k in the same order (32-wide MFMA steps in
    ascending k), so the two kernels agree BIT FOR BIT -- ragged M / N edges, one to 28 K-tiles, residual and bf16 stores included."""
    g = torch.Generator(device="cpu").manual_seed(m + 3 * n + 7 * k)
    a = torch.randn(m, k + 64, generator=g).to(DEV, dtype)[:, :k]             # lda > K
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(DEV, dtype)
    bias, add = torch.randn(n, generator=g).to(DEV), torch.randn(m, n, generator=g).to(DEV)
    monkeypatch.delenv("OVO_GEMM_TILE", raising=False)
    monkeypatch.setenv("OVO_GELU_POLY", "1")                                 # bit-identity holds for the same GELU form: the ring kernel has the polynomial only
    ring = _gemm(a, w, bias, add=add, act=1)
    ring_b = _gemm(a, w, bias, out_dtype=torch.bfloat16)
    monkeypatch.setenv("OVO_GEMM_TILE", tile)
    out = _gemm(a, w, bias, add=add, act=1)
    out_b = _gemm(a, w, bias, out_dtype=torch.bfloat16)
    ref = torch.nn.functional.gelu(a.float() @ w.float().T + bias) + add
    torch.testing.assert_close(out, ref, atol=3e-4, rtol=3e-4)
    assert torch.equal(out, ring) and torch.equal(out_b, ring_b)
    monkeypatch.delenv("OVO_GELU_POLY")                                      # the default: GELU through the LDS table (gemm_common.h: gelu_lut)
    lut = _gemm(a, w, bias, add=add, act=1)
    torch.testing.assert_close(lut, ref, atol=3e-4, rtol=3e-4)
    assert (lut - out).abs().max() < 4e-5                                    # two approximations of erf-GELU, each within 1e-5 of it
    x = add.clone()                                                          # in-place residual: C aliases add
    from ovo_amd import _lib as L
    L.gemm(a, w, x, bias=bias, add=x)
    torch.testing.assert_close(x, add + a.float() @ w.float().T + bias, atol=3e-4, rtol=3e-4)


@pytest.mark.parametrize("tile", ["256x256", "256x128"])
@pytest.mark.parametrize("m,n,k", [(4616, 3072, 1024), (1154, 1024, 448), (300, 260, 64), (700, 132, 1792), (257, 516, 128), (513, 260, 320)])
def test_gemm_pingpong_mfma32_loop_vs_mfma16_loop_and_torch(monkeypatch, tile, m, n, k):
    """The ping-pong kernel's K-loop on v_mfma_f32_32x32x16_bf16 (OVO_8P_MFMA32=1, gemm8p.hip MF = 32: another accumulator layout, so every staged
    epilogue form walks the accumulators as 4-column pieces) against the 16 x 16 x 32 loop and the fp32 product of the same rounded operands:
    f32 + residual + GELU (generic body), bf16 plain / table GELU (rounded slab), in-place f32 residual (kind 3), rotary (LDS table slice and the
    per-wave form)."""
    from ovo_amd import _lib as L
    dtype = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(m + 3 * n + 7 * k + 1)
    a = torch.randn(m, k + 64, generator=g).to(DEV, dtype)[:, :k]
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(DEV, dtype)
    bias, add = torch.randn(n, generator=g).to(DEV), torch.randn(m, n, generator=g).to(DEV)
    monkeypatch.setenv("OVO_GEMM_TILE", tile)

    def forms():
        out = {"f32_gelu_add": _gemm(a, w, bias, add=add, act=1), "bf16": _gemm(a, w, bias, out_dtype=dtype),
               "bf16_gelu": _gemm(a, w, bias, act=1, out_dtype=dtype), "bf16_qgelu_alpha": _gemm(a, w, bias, act=2, alpha=0.75, out_dtype=dtype)}
        x = add.clone()
        L.gemm(a, w, x, bias=bias, add=x)
        out["f32_inplace"] = x
        return out
    monkeypatch.setenv("OVO_8P_MFMA32", "0")
    ref16 = forms()
    monkeypatch.setenv("OVO_8P_MFMA32", "1")
    got = forms()
    z = a.float() @ w.float().T + bias
    torch.testing.assert_close(got["f32_gelu_add"], torch.nn.functional.gelu(z) + add, atol=3e-4, rtol=3e-4)
    torch.testing.assert_close(got["f32_inplace"], add + z, atol=3e-4, rtol=3e-4)
    for name in got:
        a16, a32 = ref16[name].float(), got[name].float()
        tol = 2e-2 if ref16[name].dtype == dtype else 2e-4                   # bf16 outputs: one ulp where the f32 sums straddle a rounding boundary
        assert (a16 - a32).abs().max() <= tol, (name, float((a16 - a32).abs().max()))
        assert (a16 != a32).float().mean() < 0.02, name                      # ... and only rarely


@pytest.mark.parametrize("m,n,k", [(4616, 3072, 1024), (1154, 1024, 448), (300, 260, 64), (700, 516, 1792), (257, 516, 128), (513, 260, 320), (2308, 1024, 4096)])
def test_gemm_pingpong_merged_intervals_bit_identical(monkeypatch, m, n, k):
    """The 256 x 256 ping-pong kernel with TWO barrier intervals per K-tile (OVO_8P_MERGED=1, gemm8p.hip `body2`: 32 MFMAs per wave between barriers,
    half-tiles restaged one interval after their last read) against the four-phase loop: same fragments, same k order -- every epilogue form
    bit-identical, one to 64 K-tiles (odd and even counts: both buffer parities end a tile), ragged M / N edges."""
    from ovo_amd import _lib as L
    dtype = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(m + 3 * n + 7 * k + 2)
    a = torch.randn(m, k + 64, generator=g).to(DEV, dtype)[:, :k]
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(DEV, dtype)
    bias, add = torch.randn(n, generator=g).to(DEV), torch.randn(m, n, generator=g).to(DEV)
    monkeypatch.setenv("OVO_GEMM_TILE", "256x256")

    def forms():
        out = {"f32_gelu_add": _gemm(a, w, bias, add=add, act=1), "bf16": _gemm(a, w, bias, out_dtype=dtype),
               "bf16_gelu": _gemm(a, w, bias, act=1, out_dtype=dtype), "f32": _gemm(a, w, bias)}
        x = add.clone()
        L.gemm(a, w, x, bias=bias, add=x)
        out["f32_inplace"] = x
        return out
    monkeypatch.setenv("OVO_8P_MERGED", "0")
    ref = forms()
    monkeypatch.setenv("OVO_8P_MERGED", "1")
    for rep in range(3):                                                     # (a synchronisation slip would not show every time)
        got = forms()
        for name in got:
            assert torch.equal(got[name], ref[name]), (name, rep, float((got[name].float() - ref[name].float()).abs().max()))
    torch.testing.assert_close(got["f32"], a.float() @ w.float().T + bias, atol=3e-4, rtol=3e-4)


@pytest.mark.parametrize("b,t,heads,hd", [(8, 577, 16, 64), (5, 50, 4, 72)])
def test_gemm_rope_epilogue_mfma32_loop(monkeypatch, b, t, heads, hd):
    """ovo_gemm_rope through the 32 x 32 x 16 loop (head_dim 64: the LDS table-slice form; 72: the per-wave form) against the 16 x 16 x 32 loop."""
    from ovo_amd import _lib as L
    g0 = torch.Generator().manual_seed(9)
    d, m = heads * hd, b * t
    a = torch.randn(m, d, generator=g0).to(DEV, torch.bfloat16)
    w = (torch.randn(3 * d, d, generator=g0) * d ** -0.5).to(DEV, torch.bfloat16)
    bias = torch.randn(3 * d, generator=g0).to(DEV)
    ang = (torch.rand(t, hd // 2, generator=g0) * 6.28).repeat_interleave(2, dim=1)
    cos, sin = ang.cos().contiguous().to(DEV), ang.sin().contiguous().to(DEV)
    monkeypatch.setenv("OVO_GEMM_TILE", "256x256")
    outs = []
    for mf in ("0", "1"):
        monkeypatch.setenv("OVO_8P_MFMA32", mf)
        out = torch.empty(m, 3 * d, dtype=torch.bfloat16, device=DEV)
        gg = L.gemm_desc(a, w, out, bias=bias)
        rp = L.Rope(cos.data_ptr(), sin.data_ptr(), t, hd, 2 * d, 1)
        L.check(L.load().ovo_gemm_rope(C.byref(gg), C.byref(rp), L.stream()))
        outs.append(out.float())
    assert (outs[0] - outs[1]).abs().max() <= 4e-2 and (outs[0] != outs[1]).float().mean() < 0.02


@pytest.mark.parametrize("m,n,k,act", [(13848, 3072, 1024, 0), (4616, 4096, 1024, 1), (49152, 1344, 448, 0), (4100, 1792, 448, 1), (300, 272, 320, 2),
                                       (70000, 128, 512, 0), (2308, 400, 1792, 5), (65800, 256, 384, 1), (257, 4112, 576, 0)])
def test_gemm_persistent_kernel_vs_pingpong_kernel(monkeypatch, m, n, k, act):
    """The persistent 256 x 128 kernel (gemm8q.hip: one LDS-DMA ring across a workgroup's tiles, a tile's epilogue trickling out behind the
    next tile's K-loop through counted buffer stores) against the one-tile-per-workgroup ping-pong kernel and torch: same k-order per output
    element, same epilogue arithmetic -> BIT-identical bf16 outputs.  Shapes: 1 to 11 tiles per workgroup, ragged M / N edges, 5 to 28 K-tiles
    (one and two drain steps per K-tile), every activation."""
    from ovo_amd import _lib as L
    if L.load().ovo_round_chain_params_bytes() == 0:
        pytest.skip("gemm8q.hip is not in a production build (python -m ovo_amd.build --force --experimental)")
    dtype = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(m + 3 * n + 7 * k)
    a = torch.randn(m, k + 64, generator=g).to(DEV, dtype)[:, :k]             # lda > K
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(DEV, dtype)
    bias = torch.randn(n, generator=g).to(DEV)
    monkeypatch.setenv("OVO_GEMM_TILE", "256x128")
    ref_b = _gemm(a, w, bias, act=act, alpha=0.75, out_dtype=dtype)
    ref_nb = _gemm(a, w, None, act=act, out_dtype=dtype)
    monkeypatch.setenv("OVO_GEMM_TILE", "256x128p")
    from ovo_amd import _lib as L
    lib = L.load()
    L.check(lib.ovo_profile_start())                                         # (the profiler's launch counts show which kernel ran)
    out_b = _gemm(a, w, bias, act=act, alpha=0.75, out_dtype=dtype)
    out_nb = _gemm(a, w, None, act=act, out_dtype=dtype)
    again = _gemm(a, w, bias, act=act, alpha=0.75, out_dtype=dtype)
    ms, work, cnt = (C.c_double * 9)(), (C.c_double * 9)(), (C.c_int64 * 9)()
    L.check(lib.ovo_profile_stop(ms, work, cnt, 9))
    assert cnt[0] == 3
    assert torch.equal(out_b, ref_b) and torch.equal(out_nb, ref_nb) and torch.equal(again, out_b)
    f = {0: lambda x: x, 1: torch.nn.functional.gelu, 2: lambda x: x * torch.sigmoid(1.702 * x), 5: lambda x: torch.nn.functional.gelu(x, approximate="tanh")}[act]
    ref = f(0.75 * (a.float() @ w.float().T) + bias)
    torch.testing.assert_close(out_b.float(), ref, atol=3e-2, rtol=2e-2)


@pytest.mark.parametrize("m,n,k", [(16400, 448, 128), (20000, 336, 128), (16390, 112, 192), (17000, 896, 256), (16384, 256, 256),
                                   (16500, 64, 256), (16384, 32, 256), (16385, 112, 128), (16384, 672, 256), (16384, 256, 128), (16400, 336, 128),
                                   (16400, 576, 192), (16384, 432, 192), (16390, 864, 192), (16384, 256, 192)])
def test_gemm_stream_kernel_vs_tiled_kernel_and_torch(monkeypatch, m, n, k):
    """The weights-resident streaming kernel (gemm_stream.hip: tall short-K products, the automatic choice at M >= 16384, K <= 256) against
    the fp32 product of the same rounded operands and against the tiled kernels (OVO_GEMM_NO_STREAM): both accumulate every output
    element over k in ascending 32-wide MFMA steps, so they agree bit for bit (residual, bf16 stores, ragged M, lda > K included); GELU is the LDS table here and the packed polynomial there: 4e-5."""
    dtype = torch.bfloat16
    g = torch.Generator(device="cpu").manual_seed(m + 3 * n + 7 * k)
    a = torch.randn(m, k + 64, generator=g).to(DEV, dtype)[:, :k]
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(DEV, dtype)
    bias, add = torch.randn(n, generator=g).to(DEV), torch.randn(m, n, generator=g).to(DEV)
    monkeypatch.setenv("OVO_GEMM_NO_STREAM", "1")
    monkeypatch.setenv("OVO_GELU_POLY", "1")                       # the tiled ring kernels' GELU is the packed polynomial
    tiled = _gemm(a, w, bias, add=add, act=1)
    monkeypatch.delenv("OVO_GELU_POLY")
    tiled_lin = _gemm(a, w, bias, add=add)
    tiled_b = _gemm(a, w, bias, out_dtype=torch.bfloat16)
    monkeypatch.delenv("OVO_GEMM_NO_STREAM")
    monkeypatch.setenv("OVO_GEMM_TILE", "stream")                  # forced: an unsupported shape would fall through to a tiled kernel silently
    out = _gemm(a, w, bias, add=add, act=1)                        # GELU through the LDS table (the only form the streaming kernel carries)
    out_lin = _gemm(a, w, bias, add=add)
    out_b = _gemm(a, w, bias, out_dtype=torch.bfloat16)
    out_nb = _gemm(a, w, None, out_dtype=torch.bfloat16, alpha=0.5)
    ref = torch.nn.functional.gelu(a.float() @ w.float().T + bias) + add
    torch.testing.assert_close(out, ref, atol=3e-4, rtol=3e-4)
    torch.testing.assert_close(out_nb.float(), 0.5 * (a.float() @ w.float().T), atol=0.03, rtol=0.01)
    assert torch.equal(out_lin, tiled_lin) and torch.equal(out_b, tiled_b)
    assert (out - tiled).abs().max() < 4e-5                        # table GELU against the polynomial on the same pre-activation bits
    x = add.clone()                                                # in-place residual: C aliases add
    from ovo_amd import _lib as L
    L.gemm(a, w, x, bias=bias, add=x)
    torch.testing.assert_close(x, add + a.float() @ w.float().T + bias, atol=3e-4, rtol=3e-4)


def test_gemm_stream_kernel_unwindow_rows(monkeypatch):
    """ovo_gemm_unwindow on the streaming kernel: window-major product rows land on their spatial rows, padding rows are dropped."""
    from ovo_amd import _lib as L
    B, H, W, wh, ww, n, k = 3, 100, 60, 8, 8, 112, 128              # 13 x 8 windows per image: M = 3 * 104 * 64 = 19968, H and W padded
    nwh, nww = -(-H // wh), -(-W // ww)
    M = B * nwh * nww * wh * ww
    g = torch.Generator().manual_seed(5)
    a = torch.randn(M, k, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(n, k, generator=g) * k ** -0.5).to(DEV, torch.bfloat16)
    bias = torch.randn(n, generator=g).to(DEV)
    res = torch.randn(B * H * W, n, generator=g).to(DEV)
    outs = []
    for mode in ("tiled", "stream"):
        if mode == "tiled":
            monkeypatch.setenv("OVO_GEMM_NO_STREAM", "1")
        else:
            monkeypatch.delenv("OVO_GEMM_NO_STREAM")
            monkeypatch.setenv("OVO_GEMM_TILE", "stream")
        x = res.clone()
        gg, win = L.gemm_desc(a, w, x, bias=bias, add=x, ldc=n), L.Window(B, H, W, wh, ww)      # (x holds the spatial rows, fewer than M)
        L.check(L.load().ovo_gemm_unwindow(C.byref(gg), C.byref(win), L.stream()))
        outs.append(x)
    assert torch.equal(outs[0], outs[1])
    prod = (a.float() @ w.float().T + bias).reshape(B, nwh, nww, wh, ww, n).permute(0, 1, 3, 2, 4, 5).reshape(B, nwh * wh, nww * ww, n)[:, :H, :W]
    torch.testing.assert_close(outs[1], res + prod.reshape(B * H * W, n), atol=3e-4, rtol=3e-4)


@pytest.mark.parametrize("B,H,W,wh,ww,n,k", [(2, 64, 64, 14, 14, 448, 448), (1, 20, 12, 8, 8, 96, 64), (3, 16, 16, 16, 16, 64, 128), (2, 9, 13, 4, 7, 32, 32)])
def test_gemm_unwindow_epilogue_vs_torch(B, H, W, wh, ww, n, k):
    """ovo_gemm_unwindow: rows of the product in window order (padding rows included) land on their spatial rows with the
    residual added -- Hiera's `window_unpartition` + skip connection -- also in place (C aliases add)."""
    from ovo_amd import _lib as L
    g0 = torch.Generator().manual_seed(11)
    nwh, nww = -(-H // wh), -(-W // ww)
    m = B * nwh * nww * wh * ww
    a = torch.randn(m, k, generator=g0).to(DEV, torch.bfloat16)
    w = (torch.randn(n, k, generator=g0) * k ** -0.5).to(DEV, torch.bfloat16)
    bias = torch.randn(n, generator=g0).to(DEV)
    res = torch.randn(B * H * W, n, generator=g0).to(DEV)
    z = (a.float() @ w.float().T + bias).reshape(B, nwh, nww, wh, ww, n).permute(0, 1, 3, 2, 4, 5).reshape(B, nwh * wh, nww * ww, n)
    ref = res + z[:, :H, :W].reshape(B * H * W, n)
    for inplace in (False, True):
        add = res.clone()
        out = add if inplace else torch.full((B * H * W, n), float("nan"), device=DEV)
        gg = L.gemm_desc(a, w, out, bias=bias, add=add, ldc=n)      # (out holds the spatial rows, fewer than m)
        win = L.Window(B, H, W, wh, ww)
        L.check(L.load().ovo_gemm_unwindow(C.byref(gg), C.byref(win), L.stream()))
        torch.testing.assert_close(out, ref, atol=3e-4, rtol=3e-4)
    gg.M = m - 1                                                 # M must be the padded window count
    with pytest.raises(L.OvoHipError):
        L.check(L.load().ovo_gemm_unwindow(C.byref(gg), C.byref(win), L.stream()))


@pytest.mark.parametrize("b,t,heads,hd", [(2, 37, 4, 32), (2, 577, 16, 64), (3, 50, 4, 72)])
def test_gemm_rope_epilogue_vs_rope_kernel_and_torch(b, t, heads, hd):
    """ovo_gemm_rope: the packed QKV projection with q, k rotated in the epilogue == ovo_gemm followed by the stand-alone
    rotation (up to the one bf16 rounding it saves) == the fp32 formula; v and the class-token rows are not rotated."""
    from ovo_amd import _lib as L
    g0 = torch.Generator().manual_seed(7)
    d = heads * hd
    m = b * t
    a = torch.randn(m, d, generator=g0).to(DEV, torch.bfloat16)
    w = (torch.randn(3 * d, d, generator=g0) * d ** -0.5).to(DEV, torch.bfloat16)
    bias = torch.randn(3 * d, generator=g0).to(DEV)
    ang = torch.rand(t, hd // 2, generator=g0) * 6.28
    ang[0] = 0.3                                              # a non-identity row for the class token: must stay unrotated (t0 = 1)
    ang = ang.repeat_interleave(2, dim=1)
    cos, sin = ang.cos().contiguous().to(DEV), ang.sin().contiguous().to(DEV)
    out = torch.empty(m, 3 * d, dtype=torch.bfloat16, device=DEV)
    gg = L.gemm_desc(a, w, out, bias=bias)
    rp = L.Rope(cos.data_ptr(), sin.data_ptr(), t, hd, 2 * d, 1)
    L.check(L.load().ovo_gemm_rope(C.byref(gg), C.byref(rp), L.stream()))
    z = (a.float() @ w.float().T + bias).reshape(b, t, 3, heads, hd)
    x0, x1 = z[..., 0::2], z[..., 1::2]
    c, s = cos.reshape(1, t, 1, 1, hd), sin.reshape(1, t, 1, 1, hd)
    rot = torch.stack([x0 * c[..., 0::2] - x1 * s[..., 0::2], x1 * c[..., 1::2] + x0 * s[..., 1::2]], dim=-1).flatten(-2)
    ref = z.clone()
    ref[:, 1:, :2] = rot[:, 1:, :2]
    torch.testing.assert_close(out.float().reshape(b, t, 3, heads, hd), ref, atol=2e-2, rtol=1.6e-2)     # one bf16 rounding of O(1) values
    two = _gemm(a, w, bias, out_dtype=torch.bfloat16)
    L.check(L.load().ovo_rope_qk(two.data_ptr(), b, t, heads, hd, cos.data_ptr(), sin.data_ptr(), 1, L.stream()))
    torch.testing.assert_close(out.float(), two.float(), atol=4e-2, rtol=3.2e-2)                          # two roundings vs one
    assert torch.equal(out.reshape(b, t, 3, d)[:, :, 2], two.reshape(b, t, 3, d)[:, :, 2])                # v: untouched
    assert torch.equal(out.reshape(b, t, 3 * d)[:, 0], two.reshape(b, t, 3 * d)[:, 0])                    # class token: untouched


@pytest.mark.parametrize("B,H,Tq,Tk,hd", [(2, 16, 577, 577, 64), (1, 4, 197, 197, 64), (64, 2, 16, 64, 56), (3, 1, 49, 196, 96),
                                          (2, 2, 1, 1, 8), (1, 2, 130, 70, 72), (1, 1, 4096, 4096, 56), (2, 8, 257, 257, 128),
                                          (64, 4, 16, 16, 56), (32, 8, 4, 16, 56), (8, 2, 64, 64, 56), (5, 3, 70, 50, 64), (3, 2, 17, 33, 40),   # Tk <= 64: trimmed / tiny forms
                                          (7, 3, 49, 49, 64), (9, 1, 33, 17, 24), (1, 1, 1, 64, 64), (130, 2, 16, 64, 56), (3, 2, 64, 1, 8),    # one wave per (batch, head) pair
                                          (6, 2, 196, 196, 56), (2, 2, 196, 200, 64), (2, 1, 300, 280, 64),                                   # last key tile mostly padding
                                          (40, 16, 577, 577, 64), (1, 1, 577, 592, 64), (2, 3, 100, 65, 48), (3, 2, 900, 128, 64), (1, 2, 31, 593, 64)])   # K / V resident in LDS (65..592 keys)
def test_attention_vs_torch(B, H, Tq, Tk, hd):
    from ovo_amd import _lib as L
    g = torch.Generator().manual_seed(B + H + Tq + Tk + hd)
    D = H * hd
    T = max(Tq, Tk)
    qkv = torch.randn(B, T, 3, H, hd, generator=g).to(DEV, torch.bfloat16)          # packed like the QKV GEMM output
    qkv[:, :, 0] *= 2.0                                                              # peaked softmax rows
    out = torch.zeros(B, Tq, D, dtype=torch.bfloat16, device=DEV)
    a = L.attention_packed(qkv, out, B, H, Tq, Tk, hd, scale=hd ** -0.5)
    L.check(L.load().ovo_attention(C.byref(a), L.stream()))
    q, k, v = (qkv[:, :n, i].float().permute(0, 2, 1, 3) for i, n in ((0, Tq), (1, Tk), (2, Tk)))
    ref = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1) @ v
    ref = ref.permute(0, 2, 1, 3).reshape(B, Tq, D)
    # P is rounded to bf16 before P.V (rel 2^-9) and O is stored in bf16
    torch.testing.assert_close(out.float(), ref, atol=2e-2, rtol=2e-2)
    assert (out.float() - ref).abs().mean() < 2e-3


@pytest.mark.parametrize("B,H,Tq,Tk,hd", [(2, 16, 577, 577, 64), (6, 2, 196, 196, 56), (1, 1, 4096, 4096, 56), (2, 8, 257, 257, 128), (64, 4, 16, 16, 56),
                                          (1, 2, 130, 70, 72), (4, 8, 8, 8, 32)])
def test_attention_prescaled_queries(B, H, Tq, Tk, hd):
    """ovo_attention_t.scale == 0 (ABI v9): the queries arrive multiplied by log2(e) / sqrt(hd) -- the encoders fold the factor into the q rows of
    their QKV weights in f32, before the bf16 rounding -- and the kernel applies no factor: no second rounding of the bf16 queries (ADVICE r4:
    2e-3 max / 9e-5 mean output error at unit variance with the in-kernel product, against 4e-7 without).  Compared with softmax2 of the SAME bf16
    operands in f32; peaky rows (3x variance), where the second rounding cost 7e-2."""
    from ovo_amd import _lib as L
    g = torch.Generator().manual_seed(B + H + Tq + Tk + hd + 1)
    D, T = H * hd, max(Tq, Tk)
    raw = torch.randn(B, T, 3, H, hd, generator=g)
    raw[:, :, 0] *= 3.0
    c = L.LOG2E / hd ** 0.5
    pre = raw.clone()
    pre[:, :, 0] *= c
    outs = {}
    for name, t, scale in (("prescaled", pre, 0.0), ("in_kernel", raw, hd ** -0.5)):
        qkv = t.to(DEV, torch.bfloat16)
        out = torch.zeros(B, Tq, D, dtype=torch.bfloat16, device=DEV)
        a = L.attention_packed(qkv, out, B, H, Tq, Tk, hd, scale=scale)
        L.check(L.load().ovo_attention(C.byref(a), L.stream()))
        q, k, v = (qkv[:, :n, i].float().permute(0, 2, 1, 3) for i, n in ((0, Tq), (1, Tk), (2, Tk)))
        f = math.log(2.0) if scale == 0.0 else scale
        ref = (torch.softmax(q @ k.transpose(-1, -2) * f, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, Tq, D)
        outs[name] = (out.float() - ref).abs()
    # what is left with prescaled queries: P rounded to bf16 before P V (rel 2^-9) and the bf16 store of O
    assert outs["prescaled"].max() < 3e-2 and outs["prescaled"].mean() < 1.5e-3
    assert outs["prescaled"].mean() <= outs["in_kernel"].mean() * 1.05 + 1e-5       # never worse than the form with the second rounding


@pytest.mark.parametrize("B,H,Tq,Tk,hd", [(2, 4, 577, 577, 64), (1, 2, 1100, 1100, 56), (2, 2, 196, 196, 56), (1, 2, 300, 700, 128), (1, 1, 130, 4096, 64)])
def test_attention_rescale_path(B, H, Tq, Tk, hd):
    """The online softmax keeps a reference maximum per query and only rescales when a score outgrows it by 2^6 (attention.hip, fast / slow path):
    keys whose scores jump far above everything before them -- at a late tile, for some queries only, and a slow drift upwards -- must go through
    the rare branch and still match the fp32 softmax (cdna guide rule 26: a rare data-dependent branch needs an input that forces it)."""
    g = torch.Generator().manual_seed(B + H + Tq + Tk + hd)
    D, T = H * hd, max(Tq, Tk)
    qkv = torch.randn(B, T, 3, H, hd, generator=g)
    qkv[:, :, 1] *= torch.linspace(0.2, 3.0, T).reshape(1, T, 1, 1)                  # scores drift upwards tile after tile
    for key, qrow in ((Tk - 3, 5), (Tk // 2 + 7, Tq // 2), (70, Tq - 1), (Tk - 1, 0)):
        qkv[:, key, 1] = 6.0 * qkv[:, qrow, 0] / qkv[:, qrow, 0].norm(dim=-1, keepdim=True) * hd ** 0.5   # one key far above the rest for one query
    qkv = qkv.to(DEV, torch.bfloat16)
    out = _attention_call(qkv, B, H, Tq, Tk, hd)
    q, k, v = (qkv[:, :n, i].float().permute(0, 2, 1, 3) for i, n in ((0, Tq), (1, Tk), (2, Tk)))
    ref = (torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, Tq, D)
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.float(), ref, atol=3e-2, rtol=3e-2)
    assert (out.float() - ref).abs().mean() < 3e-3


def _attention_call(qkv, B, H, Tq, Tk, hd, causal=0, scale=None, out=None):
    """ovo_attention on a packed qkv; scale None: hd ** -0.5; out None: a fresh [B, Tq, H hd] (else any bf16 tensor of that many elements)."""
    from ovo_amd import _lib as L
    if out is None:
        out = torch.zeros(B, Tq, H * hd, dtype=torch.bfloat16, device=DEV)
    a = L.attention_packed(qkv, out, B, H, Tq, Tk, hd, scale=hd ** -0.5 if scale is None else scale, causal=causal)
    L.check(L.load().ovo_attention(C.byref(a), L.stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B,H,Tq,Tk,hd", [(24, 16, 577, 577, 64), (30, 8, 196, 196, 56), (10, 16, 49, 196, 56), (2, 4, 100, 300, 64), (1, 2, 577, 592, 64),
                                          (3, 1, 33, 65, 40), (2, 2, 1200, 128, 64), (1, 1, 16, 80, 8), (300, 2, 197, 197, 64), (64, 2, 64, 64, 56),
                                          (4, 8, 256, 256, 72), (2, 16, 257, 257, 80), (2, 3, 300, 333, 96), (2, 4, 700, 1500, 128), (3, 2, 130, 200, 120), (2, 2, 90, 130, 88)])
def test_attention32_kernel_vs_16x16_kernel(B, H, Tq, Tk, hd, monkeypatch):
    """k_attention32 (32 x 32 x 16 MFMA tiles, 32 queries per wave, row sum through the ones column when head_dim <= 56) against k_attention (16 x 16 x 32
    tiles): the same softmax scheme, the same rounding points (Q prescaled to bf16, P in bf16, fp32 accumulation) -- only the summation order inside the
    products differs, so the bf16 outputs agree to an ulp or two."""
    g = torch.Generator().manual_seed(B * 7 + H + Tq + Tk + hd)
    qkv = torch.randn(B, max(Tq, Tk), 3, H, hd, generator=g).to(DEV, torch.bfloat16)
    qkv[:, :, 0] *= 2.0
    monkeypatch.setenv("OVO_ATTN32", "1")
    new = _attention_call(qkv, B, H, Tq, Tk, hd)
    monkeypatch.setenv("OVO_ATTN32", "0")
    monkeypatch.setenv("OVO_ATTN_NO_TINY", "1")
    old = _attention_call(qkv, B, H, Tq, Tk, hd)
    torch.testing.assert_close(new.float(), old.float(), atol=4e-3, rtol=1.6e-2)
    assert (new.float() - old.float()).abs().mean() < 4e-4


@pytest.mark.parametrize("M,N,K,d,win,mode,act,out", [
    (65536, 336, 128, 112, (1, 256, 256, 8, 8), 1, 0, torch.bfloat16),      # hiera_b+ stage-1 QKV: LayerNorm + window partition in the operand load
    (65536, 448, 128, 112, None, 1, 1, torch.bfloat16),                      # stage-1 FC1 + GELU
    (17424, 672, 256, 224, (1, 130, 130, 4, 4), 1, 0, torch.bfloat16),       # windows that do not tile the grid: padding rows read zeros
    (16384, 896, 256, 224, None, 1, 1, torch.bfloat16),
    (65536, 432, 192, 144, (1, 256, 256, 8, 8), 1, 0, torch.bfloat16),       # hiera_l stage 1
    (65536, 256, 128, 112, None, 2, 0, torch.float32),                       # FPN lateral: cast only
    (65536, 32, 256, 256, None, 2, 0, torch.float32),                        # conv_s0
    (65536, 224, 128, 112, (1, 256, 256, 8, 8), 2, 0, "pool"),               # stage-change skip path: projection + 2 x 2 max-pool in the epilogue (bit-equal)
    (65536, 224, 128, 112, (1, 256, 256, 8, 8), 1, 0, "pool"),
    (32768, 448, 256, 224, (2, 128, 128, 4, 4), 1, 0, "pool")])
def test_gemm_with_layernorm_in_the_operand_load(M, N, K, d, win, mode, act, out):
    """ovo_gemm_f32a (gemm_stream.hip, F32A) against the two-pass form it replaces -- LayerNorm / cast of the f32 rows in torch (same formula:
    two-pass statistics, (x - mean) * rstd * gamma + beta, bf16 RNE), then ovo_gemm on the bf16 copy.  The cast-only mode is bit-equal; with
    LayerNorm the row statistics are summed in another order, so a few normalised values round the other way: the outputs then differ by one
    operand ulp in a dot product of d terms -- at most one ulp of the stored bf16 output, on a fraction of a percent of the elements."""
    from ovo_amd import _lib as L
    lib = L.load()
    pool = out == "pool"
    out = torch.float32 if pool else out
    g = torch.Generator().manual_seed(M + N + K)
    if win is None:
        rows_src = M
        src = torch.arange(M)
    else:
        B, H, W, wh, ww = win
        nwh, nww = -(-H // wh), -(-W // ww)
        assert B * nwh * nww * wh * ww == M
        rows_src = B * H * W
        m = torch.arange(M)
        w_, p_ = m // (wh * ww), m % (wh * ww)
        b_, wr = w_ // (nwh * nww), w_ % (nwh * nww)
        y, x_ = (wr // nww) * wh + p_ // ww, (wr % nww) * ww + p_ % ww
        src = torch.where((y < H) & (x_ < W), (b_ * H + y) * W + x_, torch.full_like(m, -1))
    x = (torch.randn(rows_src, d, generator=g) * 2 + 0.5).to(DEV)
    gamma, beta = (torch.randn(d, generator=g) * 0.5 + 1).to(DEV), (torch.randn(d, generator=g) * 0.1).to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(DEV, torch.bfloat16)
    w[:, d:] = 0
    bias = torch.randn(N, generator=g).to(DEV)
    # the two-pass form
    xs = x[src.clamp(min=0).to(DEV)]
    if mode == 1:
        mean = xs.mean(1, keepdim=True)
        rstd = torch.rsqrt(((xs - mean) ** 2).mean(1, keepdim=True) + 1e-6)
        xs = (xs - mean) * rstd * gamma + beta
    a = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
    a[:, :d] = xs.to(torch.bfloat16)
    a[(src < 0).to(DEV)] = 0
    ref = _gemm(a, w, bias, out_dtype=out, act=act)
    if pool:                                                         # window order -> spatial grid -> 2 x 2 max-pool (hieradet.py do_pool; k_pool_unwindow)
        B, H, W = win[:3]
        grid = torch.empty(B * H * W, N, device=DEV)
        grid[src.to(DEV)] = ref
        ref = torch.nn.functional.max_pool2d(grid.reshape(B, H, W, N).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(-1, N).contiguous()
    got = torch.empty(ref.shape[0], N, dtype=out, device=DEV)
    q = L.gemm_desc(None, w, got, bias=bias, act=act, rows=M, ldc=N)      # (pooled: got holds a quarter of the M rows)
    wd = None
    if win is not None:
        wd = L.Window(); wd.B, wd.H, wd.W, wd.wh, wd.ww = win
    L.check(lib.ovo_gemm_f32a(C.byref(q), C.byref(wd) if wd is not None else None, x.data_ptr(), d, gamma.data_ptr(), beta.data_ptr(), 1e-6, mode,
                              int(pool), L.stream()))
    torch.cuda.synchronize()
    if mode == 2:
        assert torch.equal(got, ref)
        return
    rms = ref.float().pow(2).mean().sqrt()
    diff = (got.float() - ref.float()).abs()
    print(f"({M},{N},{K}) fused LayerNorm: max {diff.max().item() / rms.item():.2e} rms {(diff.pow(2).mean().sqrt() / rms).item():.2e} of the output rms, "
          f"{(got != ref).float().mean().item():.2%} of the elements differ")
    # (measured: 0.01 % of the outputs differ, each by ONE bf16 ulp of its own magnitude -- 2^-7 relative; rms 3e-5 of the output rms)
    if pool:                                                         # f32 outputs: a flipped bf16 operand moves a dot product by ~2^-8 |a w|, not by an output ulp
        assert diff.max() < 2e-2 * rms and diff.pow(2).mean().sqrt() < 2e-4 * rms
        return
    assert diff.max() <= ref.float().abs().max() * 2.0 ** -7 and diff.pow(2).mean().sqrt() < 2e-4 * rms and (got != ref).float().mean() < 2e-3
    if win is not None:
        pad = (src < 0).to(DEV)
        if pad.any():                                                # a padding row: zeros . W + bias
            exp = bias if act == 0 else torch.nn.functional.gelu(bias)
            torch.testing.assert_close(got[pad].float(), exp.expand(int(pad.sum()), N).to(out).float(), atol=0, rtol=0)
    small = L.Gemm.from_buffer_copy(q)
    small.M = 1024                                                   # below the streaming kernel's range: nothing launched
    assert lib.ovo_gemm_f32a(C.byref(small), None, x.data_ptr(), d, gamma.data_ptr(), beta.data_ptr(), 1e-6, mode, 0, L.stream()) == L.E_UNSUPPORTED


@pytest.mark.parametrize("rows,d,k1", [(65536, 112, 128), (32768 + 40, 224, 256), (16384 + 5, 96, 128), (20000, 192, 192), (16400, 144, 192), (24000, 288, 320)])
def test_fused_mlp_stream_vs_two_products_and_torch(rows, d, k1):
    """ovo_mlp_f32 (mlp_stream.hip): x += fc2(GELU(fc1(LayerNorm(x)))) in one launch, the hidden row never leaving the registers, against
    (a) the two launches it replaces -- ovo_gemm_f32a (LayerNorm in the operand load, table GELU) into a bf16 hidden matrix, then ovo_gemm with the
    in-place f32 residual: the same roundings and the same k order, so the results agree to f32 summation noise -- and (b) the fp32 formula in
    torch on the same bf16-rounded weights.  Ragged row counts (a last 16-row block that is partly / wholly past the end), every instantiated
    width (hiera_b+ 112 / 224, hiera_t / s 96 / 192, hiera_l 144)."""
    from ovo_amd import _lib as L
    lib = L.load()
    hid = 4 * d
    g = torch.Generator().manual_seed(rows + d)
    x0 = (torch.randn(rows, d, generator=g) * 2 + 0.5).to(DEV)
    gamma, beta = (torch.randn(d, generator=g) * 0.5 + 1).to(DEV), (torch.randn(d, generator=g) * 0.1).to(DEV)
    w1 = torch.zeros(hid, k1, dtype=torch.bfloat16, device=DEV)
    w1[:, :d] = (torch.randn(hid, d, generator=g) * d ** -0.5).to(DEV, torch.bfloat16)
    w2 = (torch.randn(d, hid, generator=g) * hid ** -0.5).to(DEV, torch.bfloat16)
    b1, b2 = torch.randn(hid, generator=g).to(DEV), torch.randn(d, generator=g).to(DEV)
    # (a) two launches
    xa = x0.clone()
    h = torch.empty(rows, hid, dtype=torch.bfloat16, device=DEV)
    q = L.gemm_desc(None, w1, h, bias=b1, act=1, rows=rows)
    rc = lib.ovo_gemm_f32a(C.byref(q), None, xa.data_ptr(), d, gamma.data_ptr(), beta.data_ptr(), 1e-6, 1, 0, L.stream())
    two = rc == 0
    if two:
        L.gemm(h, w2, xa, bias=b2, add=xa)
    # fused
    xf = torch.cat([x0, torch.full((64, d), 7.0, device=DEV)])            # guard rows behind the end: must stay untouched
    L.check(lib.ovo_mlp_f32(xf.data_ptr(), rows, d, gamma.data_ptr(), beta.data_ptr(), 1e-6, w1.data_ptr(), k1, b1.data_ptr(), hid,
                            w2.data_ptr(), hid, b2.data_ptr(), L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(xf[rows:], torch.full((64, d), 7.0, device=DEV))
    got = xf[:rows]
    # (b) torch
    mean = x0.mean(1, keepdim=True)
    ln = (x0 - mean) * torch.rsqrt(((x0 - mean) ** 2).mean(1, keepdim=True) + 1e-6) * gamma + beta
    hh = torch.nn.functional.gelu(ln.to(torch.bfloat16).float() @ w1[:, :d].float().T + b1).to(torch.bfloat16).float()
    ref = x0 + hh @ w2.float().T + b2
    rms = (ref - x0).pow(2).mean().sqrt()
    err = (got - ref).abs()
    print(f"fused MLP ({rows}, {d}): vs torch max {err.max().item():.2e} rms {err.pow(2).mean().sqrt().item():.2e} (update rms {rms.item():.2e})")
    bad = (err > 3e-2 * rms).nonzero()
    if bad.shape[0]:                                                 # diagnosis: where the outliers sit (16-row blocks, columns)
        print("   outliers:", bad.shape[0], "row blocks", sorted(set((bad[:, 0] // 16).tolist()))[:10], "rows % 16", sorted(set((bad[:, 0] % 16).tolist())),
              "columns", sorted(set(bad[:, 1].tolist()))[:32], [(int(a), int(b), float(got[a, b]), float(ref[a, b])) for a, b in bad[:4].tolist()])
    assert err.max() < 3e-2 * rms and err.pow(2).mean().sqrt() < 2e-3 * rms     # a hidden value rounding the other way moves an output by 2^-9 |h w2|
    if two:
        dd = (got - xa).abs()
        print(f"   vs the two launches: max {dd.max().item():.2e}, {(got != xa).float().mean().item():.3%} of the elements differ")
        assert dd.max() < 2e-2 * rms and dd.pow(2).mean().sqrt() < 5e-4 * rms
    assert lib.ovo_mlp_f32(xf.data_ptr(), 1024, d, gamma.data_ptr(), beta.data_ptr(), 1e-6, w1.data_ptr(), k1, b1.data_ptr(), hid,
                           w2.data_ptr(), hid, b2.data_ptr(), L.stream()) == L.E_UNSUPPORTED       # short streams: the two products


_MLP_VARIANT_RESULTS = {}


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("rows,d,k1", [(786432, 112, 128), (196608, 224, 256)])
def test_fused_mlp_stream_is_deterministic(rows, d, k1, variant, monkeypatch):
    """Repeated launches of ovo_mlp_f32 on the same input give the same bits, with other work (allocations at shifting addresses, a GEMM) between
    them: the kernel's only cross-wave state is the double-buffered weight chunks in LDS (DMA under the previous chunk's products).  Variant 0 = the
    default launch shape, 1 = one 512-thread workgroup per CU, 2 / 3 = two 256-thread workgroups per CU.  In round 5 variant 2 failed exactly this in
    EVERY launch at 786 432 rows -- a packed-f32 LayerNorm-statistics chain from the SLP vectoriser, not the LDS-DMA ring (mlp_stream.hip:
    mlp_stream_launch; the three files with an in-load LayerNorm are built with -fno-slp-vectorize) -- and is now the default shape of stage 1.  All
    variants compute a row with the same instructions: their results are identical to each other too."""
    from ovo_amd import _lib as L
    import random
    lib = L.load()
    monkeypatch.setenv("OVO_KNOBS_DYNAMIC", "1")
    if variant:
        monkeypatch.setenv("OVO_MLP_RB", str(variant))
    hid = 4 * d
    g = torch.Generator().manual_seed(rows + d)
    x0 = (torch.randn(rows, d, generator=g) * 2 + 0.5).to(DEV)
    gamma, beta = (torch.randn(d, generator=g) * 0.5 + 1).to(DEV), (torch.randn(d, generator=g) * 0.1).to(DEV)
    w1 = torch.zeros(hid, k1, dtype=torch.bfloat16, device=DEV)
    w1[:, :d] = (torch.randn(hid, d, generator=g) * d ** -0.5).to(DEV, torch.bfloat16)
    w2 = (torch.randn(d, hid, generator=g) * hid ** -0.5).to(DEV, torch.bfloat16)
    b1, b2 = torch.randn(hid, generator=g).to(DEV), torch.randn(d, generator=g).to(DEV)

    def call(x):
        L.check(lib.ovo_mlp_f32(x.data_ptr(), rows, d, gamma.data_ptr(), beta.data_ptr(), 1e-6, w1.data_ptr(), k1, b1.data_ptr(), hid,
                                w2.data_ptr(), hid, b2.data_ptr(), L.stream()))
    ref = x0.clone()
    call(ref)
    rnd, junk, big = random.Random(1), [], torch.randn(4096, 4096, device=DEV, dtype=torch.bfloat16)
    for it in range(24):
        junk.append(torch.empty(rnd.randrange(1, 1 << 22), dtype=torch.uint8, device=DEV))
        if len(junk) > 6:
            junk.pop(rnd.randrange(len(junk)))
        if it % 3 == 0:
            big @ big
        x = torch.cat([x0, torch.full((rnd.randrange(1, 64), d), 7.0, device=DEV)])
        call(x)
        assert torch.equal(x[:rows], ref), f"launch {it} differs from the first in {(x[:rows] != ref).any(1).sum().item()} rows"
    first = _MLP_VARIANT_RESULTS.setdefault((rows, d), ref.cpu())
    assert torch.equal(ref.cpu(), first), "launch shapes disagree"


def test_layernorm_embed_im2col_rope():
    from ovo_amd import _lib as L
    lib = L.load()
    g = torch.Generator().manual_seed(5)
    rows, d = 1154, 1024
    x = (torch.randn(rows, d, generator=g) * 3 + 1).to(DEV)
    gm, bt = torch.randn(d, generator=g).to(DEV), torch.randn(d, generator=g).to(DEV)
    y = torch.empty_like(x)
    L.check(lib.ovo_layernorm(L.ptr(x), d, rows, d, L.ptr(gm), L.ptr(bt), 1e-5, L.ptr(y), d, 0, L.stream()))
    ref = torch.nn.functional.layer_norm(x, (d,), gm, bt, 1e-5)
    torch.testing.assert_close(y, ref, atol=2e-5, rtol=2e-5)
    yb = torch.empty(rows, d, dtype=torch.bfloat16, device=DEV)
    L.check(lib.ovo_layernorm(L.ptr(x), d, rows, d, L.ptr(gm), L.ptr(bt), 1e-5, L.ptr(yb), d, 2, L.stream()))
    assert (yb.float() - ref).abs().max() < 0.04 and torch.equal(yb, y.to(torch.bfloat16))     # bf16 ulp at |y| ~ 8 is 0.03
    # token assembly + ln_pre
    B, P = 2, 576
    patch = torch.randn(B, P, d, generator=g).to(DEV)
    cls, pos = torch.randn(1, d, generator=g).to(DEV), torch.randn(P + 1, d, generator=g).to(DEV)
    out = torch.empty(B, P + 1, d, device=DEV)
    L.check(lib.ovo_vit_embed(L.ptr(patch), L.ptr(cls), 1, L.ptr(pos), B, P, d, L.ptr(gm), L.ptr(bt), 1e-5, L.ptr(out), L.stream()))
    tok = torch.cat([cls[None].expand(B, 1, d), patch], 1) + pos
    torch.testing.assert_close(out, torch.nn.functional.layer_norm(tok, (d,), gm, bt, 1e-5), atol=2e-5, rtol=2e-5)
    L.check(lib.ovo_vit_embed(L.ptr(patch), L.ptr(cls), 1, L.ptr(pos), B, P, d, None, None, 0.0, L.ptr(out), L.stream()))
    assert torch.equal(out, tok)
    # im2col == unfold (non-overlapping 14x14 and overlapping 7x7 / stride 4 / pad 3)
    img = torch.randn(2, 3, 56, 56, generator=g).to(DEV)
    for ksz, stride, pad in ((14, 14, 0), (7, 4, 3)):
        kreal = 3 * ksz * ksz
        kpad = (kreal + 31) // 32 * 32
        oh = (56 + 2 * pad - ksz) // stride + 1
        col = torch.full((2 * oh * oh, kpad), 7.0, dtype=torch.bfloat16, device=DEV)
        L.check(lib.ovo_im2col(L.ptr(img), 2, 3, 56, 56, ksz, stride, pad, L.ptr(col), kpad, L.stream()))
        ref = torch.nn.functional.unfold(img, ksz, padding=pad, stride=stride).transpose(1, 2).reshape(-1, kreal)
        assert torch.equal(col[:, :kreal], ref.to(torch.bfloat16)) and (col[:, kreal:] == 0).all()
    # rope: rotation is norm preserving per pair, identity on the class token, matches the oracle formula
    from oracle import vit as OV
    Bq, T, H, hd = 2, 37, 4, 32
    qkv = torch.randn(Bq, T, 3, H, hd, generator=g).to(DEV, torch.bfloat16)
    ang = torch.rand(T, hd // 2, generator=g).repeat_interleave(2, 1) * 6
    ang[0] = 0
    cos, sin = ang.cos().to(DEV), ang.sin().to(DEV)
    before = qkv.clone()
    L.check(lib.ovo_rope_qk(L.ptr(qkv), Bq, T, H, hd, L.ptr(cos), L.ptr(sin), 1, L.stream()))
    for i in (0, 1):
        ref = OV._rope(before[:, :, i].float().permute(0, 2, 1, 3).cpu(), ang.cos(), ang.sin()).permute(0, 2, 1, 3)
        ref[:, 0] = before[:, 0, i].float().cpu()
        torch.testing.assert_close(qkv[:, :, i].float().cpu(), ref, atol=0.03, rtol=0.01)
    assert torch.equal(qkv[:, :, 2], before[:, :, 2]) and torch.equal(qkv[:, 0], before[:, 0])


@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("src,crop,out", [((480, 640), None, 336), ((480, 640), (0, 320, 480, 320), 336), ((480, 640), None, 1024),
                                          ((968, 1296), (484, 432, 484, 432), 336), ((37, 53), None, 84)])
def test_resize_normalize_vs_torch(aa, src, crop, out):
    from oracle import vit as OV
    from ovo_amd.encoders.vit import SPECS, HipViT, ViTSpec
    import dataclasses
    spec = dataclasses.replace(SPECS["tiny-pe"], image_size=out)      # preprocess only reads image_size / mean / std
    g = torch.Generator().manual_seed(3)
    img = (torch.rand(3, *src, generator=g) * 255).to(torch.uint8)
    vit = object.__new__(HipViT)
    vit.spec, vit.device = spec, torch.device(DEV)
    got = HipViT.preprocess(vit, img.to(DEV), [crop or (0, 0, *src)], scale=1 / 255.0, antialias=aa)[0].cpu()
    ref = OV.resize_normalize(img, out, spec.mean, spec.std, crop, scale=1 / 255.0, antialias=aa)
    torch.testing.assert_close(got, ref, atol=2e-5, rtol=1e-5)
    got_f = HipViT.preprocess(vit, img.float().to(DEV), [crop or (0, 0, *src)], scale=1 / 255.0, antialias=aa)[0].cpu()
    assert torch.equal(got, got_f)
    # the interleaved HWC frame read in place (what the pipeline hands over) == the planar copy of it, bit for bit
    got_hwc = HipViT.preprocess(vit, img.permute(1, 2, 0).contiguous().to(DEV), [crop or (0, 0, *src)], scale=1 / 255.0, antialias=aa)[0].cpu()
    assert torch.equal(got, got_hwc)


@pytest.mark.parametrize("card,src", [("ViT-B-16-qg", (480, 640)), ("ViT-B-16-qg", (640, 480)), ("ViT-B-16-qg", (384, 384)), ("ViT-H-14-378qg", (480, 640)),
                                      ("SigLIP-384", (480, 640)), ("SigLIP", (150, 200)), ("PE-Core-L14-336", (480, 640)), ("tiny-clip", (150, 200)),
                                      ("ViT-L-14-qg", (97, 1300))])
def test_clip_preprocess_vs_torch(card, src):
    """The kept open_clip transforms (clip_utils.py:83-84): Resize on the shorter side (antialiased bicubic) + CenterCrop for the OpenAI / DFN
    cards -- a 640 x 480 frame becomes 298 x 224 and loses 37 columns on either side -- squash for the timm-hub cards; against torch's own
    antialiased interpolate, which is what torchvision's tensor Resize calls.  Only the kept window is computed."""
    from oracle import vit as OV
    from ovo_amd.encoders.vit import SPECS, HipViT
    spec = SPECS[card]
    g = torch.Generator().manual_seed(5)
    img = torch.rand(3, *src, generator=g)
    vit = object.__new__(HipViT)
    vit.spec, vit.device = spec, torch.device(DEV)
    got = HipViT.preprocess_clip(vit, img[None].to(DEV))[0].cpu()
    ref = OV.open_clip_preprocess(img, spec.image_size, spec.mean, spec.std, spec.resize_mode, spec.interpolation)
    assert got.shape == ref.shape == (3, spec.image_size, spec.image_size)
    torch.testing.assert_close(got, ref, atol=2e-5, rtol=1e-5)
    if card == "ViT-B-16-qg" and src == (480, 640):
        assert vit.clip_window(480, 640) == (224, 298, 0, 37)
    u8 = (img * 255).to(torch.uint8)
    got8 = HipViT.preprocess_clip(vit, u8[None].to(DEV), scale=1 / 255.0)[0].cpu()
    ref8 = OV.open_clip_preprocess(u8.float() / 255.0, spec.image_size, spec.mean, spec.std, spec.resize_mode, spec.interpolation)
    torch.testing.assert_close(got8, ref8, atol=3e-5, rtol=1e-5)


def test_vit_forward_vs_hf_golden():
    """HIP bf16 forward vs HuggingFace CLIP (fp32) on the golden weights/input: width 64, 2 layers, 10 tokens."""
    from oracle import vit as OV
    from ovo_amd.encoders.vit import HipViT, ViTSpec
    d = golden("hf_clip_vit")
    sd = OV.hf_clip_to_openclip({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")})
    spec = ViTSpec("hf-golden", 48, 16, 64, 2, 4, 256, 32, act="quick_gelu")
    vit = HipViT(spec, sd, device=DEV)
    x = torch.from_numpy(d["x"]).to(DEV)
    emb = vit.forward(x).cpu().numpy()
    # bf16 operands through 2 blocks: observed ~3e-3 abs on outputs of magnitude ~1
    np.testing.assert_allclose(emb, d["image_embeds"], atol=3e-2, rtol=3e-2)
    cos = (emb * d["image_embeds"]).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(d["image_embeds"], axis=1)
    assert cos.min() > 0.9995
    tok = vit.forward(x, tokens=True).cpu()
    ref = OV.vit_forward(sd, torch.from_numpy(d["x"]), patch=16, heads=4, act="quick_gelu", tokens=True)
    torch.testing.assert_close(tok, ref, atol=5e-2, rtol=5e-2)


@pytest.mark.parametrize("card,batch", [("tiny-pe", 3), ("ViT-B-16-qg", 2), ("ViT-L-14-qg", 1), ("PE-Core-L14-336", 2), ("ViT-H-14", 1), ("ViT-H-14-378qg", 1)])
def test_vit_forward_vs_oracle_full_size(card, batch):
    """Unit-normalised descriptor error vs the fp32 oracle: north_star bound 1e-3 (features) on every card of clip_utils.py:53-63
    (ViT-B/16, ViT-L/14, ViT-H/14 at 224 and 378, PE-L/14-336)."""
    from oracle import vit as OV
    from ovo_amd.encoders.vit import SPECS, HipViT, random_state
    spec = SPECS[card]
    sd = random_state(spec, seed=11)
    vit = HipViT(spec, sd, device=DEV)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(batch, 3, spec.image_size, spec.image_size, generator=g)
    rope = OV.rope_for(spec)
    torch.set_num_threads(max(1, torch.get_num_threads()))
    ref = OV.vit_forward(sd, x, patch=spec.patch, heads=spec.heads, act=spec.act, rope=rope)
    out = vit.forward(x.to(DEV)).cpu()
    nr, no = torch.nn.functional.normalize(ref, dim=-1), torch.nn.functional.normalize(out, dim=-1)
    err = (nr - no).abs().max().item()
    cos = (nr * no).sum(-1).min().item()
    print(f"{card}: max |unit feature error| = {err:.2e}, min cosine = {cos:.6f}")
    assert err < _bound(spec.out_dim) and cos > 0.9999


@pytest.mark.parametrize("m,d,n,act", [(2308, 1024, 3072, 0), (4100, 512, 2048, 1), (2100, 256, 768, 0), (2049, 448, 1344, 1)])
def test_gemm_fold_pieces_vs_torch(m, d, n, act):
    """ovo_gemm_fold_out / ovo_gemm_fold_stats / ovo_gemm_fold_in on their own: the producer's f32 result is bit-identical to ovo_gemm's, its bf16 copy is the
    rounding of that result, its partial statistics are the sums of each 64-column group; the consumer equals Linear(LayerNorm(x)) (+ GELU) in fp32 within bf16
    operand rounding, from the producer's partials and from the single partial of ovo_gemm_fold_stats alike; ragged last row block (m % 256 != 0)."""
    from ovo_amd import _lib as L
    lib = L.load()
    g0 = torch.Generator().manual_seed(m + n)
    a = (torch.randn(m, d, generator=g0)).to(DEV, torch.bfloat16)
    wo = (torch.randn(d, d, generator=g0) * d ** -0.5).to(DEV, torch.bfloat16)
    bo = (torch.randn(d, generator=g0) * 0.1).to(DEV)
    res = (torch.randn(m, d, generator=g0) + 0.4).to(DEV)
    ref_x = _gemm(a, wo, bias=bo, add=res)
    x = torch.empty_like(ref_x)
    xb = torch.empty(m, d, dtype=torch.bfloat16, device=DEV)
    parts = d // 64
    stats = torch.full((parts, m, 2), float("nan"), device=DEV)
    g = L.gemm_desc(a, wo, x, bias=bo, add=res)
    L.check(lib.ovo_gemm_fold_out(C.byref(g), L.ptr(xb), d, L.ptr(stats), m, L.stream()))
    assert torch.equal(x, ref_x)
    assert torch.equal(xb, ref_x.to(torch.bfloat16))
    grp = ref_x.double().view(m, parts, 64)
    want = torch.stack([grp.sum(-1), (grp * grp).sum(-1)], -1).permute(1, 0, 2)
    torch.testing.assert_close(stats.double(), want, rtol=2e-6, atol=2e-4)
    # consumer
    gamma, beta = (1 + 0.3 * torch.randn(d, generator=g0)), 0.2 * torch.randn(d, generator=g0)
    w, b = torch.randn(n, d, generator=g0) * d ** -0.5, 0.1 * torch.randn(n, generator=g0)
    wf, bf, cs = L.fold_layernorm(w, b, gamma, beta)
    wf_d, bf_d, cs_d = wf.to(DEV, torch.bfloat16), bf.to(DEV), cs.to(DEV)
    ref = torch.nn.functional.linear(torch.nn.functional.layer_norm(ref_x.cpu().float(), (d,), gamma, beta, 1e-5), w, b)
    if act == 1:
        ref = torch.nn.functional.gelu(ref)
    out = torch.empty(m, n, dtype=torch.bfloat16, device=DEV)
    g = L.gemm_desc(xb, wf_d, out, bias=bf_d, act=act)
    L.check(lib.ovo_gemm_fold_in(C.byref(g), None, L.ptr(stats), m, parts, d, L.ptr(cs_d), 1e-5, L.stream()))
    got = out.float().cpu()
    scale = ref.abs().max().item()
    assert (got - ref).abs().max().item() < 2.5e-2 * scale                    # bf16 operands + bf16 output
    assert ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item() < 6e-3
    one = torch.full((1, m, 2), float("nan"), device=DEV)
    xb2 = torch.empty_like(xb)
    L.check(lib.ovo_gemm_fold_stats(L.ptr(x), d, m, d, L.ptr(xb2), d, L.ptr(one), L.stream()))
    assert torch.equal(xb2, xb)
    out1 = torch.empty_like(out)
    g.C = out1.data_ptr()
    L.check(lib.ovo_gemm_fold_in(C.byref(g), None, L.ptr(one), m, 1, d, L.ptr(cs_d), 1e-5, L.stream()))
    assert (out1.float() - out.float()).abs().max().item() < 2e-2 * scale     # same rows, statistics summed in another order
    # outside the 256-row kernel's range nothing is launched
    g.M = 1024
    assert lib.ovo_gemm_fold_in(C.byref(g), None, L.ptr(stats), m, parts, d, L.ptr(cs_d), 1e-5, L.stream()) == L.E_UNSUPPORTED
    g.M, g.act = m, 2
    assert lib.ovo_gemm_fold_in(C.byref(g), None, L.ptr(stats), m, parts, d, L.ptr(cs_d), 1e-5, L.stream()) == L.E_UNSUPPORTED


@pytest.mark.parametrize("name,base,over,batch", [
    ("pe-l-336 x 4 layers (rope, 256 x 256 tiles, 16 partials)", "PE-Core-L14-336", dict(layers=4), 4),
    ("width 512, no rope (256 x 256 tiles, 8 partials)", "PE-Core-L14-336", dict(layers=3, width=512, heads=8, mlp_dim=2048, out_dim=512, image_size=224, patch=16, use_rope=False), 12),
    ("width 256 (256 x 128 tiles, 4 partials)", "PE-Core-L14-336", dict(layers=3, width=256, heads=4, mlp_dim=1024, out_dim=256, image_size=224, patch=16), 12),
])
def test_vit_layernorm_fold_vs_layernorm_kernels_and_oracle(monkeypatch, name, base, over, batch):
    """The LayerNorm fold of batched forwards (ovo_vit_layer_t.qkv_wf ..., vit.hip): rstd (bf16(x) . W'^T - mean colsum(W')) + b' in the QKV / FC1 epilogues with
    the statistics taken in the epilogue that wrote x -- against the LayerNorm kernels (OVO_VIT_LNFOLD=0, the same weights object) and the fp32 oracle."""
    import dataclasses
    from oracle import vit as OV
    from ovo_amd.encoders.vit import SPECS, HipViT, random_state
    spec = dataclasses.replace(SPECS[base], name="fold-test", **over)
    sd = random_state(spec, seed=5)
    gen = torch.Generator().manual_seed(3)
    for k in list(sd):                                   # LayerNorm weights away from (1, 0): the fold moves them into the matrices
        if ".ln_" in k and k.endswith("weight"):
            sd[k] = 1.0 + 0.3 * torch.randn(sd[k].shape, generator=gen)
        elif ".ln_" in k and k.endswith("bias"):
            sd[k] = 0.2 * torch.randn(sd[k].shape, generator=gen)
    vit = HipViT(spec, sd, device=DEV)
    assert vit.ln_fold and batch * spec.tokens >= 2048
    x = torch.randn(batch, 3, spec.image_size, spec.image_size, generator=gen)
    x = x + 0.5                                          # a non-zero mean through the residual stream
    ref = OV.vit_forward(sd, x, patch=spec.patch, heads=spec.heads, act=spec.act, rope=OV.rope_for(spec))
    monkeypatch.setenv("OVO_VIT_LNFOLD", "1")
    out_f = vit.forward(x.to(DEV)).cpu()
    out_f2 = vit.forward(x.to(DEV)).cpu()
    monkeypatch.setenv("OVO_VIT_LNFOLD", "0")
    out_p = vit.forward(x.to(DEV)).cpu()
    assert torch.equal(out_f, out_f2)                    # partial statistics are summed in a fixed order
    assert not torch.equal(out_f, out_p)                 # (the fold really ran)
    nr = torch.nn.functional.normalize(ref, dim=-1)
    ef = (nr - torch.nn.functional.normalize(out_f, dim=-1)).abs().max().item()
    ep = (nr - torch.nn.functional.normalize(out_p, dim=-1)).abs().max().item()
    print(f"{name}: max |unit feature error| folded {ef:.2e}, LayerNorm kernels {ep:.2e}")
    assert ef < _bound(spec.out_dim) and ef < 1.5 * ep + 1e-4


def test_vit_layernorm_fold_full_size_is_deterministic():
    """The headline shape (PE-L/14-336, 28 crops = 16 156 token rows, 24 layers) through the folded forward, 8 times: bit-identical outputs (partial statistics are
    summed in a fixed order; one workgroup per CU), finite, and within the descriptor bound of the LayerNorm-kernel forward of the same weights."""
    import os
    from ovo_amd.encoders.vit import SPECS, HipViT, random_state
    spec = SPECS["PE-Core-L14-336"]
    vit = HipViT(spec, random_state(spec, seed=3), device=DEV)
    assert vit.ln_fold
    x = torch.randn(28, 3, spec.image_size, spec.image_size, generator=torch.Generator().manual_seed(9)).to(DEV)
    os.environ["OVO_VIT_LNFOLD"] = "1"
    try:
        first = vit.forward(x).clone()
        for _ in range(7):
            assert torch.equal(vit.forward(x), first)
        os.environ["OVO_VIT_LNFOLD"] = "0"
        plain = vit.forward(x)
    finally:
        os.environ.pop("OVO_VIT_LNFOLD", None)
    assert torch.isfinite(first).all() and not torch.equal(first, plain)
    err = (torch.nn.functional.normalize(first, dim=-1) - torch.nn.functional.normalize(plain, dim=-1)).abs().max().item()
    print(f"folded vs LayerNorm-kernel forward, 24 layers at 16 156 rows: max |unit feature difference| = {err:.2e}")
    assert err < 1.5e-3                                   # two bf16 forwards, each within 1e-3 of the fp32 oracle (test_vit_forward_vs_oracle_full_size)


def test_siglip_forward_vs_hf_golden():
    """SigLIP tower (no class token, tanh-GELU, attention-pool head) vs HuggingFace SiglipVisionModel (fp32) on the golden
    weights / input: width 64, hidden 176 (zero padded to 192 on the device), 2 layers, 16 tokens."""
    from oracle import vit as OV
    from ovo_amd.encoders.vit import HipViT, ViTSpec
    d = golden("hf_siglip_vit")
    sd = OV.hf_siglip_to_openclip({k[2:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("w:")})
    spec = ViTSpec("hf-siglip-golden", 56, int(d["patch"]), 64, 2, int(d["heads"]), 176, 64, act="gelu_tanh", pre_ln=False,
                   cls_token=False, ln_eps=1e-6, mean=(0.5,) * 3, std=(0.5,) * 3, map_pool=True, patch_bias=True)
    vit = HipViT(spec, sd, device=DEV)
    x = torch.from_numpy(d["x"]).to(DEV)
    tok = vit.forward(x, tokens=True).cpu().numpy()
    np.testing.assert_allclose(tok, d["tokens"], atol=5e-2, rtol=5e-2)
    emb = vit.forward(x).cpu().numpy()
    np.testing.assert_allclose(emb, d["pooled"], atol=3e-2, rtol=3e-2)
    cos = (emb * d["pooled"]).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(d["pooled"], axis=1)
    assert cos.min() > 0.9995


@pytest.mark.parametrize("card,batch,layers", [("tiny-siglip", 3, None), ("SigLIP", 2, 3), ("SigLIP", 1, None), ("SigLIP-384", 1, 1), ("SigLIP2-384", 1, 1)])
def test_siglip_forward_vs_oracle(card, batch, layers):
    """SigLIP so400m shapes (width 1152, head_dim 72, hidden 4304 -> 4320 padded, 256 / 729 / 576 tokens) vs the fp32 oracle;
    `layers` trims the depth so the CPU side finishes in seconds (every block is the same code)."""
    import dataclasses
    from oracle import vit as OV
    from ovo_amd.encoders.vit import SPECS, HipViT, random_state
    spec = SPECS[card]
    if layers:
        spec = dataclasses.replace(spec, layers=layers)
    sd = random_state(spec, seed=13)
    vit = HipViT(spec, sd, device=DEV)
    x = torch.randn(batch, 3, spec.image_size, spec.image_size, generator=torch.Generator().manual_seed(3))
    tok = OV.vit_forward(sd, x, patch=spec.patch, heads=spec.heads, act=spec.act, pre_ln=False, cls_token=False, eps=spec.ln_eps, tokens=True)
    assert tok.shape[1] == spec.tokens
    ref = OV.map_pool(sd, tok, spec.heads, act=spec.act, eps=spec.ln_eps)
    out = vit.forward(x.to(DEV)).cpu()
    nr, no = torch.nn.functional.normalize(ref, dim=-1), torch.nn.functional.normalize(out, dim=-1)
    err, cos = (nr - no).abs().max().item(), (nr * no).sum(-1).min().item()
    print(f"{card}: max |unit feature error| = {err:.2e}, min cosine = {cos:.6f}")
    assert err < _bound(spec.out_dim) and cos > 0.9999
    got_tok = vit.forward(x.to(DEV), tokens=True).cpu()
    torch.testing.assert_close(got_tok, tok, atol=5e-2, rtol=5e-2)


@pytest.mark.parametrize("hw", [(100, 150), (170, 260)])
def test_textregion_predict_vs_oracle(hw):
    """Full region-descriptor path (crops -> ViT tokens -> mask resample -> stitch -> masked-mean pooling -> proj -> L2)."""
    from oracle import features as OF, vit as OV
    from ovo_amd import synthetic as syn
    from ovo_amd.encoders.vit import SPECS, HipViT, random_state
    from ovo_amd.entities.textregion import PETextRegion
    spec = SPECS["tiny-pe"]
    sd = random_state(spec, seed=4)
    vit = HipViT(spec, sd, device=DEV)
    tr = PETextRegion(vit, "PE-tiny-084", remove_global_patch=False)
    H, W = hw
    g = torch.Generator().manual_seed(8)
    img = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8)
    masks = syn.make_masks(H, W, grid=(2, 3), n_blobs=3, seed=6)
    out = tr.predict(img.to(DEV), torch.from_numpy(masks).to(DEV), scale=1 / 255.0).cpu().numpy()
    # oracle pipeline in fp32
    crops = tr._crops(H, W)
    batch = torch.stack([OV.resize_normalize(img, spec.image_size, spec.mean, spec.std, c, scale=1 / 255.0) for c in crops])
    tok = OV.vit_forward(sd, batch, patch=spec.patch, heads=spec.heads, act=spec.act, rope=OV.rope_for(spec), tokens=True)
    P, nh, nw = spec.grid, tr.crop_num_h, tr.crop_num_w
    x = OF.stitch_tokens(tok[:, 1:].numpy(), P, P * nh, P * nw, nh, nw)
    fm = OF.feature_masks(masks, P * nh, P * nw)
    dd = spec.width
    ref = OF.region_pool(x, fm, sd["attn_pool.attn.in_proj_weight"][2 * dd:], sd["attn_pool.attn.in_proj_bias"][2 * dd:],
                         sd["attn_pool.attn.out_proj.weight"], sd["attn_pool.attn.out_proj.bias"], sd["proj"])
    w_dev, cnt = tr.get_features_mask(torch.from_numpy(masks).to(DEV))
    assert np.array_equal(w_dev[:, :fm.shape[1]].float().cpu().numpy(), (fm > 0).astype(np.float32))     # {0,1} weights: exact
    assert np.array_equal(cnt.cpu().numpy(), (fm > 0).sum(1).astype(np.float32))
    empty = (fm > 0).sum(1) == 0              # a mask that covers no token: NaN in the reference (softmax of all -inf), NaN here
    assert np.isnan(out[empty]).all() and np.isnan(ref[empty]).all() and not np.isnan(out[~empty]).any()
    err = np.abs(out[~empty] - ref[~empty]).max()
    print(f"textregion {hw}: max |unit descriptor error| = {err:.2e} ({int(empty.sum())} empty masks)")
    assert err < 3e-3 and out.shape == (masks.shape[0], spec.out_dim)
    np.testing.assert_allclose(np.linalg.norm(out[~empty], axis=1), 1.0, atol=1e-5)


def test_textregion_shared_crops_equal_separate_forwards():
    """`share_identical_crops` (off by default): a frame smaller than two crop sizes per side tiles into ONE tile = the global image
    (crops = [whole, whole], textregion.py:104-143); encoding it once and using the tokens for both crops gives the same bits as the
    reference's two forwards.  A frame with distinct tiles is untouched by the switch."""
    from ovo_amd import synthetic as syn
    from ovo_amd.encoders.vit import SPECS, HipViT, random_state
    from ovo_amd.entities.textregion import PETextRegion
    spec = SPECS["tiny-pe"]
    vit = HipViT(spec, random_state(spec, seed=4), device=DEV)
    both = PETextRegion(vit, "PE-tiny-084", remove_global_patch=True, share_identical_crops=False)
    once = PETextRegion(vit, "PE-tiny-084", remove_global_patch=True, share_identical_crops=True)
    g = torch.Generator().manual_seed(3)
    for (H, W), n_fwd in (((100, 150), 1), ((170, 260), 7), ((90, 200), 3)):
        img = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8).to(DEV)
        masks = torch.from_numpy(syn.make_masks(H, W, grid=(2, 3), n_blobs=3, seed=6)).to(DEV)
        assert len(once.forward_crops(H, W)) == n_fwd and len(both.forward_crops(H, W)) == len(both._crops(H, W))
        a, b = both.predict(img, masks, scale=1 / 255.0), once.predict(img, masks, scale=1 / 255.0)
        assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))


@pytest.mark.parametrize("cls_offset,axis_order", [(1, "xy"), (0, "xy"), (1, "yx"), (0, "yx")])
def test_rope_conventions_hip_vs_oracle(cls_offset, axis_order):
    """PE's Rope2D is unpinned upstream knowledge: its two conventions are switches (ViTSpec.rope_cls_offset / rope_axis_order).  For all four
    combinations the HIP forward (tables from ovo_amd.encoders.vit.rope_tables, rotation in the QKV GEMM epilogue) must follow the oracle's
    independently written tables (oracle/vit.py:rope2d_tables) -- and the combinations must really differ."""
    import dataclasses
    from oracle import vit as OV
    from ovo_amd.encoders.vit import SPECS, HipViT, random_state, rope_tables
    spec = dataclasses.replace(SPECS["tiny-pe"], rope_cls_offset=cls_offset, rope_axis_order=axis_order)
    sd = random_state(spec, seed=21)
    cos, sin = rope_tables(spec)
    ocos, osin = OV.rope_for(spec)
    torch.testing.assert_close(cos, ocos, atol=2e-6, rtol=0)
    torch.testing.assert_close(sin, osin, atol=2e-6, rtol=0)
    x = torch.randn(2, 3, spec.image_size, spec.image_size, generator=torch.Generator().manual_seed(4))
    ref = OV.vit_forward(sd, x, patch=spec.patch, heads=spec.heads, act=spec.act, rope=(ocos, osin), tokens=True)
    out = HipViT(spec, sd, device=DEV).forward(x.to(DEV), tokens=True).cpu()
    nr, no = torch.nn.functional.normalize(ref, dim=-1), torch.nn.functional.normalize(out, dim=-1)
    assert (nr - no).abs().max().item() < 3e-3
    other = dataclasses.replace(spec, rope_cls_offset=1 - cls_offset)
    ref2 = OV.vit_forward(sd, x, patch=spec.patch, heads=spec.heads, act=spec.act, rope=OV.rope_for(other), tokens=True)
    assert (torch.nn.functional.normalize(ref2, dim=-1) - nr).abs().max().item() > 1e-2     # the switch is not a no-op
    assert SPECS["PE-Core-L14-336"].rope_cls_offset == 1 and SPECS["PE-Core-L14-336"].rope_axis_order == "xy"


@pytest.mark.parametrize("th", [0.02, 0.07])
def test_textregion_remove_global_patch_vs_oracle(th):
    """a18 (textregion.py:31-50): the folded two-GEMM score must clear the same token columns as the literal T x T form."""
    from oracle import features as OF, vit as OV
    from ovo_amd import synthetic as syn
    from ovo_amd.encoders.vit import SPECS, HipViT, random_state
    from ovo_amd.entities.textregion import PETextRegion
    spec = SPECS["tiny-pe"]
    sd = random_state(spec, seed=4)
    vit = HipViT(spec, sd, device=DEV)
    tr = PETextRegion(vit, "PE-tiny-084", remove_global_patch=True, global_patch_threshold=th)
    plain = PETextRegion(vit, "PE-tiny-084", remove_global_patch=False)
    H, W = 170, 260
    g = torch.Generator().manual_seed(8)
    img = (torch.rand(3, H, W, generator=g) * 255).to(torch.uint8)
    masks = syn.make_masks(H, W, grid=(2, 3), n_blobs=3, seed=6)
    dm = torch.from_numpy(masks).to(DEV)
    feats = tr.get_img_features(img.to(DEV), scale=1 / 255.0)
    # the device's own stitched tokens (bf16) feed the oracle: the comparison isolates the filter, not the encoder
    from ovo_amd import _lib as L
    P, nh, nw, d = spec.grid, tr.crop_num_h, tr.crop_num_w, spec.width
    G = P * P * nh * nw
    gpad = (G + 31) // 32 * 32
    x_t = torch.empty((d, gpad), dtype=torch.bfloat16, device=DEV)
    L.check(L.load().ovo_stitch_tokens_t(L.ptr(feats), feats.shape[1], 1, d, P, nh, nw, L.ptr(x_t), gpad, L.stream()))
    w0, c0 = tr.get_features_mask(dm)
    w1, c1 = tr._remove_global_patch(x_t, w0, c0, G)
    x = x_t.float().t()[:G].cpu().numpy()
    fm0 = w0[:, :G].float().cpu().numpy()
    fm_ref, diff = OF.remove_global_patch(x, fm0, th)
    got = w1[:, :G].float().cpu().numpy()
    sure = np.abs(diff - th) > 4e-3                   # bf16 unit tokens / means in the two GEMMs: ~1e-3 on a cosine
    assert sure.mean() > 0.6 and (diff[sure] < th).any() and (diff[sure] >= th).any(), "fixture does not exercise both outcomes"
    assert np.array_equal(got[:, sure], fm_ref[:, sure])
    assert np.array_equal(c1.cpu().numpy(), got.sum(1)) and np.array_equal(w0[:, :G].float().cpu().numpy(), fm0)
    # end to end: predict() with the filter == the plain pooling over the filtered weights
    out = tr.predict(img.to(DEV), dm, scale=1 / 255.0)
    plain._crops(H, W)                                   # sets the tiling state predict() would have set
    ref = plain.pe_value_with_sam2_attn((w1, c1), feats)
    assert torch.equal(torch.nan_to_num(out), torch.nan_to_num(ref))


def test_vit_flops_accounting_matches_the_launched_work():
    """`ViTSpec.flops_per_image()` against the GEMM + attention work the forward really launches (see the Hiera twin)."""
    from ovo_amd import _lib as L
    from ovo_amd.encoders.vit import SPECS, HipViT
    spec = SPECS["ViT-B-16-qg"]
    enc = HipViT(spec, None, DEV, seed=1)
    x = torch.zeros(2, 3, spec.image_size, spec.image_size, device=DEV)
    enc.forward(x, tokens=True)
    lib = L.load()
    L.check(lib.ovo_profile_start())
    enc.forward(x, tokens=True)
    ms, work, n = (C.c_double * 9)(), (C.c_double * 9)(), (C.c_int64 * 9)()
    L.check(lib.ovo_profile_stop(ms, work, n, 9))
    launched = work[1] + sum(work[k] for k in (0, 3, 4, 5, 6, 7, 8))            # attention + every GEMM family (tiled, ping-pong, streaming)
    model = 2 * spec.flops_per_image()
    assert abs(launched - model) / model < 0.03, (launched, model)


@pytest.mark.parametrize("tag,hw", [("c", (100, 150)), ("d", (170, 260))])
def test_textregion_remove_global_patch_vs_reference_golden(tag, hw):
    """a18 against the reference itself: tests/golden/textregion.npz cases c / d were produced by the reference's PETextRegion with
    remove_global_patch=True (textregion.py:31-50, threshold 0.07) on a fake PE tower.  The product path (folded two-GEMM score on
    bf16 unit tokens) must clear exactly the same token columns and pool the same descriptors."""
    import types
    from ovo_amd.entities.textregion import PETextRegion
    d = golden("textregion")
    D, patch, crop = d["proj"].shape[0], int(d["patch"]), int(d["crop"])

    class FakeTower:                                       # what PETextRegion reads of a HipViT
        spec = types.SimpleNamespace(patch=patch, image_size=crop, width=D, cls_token=True)
        device = torch.device(DEV)
        proj = torch.from_numpy(d["proj"]).to(DEV)
        pool_weights = {"attn.in_proj_weight": torch.from_numpy(d["in_proj_weight"]), "attn.in_proj_bias": torch.from_numpy(d["in_proj_bias"]),
                        "attn.out_proj.weight": torch.from_numpy(d["out_proj_weight"]), "attn.out_proj.bias": torch.from_numpy(d["out_proj_bias"])}
    tr = PETextRegion(FakeTower(), "PE-fake-%03d" % crop, remove_global_patch=True, global_patch_threshold=float(d[f"{tag}_th"]))
    tr._crops(*hw)
    gh, gw, nh, nw = d[f"{tag}_grid"].tolist()
    assert (tr.points_per_h, tr.points_per_w, tr.crop_num_h, tr.crop_num_w) == (gh, gw, nh, nw)
    masks = torch.from_numpy(unpack(d[f"{tag}_masks"], int(d[f"{tag}_mask_w"]))).to(DEV)
    w0, c0 = tr.get_features_mask(masks)
    G = gh * gw
    assert np.array_equal(w0[:, :G].float().cpu().numpy(), (d[f"{tag}_feature_masks"] > 0).astype(np.float32))
    tokens = torch.from_numpy(d[f"{tag}_tokens"]).to(DEV)
    # the filter alone: same columns cleared as the reference's kept masks
    from ovo_amd import _lib as L
    gpad = w0.shape[1]
    x_t = torch.empty((D, gpad), dtype=torch.bfloat16, device=DEV)
    L.check(L.load().ovo_stitch_tokens_t(L.ptr(tokens), tokens.shape[1], 1, D, crop // patch, nh, nw, L.ptr(x_t), gpad, L.stream()))
    w1, c1 = tr._remove_global_patch(x_t, w0, c0, G)
    assert np.array_equal(w1[:, :G].float().cpu().numpy(), (d[f"{tag}_kept_masks"] > 0).astype(np.float32))
    out = tr.pe_value_with_sam2_attn((w0, c0), tokens).cpu().numpy()
    err = np.abs(out - d[f"{tag}_out"]).max()
    print(f"textregion {tag} (remove_global_patch): max |unit descriptor error| vs the reference = {err:.2e}")
    assert err < 3e-3


def test_textregion_full_size_640x480_vs_oracle():
    """The whole TextRegion path at the benchmark's size -- 640 x 480 frame, PE-Core-L14-336, global crop + 1 x 1 tile (2 crops of
    336^2), 32 masks -- HIP vs the fp32 oracle (resize, ViT tokens, stitch, feature masks, masked-mean pooling, folded projection, L2):
    |unit-descriptor error| <= 1e-3 (north_star), i.e. what bench.py's `parity.max_abs_desc_err` reports, as a test."""
    from oracle import features as OF, vit as OV
    from ovo_amd import synthetic as syn
    from ovo_amd.encoders.vit import SPECS, HipViT, random_state
    from ovo_amd.entities.textregion import PETextRegion
    spec = SPECS["PE-Core-L14-336"]
    sd = random_state(spec, seed=0)
    vit = HipViT(spec, sd, device=DEV)
    tr = PETextRegion(vit, "PE-Core-L14-336", remove_global_patch=False)
    H, W = 480, 640
    rgb = syn.render_rgb(H, W, 5)
    masks = syn.make_masks(H, W, grid=(4, 6), n_blobs=8, seed=5)
    assert masks.shape[0] == 32
    img = torch.from_numpy(rgb.transpose(2, 0, 1).copy())
    out = tr.predict(img.to(DEV), torch.from_numpy(masks).to(DEV), scale=1 / 255.0).cpu().numpy()
    nh, nw = max(H // spec.image_size, 1), max(W // spec.image_size, 1)
    ch, cw = -(-H // nh), -(-W // nw)
    crops = [(0, 0, H, W)] + [(max(min(i * ch + ch, H) - ch, 0), max(min(j * cw + cw, W) - cw, 0), ch, cw) for i in range(nh) for j in range(nw)]
    batch = torch.stack([OV.resize_normalize(img, spec.image_size, spec.mean, spec.std, c, 1 / 255.0) for c in crops])
    tok = OV.vit_forward(sd, batch, patch=spec.patch, heads=spec.heads, act=spec.act, rope=OV.rope_for(spec), tokens=True)
    P = spec.grid
    xs = OF.stitch_tokens(tok[:, 1:].numpy(), P, P * nh, P * nw, nh, nw)
    fm = OF.feature_masks(masks, P * nh, P * nw)
    d = spec.width
    ref = OF.region_pool(xs, fm, sd["attn_pool.attn.in_proj_weight"][2 * d:], sd["attn_pool.attn.in_proj_bias"][2 * d:],
                         sd["attn_pool.attn.out_proj.weight"], sd["attn_pool.attn.out_proj.bias"], sd["proj"])
    ok = ~np.isnan(ref).any(1)
    assert ok.sum() >= 28 and np.array_equal(np.isnan(out).any(1), ~ok)
    err = np.abs(out[ok] - ref[ok]).max()
    # error budget: the GPU's tokens through the ORACLE's fp32 tail (stitch, masked mean, folded projection, L2) = what the bf16
    # trunk alone costs; the GPU tail against that = what its three roundings (tokens -> bf16, mean -> bf16, folded weights in bf16) add
    feats = tr.get_img_features(img.to(DEV), scale=1 / 255.0).cpu().numpy()
    hyb = OF.region_pool(OF.stitch_tokens(feats[:, 1:], P, P * nh, P * nw, nh, nw), fm, sd["attn_pool.attn.in_proj_weight"][2 * d:],
                         sd["attn_pool.attn.in_proj_bias"][2 * d:], sd["attn_pool.attn.out_proj.weight"], sd["attn_pool.attn.out_proj.bias"], sd["proj"])
    e_trunk, e_tail = np.abs(hyb[ok] - ref[ok]).max(), np.abs(out[ok] - hyb[ok]).max()
    rms = lambda a: float(np.sqrt((a ** 2).mean()))
    print(f"TextRegion 640x480 / PE-L/14-336 / 32 masks: max |unit descriptor error| = {err:.2e} (rms {rms(out[ok] - ref[ok]):.2e});  budget: bf16 trunk with "
          f"an fp32 tail {e_trunk:.2e} (rms {rms(hyb[ok] - ref[ok]):.2e}), the tail's own roundings {e_tail:.2e} (rms {rms(out[ok] - hyb[ok]):.2e});  "
          f"token error max {np.abs(feats - tok.numpy()).max():.2e} rms {rms(feats - tok.numpy()):.2e} of rms {rms(tok.numpy()):.2e}")
    assert err <= 1e-3


def test_batched_preprocess_equals_per_image():
    """`ovo_resize_normalize_batch` (round 5: every frame x crop of an encoder look-ahead group in one launch) against the per-image launches: the same
    kernel body per pixel -> bit-identical, for the ViT's TextRegion crops (antialiased down-scaling, HWC u8 frames read in place) and SAM2's 1024^2 input."""
    from ovo_amd.encoders.hiera import SPECS as HS, HipHiera
    from ovo_amd.encoders.vit import SPECS as VS, HipViT
    g = torch.Generator().manual_seed(5)
    frames = [torch.randint(0, 256, (480, 640, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(5)]
    vit = HipViT(VS["PE-Core-L14-336"], None, DEV, 0)
    crops = [(0, 0, 480, 640), (72, 152, 336, 336)]
    one = torch.cat([vit.preprocess(f, crops, scale=1.0 / 255.0) for f in frames])
    many = vit.preprocess_batch(frames, crops, scale=1.0 / 255.0)
    assert many.shape == one.shape and torch.equal(one, many)
    chw = [f.permute(2, 0, 1).contiguous() for f in frames]             # CHW u8 path
    assert torch.equal(torch.cat([vit.preprocess(f, crops, scale=1.0 / 255.0) for f in chw]), vit.preprocess_batch(chw, crops, scale=1.0 / 255.0))
    sam = HipHiera(HS["hiera_test"], None, DEV, 0)
    assert torch.equal(torch.cat([sam.preprocess(f) for f in frames]), sam.preprocess_batch(frames))
    mixed = frames[:2] + [frames[2][:240].contiguous()]                  # frames of different sizes: the per-image path
    assert torch.equal(torch.cat([sam.preprocess(f) for f in mixed]), sam.preprocess_batch(mixed))


def test_fast_resize_kernel_equals_generic_kernel(monkeypatch):
    """The branch-free resize of an interleaved u8 frame (`k_resize_tri_hwc3<3 / 6>`: taps beyond the filter's support carry a zero weight instead of a
    branch) against the generic kernel (OVO_RESIZE_GENERIC=1): bit-identical, for SAM2's up-scaling (3 taps), the TextRegion crops (<= 6 taps; a crop
    touching the frame's last pixel: the 4-byte load's edge case) and a single-image call."""
    from ovo_amd.encoders.hiera import SPECS as HS, HipHiera
    from ovo_amd.encoders.vit import SPECS as VS, HipViT
    g = torch.Generator().manual_seed(6)
    frames = [torch.randint(0, 256, (480, 640, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(3)]
    vit = HipViT(VS["PE-Core-L14-336"], None, DEV, 0)
    sam = HipHiera(HS["hiera_test"], None, DEV, 0)
    crops = [(0, 0, 480, 640), (72, 152, 336, 336), (144, 304, 336, 336), (0, 0, 480, 320)]       # the third ends at the frame's last pixel
    fast = (vit.preprocess_batch(frames, crops, scale=1.0 / 255.0), sam.preprocess_batch(frames), vit.preprocess(frames[0], crops[:2], scale=1.0 / 255.0))
    monkeypatch.setenv("OVO_RESIZE_GENERIC", "1")
    slow = (vit.preprocess_batch(frames, crops, scale=1.0 / 255.0), sam.preprocess_batch(frames), vit.preprocess(frames[0], crops[:2], scale=1.0 / 255.0))
    for a, b in zip(fast, slow):
        assert torch.equal(a, b), f"max |difference| {(a - b).abs().max().item():.3e}"
